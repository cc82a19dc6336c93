"""flm_fallback_opts on the host: the new entry points, their layout rules and their argument checks (no GPU).

faces = 0 / NULL must be the flm_fcn_*_opts layout byte for byte; faces > 0 adds "cand_redo", "fallback_rows" and
"fallback_counts" (and the compact decode's partials) behind cand_cnt where the call takes the candidate path, and nothing
anywhere else; no existing name moves.
"""
import ctypes as C

import pytest

from flm_amd import _lib

NAMES = (b"f1", b"f2", b"f3", b"f4", b"f5", b"act0", b"act4", b"fc6", b"fc7", b"score5", b"fuse4", b"seg_feats", b"probs",
         b"cand_sub", b"cand_tau", b"cand_keys", b"cand_cnt", b"cand_cap")
NEW = (b"cand_redo", b"fallback_rows", b"fallback_counts")
OPTION_SETS = (None, dict(candidate_cap_div=5), dict(candidate_sub_phases=8, landmark_candidates=1))
ARCH = _lib.ARCH_FCN8


def _fo(opts):
    return None if opts is None else C.byref(_lib.ForwardOpts.make(**opts))


def _fb(faces):
    return None if faces is None else C.byref(_lib.FallbackOpts.make(faces))


def _shape(n=5, h=96, w=160, c=68, dt=1, out=_lib.OUT_LANDMARKS,
           mode=_lib.DECODE_TOPN, npts=4):
    return (n, h, w, c, dt, out, mode, npts)


def _bytes_fb(shape, opts, faces, arch=ARCH):
    return _lib.load().flm_fcn_workspace_bytes_fb(arch, *shape, _fo(opts), _fb(faces))


def _off_fb(name, shape, opts, faces, arch=ARCH):
    return _lib.load().flm_fcn_workspace_offset_fb(arch, name, *shape, _fo(opts), _fb(faces))


def test_symbols_are_exported_and_declared():
    lib = _lib.load()
    for name in ("flm_fallback_opts_init", "flm_fcn_workspace_bytes_fb", "flm_fcn_workspace_offset_fb", "flm_fcn_forward_fb"):
        assert name in _lib.EXPORTS
        assert hasattr(lib, name)
    fb = _lib.FallbackOpts()
    lib.flm_fallback_opts_init(C.byref(fb))
    assert fb.struct_size == C.sizeof(_lib.FallbackOpts) == 8 and fb.faces == 0
    assert C.sizeof(_lib.ForwardOpts) == 16          # flm_forward_opts did not grow


@pytest.mark.parametrize("opts", OPTION_SETS)
@pytest.mark.parametrize("dt", (0, 1))
def test_null_and_zero_are_the_opts_layout(opts, dt):
    lib = _lib.load()
    shape = _shape(dt=dt)
    ref = lib.flm_fcn_workspace_bytes_opts(ARCH, *shape, _fo(opts))
    assert ref > 0
    for faces in (None, 0):
        assert _bytes_fb(shape, opts, faces) == ref
        for name in NAMES:
            assert _off_fb(name, shape, opts, faces) == lib.flm_fcn_workspace_offset_opts(ARCH, name, *shape, _fo(opts)), name
        for name in NEW:
            assert _off_fb(name, shape, opts, faces) == -1, name


@pytest.mark.parametrize("opts", OPTION_SETS)
@pytest.mark.parametrize("dt", (0, 1))
def test_faces_grow_the_candidate_layout_and_move_nothing(opts, dt):
    shape = _shape(dt=dt)
    n = shape[0]
    base = _bytes_fb(shape, opts, 0)
    last = base
    for faces in (1, 3, n):
        total = _bytes_fb(shape, opts, faces)
        assert total > base and total >= last
        last = total
        for name in NAMES:
            assert _off_fb(name, shape, opts, faces) == _off_fb(name, shape, opts, 0), name
        cnt = _off_fb(b"cand_cnt", shape, opts, faces)
        redo, rows, counts = (_off_fb(k, shape, opts, faces) for k in NEW)
        # behind the counts' region of n + 1 words, in that order, inside the old total .. new total
        assert cnt + 4 * (n + 1) <= redo and redo + 4 * n <= rows and rows + 4 * faces <= counts and counts + 16 <= total
        assert redo >= base - 256 and redo % 256 == 0 and rows % 256 == 0 and counts % 256 == 0


@pytest.mark.parametrize("case", [
    dict(c=21),                                   # another class count
    dict(npts=33),                                # n_points beyond the candidate path
    dict(mode=_lib.DECODE_ALL, npts=0),           # the all-pixel mode
    dict(out=_lib.OUT_PROBS, mode=0, npts=0),     # no decode at all
    dict(h=416, w=608),                           # a map of 2^17 pixels or more
])
def test_faces_add_nothing_off_the_candidate_path(case):
    shape = _shape(**case)
    assert _bytes_fb(shape, None, 0) > 0
    assert _bytes_fb(shape, None, 3) == _bytes_fb(shape, None, 0)
    for name in NEW:
        assert _off_fb(name, shape, None, 3) == -1


def test_faces_add_nothing_without_candidates_or_on_fcn32():
    shape = _shape()
    off = dict(landmark_candidates=0)
    assert _bytes_fb(shape, off, 3) == _bytes_fb(shape, off, 0) > 0
    assert _off_fb(b"cand_redo", shape, off, 3) == -1
    assert _bytes_fb(shape, None, 3, _lib.ARCH_FCN32) == _bytes_fb(shape, None, 0, _lib.ARCH_FCN32) > 0
    assert _off_fb(b"fallback_rows", shape, None, 3, _lib.ARCH_FCN32) == -1


def test_more_faces_than_the_batch_means_the_batch():
    shape = _shape()
    n = shape[0]
    assert _bytes_fb(shape, None, 10 ** 6) == _bytes_fb(shape, None, n)
    for name in NAMES + NEW:
        assert _off_fb(name, shape, None, 10 ** 6) == _off_fb(name, shape, None, n), name


def test_bad_options_are_rejected_with_the_field_named():
    lib = _lib.load()
    shape = _shape()
    neg = _lib.FallbackOpts.make(-1)
    assert lib.flm_fcn_workspace_bytes_fb(ARCH, *shape, None, C.byref(neg)) == 0
    assert b"faces" in lib.flm_last_error()
    assert lib.flm_fcn_workspace_offset_fb(ARCH, b"probs", *shape, None, C.byref(neg)) == -1
    short = _lib.FallbackOpts.make(2)
    short.struct_size = 4
    assert lib.flm_fcn_workspace_bytes_fb(ARCH, *shape, None, C.byref(short)) == 0
    assert b"struct_size" in lib.flm_last_error()
    # the forward refuses them before it looks at a pointer
    dummy = C.c_void_p(256)
    for bad, field in ((neg, b"faces"), (short, b"struct_size")):
        rc = lib.flm_fcn_forward_fb(None, ARCH, dummy, dummy, 0, *shape[:5], shape[5], shape[6], shape[7], 0.0, dummy, dummy,
                                    1 << 40, None, C.byref(bad))
        assert rc != 0
        assert field in lib.flm_last_error()


def test_python_rejects_a_negative_budget_without_a_gpu():
    from flm_amd import prediction
    with pytest.raises(ValueError, match="fallback_faces"):
        prediction.FaceTracker(None, (64, 64), 1, fallback_faces=-1)


def test_the_bookkeeping_holds_workspaces_weakly():
    """The model remembers a workspace's layout by a weak reference: the entry goes with the tensor."""
    import gc
    import weakref

    import torch
    from flm_amd.networks import LANDMARKS_MODELS
    model = LANDMARKS_MODELS["fcn_8"](68, input_height=64, input_width=64)
    ws = torch.zeros(1024, dtype=torch.uint8)
    model._fallback_note(ws, False, (0, 256, 512, 2, 3))
    counts = model.fallback_counts(ws)
    rows, redo = model.fallback_rows(ws)
    assert counts.shape == (4,) and rows.shape == (2,) and redo.shape == (3,)
    with pytest.raises(KeyError):
        model.fallback_counts(torch.zeros(1024, dtype=torch.uint8))
    with pytest.raises(KeyError):
        model.fallback_counts()                      # no forward has used a cached workspace
    ref = weakref.ref(ws)
    del ws, counts, rows, redo
    gc.collect()
    assert ref() is None and not model._fb_last
