"""Host arithmetic of the workspace layout around the candidate path's map-size limit (no GPU: size and offset queries).

The candidate key is order_bits(p) << 32 | class << 17 | pixel: 17 bits of pixel index.  The layout (flm_api_fcn.hip,
landmark_candidates_enabled) therefore holds candidate buffers only while the OUTPUT map, (h + 8) x (w + 8), has fewer
than 2^17 pixels -- 352 x 352 (360 x 360 = 129,600) is the largest square input that has them, 352 x 384 (360 x 392 =
141,120) and the default 416 x 608 geometry (424 x 616 = 261,184) have none.  Swept here over every input size in
multiples of 32 up to 1024 x 1024, both types, n_points 1, 4 and 32:

  * "cand_keys" (and with it cand_sub / cand_tau / cand_cnt / cand_cap) is in the layout exactly when
    (h + 8) * (w + 8) < 2^17;
  * above the limit landmark_candidates = 1 and 0 size the same workspace (below it the lists cost bytes);
  * the fcn_32 graph and the generic class layouts (any count but 68) never hold candidate buffers.

Every answer of -1 is paired with a non-zero flm_fcn_workspace_bytes_opts of the same arguments: the layout exists and
lacks the buffer, the query did not refuse the shape.
"""
import ctypes as C

import pytest

import flm_amd  # noqa: F401
from flm_amd import _lib

SIZES = range(32, 1025, 32)
LIMIT = 1 << 17
CAND_NAMES = (b"cand_sub", b"cand_tau", b"cand_keys", b"cand_cnt", b"cand_cap")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _queries(lib, arch, c, dt, n_points, n=1, out_mode=None):
    out_mode = _lib.OUT_LANDMARKS if out_mode is None else out_mode
    on, off = _lib.ForwardOpts.make(), _lib.ForwardOpts.make(landmark_candidates=0)

    def offset(name, h, w, opts=on):
        return lib.flm_fcn_workspace_offset_opts(arch, name, n, h, w, c, dt, out_mode, _lib.DECODE_TOPN, n_points, C.byref(opts))

    def nbytes(h, w, opts=on):
        return lib.flm_fcn_workspace_bytes_opts(arch, n, h, w, c, dt, out_mode, _lib.DECODE_TOPN, n_points, C.byref(opts))
    return offset, nbytes, on, off


@pytest.mark.parametrize("dt", [_lib.FLM_F32, _lib.FLM_BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("n_points", [1, 4, 32])
def test_candidate_buffers_exist_exactly_below_2_17_output_pixels(lib, dt, n_points):
    offset, nbytes, on, off = _queries(lib, _lib.ARCH_FCN8, 68, dt, n_points)
    below = above = 0
    for h in SIZES:
        for w in SIZES:
            has = (h + 8) * (w + 8) < LIMIT
            b_on, b_off = nbytes(h, w, on), nbytes(h, w, off)
            assert b_on > 0 and b_off > 0, (h, w, lib.flm_last_error())
            got = offset(b"cand_keys", h, w)
            assert (got >= 0) == has, (h, w, got)
            assert offset(b"cand_keys", h, w, off) == -1, (h, w)
            if has:
                below += 1
                assert b_on > b_off, (h, w)
                assert 0 < got < b_on and offset(b"cand_cap", h, w) >= 64, (h, w)
            else:
                above += 1
                assert b_on == b_off, (h, w, b_on, b_off)
                assert all(offset(nm, h, w) == -1 for nm in CAND_NAMES), (h, w)
    assert below and above
    # the two sides of the cliff by name, and the default geometry of every model class
    assert offset(b"cand_keys", 352, 352) > 0 and offset(b"cand_keys", 352, 384) == -1 and offset(b"cand_keys", 384, 352) == -1
    assert offset(b"cand_keys", 416, 608) == -1 and nbytes(416, 608, on) == nbytes(416, 608, off)
    assert offset(b"probs", 352, 384) > 0 and offset(b"probs", 416, 608) > 0


def test_landmark_stats_layout_follows_the_same_limit(lib):
    """FLM_OUT_LANDMARKS_STATS shares the landmark mode's layout rule; three faces: the limit is per face."""
    offset, nbytes, on, off = _queries(lib, _lib.ARCH_FCN8, 68, _lib.FLM_BF16, 4, n=3, out_mode=_lib.OUT_LANDMARKS_STATS)
    for h in SIZES:
        for w in SIZES:
            assert nbytes(h, w) > 0
            assert (offset(b"cand_keys", h, w) >= 0) == ((h + 8) * (w + 8) < LIMIT), (h, w)


@pytest.mark.parametrize("dt", [_lib.FLM_F32, _lib.FLM_BF16], ids=["f32", "bf16"])
def test_fcn32_and_generic_class_layouts_never_hold_candidate_buffers(lib, dt):
    for arch, c in ((_lib.ARCH_FCN32, 68), (_lib.ARCH_FCN8, 1), (_lib.ARCH_FCN8, 5), (_lib.ARCH_FCN8, 64),
                    (_lib.ARCH_FCN8, 67), (_lib.ARCH_FCN8, 69), (_lib.ARCH_FCN8, 96)):
        offset, nbytes, on, off = _queries(lib, arch, c, dt, 4)
        for h in SIZES:
            for w in SIZES:
                b_on = nbytes(h, w, on)
                assert b_on > 0 and b_on == nbytes(h, w, off), (arch, c, h, w)
                assert offset(b"cand_keys", h, w) == -1, (arch, c, h, w)
                assert offset(b"probs", h, w) > 0, (arch, c, h, w)
