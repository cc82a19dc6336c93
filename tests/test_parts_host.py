"""CPU-side checks of the face-parts calls (flm_part_affines, flm_warp_parts_frames, flm_face_openness,
alignment.FaceParts / Openness, FaceTracker(parts=, openness=)): the exports, every argument check of the three C calls
(each answers before any launch, so without a GPU), the header's constants against the Python defaults,
tests/parts_ref.py's fit against tests/stats_ref.py's weighted similarity on the gathered points, and the Python
validation."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import flm_amd  # noqa: F401
from flm_amd import _lib, alignment

import parts_ref as ref
import stats_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "flm.h")).read()
P = C.c_void_p(0x1000)        # never dereferenced: every call below is rejected before a launch
CODES = {n: int(v) for n, v in re.findall(r"(FLM_ERR_\w+)\s*=\s*(-?\d+)", HEADER)}
ARG, SHAPE = CODES["FLM_ERR_ARG"], CODES["FLM_ERR_SHAPE"]


def err():
    return _lib.load().flm_last_error().decode()


def counts(*v):
    return (C.c_int32 * len(v))(*v)


# ---- exports, constants, defaults ---------------------------------------------------------------------------------------
def test_exports_constants_and_defaults():
    lib = C.CDLL(_lib.LIB_PATH)
    for name in ("flm_part_affines", "flm_warp_parts_frames", "flm_open_opts_init", "flm_face_openness"):
        assert hasattr(lib, name) and name in _lib.EXPORTS, name
    assert _lib.load().flm_abi_version() == 2          # purely additive
    for name, v in (("FLM_PARTS_MAX", _lib.PARTS_MAX), ("FLM_PART_MAX_POINTS", _lib.PART_MAX_POINTS),
                    ("FLM_PART_MAX_SIDE", _lib.PART_MAX_SIDE), ("FLM_OPEN_REC", _lib.OPEN_REC),
                    ("FLM_OPEN_STATE", _lib.OPEN_STATE), ("FLM_OPEN_MAX_MEASURES", _lib.OPEN_MAX_MEASURES),
                    ("FLM_OPEN_MAX_PAIRS", _lib.OPEN_MAX_PAIRS)):
        assert re.search(r"#define %s %d\b" % (name, v), HEADER), name
    assert (ref.REC, ref.STATE) == (alignment.OPEN_REC, alignment.OPEN_STATE) == (4, 8)
    assert tuple(ref.STATE_EMPTY) == tuple(alignment.OPEN_STATE_EMPTY)
    # the library's defaults are the Python defaults, and both are what the header says
    o = _lib.OpenOpts.make()
    d = alignment.Openness.default(68)
    assert (o.struct_size, o.reserved, o.n_measures) == (C.sizeof(_lib.OpenOpts), 0, 3)
    got = tuple(((o.width[g][0], o.width[g][1]), tuple((o.upper[g][v], o.lower[g][v]) for v in range(o.n_pairs[g])))
                for g in range(o.n_measures))
    assert got == d.measures == alignment.Openness().measures == ref.DEFAULT_MEASURES
    nums = (o.close_below, o.open_above, o.min_closed, o.max_closed, o.min_width)
    assert nums == (d.close_below, d.open_above, d.min_closed, d.max_closed, d.min_width) == (0.18, 0.22, 0.03, 0.5, 4.0)
    assert "close_below = 0.18, open_above = 0.22, min_closed = 0.03 s, max_closed = 0.5 s, min_width = 4 px" in HEADER
    assert ref.DEFAULT_TH == dict(close_below=0.18, open_above=0.22, min_closed=0.03, max_closed=0.5)
    s = d.struct()   # the struct a call gets is field for field the Openness
    assert [s.n_pairs[g] for g in range(3)] == [2, 2, 3] and s.width[2][1] == 64 and s.lower[2][2] == 65


def test_default_parts():
    p = alignment.FaceParts.default(68)
    assert p.size == (32, 48) and len(p) == 3 and list(p.counts) == [6, 6, 20]
    assert [list(p.part(r)[0]) for r in range(3)] == [list(range(36, 42)), list(range(42, 48)), list(range(48, 68))]
    assert (p.indices[0, 6:] == -1).all() and p.indices.shape == (3, 32) and p.templates.shape == (3, 32, 2)
    for r in range(3):   # centred, and the part's width fills PART_FILL of the patch's width
        t = p.part(r)[1]
        lo, hi = t.min(axis=0), t.max(axis=0)
        assert abs((hi[0] - lo[0]) - alignment.PART_FILL * 47) < 1e-9
        assert np.allclose((lo + hi) / 2, [23.5, 15.5]) and lo.min() >= 0 and hi[0] <= 47 and hi[1] <= 31
    with pytest.raises(ValueError, match="68 landmarks"):
        alignment.FaceParts.default(5)
    with pytest.raises(ValueError, match="68 landmarks"):
        alignment.Openness.default(5)


def test_python_validation():
    FP, OP = alignment.FaceParts, alignment.Openness
    t2 = np.zeros((2, 2))
    for bad in (lambda: FP([], [], (8, 8)), lambda: FP([[1, 2]] * 9, [t2] * 9, (8, 8)), lambda: FP([[1]], [np.zeros((1, 2))], (8, 8)),
                lambda: FP([list(range(33))], [np.zeros((33, 2))], (8, 8)), lambda: FP([[1, 2]], [np.zeros((3, 2))], (8, 8)),
                lambda: FP([[1, -2]], [t2], (8, 8)), lambda: FP([[1, 2]], [t2], (0, 8)), lambda: FP([[1, 2]], [t2], (8, 257)),
                lambda: FP([[1, 2]], [t2 + np.nan], (8, 8)), lambda: FP([[1.5, 2]], [t2], (8, 8)),
                lambda: OP(()), lambda: OP([((0, 1), ())]), lambda: OP([((0, 1), ((1, 2),) * 5)]),
                lambda: OP([((0, 1), ((1, 2),))] * 9), lambda: OP(close_below=0.3, open_above=0.3),
                lambda: OP(close_below=float("nan")), lambda: OP(min_closed=-1.0), lambda: OP(min_closed=0.6),
                lambda: OP(min_width=float("nan")), lambda: OP(dt=0.0), lambda: OP(dt=float("inf")), lambda: OP([(0, 1)])):
        with pytest.raises(ValueError):
            bad()
    from flm_amd import prediction
    with pytest.raises(ValueError, match="FaceParts"):
        prediction._parts_for("eyes", 68)
    with pytest.raises(ValueError, match="Openness"):
        prediction._openness_for(3, 68)
    with pytest.raises(ValueError, match="68 landmarks"):
        prediction._parts_for(True, 5)


# ---- argument checks: flm_part_affines ----------------------------------------------------------------------------------
def affines_call(**kw):
    a = dict(lm=P, ls=2, w=None, ws=1, k=4, c=68, idx=P, tmpl=P, n=counts(6, 6, 20), r=3, aff=P, ok=P)
    a.update(kw)
    return _lib.load().flm_part_affines(None, a["lm"], a["ls"], a["w"], a["ws"], a["k"], a["c"], a["idx"], a["tmpl"], a["n"],
                                        a["r"], a["aff"], a["ok"])


PART_ERRORS = [(dict(r=0), ARG, "1 <= r <= 8"), (dict(r=9, n=counts(*[2] * 9)), ARG, "1 <= r <= 8"),
               (dict(n=counts(6, 1, 20)), ARG, "part_n[1]=1"), (dict(n=counts(6, 6, 33)), ARG, "part_n[2]=33"),
               (dict(ls=1), SHAPE, "lm_stride >= 2"), (dict(w=P, ws=0), SHAPE, "w_stride >= 1"),
               (dict(k=0), SHAPE, "1 <= k <= 65535"), (dict(k=65536), SHAPE, "1 <= k <= 65535"),
               (dict(c=0), SHAPE, "1 <= c <= 1024"), (dict(c=1025), SHAPE, "1 <= c <= 1024")]


def test_part_affines_argument_errors():
    for name in ("lm", "idx", "tmpl", "n", "aff", "ok"):
        assert affines_call(**{name: None}) == ARG, name
        assert "null" in err() and "flm_part_affines" in err()
    for kw, code, word in PART_ERRORS:
        assert affines_call(**kw) == code, kw
        assert word in err() and "part_affines" in err(), (kw, err())


# ---- argument checks: flm_warp_parts_frames -----------------------------------------------------------------------------
def warp_call(**kw):
    a = dict(frames=P, stride=96 * 128 * 3, nf=2, fh=96, fw=128, fi=None, boxes=None, lm=P, ls=2, w=None, ws=1, c=68, idx=P,
             tmpl=P, n=counts(6, 6, 20), r=3, k=4, dst=P, ph=16, pw=24, samples=1, fmt=None, src=None, aff=None, ok=None)
    a.update(kw)
    by = lambda s: None if s is None else C.byref(s)
    return _lib.load().flm_warp_parts_frames(
        None, a["frames"], a["stride"], a["nf"], a["fh"], a["fw"], a["fi"], a["boxes"], a["lm"], a["ls"], a["w"], a["ws"],
        a["c"], a["idx"], a["tmpl"], a["n"], a["r"], a["k"], a["dst"], a["ph"], a["pw"], a["samples"], by(a["fmt"]),
        by(a["src"]), a["aff"], a["ok"])


def test_warp_parts_argument_errors():
    for name in ("frames", "lm", "idx", "tmpl", "n", "dst"):
        assert warp_call(**{name: None}) == ARG, name
        assert "null" in err() and "flm_warp_parts_frames" in err()
    for kw, code, word in PART_ERRORS:
        assert warp_call(**kw) == code, kw
        assert word in err() and "warp_parts_frames" in err(), (kw, err())
    f16 = alignment.AlignedFormat("nchw", "float16").struct()
    badf = alignment.AlignedFormat().struct()
    badf.layout = 7
    small = alignment.AlignedFormat().struct()
    small.struct_size = 4
    for kw, code, word in [
            (dict(samples=3), ARG, "samples=3"), (dict(fmt=badf), ARG, "unknown layout"), (dict(fmt=small), ARG, "struct_size"),
            (dict(fmt=f16, dst=C.c_void_p(0x1001)), ARG, "not aligned"), (dict(dst=C.c_void_p(0x1002)), ARG, "not aligned"),
            (dict(nf=0), SHAPE, "nframes"), (dict(fw=1), SHAPE, "fw >= 2"), (dict(stride=100), SHAPE, "frame_stride"),
            (dict(ph=0), SHAPE, "1 <= ph, pw <= 256"), (dict(pw=257), SHAPE, "1 <= ph, pw <= 256"),
            (dict(ph=257), SHAPE, "1 <= ph, pw <= 256")]:
        assert warp_call(**kw) == code, (kw, err())
        assert word in err() and "warp_parts_frames" in err(), (kw, err())
    # the frame format's checks are those of flm_warp_affine_frames_src: an NV12 ring of odd height, a pitched BGR ring
    s = _lib.FrameFormat()
    _lib.load().flm_frame_format_init(C.byref(s))
    s.pixel = _lib.FRAME_NV12
    assert warp_call(src=s, fh=95) == SHAPE and "even" in err()
    b = _lib.FrameFormat()
    _lib.load().flm_frame_format_init(C.byref(b))
    b.y_pitch = 256
    assert warp_call(src=b) == SHAPE and "dense" in err()
    b.y_pitch, b.struct_size = 0, 4
    assert warp_call(src=b) == ARG and "struct_size" in err()


# ---- argument checks: flm_face_openness ---------------------------------------------------------------------------------
def open_call(**kw):
    # lm [2,68] records of 6 doubles at 0x10000 (the last double ends at +6496), weights inside them
    a = dict(lm=C.c_void_p(0x10000), ls=6, w=C.c_void_p(0x10010), ws=6, n=2, c=68, opts=None, slot=None, n_slots=0,
             rec=C.c_void_p(0x30000), state=C.c_void_p(0x40000), reset=C.c_void_p(0x50000), dt_dev=None, dt=0.04, status=None,
             frame_id=7)
    a.update(kw)
    return _lib.load().flm_face_openness(None, a["lm"], a["ls"], a["w"], a["ws"], a["n"], a["c"],
                                         None if a["opts"] is None else C.byref(a["opts"]), a["slot"], a["n_slots"], a["rec"],
                                         a["state"], a["reset"], a["dt_dev"], a["dt"], a["status"], a["frame_id"])


def test_openness_argument_errors():
    O = _lib.OpenOpts
    nan, inf = float("nan"), float("inf")
    for name in ("lm", "rec"):
        assert open_call(**{name: None}) == ARG, name
        assert "null" in err() and "flm_face_openness" in err()
    assert open_call(reset=None) == ARG and "needs reset_dev" in err()
    small = O.make()
    small.struct_size = 16
    res = O.make()
    res.reserved = 1
    g0, g9, v0, v5 = O.make(), O.make(), O.make(), O.make()
    g0.n_measures, g9.n_measures = 0, 9
    v0.n_pairs[1], v5.n_pairs[2] = 0, 5
    for kw, word in [(dict(opts=small), "struct_size"), (dict(opts=res), "reserved"), (dict(opts=g0), "n_measures=0"),
                     (dict(opts=g9), "n_measures=9"), (dict(opts=v0), "n_pairs[1]=0"), (dict(opts=v5), "n_pairs[2]=5"),
                     (dict(opts=O.make(close_below=0.22)), "close_below < open_above"),
                     (dict(opts=O.make(close_below=0.3)), "close_below < open_above"),
                     (dict(opts=O.make(close_below=nan)), "close_below < open_above"),
                     (dict(opts=O.make(open_above=nan)), "close_below < open_above"),
                     (dict(opts=O.make(min_closed=nan)), ">= 0"), (dict(opts=O.make(min_closed=-0.01)), ">= 0"),
                     (dict(opts=O.make(max_closed=nan)), ">= 0"), (dict(opts=O.make(min_width=-1.0)), ">= 0"),
                     (dict(opts=O.make(min_width=nan)), ">= 0"), (dict(opts=O.make(max_closed=0.01)), "below min_closed"),
                     (dict(dt=0.0), "dt finite and > 0"), (dict(dt=-1.0), "dt finite and > 0"), (dict(dt=nan), "dt finite and > 0"),
                     (dict(dt=inf), "dt finite and > 0"),
                     # outputs over inputs and over each other: rec is 2*3*4*8 = 192 bytes, state 384, reset 8
                     (dict(rec=C.c_void_p(0x10000 + 6488)), "rec_dev overlaps lm_dev"),
                     (dict(state=C.c_void_p(0x10000 - 376)), "state_dev overlaps lm_dev"),
                     (dict(reset=C.c_void_p(0x10010 + 135 * 48)), "reset_dev overlaps"),
                     (dict(slot=C.c_void_p(0x60000), n_slots=4, rec=C.c_void_p(0x60004)), "rec_dev overlaps slot_dev"),
                     (dict(dt_dev=C.c_void_p(0x60000), state=C.c_void_p(0x60008)), "state_dev overlaps dt_dev"),
                     (dict(status=C.c_void_p(0x60000), reset=C.c_void_p(0x60004)), "reset_dev overlaps status_rows_dev"),
                     (dict(state=C.c_void_p(0x30000 + 184)), "rec_dev and state_dev overlap"),
                     (dict(reset=C.c_void_p(0x40000 + 380)), "state_dev and reset_dev overlap"),
                     # with slot the outputs have n_slots rows: rec of 100 slots is 9600 bytes
                     (dict(slot=C.c_void_p(0x60000), n_slots=100, state=C.c_void_p(0x30000 + 9592)), "rec_dev and state_dev")]:
        assert open_call(**kw) == ARG, (kw, err())
        assert word in err() and "flm_face_openness" in err(), (kw, err())
    # a dt that is not used is not checked: with dt_dev, and without state
    assert open_call(dt=0.0, n=0, dt_dev=C.c_void_p(0x60000)) == SHAPE
    assert open_call(dt=0.0, n=0, state=None, reset=None) == SHAPE
    for kw, word in [(dict(n=0), "1 <= n <= 65535"), (dict(n=65536), "1 <= n <= 65535"), (dict(c=0), "1 <= c <= 1024"),
                     (dict(c=1025), "1 <= c <= 1024"), (dict(ls=1), "lm_stride >= 2"), (dict(ws=0), "w_stride >= 1"),
                     (dict(slot=P, n_slots=0), "1 <= n_slots <= 65535"), (dict(slot=P, n_slots=65536), "1 <= n_slots <= 65535")]:
        assert open_call(**kw) == SHAPE, kw
        assert word in err(), (kw, err())


# ---- the restatement ----------------------------------------------------------------------------------------------------
def test_ref_fit_is_the_weighted_similarity_of_the_gathered_points():
    tm = alignment.canonical_template(68, 96, 128)
    lm, w = ref.face_landmarks(7, 96, 128, 3, tm)
    dp = alignment.FaceParts.default(68, (17, 23))
    parts = [dp.part(r) for r in range(len(dp))] + [(i[:-1], t[:-1]) for i, t in ref.custom_parts(17, 23)]
    oks = set()
    for weights in (None, w):
        aff, ok = ref.part_affines(lm, weights, parts)
        for r, (idx, t) in enumerate(parts):
            want = stats_ref.weighted_similarity_ref(lm[:, idx], np.asarray(t, np.float64),
                                                     None if weights is None else weights[:, idx])
            assert (aff[:, r].view(np.uint32) == want.view(np.uint32)).all(), r
            ident = (aff[:, r] == np.array([[1, 0, 0], [0, 1, 0]], np.float32)).all(axis=(1, 2))
            assert (ident[ok[:, r] == 0]).all()
        oks |= set(ok.ravel().tolist())
    assert oks == {0, 1}
    # an index outside the face does not take part: the fit of the others
    idx, t = ref.custom_parts(17, 23)[1]
    a, _ = ref.part_fit(lm[0], w[0], idx, t)
    b, _ = ref.part_fit(lm[0], w[0], idx[:-1], t[:-1])
    assert (a.view(np.uint32) == b.view(np.uint32)).all()


def test_ref_openness_meaning_and_hand_count():
    # six eye points: the eye aspect ratio (|p2-p6| + |p3-p5|) / (2 |p1-p4|)
    lm = np.full((68, 2), -1.0)
    lm[36:42] = [[10, 20], [14, 17], [20, 17], [26, 20], [20, 23], [14, 23]]
    rec = ref.open_record(lm, None, ref.DEFAULT_MEASURES[0], 4.0)
    assert rec[2] == 1.0 and rec[1] == 16.0 and rec[3] == 12.0 and rec[0] == (12.0 / 2.0) / 16.0
    assert (ref.open_record(lm, None, ref.DEFAULT_MEASURES[1], 4.0) == [-1.0, -1.0, 0.0, -1.0]).all()
    assert (ref.open_record(lm, None, ref.DEFAULT_MEASURES[0], 16.5) == [-1.0, 16.0, 0.0, 12.0]).all()
    # the scripted closures give the hand-counted events
    o, not_ok, resets, events = ref.eye_script()
    th = dict(ref.DEFAULT_TH, min_closed=0.05, max_closed=0.2)
    n = o.shape[1]
    state = np.tile(np.array(ref.STATE_EMPTY), (n, 3, 1))
    reset = np.zeros(n, np.int32)
    rec = np.zeros((n, 3, 4))
    for t in range(o.shape[0]):
        for tt, s in resets:
            if tt == t:
                reset[s] = 1
        ref.openness(ref.eye_landmarks(o[t], {s for tt, s in not_ok if tt == t}), None, ref.DEFAULT_MEASURES, 4.0, th,
                     rec=rec, state=state, reset=reset, dt=0.04, frame_id=100 + t)
        assert not reset.any()
    for g in range(3):
        assert state[:, g, 2].tolist() == [float(v) for v in events]
    assert state[0, 0, 6] == 106.0 and state[3, 0, 6] == 106.0 and state[1, 0, 6] == -1.0
    assert abs(state[0, 0, 3] - 0.12) < 1e-12 and abs(state[2, 0, 3] - 0.28) < 1e-12 and abs(state[4, 0, 3] - 0.04) < 1e-12
