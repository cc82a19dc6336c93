"""GPU parity of the tracking calls: flm_track_seed, flm_landmarks_from_crop and flm_track_step against tests/track_ref.py
(the header's arithmetic in numpy float64), bit for bit on every output; the fused step against the separate calls it
replaces; the seeded crop against flm_crop_resize; prediction.FaceTracker against the same sequence made by hand.
Every comparison of the tracking arithmetic is exact: each operation is one IEEE float64 operation on both sides.
"""
import numpy as np
import pytest
import torch

import nv12_ref
import track_ref

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
IN, GRID, FH, FW = 64, 72, 270, 480
SC = IN / GRID
KS, CS = (1, 3, 65), (1, 5, 68, 130)      # C = 130: the thread loop wraps (two full turns and a tail of 2)
LIMITS = dict(min_points=3, min_score=0.3, min_side=20.0, max_side=200.0)
# kinds of face, by what its matrix, its landmarks or its box exercise
IDENT, ROT90, MIRROR, DET0, NANM, NONE_OK, ONE_OK, TWO_OK, NEGATIVE, DEADBOX, PLAIN, FAR, TINY = range(13)


@pytest.fixture(scope="module")
def mods():
    import flm_amd  # noqa: F401
    from flm_amd import _lib, alignment, prediction
    _lib.load()
    return _lib, alignment, prediction


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def bits_equal(got, exp):
    """Bit equality of a CUDA tensor and a numpy array of the same type (NaNs and signed zeros compare by their bits)."""
    got = got.cpu().numpy()
    assert got.dtype == exp.dtype and got.shape == exp.shape, (got.dtype, exp.dtype, got.shape, exp.shape)
    u = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    return np.array_equal(np.ascontiguousarray(got).view(u), np.ascontiguousarray(exp).view(u))


def similarity(scale, deg, tx, ty):
    th = np.deg2rad(deg)
    a, b = scale * np.cos(th), scale * np.sin(th)
    return np.array([[a, -b, tx], [b, a, ty]], f32)


def make_case(k, c, seed):
    """K faces of the kinds above (all thirteen when K = 65), C landmarks on the output grid with their weights, the crop
    matrices and boxes, and two templates."""
    from flm_amd import alignment
    rng = np.random.default_rng(seed)
    kinds = {1: [PLAIN], 3: [PLAIN, ROT90, DEADBOX]}.get(k) or [i % 13 for i in range(k)]
    tc = alignment.canonical_template(c, IN, IN)
    ta = alignment.canonical_template(c, 112, 112)
    m = np.zeros((k, 2, 3), f32)
    boxes = np.zeros((k, 4), np.int32)
    lm = np.zeros((k, c, 2), f64)
    w = rng.uniform(0.05, 1.0, (k, c))
    ctr = (IN - 1) / 2.0
    for f, kind in enumerate(kinds):
        s, deg = rng.uniform(0.4, 2.5), rng.uniform(-45, 45)
        cx, cy = rng.uniform(120, 360), rng.uniform(80, 190)       # the frame point at the crop's centre
        if kind == NEGATIVE:
            s, cx, cy = 0.5, 5.0, 5.0                              # the crop hangs over the frame's top-left corner
        elif kind == FAR:
            cx = FW + 200.0                                        # the face has left the frame to the right
        elif kind == TINY:
            s = 40.0                                               # the crop covers 1.6 frame px
        m[f] = similarity(s, deg, 0, 0)
        m[f, :, 2] = ctr - m[f, :, :2].astype(f64) @ np.array([cx, cy])
        boxes[f] = [int(cx) - 40, int(cy) - 40, int(cx) + 40, int(cy) + 40]
        if kind == FAR:
            boxes[f] = [FW - 30, 60, FW + 50, 140]                 # (its last box still touched the frame)
        lm[f] = rng.uniform(0, GRID - 1, (c, 2))
        if kind == IDENT:
            m[f] = [[1, 0, 0], [0, 1, 0]]
        elif kind == ROT90:
            m[f] = [[0, -1, 250], [1, 0, -100]]
        elif kind == MIRROR:
            m[f] = [[-1.25, 0, 300], [0, 1.25, -60]]
        elif kind == DET0:
            m[f] = [[1, 2, 3], [2, 4, 5]]
        elif kind == NANM:
            m[f, rng.integers(0, 2), rng.integers(0, 3)] = np.nan
        elif kind in (NONE_OK, ONE_OK, TWO_OK):
            keep = rng.permutation(c)[:kind - NONE_OK]
            rej = np.setdiff1d(np.arange(c), keep)
            lm[f, rej, rng.integers(0, 2, len(rej))] = -1.0      # one negative coordinate rejects the point
        elif kind == NEGATIVE:
            lm[f, 0] = track_ref.apply(m[f], np.array([[30.0, 30.0]]))[0] / SC        # inside the frame
            lm[f, 1 % c] = track_ref.apply(m[f], np.array([[-10.0, -10.0]]))[0] / SC  # in the crop, outside the frame
            lm[f, 0] = track_ref.apply(m[f], np.array([[30.0, 30.0]]))[0] / SC        # (C = 1: the point inside stays)
        elif kind == DEADBOX:
            boxes[f] = [[FW + 5, 10, FW + 85, 90], [0, 0, 0, 0], [-90, -90, -10, -10]][f % 3]
        if kind in (PLAIN, FAR, TINY, IDENT, ROT90, MIRROR):
            # landmarks a network could have decoded: the crop template under a further small similarity, plus noise
            q = similarity(rng.uniform(0.8, 1.25), rng.uniform(-15, 15), rng.uniform(-4, 4), rng.uniform(-4, 4))
            lm[f] = (track_ref.apply(q, tc) + rng.normal(0, 0.3, (c, 2))) / SC
            lm[f] = np.where(lm[f] < 0, 0.0, lm[f])
        if f % 5 == 0:
            w[f] *= 0.3                                            # a face of low scores
        # weights: a zero, a NaN, a negative one (all three leave their point out)
        if c >= 5:
            w[f, rng.permutation(c)[:3]] = [0.0, np.nan, -0.5]
    if c == 1:
        w[:, 0] = np.where(np.arange(k) % 4 == 0, np.nan, w[:, 0])
    return dict(k=k, c=c, kinds=kinds, lm=lm, w=w, m=m, boxes=boxes, tc=tc, ta=ta)


def raw_step(L, case, stride, weighted, align=True, limits=None, alias=False):
    """flm_track_step through ctypes on fresh buffers filled with junk -> five tensors (m_align None without `align`)."""
    import ctypes as C
    k, c = case["k"], case["c"]
    rng = np.random.default_rng(5)
    rec = rng.uniform(-3, 99, (k, c, stride))                    # junk in the columns nobody may read
    rec[..., :2] = case["lm"]
    if stride > 2:
        rec[..., 2] = case["w"]
    rec_d = dev(rec)
    w_d, ws = None, 1
    if weighted:
        w_d, ws = (rec_d.view(-1)[2:], stride) if stride > 2 else (dev(case["w"]), 1)
    m_d, b_d, tc_d, ta_d = dev(case["m"]), dev(case["boxes"]), dev(case["tc"]), dev(case["ta"])
    lmf = torch.full((k, c, 2), 777.0, dtype=torch.float64, device="cuda")
    ma = torch.full((k, 2, 3), 777.0, dtype=torch.float32, device="cuda") if align else None
    mn = m_d if alias else torch.full((k, 2, 3), 777.0, dtype=torch.float32, device="cuda")
    bn = b_d if alias else torch.full((k, 4), 777, dtype=torch.int32, device="cuda")
    st = torch.full((k,), 777, dtype=torch.int32, device="cuda")
    opts = L.TrackOpts.make(**(limits or {}))
    L.check(L.load().flm_track_step(L.stream_ptr(), L.ptr(rec_d), stride, None if w_d is None else L.ptr(w_d), ws, L.ptr(m_d),
                                    L.ptr(b_d), k, c, SC, SC, IN, IN, FH, FW, L.ptr(tc_d),
                                    L.ptr(ta_d) if align else None, C.byref(opts), L.ptr(lmf),
                                    None if ma is None else L.ptr(ma), L.ptr(mn), L.ptr(bn), L.ptr(st)), "flm_track_step")
    return dict(lm_frame=lmf, m_align=ma, m_next=mn, boxes_next=bn, status=st)


def same(got, exp):
    return all(bits_equal(got[n], exp[n]) for n in ("lm_frame", "m_align", "m_next", "boxes_next", "status")
               if exp[n] is not None and got[n] is not None)


_REF = {}


def reference(case, weighted, limits):
    key = (case["k"], case["c"], weighted, limits is not None)
    if key not in _REF:
        _REF[key] = track_ref.step(case["lm"], case["w"] if weighted else None, case["m"], case["boxes"], SC, SC, IN, IN, FH,
                                   FW, case["tc"], case["ta"], **(limits or {}))
    return _REF[key]


@pytest.fixture(scope="module")
def cases():
    return {(k, c): make_case(k, c, 100 * k + c) for k in KS for c in CS}


def test_the_cases_hold_what_they_promise(cases):
    """A condition on the inputs: the 65-face cases reach every status bit, every rejection, and tracked faces."""
    for c in CS:
        case = cases[(65, c)]
        assert set(case["kinds"]) == set(range(13))
        ref = track_ref.step(case["lm"], case["w"], case["m"], case["boxes"], SC, SC, IN, IN, FH, FW, case["tc"], case["ta"],
                             **LIMITS)
        seen = int(np.bitwise_or.reduce(ref["status"]))
        want = 31 if c >= 5 else 7                # (C = 1 never fits: the identity is neither too small nor outside)
        assert seen & want == want, (c, seen)
        plain = track_ref.step(case["lm"], None, case["m"], case["boxes"], SC, SC, IN, IN, FH, FW, case["tc"], case["ta"])
        kinds = np.array(case["kinds"])
        if c >= 5:
            assert (plain["status"][kinds == PLAIN] == 0).all() and (plain["boxes_next"][kinds == PLAIN, 2] > 0).all()
            neg = plain["lm_frame"][kinds == NEGATIVE]
            assert (neg[:, 0] >= 0).all() and (neg[:, 1] == -1).all()
            assert (case["lm"][kinds == NEGATIVE][:, 1] >= 0).all()      # (a point the decode had kept)
            assert (plain["status"][kinds == FAR] == track_ref.OUTSIDE).all()
        for kind in (DET0, NANM, NONE_OK, DEADBOX):
            assert (plain["lm_frame"][kinds == kind] == -1).all(), kind
        assert (plain["status"][kinds == DEADBOX] & track_ref.DEAD).all()
        assert ((plain["lm_frame"][kinds == ONE_OK, :, 0] >= 0).sum(1) == 1).all()
        assert ((plain["lm_frame"][kinds == TWO_OK, :, 0] >= 0).sum(1) == min(2, c)).all()


@pytest.mark.parametrize("c", CS)
@pytest.mark.parametrize("k", KS)
def test_seed_and_back_projection_match_the_reference(mods, cases, k, c):
    L, A, P = mods
    case = cases[(k, c)]
    rng = np.random.default_rng(k + c)
    boxes = np.concatenate([case["boxes"], rng.integers(-50, 500, (k, 4)).astype(np.int32)])   # (many of them inverted)
    m, st = A.track_seed_device(dev(boxes), (IN, 96), (FH, FW))
    em, es = track_ref.seed(boxes, IN, 96, FH, FW)
    assert bits_equal(m, em) and bits_equal(st, es)
    exp = track_ref.landmarks_from_crop(case["lm"], case["m"], SC, SC)
    got = A.landmarks_from_crop_device(dev(case["lm"]), dev(case["m"]), (GRID, GRID), (IN, IN))
    assert bits_equal(got, exp)
    rec = rng.uniform(-3, 99, (k, c, 6))
    rec[..., :2] = case["lm"]
    got6 = A.landmarks_from_crop_device(dev(rec)[..., :2], dev(case["m"]), (GRID, GRID), (IN, IN))   # read at stride 6
    assert bits_equal(got6, exp)
    # anisotropic scales
    exp = track_ref.landmarks_from_crop(case["lm"], case["m"], 96 / 104, SC)
    assert bits_equal(A.landmarks_from_crop_device(dev(case["lm"]), dev(case["m"]), (GRID, 104), (IN, 96)), exp)


@pytest.mark.parametrize("c", CS)
@pytest.mark.parametrize("k", KS)
def test_step_matches_the_reference(mods, cases, k, c):
    L, A, P = mods
    case = cases[(k, c)]
    for weighted in (False, True):
        for limits in (None, LIMITS):
            exp = reference(case, weighted, limits)
            for stride in (2, 6):
                got = raw_step(L, case, stride, weighted, True, limits)
                for name in ("lm_frame", "m_align", "m_next", "boxes_next", "status"):
                    assert bits_equal(got[name], exp[name]), (name, weighted, limits, stride)
                # without the aligned pair the other four outputs do not change
                assert same(raw_step(L, case, stride, weighted, False, limits), exp)
            # the crop's own matrices and boxes as the destination
            assert same(raw_step(L, case, 6, weighted, True, limits, alias=True), exp)


@pytest.mark.parametrize("c", CS)
@pytest.mark.parametrize("k", KS)
def test_step_is_the_composition_of_the_separate_calls(mods, cases, k, c):
    L, A, P = mods
    case = cases[(k, c)]
    lm, m, w = dev(case["lm"]), dev(case["m"]), dev(case["w"])
    tc, ta = dev(case["tc"]), dev(case["ta"])
    dead = dev(np.array([track_ref.box_empty(b, FH, FW) for b in case["boxes"]]))
    for wd in (None, w):
        lmf, ma, mn, bn, st = A.track_step_device(lm, m, dev(case["boxes"]), (GRID, GRID), (IN, IN), (FH, FW), tc, ta, weights=wd)
        sep = A.landmarks_from_crop_device(lm, m, (GRID, GRID), (IN, IN))
        sep[dead] = -1.0
        assert torch.equal(lmf, sep)
        ones = torch.ones_like(w) if wd is None else wd
        assert torch.equal(ma.view(torch.int32), A.similarity_device(sep, ta, weights=ones).view(torch.int32))
        fit = A.similarity_device(sep, tc, weights=ones)
        ok = st == 0
        assert torch.equal(mn[ok].view(torch.int32), fit[ok].view(torch.int32))
        eye = torch.tensor([[1, 0, 0], [0, 1, 0]], dtype=torch.float32, device="cuda")
        assert (mn[~ok] == eye).all() and (bn[~ok] == 0).all()


def test_seeded_crop_is_the_crop_resize_of_the_box(mods):
    """For a box inside the frame and no smaller than the network input every tap of the warp lies inside the box, where
    the float bilinear of the warp and the 11-bit fixed-point bilinear of flm_crop_resize weigh the same four pixels:
    they differ by at most one in value (one rounding), on every pixel.  A box SMALLER than the input is enlarged, and
    then the outermost input pixels sample half a source pixel beyond the box: flm_crop_resize replicates the box's
    edge there, the warp reads the frame's real pixels -- those rims are compared on the whole-frame box only, where
    both clamp at the frame's edge."""
    L, A, P = mods
    rng = np.random.default_rng(9)
    fh, fw, n = 64, 96, 32
    frame = rng.integers(0, 256, (1, fh, fw, 3), dtype=np.uint8)
    frame[0] = (frame[0].astype(f64) * 0.25 + np.linspace(0, 190, fw)[None, :, None]).astype(np.uint8)  # texture on a ramp
    boxes = np.array([[10, 5, 50, 45], [33, 20, 65, 52], [0, 0, 64, 64], [41, 7, 78, 44], [32, 0, 96, 64 - 15]], np.int32)
    boxes[4] = [47, 3, 96, 52]                                   # 49 px, touching the frame's right edge
    fd, bd = dev(frame), dev(boxes)
    m, st = A.track_seed_device(bd, (n, n), (fh, fw))
    assert not st.any()
    u8 = A.AlignedFormat("nhwc", "uint8")
    idx = torch.zeros(len(boxes), dtype=torch.int32, device="cuda")
    got = A.warp_frames_device(fd, m, n, n, frame_index_dev=idx, boxes_dev=bd, fmt=u8)
    exp = P.crop_faces_device(fd[0], None, n, n, boxes_dev=bd)
    d = (got.to(torch.int16) - exp.to(torch.int16)).abs()
    print("seeded crops: %d of %d values differ from flm_crop_resize (by at most %d)" % (int((d > 0).sum()), d.numel(), int(d.max())))
    assert int(d.max()) <= 1
    assert exp.float().std() > 20
    # the whole frame, enlarged: both sides clamp at the frame's edge
    whole = dev(np.array([[0, 0, fw, fh]], np.int32))
    m, st = A.track_seed_device(whole, (80, 120), (fh, fw))
    got = A.warp_frames_device(fd, m, 80, 120, boxes_dev=whole, fmt=u8)
    exp = P.crop_faces_device(fd[0], None, 80, 120, boxes_dev=whole)
    d = (got.to(torch.int16) - exp.to(torch.int16)).abs()
    print("whole frame x1.25: %d of %d values differ (by at most %d)" % (int((d > 0).sum()), d.numel(), int(d.max())))
    assert int(d.max()) <= 1


# ---- FaceTracker against the sequence made by hand --------------------------------------------------------------------
RH, RW = 64, 96
FACES = [(20, 8, 60, 50), (40, 2, 90, 60), (-6, 20, 30, 58)]       # detector boxes for slots 0, 2, 3; slot 1 stays empty
SLOTS = [0, 2, 3]


@pytest.fixture(scope="module")
def rings(mods):
    L, A, P = mods
    rng = np.random.default_rng(31)
    bgr = rng.integers(0, 256, (2, RH, RW, 3), dtype=np.uint8)
    nv = np.stack([nv12_ref.pack_slot(*nv12_ref.bgr_to_nv12(bgr[f], "bt709"), RW, RH, RH * 3 // 2) for f in range(2)])
    return {"bgr": (dev(bgr), None), "nv12": (dev(nv), A.FrameFormat.nv12(RH, RW, matrix="bt709"))}


@pytest.fixture(scope="module", params=["f32", "bf16"])
def model(request):
    from flm_amd.networks import LANDMARKS_MODELS
    from flm_amd.weights import synth_fcn8_weights
    m = LANDMARKS_MODELS["fcn_8"](68, input_height=64, input_width=64, dtype=request.param)
    m.load_weights(synth_fcn8_weights(68, seed=2))
    return m


def by_hand(mods, model, ring, ff, weights, aligned_format, frames):
    """FaceTracker's documented sequence through the public pieces, nothing aliased, for the frames `frames`."""
    L, A, P = mods
    cap = 4
    boxes = torch.zeros((cap, 4), dtype=torch.int32, device="cuda")
    m = torch.eye(2, 3, dtype=torch.float32, device="cuda").repeat(cap, 1, 1).contiguous()
    sq = dev(np.asarray(P.face_boxes([list(b) for b in FACES]), np.int32))
    sm, _ = A.track_seed_device(sq, (64, 64), (RH, RW))
    for i, s in enumerate(SLOTS):
        boxes[s], m[s] = sq[i], sm[i]
    tc, ta = dev(A.canonical_template(68, 64, 64)), dev(A.canonical_template(68, 112, 112))
    out = []
    for fi in frames:
        idx = torch.full((cap,), fi, dtype=torch.int32, device="cuda")
        crops = A.warp_frames_device(ring, m, 64, 64, frame_index_dev=idx, boxes_dev=boxes, fmt=A.AlignedFormat("nhwc", "uint8"), src=ff)
        if weights is None:
            lm, wd = model.forward_device(crops, "landmarks", n_points=4, thresh=0.0), None
        else:
            rec = model.forward_device(crops, "landmark_stats", n_points=4, thresh=0.0)
            lm, wd = rec[..., :2].contiguous(), rec[..., 2].contiguous()
        lmf, ma, mn, bn, st = A.track_step_device(lm, m, boxes, (72, 72), (64, 64), (RH, RW), tc, ta, weights=wd)
        aligned = A.warp_frames_device(ring, ma, 112, 112, frame_index_dev=idx, boxes_dev=boxes, fmt=aligned_format, src=ff)
        out.append((aligned, ma, lmf, st, crops))
        m, boxes = mn, bn
    return out


@pytest.mark.parametrize("source", ["bgr", "nv12"])
def test_face_tracker_is_the_sequence_made_by_hand(mods, rings, model, source):
    L, A, P = mods
    ring, ff = rings[source]
    frames = [1, 0]
    eye = torch.tensor([[1, 0, 0], [0, 1, 0]], dtype=torch.float32, device="cuda")
    plain = None
    for weights, fmt in ((None, None), ("score", None), (None, A.AlignedFormat.matcher())):
        tr = P.FaceTracker(model, (RH, RW), 4, weights=weights, aligned_format=fmt, frame_format=ff)
        tr.seed(SLOTS, FACES)
        assert tr.lost() == [1]
        exp = by_hand(mods, model, ring, ff, weights, fmt, frames)
        got = []
        for t, fi in enumerate(frames):
            aligned, m, lm, st = tr.step(ring, fi)
            got.append((aligned.clone(), m.clone(), lm.clone(), st.clone()))
            for a, b in zip(got[-1], exp[t][:4]):
                assert a.dtype == b.dtype and a.is_cuda and a.shape == b.shape
                assert torch.equal(a, b), (t, weights, fmt)
            # the slot nobody seeded: no face, no pixels
            assert int(st[1]) & L.TRACK_DEAD and torch.equal(m[1], eye) and (lm[1] == -1).all()
            # (the warp's zero fill goes through the format like any value: 0 * scale + bias = -1 for the matcher)
            assert (aligned[1] == (0.0 if fmt is None else -1.0)).all()
            assert not exp[t][4][1].any() and exp[t][4][0].any()
        print(source, weights, "status per frame:", [g[3].tolist() for g in got])
        assert got[0][0][0].any()                                  # a seeded slot has an aligned face in its first frame
        assert tr.lost() == [i for i in range(4) if int(got[-1][3][i]) != 0]
        if (weights, fmt) == (None, None):
            plain = got
        elif weights is None:                                      # the matcher's format changes `aligned` alone
            for t in range(2):
                assert got[t][0].dtype == torch.float16 and tuple(got[t][0].shape) == (4, 3, 112, 112)
                for a, b in zip(got[t][1:], plain[t][1:]):
                    assert torch.equal(a, b)
    with pytest.raises(ValueError):                                # a ring slot that is not there
        tr.step(ring, 2)
