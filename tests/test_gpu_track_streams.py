"""GPU parity of flm_track_associate_streams against tests/track_streams_ref.py (a loop over the streams around the
single association's reference, the i*K offset on det_slot, the skip rule): through ctypes, on buffers pre-filled with
junk, bit for bit on all eight tensors -- m_crop, boxes, status, misses, state, det_slot, slot_det, counts.  Every
comparison is exact.  Then the call against flm_track_associate on the device at S = 1, the skips, the isolation of two
identical streams, the Python wrapper, and FaceTracker(streams=2) end to end against the same sequence made by hand from
the single-stream pieces.

torch.cuda.set_sync_debug_mode("error") is honoured by this torch build on ROCm (a .item() inside it raises, which the
tests check first), so the wrapper, the step and the update with device inputs run inside it.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import nv12_ref
import track_assoc_ref as ref
import track_streams_ref as sref

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
FH, FW, IH, IW = 270, 480, 64, 96
NAMES = sref.NAMES
OPTS = dict(max_misses=2, refresh_iou=0.6)
OUTCOMES = ("matched", "born", "refreshed", "duplicates", "unconfirmed", "void")


@pytest.fixture(scope="module")
def mods():
    import flm_amd  # noqa: F401
    from flm_amd import _lib, alignment, prediction
    _lib.load()
    return _lib, alignment, prediction


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def bits_equal(got, exp):
    got = got.cpu().numpy()
    assert got.dtype == exp.dtype and got.shape == exp.shape, (got.dtype, exp.dtype, got.shape, exp.shape)
    u = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    return np.array_equal(np.ascontiguousarray(got).view(u), np.ascontiguousarray(exp).view(u))


class sync_error:
    """Inside: a transfer or a synchronisation raises (checked on entry when `probe` is given)."""

    def __init__(self, probe=None):
        self.probe = probe

    def __enter__(self):
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        if self.probe is not None:
            try:
                with pytest.raises(RuntimeError):      # (the mode is live in this build: a download raises)
                    self.probe.item()
            except BaseException:
                torch.cuda.set_sync_debug_mode("default")
                raise

    def __exit__(self, *exc):
        torch.cuda.set_sync_debug_mode("default")


# ---- scenes ------------------------------------------------------------------------------------------------------------
def junk_state(n, c, seed):
    """Track state as a caller might hold it: arbitrary matrices, status words and filter state (NaNs among them)."""
    rng = np.random.default_rng(seed)
    m = rng.normal(0, 3, (n, 2, 3)).astype(f32)
    status = rng.choice([0, 0, 0, 1, 3, 8, 16, 32, 64, 0x7fffff00], n).astype(np.int32)
    misses = rng.integers(0, 3, n).astype(np.int32)
    state = None
    if c:
        state = rng.normal(50, 40, (n, c, 6))
        state[rng.random((n, c, 6)) < 0.05] = np.nan
    return m, status, misses, state


def clustered(k, d, seed, fh=FH, fw=FW, lo=8, hi=120):
    """One stream's K track boxes and D detector boxes of lo..hi px: roughly a third of each has a partner on the other
    side (the same face, jittered), a few tracks sit in pairs on one face, a fifth of the slots holds no face, some boxes
    hang over the frame's edge, a tenth of the detections (one at least, from two rows on) is void."""
    rng = np.random.default_rng(seed)

    def box():
        w, h = rng.integers(lo, hi + 1, 2)
        x0, y0 = rng.integers(-w // 3, fw - 2 * w // 3), rng.integers(-h // 3, fh - 2 * h // 3)
        return np.array([x0, y0, x0 + w, y0 + h])

    def near(b, amp):
        j = rng.integers(-amp, amp + 1, 4)
        return b + np.maximum(1, (b[2] - b[0]) // 10) * j // 4

    tracks = np.stack([box() for _ in range(k)])
    dets = np.stack([box() for _ in range(d)])
    n = max(1, min(k, d) // 3) if min(k, d) > 1 else 1
    ts, js = rng.permutation(k)[:n], rng.permutation(d)[:n]
    for t, j in zip(ts, js):
        dets[j] = near(tracks[t], 3)
        dets[j][[1, 3]] -= int(abs((dets[j][3] - dets[j][1]) * 0.1))        # (the box maths moves it back down)
    for t in rng.permutation(k)[:k // 8]:                                    # a second track on a face
        tracks[t] = near(tracks[(t + 1) % k], 1)
    for t in rng.permutation(k)[:(k + 4) // 5]:                              # slots without a face
        tracks[t] = [[0, 0, 0, 0], [fw + 3, 5, fw + 40, 60], [50, 50, 40, 90], [-70, -70, -2, -2]][t % 4]
    for j in rng.permutation(d)[:max(d // 10, 1 if d > 1 else 0)]:           # void detections
        dets[j] = [[2 ** 28 + 1, 0, 9, 9], [60, 60, 50, 50], [fw + 9, 9, fw + 90, 90], [-2 ** 31, 0, 5, 5]][j % 4]
    return tracks.astype(np.int32), dets.astype(np.int32)


def streams_scene(s, k, d, c, seed=0):
    """S streams, each with its own seed and its own count -> (det [S,D,4], n_det [S], boxes [S*K,4], m, status, misses,
    state).  The counts lie in [3D/4, D] and are never negative here (the skips have a test of their own)."""
    rng = np.random.default_rng(7000 + 100 * s + 10 * k + d + seed)
    tr, de = zip(*[clustered(k, d, 1000 * k + d + 31 * i + seed) for i in range(s)])
    n_det = rng.integers(d - d // 4, d + 1, s).astype(np.int32)
    m, status, misses, state = junk_state(s * k, c, k + d + s + seed)
    return np.stack(de), n_det, np.concatenate(tr), m, status, misses, state


def gpu_streams(L, det, n_det, k, boxes, m, status, misses, state, frame=(FH, FW), **opts):
    """flm_track_associate_streams through ctypes on fresh device buffers; the outputs are pre-filled with junk."""
    det = np.asarray(det, np.int32)
    s, d = det.shape[:2]
    n = s * k
    t = dict(m_crop=dev(np.asarray(m, f32)), boxes=dev(np.asarray(boxes, np.int32)), status=dev(np.asarray(status, np.int32)),
             misses=dev(np.asarray(misses, np.int32)), state=None if state is None else dev(np.asarray(state, f64)),
             det_slot=torch.full((s, d), 777, dtype=torch.int32, device="cuda"),
             slot_det=torch.full((n,), 777, dtype=torch.int32, device="cuda"),
             counts=torch.full((s, 8), 777, dtype=torch.int32, device="cuda"))
    assert t["boxes"].shape == (n, 4) and t["m_crop"].shape == (n, 2, 3) and t["status"].shape == (n,) and t["misses"].shape == (n,)
    assert state is None or t["state"].shape[0] == n
    det_d = dev(det)
    n_d = None if n_det is None else dev(np.asarray(n_det, np.int32))
    assert n_d is None or n_d.shape == (s,)
    c = 1 if state is None else int(np.asarray(state).shape[1])
    o = L.TrackAssocOpts.make(**opts)
    L.check(L.load().flm_track_associate_streams(
        L.stream_ptr(), L.ptr(det_d), None if n_d is None else L.ptr(n_d), s, d, k, c, IH, IW, frame[0], frame[1], C.byref(o),
        L.ptr(t["m_crop"]), L.ptr(t["boxes"]), L.ptr(t["status"]), L.ptr(t["misses"]),
        None if state is None else L.ptr(t["state"]), L.ptr(t["det_slot"]), L.ptr(t["slot_det"]), L.ptr(t["counts"])),
        "flm_track_associate_streams")
    assert torch.equal(det_d.cpu(), torch.from_numpy(det))          # (the detections are read only)
    return t


def check(L, det, n_det, k, boxes, m, status, misses, state, **opts):
    """GPU against reference on all eight tensors -> the reference's result."""
    exp = sref.associate_streams(det, n_det, m, boxes, status, misses, state, k, IH, IW, FH, FW, **opts)
    got = gpu_streams(L, det, n_det, k, boxes, m, status, misses, state, **opts)
    for name in NAMES:
        if exp[name] is None:
            assert got[name] is None
            continue
        assert bits_equal(got[name], exp[name]), (name, opts, got[name].cpu().numpy().reshape(-1).tolist()[:40],
                                                  exp[name].reshape(-1).tolist()[:40])
    return exp


# (S, K, D, C): the one-wave form from one item to full, with more streams than a CU holds; CAP 256 with K, then D,
# beyond a wave and the other side inside one; CAP 1024 just over 256 and full.  C: the state absent, 1, 68.
SIZES = [(1, 1, 1, 0), (2, 3, 5, 68), (5, 16, 16, 1), (70, 64, 64, 1), (3, 65, 7, 68), (3, 7, 130, 0), (2, 300, 257, 1),
         (2, 1024, 1024, 0)]


@pytest.mark.parametrize("s,k,d,c", SIZES)
def test_random_scenes_match_the_reference(mods, s, k, d, c):
    L = mods[0]
    det, n_det, boxes, m, status, misses, state = streams_scene(s, k, d, c)
    exp = check(L, det, n_det, k, boxes, m, status, misses, state, **OPTS)
    cnt = dict(zip(ref.COUNTS, exp["counts"].sum(0).tolist()))
    print(s, k, d, c, n_det.tolist()[:8], cnt)
    named = exp["det_slot"] >= 0
    lo = (np.arange(s) * k)[:, None]
    assert ((exp["det_slot"] >= lo) & (exp["det_slot"] < lo + k))[named].all()      # every named slot is the stream's own
    if s > 1 and k > 1:
        assert (exp["det_slot"][1:] >= k).any()                                     # (and the offset is in the data)
    if k >= 64:                                  # a condition on the inputs: over the streams every outcome occurs
        assert all(cnt[n] > 0 for n in OUTCOMES), cnt


@pytest.mark.parametrize("c", [0, 1, 68])
def test_state_absent_and_given(mods, c):
    L = mods[0]
    det, n_det, boxes, m, status, misses, state = streams_scene(5, 16, 16, c, seed=5)
    exp = check(L, det, n_det, 16, boxes, m, status, misses, state, refresh_iou=0.95, match_iou=0.2)
    restarted = int(exp["counts"][:, 1].sum() + exp["counts"][:, 2].sum())
    assert restarted > 0
    if c:
        reset = (exp["state"] == -1.0).all((1, 2))
        assert reset.sum() == restarted
        assert np.array_equal(exp["state"][~reset].view(np.uint64), state[~reset].view(np.uint64))


def single(L, det, n_det, boxes, m, status, misses, state, **opts):
    """flm_track_associate on the device, for one stream."""
    d, k = len(det), len(boxes)
    t = dict(m_crop=dev(m), boxes=dev(boxes), status=dev(status), misses=dev(misses), state=None if state is None else dev(state),
             det_slot=torch.full((d,), 777, dtype=torch.int32, device="cuda"),
             slot_det=torch.full((k,), 777, dtype=torch.int32, device="cuda"),
             counts=torch.full((8,), 777, dtype=torch.int32, device="cuda"))
    det_d = dev(det)
    n_d = None if n_det is None else torch.tensor([n_det], dtype=torch.int32, device="cuda")
    o = L.TrackAssocOpts.make(**opts)
    L.check(L.load().flm_track_associate(
        L.stream_ptr(), L.ptr(det_d), None if n_d is None else L.ptr(n_d), d, k, 1 if state is None else state.shape[1], IH, IW,
        FH, FW, C.byref(o), L.ptr(t["m_crop"]), L.ptr(t["boxes"]), L.ptr(t["status"]), L.ptr(t["misses"]),
        None if state is None else L.ptr(t["state"]), L.ptr(t["det_slot"]), L.ptr(t["slot_det"]), L.ptr(t["counts"])),
        "flm_track_associate")
    return t


@pytest.mark.parametrize("k,d", [(16, 16), (65, 64), (300, 257)])
def test_one_stream_is_the_single_call_on_the_device(mods, k, d):
    L = mods[0]
    det, n_det, boxes, m, status, misses, state = streams_scene(1, k, d, 3, seed=9)
    for n in (None, int(n_det[0]), 0, d):
        a = single(L, det[0], n, boxes, m, status, misses, state, **OPTS)
        b = gpu_streams(L, det, None if n is None else [n], k, boxes, m, status, misses, state, **OPTS)
        for name in NAMES:
            assert torch.equal(a[name].view(torch.int64) if name == "state" else a[name].view(torch.int32).reshape(-1),
                               b[name].view(torch.int64) if name == "state" else b[name].view(torch.int32).reshape(-1)), (name, n)
    assert int(a["counts"][0]) > 0


def test_skipped_streams_keep_their_bits(mods):
    L = mods[0]
    s, k, d = 5, 16, 16
    det, _, boxes, m, status, misses, state = streams_scene(s, k, d, 4, seed=3)
    n_det = [-1, 0, 16, -7, 3]
    assert np.isnan(state[:k]).any() and np.isnan(state[3 * k:4 * k]).any()
    exp = check(L, det, n_det, k, boxes, m, status, misses, state, dup_iou=2.0, **OPTS)
    for i in (0, 3):                             # (the reference, which the device equals: the junk is where it was)
        sl = slice(i * k, (i + 1) * k)
        for name, x in (("m_crop", m), ("boxes", boxes), ("status", status), ("misses", misses), ("state", state)):
            u = {4: np.uint32, 8: np.uint64}[x.dtype.itemsize]
            assert np.array_equal(exp[name][sl].view(u), x[sl].view(u)), (i, name)
        assert (exp["det_slot"][i] == -1).all() and (exp["slot_det"][sl] == -1).all() and not exp["counts"][i].any()
    # stream 1 ran and found nothing: every live slot counts a miss, or ends for the misses it had
    sl = slice(k, 2 * k)
    live = np.array([not ref.empty(ref.clip(b, FH, FW)) for b in boxes[sl]])
    ended = live & (misses[sl] + 1 >= 2)
    assert live.sum() > 8 and ended.any() and (live & ~ended).any()
    assert np.array_equal(exp["misses"][sl][live & ~ended], misses[sl][live & ~ended] + 1)
    assert (exp["status"][sl][ended] & ref.UNCONFIRMED).all() and exp["counts"][1].tolist() == [0, 0, 0, 0, int(ended.sum()), 0, 0, 0]
    assert exp["counts"][2][0] > 0


def test_two_identical_streams_do_not_see_each_other(mods):
    L = mods[0]
    k, d = 16, 16
    det, n_det, boxes, m, status, misses, state = streams_scene(1, k, d, 2, seed=11)
    two = lambda x: np.concatenate([x, x])
    exp = check(L, two(det), two(n_det), k, two(boxes), two(m), two(status), two(misses), two(state), **OPTS)
    for name in ("m_crop", "boxes", "status", "misses", "slot_det"):
        assert np.array_equal(exp[name][:k].view(np.uint32), exp[name][k:].view(np.uint32)), name
    assert np.array_equal(exp["state"][:k].view(np.uint64), exp["state"][k:].view(np.uint64))
    assert np.array_equal(exp["counts"][0], exp["counts"][1]) and exp["counts"][0][0] > 0
    ds0, ds1 = exp["det_slot"]
    assert np.array_equal(np.where(ds0 >= 0, ds0 + k, ds0), ds1)
    # the two streams as ONE stream of 2K slots: every live slot of the second half ends as a duplicate of the first
    one = ref.associate(two(det[0]), None, two(m), two(boxes), two(status), two(misses), None, IH, IW, FH, FW, **OPTS)
    assert one["counts"][3] > exp["counts"][:, 3].sum() + k // 2
    assert ((exp["status"][k:] & ref.DUPLICATE) != 0).sum() == ((exp["status"][:k] & ref.DUPLICATE) != 0).sum()


def test_wrapper_returns_what_the_raw_call_writes(mods):
    L, A, P = mods
    s, k, d = 5, 16, 16
    det, n_det, boxes, m, status, misses, state = streams_scene(s, k, d, 3, seed=2)
    n_det[3] = -1
    exp = sref.associate_streams(det, n_det, m, boxes, status, misses, state, k, IH, IW, FH, FW, **OPTS)
    t = [dev(x) for x in (m, boxes, status, misses, state)]
    det_d, n_d = dev(det), dev(n_det)
    assoc = A.TrackAssociation(**OPTS)
    with sync_error(probe=n_d):
        ds, sd, cnt = A.track_associate_streams_device(det_d, t[0], t[1], t[2], t[3], k, (IH, IW), (FH, FW), n_det=n_d,
                                                       state=t[4], assoc=assoc)
    for got, name in zip(t + [ds, sd, cnt], NAMES):
        assert bits_equal(got, exp[name]), name
    # the keyword tensors name where to write
    t = [dev(x) for x in (m, boxes, status, misses, state)]
    outs = [torch.full(sh, 5, dtype=torch.int32, device="cuda") for sh in ((s, d), (s * k,), (s, 8))]
    r = A.track_associate_streams_device(det_d, *t[:4], k, (IH, IW), (FH, FW), n_det=n_d, state=t[4], assoc=assoc,
                                         det_slot=outs[0], slot_det=outs[1], counts=outs[2])
    assert all(a is b for a, b in zip(r, outs)) and all(bits_equal(a, exp[n]) for a, n in zip(outs, NAMES[5:]))
    with pytest.raises(ValueError, match="1024"):
        A.track_associate_streams_device(torch.zeros((s, 1025, 4), dtype=torch.int32, device="cuda"), *t[:4], k, (IH, IW), (FH, FW))
    with pytest.raises(ValueError, match="n_det"):
        A.track_associate_streams_device(det_d, *t[:4], k, (IH, IW), (FH, FW), n_det=n_d[:-1])
    with pytest.raises(ValueError, match="m_crop"):
        A.track_associate_streams_device(det_d, *t[:4], k - 1, (IH, IW), (FH, FW))
    with pytest.raises(ValueError, match="misses"):
        A.track_associate_streams_device(det_d, t[0], t[1], t[2], t[3][:-1], k, (IH, IW), (FH, FW))
    with pytest.raises(ValueError, match="state"):
        A.track_associate_streams_device(det_d, *t[:4], k, (IH, IW), (FH, FW), state=t[4][:, :, :5])
    with pytest.raises(ValueError, match="counts"):
        A.track_associate_streams_device(det_d, *t[:4], k, (IH, IW), (FH, FW), counts=outs[2][:1])


# ---- FaceTracker(streams=2) --------------------------------------------------------------------------------------------
RH, RW, CAP, K = 64, 96, 6, 3
FACES = [(20, 8, 60, 50), (40, 2, 90, 60), (-6, 20, 30, 58), (30, 10, 80, 60)]
SEEDS = {0: ([0, 2], FACES[:2]), 1: ([1, 2], FACES[2:])}        # stream -> (its local slots, the boxes)
FRAMES = [(0, 4), (1, 5), (2, 6), (3, 7)]                       # stream 0 reads ring slots 0-3, stream 1 slots 4-7
DETS = {0: [[(22, 10, 60, 48), (70, 30, 96, 62), (0, 0, 20, 20), (-6, 22, 30, 58)],
            [(40, 4, 88, 58), (2 ** 30, 0, 5, 5), (60, 20, 96, 60)]],
        2: [[(40, 4, 88, 58), (10, 10, 50, 50), (2 ** 30, 0, 5, 5), (60, 20, 96, 60), (0, 30, 30, 64)], None]}


@pytest.fixture(scope="module")
def rings(mods):
    L, A, P = mods
    rng = np.random.default_rng(31)
    bgr = rng.integers(0, 256, (8, RH, RW, 3), dtype=np.uint8)
    nv = np.stack([nv12_ref.pack_slot(*nv12_ref.bgr_to_nv12(bgr[f], "bt709"), RW, RH, RH * 3 // 2) for f in range(8)])
    return {"bgr": (dev(bgr), None), "nv12": (dev(nv), A.FrameFormat.nv12(RH, RW, matrix="bt709"))}


@pytest.fixture(scope="module")
def model():
    from flm_amd.networks import LANDMARKS_MODELS
    from flm_amd.weights import synth_fcn8_weights
    m = LANDMARKS_MODELS["fcn_8"](68, input_height=64, input_width=64, dtype="bf16")
    m.load_weights(synth_fcn8_weights(68, seed=2))
    return m


def by_hand(mods, model, ring, ff, assoc, smooth):
    """The sequence at the batch of 6 from the single-stream pieces: a hand-made frame_index_dev, the warps, the forward,
    track_step_device, and track_associate_device once per stream on the contiguous slices.  -> the steps' (aligned,
    m_align, lm_frame, status), the updates' (det_slot [2,D], slot_det [6], counts [2,8]) and the state."""
    L, A, P = mods
    boxes = torch.zeros((CAP, 4), dtype=torch.int32, device="cuda")
    m = torch.eye(2, 3, dtype=torch.float32, device="cuda").repeat(CAP, 1, 1).contiguous()
    status = torch.full((CAP,), L.TRACK_DEAD, dtype=torch.int32, device="cuda")
    misses = torch.zeros((CAP,), dtype=torch.int32, device="cuda")
    state = torch.full((CAP, 68, 6), -1.0, dtype=torch.float64, device="cuda") if smooth else None
    for i, (slots, faces) in SEEDS.items():
        sq = dev(np.asarray(P.face_boxes([list(b) for b in faces]), np.int32))
        sm, ss = A.track_seed_device(sq, (64, 64), (RH, RW))
        for j, t in enumerate(slots):
            boxes[i * K + t], m[i * K + t], status[i * K + t] = sq[j], sm[j], ss[j]
    tc, ta = dev(A.canonical_template(68, 64, 64)), dev(A.canonical_template(68, 112, 112))
    filt = dict(filter=A.LandmarkFilter(), state=state) if smooth else {}
    steps, ups = [], {}
    for t, fi in enumerate(FRAMES):
        idx = dev(np.repeat(np.asarray(fi, np.int32), K))
        crops = A.warp_frames_device(ring, m, 64, 64, frame_index_dev=idx, boxes_dev=boxes, fmt=A.AlignedFormat("nhwc", "uint8"), src=ff)
        lm = model.forward_device(crops, "landmarks", n_points=4, thresh=0.0)
        lmf, ma, mn, bn, st = A.track_step_device(lm, m, boxes, (72, 72), (64, 64), (RH, RW), tc, ta, **filt)
        aligned = A.warp_frames_device(ring, ma, 112, 112, frame_index_dev=idx, boxes_dev=boxes, src=ff)
        steps.append((aligned, ma, lmf, st.clone()))
        m, boxes, status = mn, bn, st
        if t in DETS:
            d = max(len(x) for x in DETS[t] if x is not None)
            ds = torch.full((2, d), -1, dtype=torch.int32, device="cuda")
            sd = torch.full((CAP,), -1, dtype=torch.int32, device="cuda")
            cnt = torch.zeros((2, 8), dtype=torch.int32, device="cuda")
            for i, rows in enumerate(DETS[t]):
                if rows is None:
                    continue
                sl = slice(i * K, (i + 1) * K)
                a, b, c = A.track_associate_device(dev(np.asarray(rows, np.int32)), m[sl], boxes[sl], status[sl], misses[sl],
                                                   (64, 64), (RH, RW), state=None if state is None else state[sl], assoc=assoc)
                ds[i, :len(rows)] = torch.where(a >= 0, a + i * K, a)
                sd[sl], cnt[i] = b, c
            ups[t] = (ds, sd, cnt)
    return steps, ups, (m, boxes, status, misses, state)


def view_bits(x):
    return x.view(torch.int64) if x.dtype == torch.float64 else x.view(torch.int32) if x.dtype == torch.float32 else x


@pytest.mark.parametrize("smooth", [None, True])
@pytest.mark.parametrize("source", ["bgr", "nv12"])
def test_face_tracker_of_two_streams_is_the_sequence_made_by_hand(mods, rings, model, source, smooth):
    L, A, P = mods
    ring, ff = rings[source]
    assoc = A.TrackAssociation(max_misses=2, refresh_iou=0.5)
    exp_steps, exp_ups, exp_state = by_hand(mods, model, ring, ff, assoc, smooth)
    for how in ("host", "device"):
        tr = P.FaceTracker(model, (RH, RW), CAP, frame_format=ff, associate=assoc, smooth=smooth, streams=2)
        assert (tr.streams, tr.slots_per_stream) == (2, K)
        for i, (slots, faces) in SEEDS.items():
            tr.seed(slots, faces, stream=i)
        for t, fi in enumerate(FRAMES):
            if how == "host":
                got = [x.clone() for x in tr.step(ring, list(fi))]
            else:
                fi_d = torch.tensor(fi, dtype=torch.int32, device="cuda")
                with sync_error(probe=fi_d if t == 0 else None):
                    got = [x.clone() for x in tr.step(ring, fi_d)]
            for a, b in zip(got, exp_steps[t]):
                assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(view_bits(a), view_bits(b)), (how, t)
            if t not in DETS:
                continue
            lens = [-1 if x is None else len(x) for x in DETS[t]]
            d = max(lens)
            if how == "host":
                up = tr.update(DETS[t])
                assert up[0].shape == (2, d)
            else:                                  # the detectors' fixed buffers of 8 rows and their counts, on the device
                buf = np.full((2, 8, 4), 12345, np.int32)
                for i, rows in enumerate(DETS[t]):
                    if rows is not None:
                        buf[i, :len(rows)] = rows
                buf, n = dev(buf), dev(np.asarray(lens, np.int32))
                with sync_error():
                    up = tr.update(buf, n)
                assert up[0].shape == (2, 8) and (up[0][:, d:] == -1).all()
                up = (up[0][:, :d], up[1], up[2])
            for a, b in zip(up, exp_ups[t]):
                assert a.is_cuda and a.dtype == torch.int32 and torch.equal(a, b), (how, t, a.tolist(), b.tolist())
        for name, e in zip(("m_crop", "boxes", "status", "misses", "filter_state"), exp_state):
            g = getattr(tr, name)
            assert (g is None and e is None) or torch.equal(view_bits(g), view_bits(e)), (how, name)
        assert tr.lost() == [i for i in range(CAP) if int(exp_state[2][i]) != 0]
    print(source, smooth, "counts per update:", {t: u[2].tolist() for t, u in exp_ups.items()}, "status:", exp_state[2].tolist())
    # every stream holds a free slot and a valid detection at the first update: each confirms or starts a track there
    assert int((exp_ups[0][2][:, 0] + exp_ups[0][2][:, 1]).min()) > 0
    assert (exp_ups[0][0][1][exp_ups[0][0][1] >= 0] >= K).all()                          # stream 1's detections name its own slots
    assert not exp_ups[2][2][1].any() and (exp_ups[2][1][K:] == -1).all()               # the skipped stream
    st = exp_steps[1][3]
    assert ((st[:K] & L.TRACK_DEAD) == 0).any() and ((st[K:] & L.TRACK_DEAD) == 0).any()   # both streams held a face after it


@pytest.mark.parametrize("smooth", [None, True])
def test_one_stream_is_the_tracker_of_before(mods, rings, model, smooth):
    """A tracker made with streams=1 returns the bits of a tracker made without the argument."""
    L, A, P = mods
    ring, ff = rings["nv12"]
    out = []
    for kw in ({}, dict(streams=1)):
        tr = P.FaceTracker(model, (RH, RW), 4, frame_format=ff, smooth=smooth, best_shot=True,
                           associate=A.TrackAssociation(max_misses=2, refresh_iou=0.5), **kw)
        tr.seed([0, 2], FACES[:2])
        tr.seed([1], FACES[2:3], **({} if not kw else dict(stream=0)))
        res = []
        for t, fi in enumerate((1, 0, 5)):
            res += [x.clone() for x in tr.step(ring, fi)]
            if t < 2:
                res += [x.clone() for x in tr.update(DETS[2 * t][0])]
        res += [x.clone() for x in tr.best()] + [tr.m_crop, tr.boxes, tr.misses] + ([tr.filter_state] if smooth else [])
        out.append(res)
        with pytest.raises(ValueError, match="\\[1, 4\\]|divides"):
            P.FaceTracker(model, (RH, RW), 4, streams=3)
    assert len(out[0]) == len(out[1])
    for a, b in zip(*out):
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(view_bits(a), view_bits(b))
    assert out[0][0].any()
