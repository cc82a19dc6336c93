"""GPU parity of flm_track_associate against tests/track_assoc_ref.py (the header's arithmetic in Python integers, with
the true greedy loop): through ctypes, on buffers pre-filled with junk, bit for bit on all eight tensors -- m_crop, boxes,
status, misses, state, det_slot, slot_det, counts.  Every comparison is exact.  Then FaceTracker.update against
FaceTracker.seed, and FaceTracker end to end against the same sequence made by hand from the public pieces.

torch.cuda.set_sync_debug_mode("error") is honoured by this torch build on ROCm (a .item() inside it raises, which the
test checks first), so the update with device inputs runs inside it.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import nv12_ref
import track_assoc_ref as ref

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
FH, FW, IH, IW = 270, 480, 64, 96
NAMES = ("m_crop", "boxes", "status", "misses", "state", "det_slot", "slot_det", "counts")
PLAIN = dict(square=False, dup_iou=2.0)         # (detections used as given, no duplicate rule)


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


def junk_state(k, c, seed):
    """Track state as a caller might hold it: arbitrary matrices, status words and filter state (NaNs among them)."""
    rng = np.random.default_rng(seed)
    m = rng.normal(0, 3, (k, 2, 3)).astype(f32)
    status = rng.choice([0, 0, 0, 1, 3, 8, 16, 32, 64, 0x7fffff00], k).astype(np.int32)
    misses = rng.integers(0, 3, k).astype(np.int32)
    state = None
    if c:
        state = rng.normal(50, 40, (k, c, 6))
        state[rng.random((k, c, 6)) < 0.05] = np.nan
    return m, status, misses, state


def gpu(L, det, boxes, m, status, misses, state, n_det=None, frame=(FH, FW), **opts):
    """flm_track_associate through ctypes on fresh device buffers; the outputs are pre-filled with junk."""
    det = np.asarray(det, np.int32).reshape(-1, 4)
    boxes = np.asarray(boxes, np.int32).reshape(-1, 4)
    d, k = len(det), len(boxes)
    t = dict(m_crop=dev(np.asarray(m, f32)), boxes=dev(boxes), status=dev(np.asarray(status, np.int32)),
             misses=dev(np.asarray(misses, np.int32)), state=None if state is None else dev(np.asarray(state, f64)),
             det_slot=torch.full((d,), 777, dtype=torch.int32, device="cuda"),
             slot_det=torch.full((k,), 777, dtype=torch.int32, device="cuda"),
             counts=torch.full((8,), 777, dtype=torch.int32, device="cuda"))
    det_d = dev(det)
    n_d = None if n_det is None else torch.tensor([n_det], dtype=torch.int32, device="cuda")
    c = 1 if state is None else int(np.asarray(state).shape[1])
    o = L.TrackAssocOpts.make(**opts)
    L.check(L.load().flm_track_associate(
        L.stream_ptr(), L.ptr(det_d), None if n_d is None else L.ptr(n_d), d, k, c, IH, IW, frame[0], frame[1], C.byref(o),
        L.ptr(t["m_crop"]), L.ptr(t["boxes"]), L.ptr(t["status"]), L.ptr(t["misses"]),
        None if state is None else L.ptr(t["state"]), L.ptr(t["det_slot"]), L.ptr(t["slot_det"]), L.ptr(t["counts"])),
        "flm_track_associate")
    assert torch.equal(det_d.cpu(), torch.from_numpy(det))          # (the detections are read only)
    return t


def check(L, det, boxes, m, status, misses, state, n_det=None, frame=(FH, FW), **opts):
    """GPU against reference on all eight tensors -> the reference's result."""
    exp = ref.associate(det, n_det, m, boxes, status, misses, state, IH, IW, frame[0], frame[1], **opts)
    got = gpu(L, det, boxes, m, status, misses, state, n_det, frame, **opts)
    for name in NAMES:
        if exp[name] is None:
            assert got[name] is None
            continue
        assert bits_equal(got[name], exp[name]), (name, opts, n_det, got[name].cpu().numpy().tolist()[:40], exp[name].tolist()[:40])
    return exp


# ---- random scenes ---------------------------------------------------------------------------------------------------
def clustered(k, d, seed, fh=FH, fw=FW, lo=8, hi=120):
    """K track boxes and D detector boxes of lo..hi px: roughly a third of each has a partner on the other side (the
    same face, jittered), a few tracks sit in pairs on one face, a fifth of the slots holds no face, some boxes hang over
    the frame's edge, some detections are void."""
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
    for j in rng.permutation(d)[:d // 10]:                                   # void detections
        dets[j] = [[2 ** 28 + 1, 0, 9, 9], [60, 60, 50, 50], [fw + 9, 9, fw + 90, 90], [-2 ** 31, 0, 5, 5]][j % 4]
    return tracks.astype(np.int32), dets.astype(np.int32)


SIZES = [(1, 1), (3, 5), (64, 65), (65, 64), (257, 130), (1024, 1024)]
_CASES = {}


def scene(k, d):
    """One scene and one reference result per size, shared by the tests that need them."""
    if (k, d) not in _CASES:
        tracks, dets = clustered(k, d, 1000 * k + d)
        m, status, misses, state = junk_state(k, 5 if k < 1024 else 2, k + d)
        _CASES[(k, d)] = (dets, tracks, m, status, misses, state)
    return _CASES[(k, d)]


@pytest.mark.parametrize("k,d", SIZES)
def test_random_scenes_match_the_reference(mods, k, d):
    L = mods[0]
    exp = check(L, *scene(k, d), max_misses=2, refresh_iou=0.6)
    cnt = dict(zip(ref.COUNTS, exp["counts"].tolist()))
    print(k, d, cnt)
    if k >= 64:                                  # a condition on the inputs: every outcome occurs
        assert all(cnt[n] > 0 for n in ("matched", "born", "refreshed", "duplicates", "unconfirmed", "void")), cnt
        assert cnt["matched"] >= min(k, d) // 6
    if (k, d) == (257, 130):
        assert cnt["dropped"] == 0               # (more free slots than detections: the dropped ones are in "no free slot")


def test_a_frame_of_32768_squared(mods):
    """Boxes up to the whole frame: area and inter reach 2^30, uni 2^31, the products of the order 2^61."""
    L = mods[0]
    fh = fw = 32768
    tracks, dets = clustered(65, 64, 77, fh, fw, lo=8, hi=32768)
    tracks[:4] = [[0, 0, fw, fh], [0, 0, fw, fh - 1], [1, 0, fw, fh], [-5, -5, fw + 5, fh + 5]]
    dets[:3] = [[0, 0, fw, fh], [0, 1, fw, fh], [0, 0, fw - 1, fh]]
    m, status, misses, state = junk_state(65, 3, 5)
    for opts in (dict(square=False, dup_iou=2.0), dict(square=False, dup_iou=0.9999), dict(square=True, dup_iou=2.0, match_iou=0.0)):
        exp = check(L, dets, tracks, m, status, misses, state, frame=(fh, fw), **opts)
    assert exp["counts"][0] > 10
    exp = check(L, dets, tracks, m, status, misses, state, frame=(fh, fw), square=False, dup_iou=2.0, match_iou=0.9)
    # t0 and t3 cover the whole frame like d0: the lower slot takes it; t3 then has d1 and d2 at (2^30 - 2^15) / 2^30: the
    # lower detection; t1 takes d2 from t2
    assert exp["slot_det"][:4].tolist() == [0, 2, -1, 1]


# ---- crafted cases, each checked by eye in the reference first ---------------------------------------------------------
def plain_state(k, c=0):
    m, status, misses, state = junk_state(k, c, 3)
    return m, np.zeros(k, np.int32), np.zeros(k, np.int32), state


def test_identical_boxes_only_the_tie_rule_decides(mods):
    L = mods[0]
    b = np.tile([100, 60, 160, 120], (64, 1))
    exp = check(L, b, b, *plain_state(64), **PLAIN)
    assert exp["slot_det"].tolist() == list(range(64)) and exp["det_slot"].tolist() == list(range(64))
    # with the duplicate rule every slot but the lowest ends, and 63 detections find no free slot
    exp = check(L, b, b, *plain_state(64), square=False)
    assert exp["counts"].tolist() == [1, 0, 0, 63, 0, 63, 0, 0] and exp["slot_det"][0] == 0


def test_exactly_half_matches_and_one_pixel_less_does_not(mods):
    L = mods[0]
    tracks = [[0, 0, 30, 10], [0, 100, 30, 110]]
    dets = [[11, 100, 41, 110], [10, 0, 40, 10]]        # inter/uni = 190/410, and 200/400
    assert ref.inter(tracks[0], dets[1]) * 2 == 600 - ref.inter(tracks[0], dets[1])
    exp = check(L, dets, tracks, *plain_state(2), match_iou=0.5, **PLAIN)
    assert exp["slot_det"].tolist() == [1, -1] and exp["det_slot"].tolist() == [-2, 0] and exp["misses"].tolist() == [0, 1]


def test_duplicate_chain(mods):
    """A ~ B ~ C with A and C apart: B ends because of A, C because of B, although B is a duplicate itself."""
    L = mods[0]
    tracks = [[0, 0, 100, 100], [50, 0, 150, 100], [100, 0, 200, 100], [300, 0, 400, 100]]
    assert ref.inter(tracks[0], tracks[2]) == 0
    exp = check(L, [[300, 0, 400, 100]], tracks, *plain_state(4), dup_iou=1 / 3, square=False)
    assert exp["status"].tolist() == [0, 32, 32, 0] and exp["counts"].tolist() == [1, 0, 0, 2, 0, 0, 0, 0]
    exp = check(L, [[300, 0, 400, 100]], tracks, *plain_state(4), dup_iou=0.34, square=False)
    assert exp["status"].tolist() == [0, 0, 0, 0]


def test_contested_detections_and_tracks(mods):
    L = mods[0]
    # a detection over two tracks: the better overlap wins, the other track misses
    tracks = [[0, 0, 100, 100], [40, 0, 140, 100]]
    exp = check(L, [[30, 0, 130, 100]], tracks, *plain_state(2), **PLAIN)
    assert exp["slot_det"].tolist() == [-1, 0] and exp["misses"].tolist() == [1, 0]
    # a track over two detections: the better one matches, the other is dropped (no free slot) or born (one free)
    dets = [[20, 0, 120, 100], [5, 0, 105, 100]]
    exp = check(L, dets, [[0, 0, 100, 100]], *plain_state(1), **PLAIN)
    assert exp["det_slot"].tolist() == [-2, 0]
    exp = check(L, dets, [[0, 0, 100, 100], [0, 0, 0, 0]], *plain_state(2), **PLAIN)
    assert exp["det_slot"].tolist() == [1, 0] and exp["slot_det"].tolist() == [1, 0]
    # greedy, not optimal: (t0,d0) is the best pair and takes d0 from t1, which falls back to nothing
    tracks = [[0, 0, 100, 100], [10, 0, 110, 100]]
    dets = [[2, 0, 102, 100], [-60, 0, 40, 100]]
    exp = check(L, dets, tracks, *plain_state(2), **PLAIN)
    assert exp["slot_det"].tolist() == [0, -1]
    # a second round: t1's first choice d0 goes to t0, then t1 takes d1
    dets = [[2, 0, 102, 100], [40, 0, 140, 100]]
    exp = check(L, dets, tracks, *plain_state(2), **PLAIN)
    assert exp["slot_det"].tolist() == [0, 1]


def test_boxes_outside_the_frame_and_void_detections(mods):
    L = mods[0]
    tracks = [[-30, -30, 40, 40], [FW - 20, 100, FW + 60, 180], [FW + 5, 10, FW + 50, 60], [0, FH, 50, FH + 50],
              [-2 ** 31, -2 ** 31, 2 ** 31 - 1, 2 ** 31 - 1], [2 ** 31 - 1, 0, -2 ** 31, 50]]
    dets = [[-25, -35, 45, 40], [FW - 25, 100, FW + 55, 180], [2 ** 28 + 1, 0, 10, 10], [0, 0, 10, -2 ** 28 - 1],
            [60, 60, 50, 50], [FW, 0, FW + 30, 30], [-2 ** 28, -2 ** 28, 2 ** 28, 2 ** 28], [200, 200, 200, 260]]
    for sq in (False, True):
        exp = check(L, dets, tracks, *plain_state(6, 4), square=sq, dup_iou=2.0, match_iou=0.05)
        assert exp["det_slot"][2:6].tolist() == [-1] * 4 and exp["counts"][6] == (5 if not sq else 4), exp
        assert exp["slot_det"][0] == 0 and exp["slot_det"][1] == 1
    # (a zero-width box is void as given; the box maths gives it the width of its height)
    assert exp["det_slot"][7] >= 0


def test_the_device_count(mods):
    L = mods[0]
    tracks, dets = clustered(9, 12, 4)
    st = junk_state(9, 2, 8)
    junk = np.array([[2 ** 31 - 1, -2 ** 31, 7, 7], [0, 0, 300, 300]], np.int32)
    seen = set()
    for n in (0, 12, 7, -3, 13, 2 ** 31 - 1, -2 ** 31):
        rows = dets.copy()
        if 0 <= n < 12:
            rows[n:] = junk[np.arange(12 - n) % 2]               # junk behind the count: never read
        exp = check(L, rows, tracks, *st, n_det=n, max_misses=2)
        nd = min(max(n, 0), 12)
        assert (exp["det_slot"][nd:] == -1).all()
        seen.add(tuple(exp["det_slot"].tolist()))
    assert len(seen) == 3                                          # 0 rows, 7 rows, all 12
    base = ref.associate(dets, None, st[0], tracks, st[1], st[2], st[3], IH, IW, FH, FW, max_misses=2)
    assert tuple(base["det_slot"].tolist()) in seen


def test_no_free_slot(mods):
    L = mods[0]
    tracks = [[0, 0, 50, 50], [100, 0, 150, 50], [200, 0, 250, 50]]
    dets = [[300, 100, 350, 150], [100, 0, 150, 50], [300, 200, 350, 250]]
    exp = check(L, dets, tracks, *plain_state(3), **PLAIN)
    assert exp["det_slot"].tolist() == [-2, 1, -2] and exp["counts"].tolist() == [1, 0, 0, 0, 0, 2, 0, 0]
    # a slot killed in this call is not reused in it
    exp = check(L, dets, tracks, *plain_state(3), max_misses=1, **PLAIN)
    assert exp["det_slot"].tolist() == [-2, 1, -2] and exp["status"].tolist() == [64, 0, 64]
    assert (exp["boxes"][[0, 2]] == 0).all()


@pytest.mark.parametrize("c", [0, 1, 68, 130])
def test_options_and_state(mods, c):
    """square 0 and 1, refresh on and off, the state absent and given: restarted and born slots lose their history, every
    other row keeps its junk bits."""
    L = mods[0]
    tracks, dets = clustered(12, 14, 21)
    m, status, misses, state = junk_state(12, c, 6)
    hist = set()
    for sq in (False, True):
        for refresh in (0.0, 0.5, 0.95, 5.0):
            exp = check(L, dets, tracks, m, status, misses, state, square=sq, refresh_iou=refresh, match_iou=0.2)
            hist.add((exp["counts"][0], exp["counts"][2]))
            if c:
                reset = (exp["state"] == -1.0).all((1, 2))
                assert reset.sum() == exp["counts"][1] + exp["counts"][2]
                keep = ~reset
                assert np.array_equal(exp["state"][keep].view(np.uint64), np.asarray(state)[keep].view(np.uint64))
            if refresh == 0.0:
                assert exp["counts"][2] == 0
            if refresh == 5.0:
                assert exp["counts"][2] == exp["counts"][0] > 0
    assert len(hist) >= 3


@pytest.mark.parametrize("max_misses", [0, 1, 3])
def test_three_calls_in_a_row_count_the_misses(mods, max_misses):
    L = mods[0]
    tracks = np.array([[0, 0, 50, 50], [100, 0, 150, 50], [200, 0, 250, 50], [0, 0, 0, 0], [300, 100, 340, 140]], np.int32)
    dets = [[[100, 0, 150, 50]], [[100, 0, 150, 50], [200, 0, 250, 50]], [[400, 200, 440, 240]]]
    m, status, misses, _ = plain_state(5)
    misses[:] = [0, 2, 0, 2 ** 31 - 1, 2 ** 31 - 1]      # (slot 3 holds no face: its counter is not touched until it is born)
    M, N = 2 ** 31 - 1, -2 ** 31                         # (slot 4 is never matched: its counter wraps as a uint32 does)
    want = {0: [[1, 0, 1, M, N], [2, 0, 0, M, N + 1], [3, 1, 1, 0, N + 2]],
            # max_misses = 1: slots 0 and 2 end in the first call; the second call's new detection is born into slot 0
            1: [[0, 0, 0, M, N], [0, 0, 0, M, N + 1], [0, 0, 0, M, N + 2]],
            3: [[1, 0, 1, M, N], [2, 0, 0, M, N + 1], [0, 1, 1, 0, N + 2]]}[max_misses]
    for call in range(3):
        exp = check(L, dets[call], tracks, m, status, misses, None, max_misses=max_misses, **PLAIN)
        assert exp["misses"].tolist() == want[call], (call, exp["misses"].tolist())
        m, tracks, status, misses = exp["m_crop"], exp["boxes"], exp["status"], exp["misses"]
    assert (status[0] == 64) == (max_misses in (1, 3))


def test_wrapper_returns_what_the_raw_call_writes(mods):
    L, A, P = mods
    dets, tracks, m, status, misses, state = scene(64, 65)
    exp = ref.associate(dets, None, m, tracks, status, misses, state, IH, IW, FH, FW, max_misses=2, refresh_iou=0.6)
    t = [dev(x) for x in (m, tracks, status, misses, state)]
    ds, sd, cnt = A.track_associate_device(dev(dets), t[0], t[1], t[2], t[3], (IH, IW), (FH, FW), state=t[4],
                                           assoc=A.TrackAssociation(max_misses=2, refresh_iou=0.6))
    for got, name in zip(t + [ds, sd, cnt], NAMES):
        assert bits_equal(got, exp[name]), name
    with pytest.raises(ValueError, match="1024"):
        A.track_associate_device(torch.zeros((1025, 4), dtype=torch.int32, device="cuda"), *t[:4], (IH, IW), (FH, FW))
    with pytest.raises(ValueError, match="n_det"):
        A.track_associate_device(dev(dets), *t[:4], (IH, IW), (FH, FW), n_det=torch.zeros(2, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match="misses"):
        A.track_associate_device(dev(dets), t[0], t[1], t[2], t[3][:-1], (IH, IW), (FH, FW))
    with pytest.raises(ValueError, match="state"):
        A.track_associate_device(dev(dets), *t[:4], (IH, IW), (FH, FW), state=t[4][:, :, :5])


# ---- FaceTracker ---------------------------------------------------------------------------------------------------------
RH, RW = 64, 96
FACES = [(20, 8, 60, 50), (40, 2, 90, 60), (-6, 20, 30, 58)]
SLOTS = [0, 2, 3]
DETS = [[(22, 10, 60, 48), (70, 30, 96, 62), (0, 0, 20, 20), (-6, 22, 30, 58)],
        [(40, 4, 88, 58), (10, 10, 50, 50), (2 ** 30, 0, 5, 5), (60, 20, 96, 60), (0, 30, 30, 64)]]


class _Stub:
    n_classes, input_height, input_width, output_height, output_width = 68, 64, 64, 72, 72


def test_update_on_a_dead_tracker_is_seed(mods):
    L, A, P = mods
    boxes = [(20, 8, 60, 50), (40, 2, 90, 60), (-6, 20, 30, 58), (100, 100, 131, 160), (300, 5, 420, 99)]
    for smooth in (None, True):
        a = P.FaceTracker(_Stub(), (FH, FW), 7, smooth=smooth)
        b = P.FaceTracker(_Stub(), (FH, FW), 7, smooth=smooth)
        ds, sd, cnt = a.update(boxes)
        b.seed(range(5), boxes)
        for name in ("m_crop", "boxes", "status", "misses"):
            assert torch.equal(getattr(a, name).view(torch.int32), getattr(b, name).view(torch.int32)), name
        assert ds.tolist() == [0, 1, 2, 3, 4] and sd.tolist() == [0, 1, 2, 3, 4, -1, -1]
        assert cnt.tolist() == [0, 5, 0, 0, 0, 0, 0, 0] and not a.status[:5].any() and a.status[5:].tolist() == [1, 1]
        if smooth:
            assert torch.equal(a.filter_state, b.filter_state) and (a.filter_state == -1).all()


@pytest.fixture(scope="module")
def rings(mods):
    L, A, P = mods
    rng = np.random.default_rng(31)
    bgr = rng.integers(0, 256, (2, RH, RW, 3), dtype=np.uint8)
    nv = np.stack([nv12_ref.pack_slot(*nv12_ref.bgr_to_nv12(bgr[f], "bt709"), RW, RH, RH * 3 // 2) for f in range(2)])
    return {"bgr": (dev(bgr), None), "nv12": (dev(nv), A.FrameFormat.nv12(RH, RW, matrix="bt709"))}


@pytest.fixture(scope="module")
def model():
    from flm_amd.networks import LANDMARKS_MODELS
    from flm_amd.weights import synth_fcn8_weights
    m = LANDMARKS_MODELS["fcn_8"](68, input_height=64, input_width=64, dtype="bf16")
    m.load_weights(synth_fcn8_weights(68, seed=2))
    return m


def by_hand(mods, model, ring, ff, frames, dets, assoc, smooth):
    """seed, then for every frame a step and -- where `dets` is given -- an association, through the public pieces,
    nothing aliased by the step.  -> the steps' (aligned, m_align, lm_frame, status) and the associations' outputs."""
    L, A, P = mods
    cap = 4
    boxes = torch.zeros((cap, 4), dtype=torch.int32, device="cuda")
    m = torch.eye(2, 3, dtype=torch.float32, device="cuda").repeat(cap, 1, 1).contiguous()
    status = torch.full((cap,), L.TRACK_DEAD, dtype=torch.int32, device="cuda")
    misses = torch.zeros((cap,), dtype=torch.int32, device="cuda")
    state = torch.full((cap, 68, 6), -1.0, dtype=torch.float64, device="cuda") if smooth else None
    sq = dev(np.asarray(P.face_boxes([list(b) for b in FACES]), np.int32))
    sm, ss = A.track_seed_device(sq, (64, 64), (RH, RW))
    for i, s in enumerate(SLOTS):
        boxes[s], m[s], status[s] = sq[i], sm[i], ss[i]
    tc, ta = dev(A.canonical_template(68, 64, 64)), dev(A.canonical_template(68, 112, 112))
    filt = dict(filter=A.LandmarkFilter(), state=state) if smooth else {}
    steps, ups = [], []
    for t, fi in enumerate(frames):
        idx = torch.full((cap,), fi, dtype=torch.int32, device="cuda")
        crops = A.warp_frames_device(ring, m, 64, 64, frame_index_dev=idx, boxes_dev=boxes, fmt=A.AlignedFormat("nhwc", "uint8"), src=ff)
        lm = model.forward_device(crops, "landmarks", n_points=4, thresh=0.0)
        lmf, ma, mn, bn, st = A.track_step_device(lm, m, boxes, (72, 72), (64, 64), (RH, RW), tc, ta, **filt)
        aligned = A.warp_frames_device(ring, ma, 112, 112, frame_index_dev=idx, boxes_dev=boxes, src=ff)
        steps.append((aligned, ma, lmf, st.clone()))
        m, boxes, status = mn, bn, st
        if dets is not None:
            ups.append(A.track_associate_device(dev(np.asarray(dets[t], np.int32)), m, boxes, status, misses, (64, 64), (RH, RW),
                                                state=state, assoc=assoc))
    return steps, ups, (m, boxes, status, misses, state)


@pytest.mark.parametrize("smooth", [None, True])
@pytest.mark.parametrize("source", ["bgr", "nv12"])
def test_face_tracker_with_updates_is_the_sequence_made_by_hand(mods, rings, model, source, smooth):
    L, A, P = mods
    ring, ff = rings[source]
    frames = [1, 0]
    assoc = A.TrackAssociation(max_misses=2, refresh_iou=0.5)
    exp_steps, exp_ups, exp_state = by_hand(mods, model, ring, ff, frames, DETS, assoc, smooth)
    trackers = {}
    for how in ("host", "device"):
        tr = P.FaceTracker(model, (RH, RW), 4, frame_format=ff, associate=assoc, smooth=smooth)
        tr.seed(SLOTS, FACES)
        for t, fi in enumerate(frames):
            got = [x.clone() for x in tr.step(ring, fi)]
            for a, b in zip(got, exp_steps[t]):
                assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), (how, t)
            if how == "host":
                up = tr.update(DETS[t])
            else:                                  # a detector's fixed buffer of 8 rows and its count, both on the device
                buf = torch.full((8, 4), 12345, dtype=torch.int32, device="cuda")
                buf[:len(DETS[t])] = dev(np.asarray(DETS[t], np.int32))
                n = torch.tensor([len(DETS[t])], dtype=torch.int32, device="cuda")
                torch.cuda.synchronize()
                torch.cuda.set_sync_debug_mode("error")
                try:
                    if t == 0:
                        with pytest.raises(RuntimeError):      # (the mode is live in this build: a download raises)
                            n.item()
                    up = tr.update(buf, n)
                finally:
                    torch.cuda.set_sync_debug_mode("default")
                assert (up[0][len(DETS[t]):] == -1).all()
                up = (up[0][:len(DETS[t])], up[1], up[2])
            for a, b in zip(up, exp_ups[t]):
                assert a.is_cuda and a.dtype == torch.int32 and torch.equal(a, b), (how, t, a.tolist(), b.tolist())
        trackers[how] = tr
        for name, e in zip(("m_crop", "boxes", "status", "misses", "filter_state"), exp_state):
            g = getattr(tr, name)
            assert (g is None and e is None) or torch.equal(g.view(torch.int64) if g.dtype == torch.float64 else g.view(torch.int32),
                                                            e.view(torch.int64) if e.dtype == torch.float64 else e.view(torch.int32)), name
    print(source, smooth, "counts per update:", [u[2].tolist() for u in exp_ups], "status:", exp_state[2].tolist())
    assert sum(int(u[2][1]) for u in exp_ups) > 0                 # detections did start tracks
    assert int(exp_ups[0][2][5]) + int(exp_ups[1][2][5]) > 0      # and the four slots did run out


@pytest.mark.parametrize("source", ["bgr", "nv12"])
def test_a_tracker_that_never_updates_has_not_moved(mods, rings, model, source):
    """step's four outputs, for a tracker that is only seeded and stepped, are those of the sequence as it was before
    `update` existed, made by hand from the pieces of before."""
    L, A, P = mods
    ring, ff = rings[source]
    frames = [1, 0, 1]
    exp_steps, _, _ = by_hand(mods, model, ring, ff, frames, None, None, None)
    tr = P.FaceTracker(model, (RH, RW), 4, frame_format=ff)
    tr.seed(SLOTS, FACES)
    for t, fi in enumerate(frames):
        for a, b in zip(tr.step(ring, fi), exp_steps[t]):
            assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), t
    assert tr.lost() == [i for i in range(4) if int(exp_steps[-1][3][i]) != 0]
    assert not tr.misses.any()
