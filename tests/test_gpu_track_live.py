"""GPU parity of flm_track_gather_live against tests/track_live_ref.py through ctypes, on buffers pre-filled with junk
(NaNs included), bit for bit on every output and every in/out tensor, over the sizes at which a scan goes wrong and two
consecutive calls, so that reset, age and cursor carry over; the wrapper inside sync-debug "error"; and
FaceTracker.step_live against a sequence made by hand at the same batch from the numpy row map -- at a budget that holds
every slot, at a budget of two with four and five live slots (the rotation, the waits, a birth), with device arguments,
and at streams=1 mixed with `step` and `step_active`.  Every comparison is exact.
"""
import numpy as np
import pytest
import torch

import nv12_ref
import track_live_ref as lref

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
NAN, INF = float("nan"), float("inf")
FH, FW = 270, 480


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
    u = {1: np.uint8, 4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    return np.array_equal(np.ascontiguousarray(got).view(u), np.ascontiguousarray(exp).view(u))


def view_bits(x):
    return x.view(torch.int64) if x.dtype == torch.float64 else x.view(torch.int32) if x.dtype == torch.float32 else x


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(view_bits(a), view_bits(b))


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


def junk64(rng, shape, lo, hi, p_nan=0.08):
    x = rng.uniform(lo, hi, shape)
    x[rng.random(shape) < p_nan] = np.nan
    return x


# ---- flm_track_gather_live ---------------------------------------------------------------------------------------------
# S*K below, at and across a wave (63, 64, 65), across the workgroup's chunk of 1024 slots (1023, 1025), and at the limit
SHAPES = {1: (1, 1), 9: (3, 3), 63: (7, 9), 64: (4, 16), 65: (5, 13), 1023: (33, 31), 1025: (41, 25), 65535: (4369, 15)}
# boxes without pixels: plainly empty, and empty only after the clip to fh x fw
EMPTY = [(0, 0, 0, 0), (-40, 10, 0, 60), (FW, 10, FW + 30, 60), (10, FH, 60, FH + 9), (50, 50, 50, 90), (90, 40, 60, 80),
         (-9, -9, 0, 0), (FW + 1, FH + 1, FW + 9, FH + 9)]
LIVE = [(20, 10, 80, 70), (-10, -10, 30, 30), (FW - 1, FH - 1, FW + 50, FH + 50), (0, 0, FW, FH), (-5, 100, 1, 101)]
DT_VALUES = [1 / 30, 0.0, NAN, -0.5, INF, 0.04, 1e-3]
# (how many slots are eligible against the budget, the cursor, the mask, the optional groups: f = frame_idx_stream,
#  d = dt_stream (else the scalar dt), a = age, q = best_q, r = reset)
SCENARIOS = [
    ("all", "zero", "null", "fdaqr"),
    ("all_gt", "mid", "null", "fdaqr"),
    ("none", "null", "null", ""),
    ("lt", "last", "mixed", "fdaqr"),
    ("eq", "outside", "mixed", "aq"),
    ("gt1", "last", "null", "r"),
    ("gt1", "mid", "mixed", "fdaqr"),
    ("all", "mid", "off", "fdaqr"),
    ("gt1", "null", "null", "fa"),
    ("eq", "negative", "null", "dar"),
]
CASES = [(t, i) for t in SHAPES for i in range(len(SCENARIOS)) if t != 65535 or i in (1, 3, 6)]


def live_case(total, scenario, seed):
    s, k = SHAPES[total]
    fill, cur, mask, opt = scenario
    rng = np.random.default_rng(seed)
    on = {"null": None, "off": np.zeros(s, np.int32),
          "mixed": rng.choice([0, 1, 1, -3, 7], s).astype(np.int32)}[mask]
    cand = np.array([g for g in range(total) if on is None or on[g // k] != 0], np.int64)
    e = {"all": len(cand), "all_gt": len(cand), "none": 0, "lt": len(cand) // 3, "eq": max(1, len(cand) // 2),
         "gt1": max(2, len(cand) // 2)}[fill]
    e = min(e, len(cand))
    n = {"all": e, "all_gt": e // 3, "none": 3, "lt": e + 2, "eq": e, "gt1": e - 1}[fill]
    n = int(min(max(n, 1), 65535))
    boxes = np.array([EMPTY[g % len(EMPTY)] for g in range(total)], np.int32)
    for g in rng.permutation(cand)[:e]:
        boxes[g] = LIVE[g % len(LIVE)]
    if on is not None:                                       # a stream that is off may hold anything: it is not looked at
        for g in range(total):
            if on[g // k] == 0 and g % 2:
                boxes[g] = LIVE[g % len(LIVE)]
    eligible = sum(1 for g in cand if not lref.box_empty(boxes[g], FH, FW))
    assert eligible == e
    c = dict(s=s, k=k, n=n, e=e, on=on, boxes=boxes, m=junk64(rng, (total, 2, 3), -3, 3).astype(f32),
             cursor={"null": None, "zero": 0, "mid": total // 2, "last": total - 1, "outside": total, "negative": -7}[cur],
             fi=rng.integers(0, 8, s).astype(np.int32) if "f" in opt else None,
             dts=np.array([DT_VALUES[(i + seed) % len(DT_VALUES)] for i in range(s)], f64) if "d" in opt and "a" in opt else None,
             dt=0.04 if "a" in opt and "d" not in opt else 0.0,
             age=junk64(rng, (total,), -0.5, 2.0) if "a" in opt else None,
             bq=junk64(rng, (total,), -1, 1) if "q" in opt else None,
             reset=rng.choice([0, 0, 1, 7, -3], total).astype(np.int32) if "r" in opt else None)
    return c


def gpu_live(L, c, t):
    """One call on the device tensors `t` (the in/out ones written in place) -> the compact outputs, pre-filled with junk."""
    n = c["n"]
    full = lambda shape, v, dt: torch.full(shape, v, dtype=dt, device="cuda")
    o = dict(slot=full((n,), 777, torch.int32), m=full((n, 2, 3), NAN, torch.float32), boxes=full((n, 4), 777, torch.int32),
             frame_index=full((n,), 777, torch.int32), dt=None if t["age"] is None else full((n,), NAN, torch.float64),
             best_q=None if t["bq"] is None else full((n,), NAN, torch.float64),
             reset=None if t["reset"] is None else full((n,), 777, torch.int32), counts=full((4,), 777, torch.int32))
    p = lambda x: None if x is None else L.ptr(x)
    L.check(L.load().flm_track_gather_live(
        L.stream_ptr(), p(t["on"]), c["s"], c["k"], FH, FW, n, p(t["fi"]), p(t["dts"]), c["dt"], L.ptr(t["m"]), L.ptr(t["boxes"]),
        p(t["bq"]), p(t["reset"]), p(t["age"]), p(t["cursor"]), L.ptr(o["slot"]), L.ptr(o["m"]), L.ptr(o["boxes"]),
        L.ptr(o["frame_index"]), p(o["dt"]), p(o["best_q"]), p(o["reset"]), L.ptr(o["counts"])), "flm_track_gather_live")
    return o


def device_tensors(c):
    t = {name: None if c[name] is None else dev(c[name]) for name in ("on", "fi", "dts", "m", "boxes", "bq", "reset", "age")}
    t["cursor"] = None if c["cursor"] is None else dev(np.array([c["cursor"]], np.int32))
    return t


@pytest.mark.parametrize("total,scenario", CASES)
def test_gather_live_matches_the_reference_over_two_calls(mods, total, scenario):
    L = mods[0]
    c = live_case(total, SCENARIOS[scenario], 100 * scenario + total % 97)
    t = device_tensors(c)
    reset, age, cursor = c["reset"], c["age"], c["cursor"]
    for call in range(2):
        exp = lref.gather_live(c["m"], c["boxes"], c["s"], c["k"], FH, FW, c["n"], stream_on=c["on"], frame_idx_stream=c["fi"],
                               dt_stream=c["dts"], dt=c["dt"], best_q=c["bq"], reset=reset, age=age, cursor=cursor)
        o = gpu_live(L, c, t)
        for name in ("slot", "m", "boxes", "frame_index", "dt", "best_q", "reset", "counts"):
            if exp[name] is None:
                assert o[name] is None, name
            else:
                assert bits_equal(o[name], exp[name]), (name, call, o[name].cpu().numpy()[:8], exp[name][:8])
        # what is only read keeps its bits; the in/out tensors are the reference's
        assert bits_equal(t["m"], c["m"]) and bits_equal(t["boxes"], c["boxes"])
        for name, glob in (("bq", c["bq"]), ("reset", exp["reset_global"]), ("age", exp["age_global"])):
            assert (t[name] is None and glob is None) or bits_equal(t[name], glob), (name, call)
        if cursor is not None:
            assert int(t["cursor"].cpu()[0]) == exp["cursor_global"] == exp["counts"][3]
        e, served = int(exp["counts"][0]), int(exp["counts"][1])
        assert e == c["e"] and served == min(e, c["n"]) and (exp["slot"][served:] == -1).all()
        reset, age, cursor = exp["reset_global"], exp["age_global"], exp["cursor_global"]


def test_the_wrapper_returns_what_the_raw_call_writes_without_a_synchronisation(mods):
    L, A, P = mods
    c = live_case(65, SCENARIOS[6], 5)
    exp = lref.gather_live(c["m"], c["boxes"], c["s"], c["k"], FH, FW, c["n"], stream_on=c["on"], frame_idx_stream=c["fi"],
                           dt_stream=c["dts"], best_q=c["bq"], reset=c["reset"], age=c["age"], cursor=c["cursor"])
    t = device_tensors(c)
    mine = torch.full((4,), 777, dtype=torch.int32, device="cuda")
    with sync_error(probe=mine):
        snap = A.track_gather_live_device(t["m"], t["boxes"], c["k"], (FH, FW), c["n"], stream_on=t["on"], frame_index=t["fi"],
                                          dt=t["dts"], best_q=t["bq"], reset=t["reset"], age=t["age"], cursor=t["cursor"],
                                          out=dict(counts=mine))
    assert snap["counts"] is mine and sorted(snap) == ["best_q", "boxes", "counts", "dt", "frame_index", "m", "reset", "slot"]
    for name in snap:
        assert bits_equal(snap[name], exp[name]), name
    assert bits_equal(t["reset"], exp["reset_global"]) and bits_equal(t["age"], exp["age_global"])
    assert int(t["cursor"].cpu()[0]) == exp["cursor_global"]
    # the scalar dt, and nothing optional
    exp = lref.gather_live(c["m"], c["boxes"], c["s"], c["k"], FH, FW, 7, dt=0.25, age=exp["age_global"])
    with sync_error():
        snap = A.track_gather_live_device(t["m"], t["boxes"], c["k"], (FH, FW), 7, dt=0.25, age=t["age"])
        bare = A.track_gather_live_device(t["m"], t["boxes"], c["k"], (FH, FW), 7)
    assert sorted(snap) == ["boxes", "counts", "dt", "frame_index", "m", "slot"] and bits_equal(snap["dt"], exp["dt"])
    assert bits_equal(t["age"], exp["age_global"])
    assert sorted(bare) == ["boxes", "counts", "frame_index", "m", "slot"] and bits_equal(bare["slot"], exp["slot"])
    with pytest.raises(ValueError, match="needs its input"):
        A.track_gather_live_device(t["m"], t["boxes"], c["k"], (FH, FW), 7, out=dict(dt=snap["dt"]))
    with pytest.raises(ValueError, match="overlap"):
        A.track_gather_live_device(t["m"], t["boxes"], c["k"], (FH, FW), 7, out=dict(m=t["m"][:7]))
    with pytest.raises(ValueError, match="slots_per_stream"):
        A.track_gather_live_device(t["m"], t["boxes"], 4, (FH, FW), 7)
    with pytest.raises(ValueError, match="budget"):
        A.track_gather_live_device(t["m"], t["boxes"], c["k"], (FH, FW), 0)
    with pytest.raises(ValueError, match="dt goes with age"):
        A.track_gather_live_device(t["m"], t["boxes"], c["k"], (FH, FW), 7, dt=0.1)
    for bad in (None, 0.0, NAN, INF, True):
        with pytest.raises(ValueError, match="with age, dt"):
            A.track_gather_live_device(t["m"], t["boxes"], c["k"], (FH, FW), 7, dt=bad, age=t["age"])
    with pytest.raises(ValueError, match="stream_on"):
        A.track_gather_live_device(t["m"], t["boxes"], c["k"], (FH, FW), 7, stream_on=t["on"][:-1])
    with pytest.raises(ValueError, match="cursor"):
        A.track_gather_live_device(t["m"], t["boxes"], c["k"], (FH, FW), 7, cursor=t["fi"])


# ---- FaceTracker.step_live ---------------------------------------------------------------------------------------------
RH, RW, CAP, S, K = 64, 96, 9, 3, 3
FACES = [(20, 8, 60, 50), (40, 2, 90, 60), (-6, 20, 30, 58), (30, 10, 80, 60)]
SEEDS = {0: ([0, 2], FACES[:2]), 1: ([1], FACES[2:3]), 2: ([0], FACES[3:])}       # stream -> (its local slots, the boxes)
SEEDED = [0, 2, 4, 6]                                                              # ... as global slots: four of the nine
STATE = ("m_crop", "boxes", "status", "misses")
BEST = ("gallery", "best_q", "best_frame", "best_M", "best_landmarks", "best_rec", "_best_reset")
RING_SLOT = lambda t, i: (3 * t + 2 * i + 1) % 8            # the ring slot stream i reads at tick t


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


def make_tracker(mods, model, ff, smooth, best_shot, streams=S, capacity=CAP):
    L, A, P = mods
    return P.FaceTracker(model, (RH, RW), capacity, frame_format=ff, smooth=smooth, best_shot=best_shot,
                         weights="score" if best_shot else None, associate=A.TrackAssociation(match_iou=2.0), streams=streams)


def state_of(tr):
    names = STATE + (("filter_state",) if tr.smooth is not None else ()) + (BEST if tr.best_shot is not None else ())
    return {n: getattr(tr, n).clone() for n in names}


def assert_state(a, b, what):
    assert sorted(a) == sorted(b)
    for name in a:
        assert same(a[name], b[name]), (name,) + tuple(what)


def live_now(tr):
    """The slots of `tr` that hold a box with pixels, from a download."""
    return [g for g, b in enumerate(tr.boxes.cpu().numpy()) if not lref.box_empty(b, RH, RW)]


def new_mirror(tr):
    """What the hand sequence keeps on the host in place of the tracker's slot_age and live_cursor."""
    return dict(age=np.zeros(tr.capacity, f64), cursor=0, counts=None, dt=None)


def hand_tick(mods, tr, mir, model, ring, ff, fi, budget, on, dts, frame_id):
    """One tick of `step_live` made by hand on the tensors of `tr` at the SAME batch: the rows come from the numpy row map
    on a download of the state; then the warps on the hand-gathered matrices, the forward, track_step_rows_device on
    those rows with the reference's time steps, and the dense best update on gathered copies of the served slots,
    scattered back.  mir: the host mirror of slot_age and live_cursor (`new_mirror`), updated."""
    L, A, P = mods
    smooth, best = tr.smooth is not None, tr.best_shot is not None
    ref = lref.gather_live(tr.m_crop.cpu().numpy(), tr.boxes.cpu().numpy(), tr.streams, tr.slots_per_stream, RH, RW, budget,
                           stream_on=on, frame_idx_stream=fi, dt_stream=dts if smooth else None,
                           best_q=tr.best_q.cpu().numpy() if best else None,
                           reset=tr._best_reset.cpu().numpy() if best else None, age=mir["age"] if smooth else None,
                           cursor=mir["cursor"])
    if smooth:
        mir["age"] = ref["age_global"]
    mir["cursor"], mir["counts"], mir["dt"] = ref["cursor_global"], ref["counts"], ref["dt"]
    served = int(ref["counts"][1])
    slot_d, m_c, b_c, idx = dev(ref["slot"]), dev(ref["m"]), dev(ref["boxes"]), dev(ref["frame_index"])
    crops = A.warp_frames_device(ring, m_c, 64, 64, frame_index_dev=idx, boxes_dev=b_c, samples=tr.crop_samples,
                                 fmt=A.AlignedFormat("nhwc", "uint8"), src=ff)
    if tr.weights is None:
        lm, wd = model.forward_device(crops, "landmarks", n_points=tr.n_points, thresh=tr.thresh), None
    else:
        rec = model.forward_device(crops, "landmark_stats", n_points=tr.n_points, thresh=tr.thresh)
        lm, wd = rec[..., :2], rec[..., 2]
    filt = dict(filter=tr.smooth, dt=dev(ref["dt"]), state=tr.filter_state) if smooth else {}
    lmf, ma, st = A.track_step_rows_device(lm, m_c, b_c, slot_d, (72, 72), (64, 64), (RH, RW), tr.crop_template, tr.m_crop,
                                           tr.boxes, tr.status, tmpl_align=tr.template, weights=wd, **tr.limits, **filt)
    aligned = A.warp_frames_device(ring, ma, 112, 112, frame_index_dev=idx, boxes_dev=b_c, samples=tr.samples,
                                   fmt=tr.aligned_format, src=ff)
    if best:
        qrec = A.face_quality_device(aligned, tr.aligned_format, tr.best_shot.quality)
        tr._best_reset.copy_(dev(ref["reset_global"]))       # the pending resets of the served slots moved into the snapshot
        if served:
            g = dev(ref["slot"][:served].astype(np.int64))
            names = ("best_q", "gallery", "best_frame", "best_M", "best_landmarks", "best_rec")
            c = {nm: getattr(tr, nm).index_select(0, g).contiguous() for nm in names}
            bq_out = torch.empty_like(c["best_q"])
            A.track_best_update_device(aligned[:served], qrec[:served], lmf[:served], c["best_q"], bq_out, c["gallery"],
                                       c["best_frame"], frame_id, status=st[:served], reset=dev(ref["reset"][:served]),
                                       weights=None if wd is None else wd[:served], m=ma[:served], opts=tr.best_shot,
                                       best_m=c["best_M"], best_lm=c["best_landmarks"], best_rec=c["best_rec"])
            c["best_q"] = bq_out
            for nm in names:
                getattr(tr, nm).index_copy_(0, g, c[nm])
    tr._steps += 1
    return aligned, ma, lmf, st, slot_d


def assert_mirror(tr, mir, what):
    if tr.smooth is not None:
        assert bits_equal(tr.slot_age, mir["age"]), what
    assert int(tr.live_cursor.cpu()[0]) == mir["cursor"], what
    assert bits_equal(tr.live_counts, mir["counts"]), what


def seed_four(trackers):
    for tr in trackers:
        for i, (slots, faces) in SEEDS.items():
            tr.seed(slots, faces, stream=i)


@pytest.mark.parametrize("best_shot", [None, True])
@pytest.mark.parametrize("smooth", [None, True])
@pytest.mark.parametrize("source", ["bgr", "nv12"])
def test_a_budget_for_every_slot_is_the_sequence_made_by_hand(mods, rings, model, source, smooth, best_shot):
    """(a): budget 9 over three steps; the returned tensors and the whole state after every step, and the slots that were
    dead before a step bit-equal to before -- their status included, which `step` would overwrite."""
    L, A, P = mods
    ring, ff = rings[source]
    hand, live = [make_tracker(mods, model, ff, smooth, best_shot) for _ in range(2)]
    seed_four((hand, live))
    mir = new_mirror(hand)
    hand.status[7] = live.status[7] = L.TRACK_SCALE | L.TRACK_DEAD       # a reason a dead slot keeps
    rows_alive = 0
    for t in range(3):
        fi = [RING_SLOT(t, i) for i in range(S)]
        dts = [0.04, 0.05, 1 / 30]
        fid = 100 + t if best_shot and t == 1 else None
        before, alive = state_of(live), live_now(live)
        if t == 0:
            assert alive == SEEDED
        exp = hand_tick(mods, hand, mir, model, ring, ff, fi, CAP, None, dts, hand._steps if fid is None else fid)
        kw = {} if fid is None else dict(frame_id=fid)
        if smooth:
            kw["dt"] = dts
        got = live.step_live(ring, fi, CAP, **kw)
        assert len(got) == 5
        for a, b in zip(got, exp):
            assert same(a, b), (source, t)
        assert_state(state_of(live), state_of(hand), (source, t))
        assert_mirror(live, mir, (source, t))
        assert got[4].tolist() == alive + [-1] * (CAP - len(alive))      # E <= N: ascending from the cursor, which stays 0
        n = len(alive)
        assert not got[0][n:].any() and (got[3][n:] == L.TRACK_DEAD).all() and (got[2][n:] == -1).all()
        assert torch.equal(got[1][n:].cpu(), torch.eye(2, 3).repeat(CAP - n, 1, 1))
        dead = [g for g in range(CAP) if g not in alive]
        after = state_of(live)
        for name in after:
            assert same(after[name][dead], before[name][dead]), (name, t)
        assert live._steps == hand._steps == t + 1
        rows_alive += int((got[3][:n] == 0).sum())
    assert int(live.status[7]) == L.TRACK_SCALE | L.TRACK_DEAD and 7 in live.lost()
    assert rows_alive > 0
    print(source, smooth, best_shot, "rows alive:", rows_alive, "status:", live.status.tolist())


BORN = 1 * K + 0                                            # stream 1's lowest free slot: where the update's detection is born
ACTIVE = (None, [0, 1, 2], [2, 0], None)                    # the streams that deliver a frame at every tick


@pytest.mark.parametrize("best_shot", [None, True])
@pytest.mark.parametrize("smooth", [None, True])
@pytest.mark.parametrize("source", ["bgr", "nv12"])
def test_a_budget_of_two_rotates_through_the_live_slots(mods, rings, model, source, smooth, best_shot):
    """(b) and (c): four ticks at budget 2 with four live slots, then five (an update starts a track after the first
    tick), a stream that sits a tick out, and whatever tracks the ticks lose -- with host arguments, and with `active`,
    `frame_index` and `dt` on the device inside sync-debug "error" -- against the sequence made by hand after every tick."""
    L, A, P = mods
    ring, ff = rings[source]
    hand, host, devc = [make_tracker(mods, model, ff, smooth, best_shot) for _ in range(3)]
    trackers = (hand, host, devc)
    seed_four(trackers)
    mir = new_mirror(hand)
    last_frame = [None] * S                                  # the tick of every stream's last frame
    last_served = {g: -1 for g in SEEDED}                    # the tick every live slot was served last (a seed: the tick before)
    served_all, lost_rows, born_served = [], 0, None
    for t, active in enumerate(ACTIVE):
        streams_on = list(range(S)) if active is None else active
        on = None if active is None else [1 if i in active else 0 for i in range(S)]
        fi = [RING_SLOT(t, i) for i in range(S)]
        dts = [(1 if last_frame[i] is None else t - last_frame[i]) / 30.0 for i in range(S)]
        for i in streams_on:
            last_frame[i] = t
        fid = 1000 + 7 * t if best_shot and t % 2 else None
        before, alive = state_of(hand), live_now(hand)
        exp = hand_tick(mods, hand, mir, model, ring, ff, fi, 2, on, dts, hand._steps if fid is None else fid)
        # host forms: the entries of the streams that sit out are None
        kw = {} if fid is None else dict(frame_id=fid)
        if smooth:
            kw["dt"] = [dts[i] if i in streams_on else None for i in range(S)]
        got = host.step_live(ring, [fi[i] if i in streams_on else None for i in range(S)], 2, active=active, **kw)
        # device forms: nothing is transferred, nothing synchronises
        mask_d, fi_d = dev(np.asarray([1] * S if on is None else on, np.int32)), dev(np.asarray(fi, np.int32))
        if smooth:
            kw["dt"] = dev(np.asarray(dts, f64))
        with sync_error(probe=fi_d if t == 0 else None):
            got_d = devc.step_live(ring, fi_d, 2, active=mask_d, **kw)
        for how, res, tr in (("host", got, host), ("device", got_d, devc)):
            assert len(res) == 5
            for a, b in zip(res, exp):
                assert same(a, b), (how, t)
            assert_state(state_of(tr), state_of(hand), (how, t))
            assert_mirror(tr, mir, (how, t))
            assert tr._steps == hand._steps == t + 1
        # the rotation: the eligible slots in cyclic order from the cursor, two at a time
        eligible = [g for g in alive if g // K in streams_on]
        rows = [g for g in got[4].tolist() if g >= 0]
        assert mir["counts"].tolist()[:3] == [len(eligible), min(2, len(eligible)), max(0, len(eligible) - 2)]
        assert set(rows) <= set(eligible) and len(rows) == min(2, len(eligible))
        served_all += rows
        # a served row's dt is its stream's plus its wait: the time since the slot was served last
        for r, g in enumerate(rows):
            if smooth:
                assert abs(mir["dt"][r] - (t - last_served[g]) / 30.0) < 1e-12, (t, g, mir["dt"][r])
            last_served[g] = t
        lost_rows += int((got[3][:len(rows)] != 0).sum())
        # whoever sat out -- live slots beyond the budget, dead slots, the slots of a stream that is off -- kept every bit
        after = state_of(host)
        sat_out = [g for g in range(CAP) if g not in rows]
        for name in after:
            assert same(after[name][sat_out], before[name][sat_out]), (name, t)
        if t == 0:                       # a detection in stream 1: a birth in its lowest free slot
            for tr in trackers:
                if best_shot:
                    tr.best_q[BORN] = 9.0                    # (more than any face reaches: only a reset lets one in)
                up = tr.update([None, [(50, 10, 90, 50)], None])
            assert up[2][1].tolist()[:2] == [0, 1] and int(up[0][1][0]) == BORN
            last_served[BORN] = 0
        elif best_shot and born_served is None:              # the birth's pending reset waits for the tick that serves it
            if BORN in rows:
                born_served = t
                assert int(host._best_reset[BORN]) == 0 and float(host.best_q[BORN]) != 9.0
            else:
                assert int(host._best_reset[BORN]) == 1 and float(host.best_q[BORN]) == 9.0
    assert set(SEEDED) <= set(served_all) and BORN in served_all          # nobody starves
    assert born_served is not None or not best_shot
    assert lost_rows > 0                                     # a track was lost on the way: it is no row from then on
    print(source, smooth, best_shot, "served:", served_all, "rows lost:", lost_rows, "status:", host.status.tolist())


@pytest.mark.parametrize("best_shot", [None, True])
@pytest.mark.parametrize("smooth", [None, True])
def test_one_stream_mixed_with_step_and_step_active(mods, rings, model, smooth, best_shot):
    """(d): streams=1; `step_live` below capacity, `step`, `step_active` and `step_live` again: a slot that waited and is
    then served by `step` or `step_active` has waited no longer."""
    L, A, P = mods
    ring, ff = rings["nv12"]
    hand, two = [make_tracker(mods, model, ff, smooth, best_shot, streams=1, capacity=4) for _ in range(2)]
    for tr in (hand, two):
        tr.seed([0, 2, 3], FACES[:3])
    mir = new_mirror(hand)
    dt = dict(dt=0.05) if smooth else {}
    for t, (how, fi) in enumerate((("live", 1), ("step", 0), ("live", 5), ("active", 2), ("live", 7), ("live", 3))):
        budget = 4 if t == 5 else 2
        if how == "live":
            exp = hand_tick(mods, hand, mir, model, ring, ff, [fi], budget, None, [0.05], hand._steps)
            got = two.step_live(ring, fi if t else [fi], budget, **dt)
            assert_mirror(two, mir, t)
        elif how == "step":
            exp, got = hand.step(ring, fi, **dt), two.step(ring, fi, **dt)
        else:
            exp, got = hand.step_active(ring, fi, [0], **dt), two.step_active(ring, fi, [0], **dt)
        for a, b in zip(got, exp):
            assert same(a, b), (t, how)
        assert_state(state_of(two), state_of(hand), (t, how))
        if smooth and how != "live":                         # every slot was served: nobody has waited
            assert not two.slot_age.any()
            mir["age"][:] = 0.0
        elif smooth and t == 0:
            assert float(two.slot_age[3]) == 0.05 and not two.slot_age[:3].any()         # three live, two served: slot 3 waits
    assert two._steps == hand._steps == 6
