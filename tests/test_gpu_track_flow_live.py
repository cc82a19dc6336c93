"""FaceTracker.step_flow_live on the GPU, in the configuration of tests/test_gpu_track_flow.py (its fixtures and helpers
are used as they are): 2 streams x 2 slots, bf16 fcn_8 at 64x64 with synthetic weights, the translated 1080p ring.
`step_live` then `step_flow_live` give, at each row's slot, the bits `step` then `step_flow` give on a twin tracker, with
each of smooth, weights="score", best_shot and pose and with all of them; an empty slot, a slot born by `update`, a slot
the key tick's budget left out, a lost track and an inactive stream are no rows and keep every bit; on the translated ring
the landmarks move by the frame's shift; and the existing calls keep their bits and their host rule."""
import numpy as np
import pytest
import torch

import flow_ref
import test_gpu_track_flow as base
from test_gpu_track_flow import frames, mods, model, ring  # noqa: F401  (fixtures)
from test_gpu_track_flow import CAP, CONFIGS, LARGE, RH, RW, SHIFT, SMALL, same

pytestmark = pytest.mark.gpu
SMALL4 = SMALL + [(1200, 700, 1328, 828)]                     # a face for slot 3 too
LARGE4 = LARGE + [(1136, 636, 1392, 892)]
STATE = tuple(k for k in base.STATE if k != "frame_slots") + ("flow_frame", "flow_ready")   # (step_live keeps frame_slots)
OWN = ("slot_age", "misses", "_best_reset")                   # what else the tracker keeps per slot


def state_of(tr, names=STATE):
    return {k: getattr(tr, k).clone() for k in names if getattr(tr, k, None) is not None}


def pin_slots(A, tr, boxes, slots):
    """base.pin for some slots alone: the crops of the next tick set by hand, behind the tracker's back (so the history
    rule does not see it, as a crop the track step placed)."""
    m, b, st = base.seeded(A, boxes)
    idx = torch.tensor(slots, device="cuda")
    tr.m_crop[idx] = m[:len(slots)]
    tr.boxes[idx] = b[:len(slots)]
    tr.status[idx] = st[:len(slots)]


def rows_equal_twin(name, res, twin_res, tr, twin, before=None):
    """Every returned tensor at a served row equals the twin's at the row's slot, and so does the state there."""
    slots = res[4].cpu().tolist()
    served = [(r, g) for r, g in enumerate(slots) if g >= 0]
    for i, (a, b) in enumerate(zip(res[:4], twin_res)):
        for r, g in served:
            assert same(a[r], b[g]), (name, "result", i, r, g)
    at = torch.tensor([g for _, g in served], device="cuda")
    mine, theirs = state_of(tr), state_of(twin)
    assert set(mine) == set(theirs)
    kept = at[tr.flow_ready[at] == 1]                          # a row that was lost keeps the history it had: the put
    for k in mine:                                             # moves only rows served with status 0
        where = kept if k in ("_flow_lm", "_flow_w") else at
        assert same(mine[k][where], theirs[k][where]), (name, "state", k)
    for r, g in enumerate(slots):                              # the rows past the served ones are inert
        if g < 0:
            assert int(res[3][r]) != 0 and (res[2][r] == -1.0).all() and (tr.flow_flags[r] == 1).all()
    return served


@pytest.mark.parametrize("name", list(CONFIGS))
def test_live_key_tick_then_live_flow_tick_equal_step_then_step_flow(mods, model, ring, name):   # (a)
    _, A, P = mods
    kw = CONFIGS[name]
    flow = A.LandmarkFlow(levels=3)
    tr, twin = base.make(P, model, flow=flow, **kw), base.make(P, model, flow=flow, **kw)
    for t in (tr, twin):
        t.seed(list(range(CAP)), SMALL4)
    dt = dict(dt=0.04) if "smooth" in kw else {}
    key, key_twin = tr.step_live(ring, [0, 0], CAP, **dt), twin.step(ring, [0, 0], **dt)
    assert key[4].cpu().tolist() == list(range(CAP))           # every slot is live: row r is slot r
    rows_equal_twin(name, key, key_twin, tr, twin)
    assert torch.equal(tr.flow_ready.bool(), tr.status == 0) and torch.equal(twin.flow_ready.bool(), twin.status == 0)
    assert int(tr.flow_ready.sum()) >= 3, tr.status            # the comparison below is of live tracks
    lost = (tr.status != 0).cpu().tolist()                     # a track the key tick lost is no row; the twin carries it
    for t in (tr, twin):
        base.pin(A, t, LARGE4)
    on_dev = torch.tensor([1, 1], dtype=torch.int32).cuda()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")                    # nothing goes up or comes down in a flow tick
    try:
        res = tr.step_flow_live(ring, on_dev, CAP, **dt)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    want = twin.step_flow(ring, [1, 1], **dt)
    served = rows_equal_twin(name, res, want, tr, twin)
    assert [g for _, g in served] == [g for g in range(CAP) if not lost[g]]
    n = len(served)
    assert same(tr.flow_flags[:n], twin.flow_flags[[g for _, g in served]]) and same(tr.flow_err[:n], twin.flow_err[[g for _, g in served]])
    assert (tr.flow_fb == -1.0).all() and tuple(tr.flow_flags.shape) == (CAP, 68)
    assert int((tr.flow_flags[:n] == 0).sum()) > 68            # the tick carried landmarks, not only rejections
    assert tr.flow_counts.cpu().tolist()[:5] == [CAP, n, n, 0, CAP - n]   # (the pin gave a lost slot a box, not a history)
    with pytest.raises(ValueError, match="may follow only step or step_flow"):   # step_flow's own host rule stays
        tr.step_flow(ring, [2, 2], **dt)


def test_an_empty_slot_is_no_row_and_keeps_every_bit(mods, model, ring):      # (b)
    _, A, P = mods
    kw = CONFIGS["all"]
    flow = A.LandmarkFlow(levels=3)
    tr, twin = base.make(P, model, flow=flow, **kw), base.make(P, model, flow=flow, **kw)
    for t in (tr, twin):
        t.seed(list(range(3)), SMALL)
    tr.step_live(ring, [0, 0], 3, dt=0.04)
    twin.step(ring, [0, 0], dt=0.04)
    for t in (tr, twin):
        base.pin(A, t, LARGE)
    before = state_of(tr, STATE + OWN)
    res = tr.step_flow_live(ring, [1, 1], 3, dt=0.04)
    want = twin.step_flow(ring, [1, 1], dt=0.04)
    served = rows_equal_twin("empty", res, want, tr, twin)
    assert 3 not in [g for _, g in served] and len(served) >= 2
    for k, v in state_of(tr, STATE + OWN).items():
        if v.dim() and v.shape[0] == CAP:
            assert same(v[3], before[k][3]), k


def test_a_birth_between_the_ticks_is_no_row_until_the_next_key_tick(mods, model, ring):   # (c)
    _, A, P = mods
    tr = base.make(P, model, flow=A.LandmarkFlow(levels=3), smooth=True, best_shot=True)
    tr.seed(list(range(3)), SMALL)
    tr.step_live(ring, [0, 0], CAP, dt=0.04)
    ready = tr.flow_ready.clone()
    pin_slots(A, tr, LARGE, [0, 1, 2])
    m2 = tr.m_crop[2].clone()
    tr.flow_ready[3] = 1                                       # (as if the slot had held a track with a history)
    tr.update([None, [list(SMALL4[3])]])                       # stream 1: a detection no track overlaps -> born in slot 3
    assert same(tr.m_crop[2], m2)
    assert not tr.boxes[3].eq(0).all() and int(tr.flow_ready[3]) == 0
    assert torch.equal(tr.flow_ready[:3], ready[:3])          # an update that writes no matrix takes no history away
    before = state_of(tr, STATE + OWN)
    res = tr.step_flow_live(ring, [1, 1], CAP, dt=0.04)
    slots = res[4].cpu().tolist()
    counts = tr.flow_counts.cpu().tolist()
    assert 3 not in slots and counts[4] == 1 and counts[0] == counts[1] + 1 and counts[2] == counts[1] >= 2, (slots, counts)
    for k, v in state_of(tr, STATE + OWN).items():
        if v.dim() and v.shape[0] == CAP and k != "slot_age":
            assert same(v[3], before[k][3]), k
    assert float(tr.slot_age[3]) == 0.04                       # it waited one tick: its first dt says so
    nxt = tr.step_live(ring, [2, 2], CAP, dt=0.04)
    assert 3 in nxt[4].cpu().tolist() and float(tr.slot_age[3]) == 0.0
    assert int(tr.flow_ready[3]) == int(tr.status[3] == 0)


def test_a_slot_the_key_ticks_budget_left_out_is_not_flowed(mods, model, ring):            # (d)
    _, A, P = mods
    tr = base.make(P, model, flow=A.LandmarkFlow(levels=3))
    tr.seed(list(range(3)), SMALL)
    key = tr.step_live(ring, [0, 0], 2)
    assert key[4].cpu().tolist() == [0, 1] and int(tr.flow_ready[2]) == 0
    lost = int((key[3] != 0).sum())                            # (the pin below gives a lost slot a box, not a history)
    base.pin(A, tr, LARGE)
    before = state_of(tr)
    res = tr.step_flow_live(ring, [1, 1], CAP)
    slots, counts = res[4].cpu().tolist(), tr.flow_counts.cpu().tolist()
    assert 2 not in slots and set(g for g in slots if g >= 0) <= {0, 1} and counts[4] == 1 + lost, (slots, counts)
    for k, v in state_of(tr).items():
        assert same(v[2], before[k][2]), k
    # the other way round: a slot with a history that the FLOW tick's budget leaves out loses it
    tr2 = base.make(P, model, flow=A.LandmarkFlow(levels=3))
    tr2.seed(list(range(3)), SMALL)
    tr2.step_live(ring, [0, 0], CAP)
    had = tr2.flow_ready.clone()
    base.pin(A, tr2, LARGE)
    res = tr2.step_flow_live(ring, [1, 1], 1)
    g = int(res[4][0])
    others = [s for s in range(CAP) if s != g]
    assert g >= 0 and int(tr2.flow_ready[others].sum()) == 0 and int(had.sum()) >= 2
    assert tr2.flow_counts.cpu().tolist()[1:4] == [int(had.sum()), 1, int(had.sum()) - 1]


def test_a_track_the_key_tick_lost_is_not_flowed(mods, model, ring):                       # (e)
    _, A, P = mods
    tr = base.make(P, model, flow=A.LandmarkFlow(levels=3), max_side=1.0)    # every face is larger: TRACK_SCALE
    tr.seed(list(range(3)), SMALL)
    key = tr.step_live(ring, [0, 0], CAP)
    assert (key[3][:3] != 0).all() and int(tr.flow_ready.sum()) == 0
    res = tr.step_flow_live(ring, [1, 1], CAP)
    assert (res[4] == -1).all() and tr.flow_counts.cpu().tolist()[:5] == [0, 0, 0, 0, 0]


def test_an_inactive_stream_is_not_touched_and_flows_on_its_next_tick(mods, model, ring):   # (f)
    _, A, P = mods
    tr = base.make(P, model, flow=A.LandmarkFlow(levels=3), smooth=True, best_shot=True)
    tr.seed(list(range(3)), SMALL)
    tr.step_live(ring, [0, 0], CAP, dt=0.04)
    base.pin(A, tr, LARGE)
    assert int(tr.flow_ready[2]) == 1 and int(tr.flow_frame[2]) == 0, tr.status
    before = state_of(tr, STATE + OWN)
    res = tr.step_flow_live(ring, [1, None], CAP, active=[0], dt=0.04)
    assert set(g for g in res[4].cpu().tolist() if g >= 0) <= {0, 1}
    for k, v in state_of(tr, STATE + OWN).items():
        if v.dim() and v.shape[0] == CAP:
            assert same(v[2:], before[k][2:]), k
    res = tr.step_flow_live(ring, [None, 1], CAP, active=torch.tensor([0, 1], dtype=torch.int32).cuda(), dt=[0.04, 0.08])
    assert res[4].cpu().tolist()[0] == 2                       # flowed from its own previous frame, ring slot 0, to slot 1
    assert int(tr.flow_frame[2]) == 1 or int(tr.status[2]) != 0
    assert int((tr.flow_flags[0] == 0).sum()) > 34


def test_flow_landmarks_move_with_the_frame(mods, model, ring):                             # (g)
    """`step` then `step_flow_live` on the translated ring: the assertion of the translation test of
    tests/test_gpu_track_flow.py, on rows."""
    _, A, P = mods
    flow = A.LandmarkFlow(levels=3, max_fb=1.0)
    tr = base.make(P, model, flow=flow)
    tr.seed(list(range(3)), SMALL)
    tr.step(ring, [0, 0])
    base.pin(A, tr, LARGE)
    m = tr.m_crop.cpu().numpy().astype(np.float64)
    lm_prev = tr._flow_lm.cpu().numpy()
    res = tr.step_flow_live(ring, [1, 1], CAP)
    slots = np.asarray(res[4].cpu().tolist())
    rows = np.flatnonzero(slots >= 0)
    faces = slots[rows]
    assert len(rows) >= 2 and 3 not in faces
    lm_now, flags = res[2].cpu().numpy()[rows], tr.flow_flags.cpu().numpy()[rows]
    live = (lm_prev[faces] >= 0).all(axis=2)
    rejected = live & (flags != 0)
    share = rejected.sum() / live.sum()
    scale = np.sqrt(m[faces, 0, 0] ** 2 + m[faces, 1, 0] ** 2)
    tol = 0.1 / scale
    ok = live & ~rejected
    move = lm_now - lm_prev[faces]
    worst = (np.abs(move - np.asarray(SHIFT, np.float64))[ok].reshape(-1, 2) / np.repeat(tol, ok.sum(axis=1))[:, None]).max()
    fb = tr.flow_fb.cpu().numpy()[rows]
    print("live", int(live.sum()), "rejected", int(rejected.sum()), "by the round trip alone", int((flags == 64).sum()),
          "worst error / tolerance", worst, "largest accepted round trip, px", float(np.sqrt(fb[ok].max())))
    assert live.sum() >= 68 * 2 and share < 0.1, (live.sum(), share)
    assert worst <= 1.0, worst
    assert (fb[ok] >= 0).all() and (fb[ok] <= 1.0).all()


def test_step_flow_keeps_its_bits_and_takes_the_check(mods, model, ring):                   # (h)
    """`step_flow` with max_fb=None still equals the chain by hand (flm_landmark_flow); with max_fb it runs the rows
    kernel with slot[r] = r: the flags other than FB and the landmarks FB leaves are those without the check."""
    _, A, P = mods
    kw = CONFIGS["all"]
    tr = base.make(P, model, flow=A.LandmarkFlow(levels=3), **kw)
    chk = base.make(P, model, flow=A.LandmarkFlow(levels=3, max_fb=1.0), **kw)
    for t in (tr, chk):
        t.seed(list(range(3)), SMALL)
        t.step(ring, [0, 0], dt=0.04)
        base.pin(A, t, LARGE)
    want, state, raw = base.flow_tick_by_hand(A, tr, ring, [1, 1], 1, 0.04)
    res = tr.step_flow(ring, [1, 1], dt=0.04)
    for i, (a, b) in enumerate(zip(res, want)):
        assert same(a, b), i
    for k, v in state.items():
        assert same(getattr(tr, k), v), k
    assert same(tr.flow_flags, raw[3]) and same(tr.flow_err, raw[2]) and (tr.flow_fb == -1.0).all()
    ok = tr.status == 0
    assert torch.equal(tr.flow_ready.bool(), ok) and same(tr.flow_frame[ok], tr.frame_slots[ok]) and int(ok.sum()) >= 2
    chk.step_flow(ring, [1, 1], dt=0.04)
    assert torch.equal(chk.flow_flags & ~64, tr.flow_flags) and same(chk.flow_err, tr.flow_err)
    ran = (chk.flow_fb >= 0) | ((chk.flow_flags == 64) & (chk.flow_fb == -1.0))    # (or did not finish: NOT_FINITE)
    assert torch.equal(ran, tr.flow_flags == 0)
    keep = (chk.flow_flags & 64) == 0
    assert same(chk._flow_crop_lm[keep], tr._flow_crop_lm[keep])


def test_host_rules(mods, model, ring):                                                      # (i)
    _, A, P = mods
    plain = base.make(P, model)
    plain.seed([0], SMALL[:1])
    with pytest.raises(ValueError, match="step_flow_live needs a tracker made with flow"):
        plain.step_flow_live(ring, [0, 0], 2)
    plain.step_live(ring, [0, 0], 2)
    assert not hasattr(plain, "flow_ready") and not hasattr(plain, "flow_counts")    # without flow nothing more is allocated
    tr = base.make(P, model, flow=A.LandmarkFlow(levels=3), best_shot=True, exits=4)
    res = tr.step_flow_live(ring, [0, 0], 2)                   # may follow any call: a new tracker has nobody to serve
    assert (res[4] == -1).all() and tr._steps == 1             # and counts as a step
    tr.seed([0, 2], [SMALL[0], SMALL[2]])
    tr.step(ring, [0, 0])
    assert tr.flow_ready.cpu().tolist() == [int(v == 0) for v in tr.status.cpu().tolist()]
    tr.seed([2], SMALL[2:])
    assert int(tr.flow_ready[2]) == 0                          # a seed writes the crop matrix
    tr.step(ring, [0, 0])
    tr.retire(flush=True)
    assert int(tr.flow_ready.sum()) == 0
