"""The row forms of prediction.FaceTracker -- `step_live`, `step_flow_live`, `step_active` -- in closed loop on the GPU against
the rendered ground truth of tests/scenario.py, all options on: weights="score", best_shot, pose, views, exits, mesh and
flow, 2 streams x 4 slots, samples=1, TICKS ticks on the tracker's own output, `update` on every KEY-th tick.

The landmark model is scenario.RowTruthSource (the truth of every row's slot through the snapshot's matrix of that row), so
the gather, the rows step, the filter and its waits, the pending best-shot resets, the history rule, the retire call, pose,
both warps, best shots and views run as shipped.  The expectations are the `check_*` functions of tests/scenario.py;
tests/test_scenario_host.py shows on the CPU, with the numpy references in the device's place, that the references alone
keep every track under each schedule and that a swapped row map, a row written to another slot, a wait dropped from dt, a
pending reset used up for an unserved slot and a history kept for a slot the budget left out each fail one of them.

The schedules (scenario.SCHEDULES; the final ones -- none had to be changed for the reference-alone condition):
  L-full    `step_live(budget=CAP)` on the detector's ticks, `step_flow_live(budget=CAP)` between, every stream, then
            `retire(flush=True)`.  Tracker A of tests/test_gpu_scenario.py runs beside it on `step` / `step_flow`, and every
            served row, the state of every slot and everything handed out at the end equal A's BIT FOR BIT, but for the
            differences the docstrings state (ALLOWED below): the `status` of a slot that is no row keeps its reason
            where `step` writes TRACK_DEAD, `frame_slots` is not maintained, and -- the same rule, stated in the class
            docstring -- the `pose` of a slot that is no row keeps its bits where `step` writes the not-ok record.  The
            private flow history (`_flow_lm`, `_flow_w`) is compared at the slots served with status 0: `step` writes
            it for every slot, the rows for the ones whose `flow_ready` they set.
  L-budget  `step_live(budget=3)` at every tick: four faces are live for most of the script, so every tick leaves one
            out, every slot waits one tick in four and is then cut by a crop that is two ticks old.  Against truth
            (check_truth, with the landmark bound derived on the CPU from the reference's lagged crop matrix), the
            rotation, `live_counts` against tests/track_live_ref.py, every bit of an unserved slot, the history rule;
            a second tracker with smooth=True equals tests/track_filter_ref.py bit for bit under each slot's own dt.
            The budget leaves P2 out at its scripted exit, tick 12: it is dropped at tick 13 and queued at tick 14.  P1
            moves left by 4 px a tick: a crop two ticks old puts a jaw point or two left of its first column, where
            the step rejects them; the reference says which (5 points of the run), and exactly those come back (-1,-1).
  L-clock   `step_active`, stream 0 at every tick, stream 1 at every second one.  Against truth as L-budget; the slots of
            stream 1 keep every bit across the ticks it sits out (gallery, views, pending resets, exit state; the retire
            call runs over all slots, so P2's exit is queued at tick 13, a tick of stream 0 alone: once, with that tick's
            frame id, the tick after the one whose row returned TRACK_OUTSIDE).

Measured on an MI355X (each test prints its figures): L-full: 125 rows, 93 of them flow rows, every bit tracker A's; 4 rows
served per tick (3 while slot 5 is empty); the state differs in `status` and `pose` of the slots that are no row, nowhere
else.  L-budget: landmarks 1.71e-13 px, 0.173 of the lagged-crop bound (at most 1.97e-12); both fits 0.787 of the float32
bound; the worst aligned and the worst mesh pixel 0.896 of B_align; head pose 3.21e-15 rad against 1.91e-12; 3 rows served
at every tick, the longest wait 1 tick; 5 truth points outside a lagged crop, each rejected; with smooth=True 12328
coordinates moved by the filter, every bit the reference's, the rows' dt one or two ticks.  L-clock: landmarks 1.71e-13 px,
0.118 of the bound; fits 0.765; aligned and mesh 0.896 of B_align; head pose 3.21e-15 rad; stream 1 sat out 16 ticks; P2
dropped at tick 12 and queued with frame id 13."""
import numpy as np
import pytest
import torch

import scenario as sc
import track_ref

pytestmark = pytest.mark.gpu
Q = 16
OUTSIDE = track_ref.OUTSIDE

# the per-slot state of a tracker with every option, by attribute; smoothing adds SMOOTH
STATE = ("m_crop", "boxes", "status", "misses", "gallery", "best_q", "best_frame", "best_M", "best_landmarks", "best_rec",
         "_best_reset", "pose", "track_id", "born_frame", "_born", "_exit_stale", "exit_row", "view_gallery", "view_q",
         "view_frame", "view_M", "view_landmarks", "view_pose", "flow_frame", "flow_ready", "_flow_lm", "_flow_w")
SMOOTH = ("filter_state", "slot_age")
OTHER = ("live_cursor", "flow_cursor", "exit_head", "exit_meta", "frame_slots")
RENAMED = {"_best_reset": "best_reset"}                       # the names scenario.RowsReference uses
# L-full: where a tracker on the row forms may differ from tracker A, as the docstrings of step_live state
ALLOWED = ("status of a slot that is no row: it keeps its reason where step writes TRACK_DEAD",
           "frame_slots: not maintained by the row forms",
           "pose of a slot that is no row: it keeps its bits where step writes the not-ok record (the class docstring)")
HISTORY = ("_flow_lm", "_flow_w")                             # private: step overwrites the empty slots' rows


@pytest.fixture(scope="module")
def mods():
    import flm_amd  # noqa: F401
    from flm_amd import _lib, alignment, prediction
    _lib.load()
    return _lib, alignment, prediction


@pytest.fixture(scope="module")
def S():
    return sc.Script()


@pytest.fixture(scope="module")
def ring(S):
    return torch.from_numpy(S.frames()).cuda()


def options(A):
    return dict(weights="score", best_shot=A.BestShot(sharp_ref=sc.SHARP_REF), pose=True,
                views=A.PoseViews(sharp_ref=sc.SHARP_REF), exits=Q, mesh=True, flow=True)


def make(P, S, source, **kw):
    tr = P.FaceTracker(source, (sc.FH, sc.FW), sc.CAP, out_size=(sc.OUT, sc.OUT), streams=sc.STREAMS, samples=1, **kw)
    source.bind(tr)
    return tr


def state(tr):
    names = STATE + OTHER + (SMOOTH if tr.smooth is not None else ())
    return {RENAMED.get(n, n): getattr(tr, n).clone() for n in names}


def host(x):
    if isinstance(x, torch.Tensor):
        return x.detach().cpu().numpy()
    if isinstance(x, dict):
        return {k: host(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)) and x and isinstance(x[0], torch.Tensor):
        return [host(v) for v in x]
    return x


def rows_tick(tr, src, S, ring, t, schedule):
    """`update` on a detector's tick, then the schedule's row call: one record in the format of scenario.check_*."""
    call, on, budget = schedule(t)
    src.tick = t
    rec = dict(t=t, call=call, on=list(on), budget=budget)
    if S.is_key(t):
        det, who = S.detections(t)
        rec["det_dev"], rec["det_n"] = tr.update(det)[0].clone(), [len(w) for w in who]
    rec["pre"] = state(tr)
    fi = [S.ring_slot(s, t) if s in on else None for s in range(sc.STREAMS)]
    if call == "live":
        res = tr.step_live(ring, fi, budget, frame_id=t)
        rec["counts"] = tr.live_counts.clone()
    elif call == "flow":
        res = tr.step_flow_live(ring, fi, budget, frame_id=t)
        rec["counts"] = tr.flow_counts.clone()
        rec["flags"], rec["w"], rec["sent"] = tr.flow_flags.clone(), tr._flow_crop_w[:budget].clone(), tr._flow_crop_lm[:budget].clone()
    else:
        res = tr.step_active(ring, fi, on, frame_id=t)
    rec.update(aligned=res[0].clone(), M=res[1].clone(), lm=res[2].clone(), status_rows=res[3].clone(), slot=res[4].clone(),
               mesh=tr.mesh_faces.clone(), post=state(tr))
    if call != "flow":
        slot, rec["m_c"], rec["sent"], rec["dt_c"] = src.rows[t]
        rec["slot_seen"] = slot
    return rec


def finish(rec):
    """A record on the host; what the checkers want beside the tensors."""
    rec = {k: host(v) for k, v in rec.items()}
    if "det_dev" in rec:
        rec["det_slot"] = [rec["det_dev"][s][:n].tolist() for s, n in enumerate(rec["det_n"])]
    n = len(rec["slot"])
    if rec["call"] != "flow":
        assert np.array_equal(rec["slot_seen"], rec["slot"])          # the snapshot the model saw is the one returned
        rec["w"] = np.ones((n, sc.C))
    inert = rec["slot"] < 0
    rec["boxes_c"] = np.where(inert[:, None], 0, rec["pre"]["boxes"][np.clip(rec["slot"], 0, sc.CAP - 1)]).astype(np.int32)
    return rec


def run_rows(P, A, S, ring, name, truth=None, **kw):
    src = sc.RowTruthSource(S, truth=truth)
    tr = make(P, S, src, **options(A), **kw)
    out = [rows_tick(tr, src, S, ring, t, sc.SCHEDULES[name]) for t in range(sc.TICKS)]
    torch.cuda.synchronize()
    return tr, [finish(rec) for rec in out]


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def common_checks(rec):
    sc.check_row_map(rec)
    sc.check_rows_written(rec)
    sc.check_untouched(rec)
    sc.check_flow_ready(rec)


def exit_of_p2(S, records):
    """P2's exit is queued once: by the tick after the one whose row returned TRACK_OUTSIDE, with that tick's frame id."""
    ids = S.track_ids()
    p2 = [f for f in S.faces if f.name == "P2"][0]
    (dropped,) = [rec["t"] for rec in records for r, g in sc.served(rec).items() if rec["status_rows"][r] == OUTSIDE]
    for rec in records:
        head = rec["post"]["exit_head"].tolist()
        want = [int(rec["t"] > dropped), sum(1 for f in S.faces if f.first <= rec["t"]), 0, 0]
        assert head == want, (rec["t"], head, want)
    meta = records[-1]["post"]["exit_meta"][0].tolist()
    assert meta[:4] == [ids["P2"], p2.global_slot, p2.first, dropped + 1] and meta[5:] == [OUTSIDE, 0, 0], meta
    return dropped, meta


# ---- L-full ---------------------------------------------------------------------------------------------------------------
def test_l_full_equals_tracker_a_bit_for_bit(mods, S, ring):
    _, A, P = mods
    src_a, src_l = sc.TruthSource(S), sc.RowTruthSource(S)
    ta, tl = make(P, S, src_a, **options(A)), make(P, S, src_l, **options(A))
    ticks = []
    for t in range(sc.TICKS):
        src_a.tick = t
        slots = [S.ring_slot(s, t) for s in range(sc.STREAMS)]
        if S.is_key(t):
            ta.update(S.detections(t)[0])
        res = (ta.step if S.is_key(t) else ta.step_flow)(ring, slots, frame_id=t)
        a = dict(aligned=res[0].clone(), M=res[1].clone(), lm=res[2].clone(), status=res[3].clone(), mesh=ta.mesh_faces.clone(),
                 flags=ta.flow_flags.clone(), post=state(ta))
        ticks.append((a, rows_tick(tl, src_l, S, ring, t, sc.schedule_full)))
    end = []
    for tr in (ta, tl):
        tr.retire(flush=True, frame_id=sc.TICKS)
        end.append(dict(best=list(tr.best()), views=list(tr.views()), exits=list(tr.exits()), exit_views=list(tr.exit_views()),
                        track_id=tr.track_id, exit_rec=tr.exit_rec, born_frame=tr.born_frame))
    torch.cuda.synchronize()
    end = [{k: host(v) for k, v in e.items()} for e in end]
    rows_served, n_rows, n_flow, differing = [], 0, 0, set()
    for a, rec in ticks:
        a, rec = host(a), finish(rec)
        t, key = rec["t"], S.is_key(rec["t"])
        common_checks(rec)
        # the served slots: exactly the ones that hold a face -- on a flow tick, a face with a history: the same ones
        holds = [g for g in range(sc.CAP) if S.face_in(g, t) is not None]
        got = sorted(sc.served(rec).values())
        assert got == holds, (t, got, holds)
        if key:
            assert rec["counts"].tolist()[:3] == [len(holds), len(holds), 0], (t, rec["counts"])
        else:
            assert rec["counts"].tolist()[:5] == [len(holds), len(holds), len(holds), 0, 0], (t, rec["counts"])
            assert all(rec["pre"]["flow_ready"][g] == 1 for g in holds), t
            n_flow += len(holds)
        rows_served.append(len(got))
        for r in range(len(rec["slot"])):
            g = int(rec["slot"][r])
            if g < 0:
                assert rec["status_rows"][r] == track_ref.DEAD and not rec["aligned"][r].any() and not rec["mesh"][r].any(), (t, r)
                assert (rec["lm"][r] == -1.0).all() and same(rec["M"][r], track_ref.IDENTITY), (t, r)
                continue
            n_rows += 1
            for name, mine, theirs in (("aligned", rec["aligned"][r], a["aligned"][g]), ("M", rec["M"][r], a["M"][g]),
                                       ("landmarks", rec["lm"][r], a["lm"][g]), ("status", rec["status_rows"][r], a["status"][g]),
                                       ("mesh", rec["mesh"][r], a["mesh"][g])) + (
                                           () if key else (("flow_flags", rec["flags"][r], a["flags"][g]),)):
                assert same(np.asarray(mine), np.asarray(theirs)), (t, g, name)
            for name in HISTORY if rec["status_rows"][r] == 0 else ():          # (a row that lost its track leaves no history)
                assert same(rec["post"][name][g], a["post"][name][g]), (t, g, name)
        # everything else, slot by slot: no difference but those of ALLOWED
        rows = set(got)
        for name, mine in rec["post"].items():
            theirs = a["post"][name]
            if name in HISTORY or name in ("live_cursor", "flow_cursor"):
                continue
            if name == "frame_slots":                                   # ALLOWED[1]
                assert not mine.any() and theirs.tolist() == [S.ring_slot(g // sc.SLOTS, t) for g in range(sc.CAP)], t
                continue
            if mine.ndim == 0 or mine.shape[0] != sc.CAP:
                assert same(mine, theirs), (t, name)
                continue
            for g in range(sc.CAP):
                if same(mine[g], theirs[g]):
                    continue
                differing.add(name)
                assert name in ("status", "pose") and g not in rows, \
                    "L-full differs from tracker A in %s of slot %d at tick %d" % (name, g, t)
                assert same(mine[g], rec["pre"][name][g]), (t, g, name)      # kept, where step writes the record of no face
                assert theirs[g] & track_ref.DEAD if name == "status" else theirs[g][14] == 0.0, (t, g, name, theirs[g])
        for g in rows:                                                  # pose, ids and history at the served slots, by name
            for name in ("pose", "track_id"):
                assert same(rec["post"][name][g], a["post"][name][g]), (t, g, name)
    assert "status" in differing and differing <= {"status", "pose"}, differing    # (the kept reason shows: P2's TRACK_OUTSIDE)
    ea, el = end
    for name in ea:
        if isinstance(ea[name], list):
            for i, (x, y) in enumerate(zip(ea[name], el[name])):
                assert same(x, y), (name, i)
        else:
            assert same(ea[name], el[name]), name
    assert (el["track_id"] == -1).all() and el["exits"][5].tolist() == [len(S.faces), len(S.faces), 0, 0]
    print("L-full: %d rows (%d of them flow rows) equal tracker A bit for bit; rows served per tick %s; state differs in %s alone"
          % (n_rows, n_flow, rows_served, sorted(differing)))
    assert n_flow >= 80 and n_rows >= 120 and len(ALLOWED) == 3


# ---- L-budget and L-clock ---------------------------------------------------------------------------------------------------
def against_truth(S, tr, records, ref):
    worst, ids = {}, S.track_ids()
    seen = sc.check_lifetimes(S, records)
    for rec, rref in zip(records, ref):
        common_checks(rec)
        sc.check_truth(S, rec, rref, worst, mesh=tr.mesh, ids=ids)
    assert ids == {"P0": 0, "P1": 1, "H": 2, "P2": 3, "P3": 4}          # the reborn slot got the next id
    return worst, seen


def figures(name, worst, extra):
    print("%s: landmarks %.2e px, %.3f of the lagged-crop bound (largest bound %.2e); fits %.3f of the float32 bound; aligned "
          "%.3f and mesh %.3f of B_align; head pose %.2e rad (bound %.2e); %s"
          % (name, worst["lm_px"], worst["lm"], worst["lm_bound"], worst["fit"], worst["aligned"], worst["mesh"], worst["pose"],
             worst["pose_tol"], extra))


def test_l_budget_follows_the_truth_and_rotates(mods, S, ring):
    _, A, P = mods
    ref = sc.RowsReference(S, sc.schedule_budget).run()
    tr, records = run_rows(P, A, S, ring, "budget", truth=S.truth(rendered=True))
    worst, seen = against_truth(S, tr, records, ref)
    longest, per_tick = sc.check_rotation(records)
    assert longest == 1 and set(per_tick) == {sc.BUDGET}
    dropped, meta = exit_of_p2(S, records)
    assert dropped == sc.P2_EXIT + 1                                    # left out at its scripted exit, dropped a tick later
    crossing = [rec["det_slot"][0] for rec in records if "det_slot" in rec]
    assert {tuple(c) for c in crossing} == {(0, 1), (1, 0)}             # the detections swap where the faces pass
    lost = sum(int((rec["lm"][r] < 0).all(1).sum()) for rec in records for r in sc.served(rec))
    figures("L-budget", worst, "rows served per tick %s; longest wait %d tick; served %s; %d truth points outside a lagged "
            "crop, each rejected" % (sorted(set(per_tick)), longest, {k: len(v) for k, v in seen.items()}, lost))


def test_l_budget_smooths_as_the_reference_under_each_slots_own_dt(mods, S, ring):
    _, A, P = mods
    tr, records = run_rows(P, A, S, ring, "budget", truth=S.truth(rendered=True), smooth=True)
    sc.check_lifetimes(S, records)
    for rec in records:
        common_checks(rec)
    longest, per_tick = sc.check_rotation(records)
    moved = sc.check_smoothing(S, records)
    dt = sc.filter_dt()
    waits = sorted({round(float(v) / dt) for rec in records for r, v in enumerate(rec["dt_c"]) if rec["slot"][r] >= 0})
    print("L-budget, smooth: %d coordinates moved by the filter, every bit the reference's; the rows' dt in ticks %s; longest "
          "wait %d tick" % (moved, waits, longest))
    assert moved > 1000 and waits == [1, 2] and longest == 1


def test_l_clock_follows_the_truth_and_leaves_the_idle_stream_alone(mods, S, ring):
    _, A, P = mods
    ref = sc.RowsReference(S, sc.schedule_clock).run()
    tr, records = run_rows(P, A, S, ring, "clock")
    worst, seen = against_truth(S, tr, records, ref)
    idle = 0
    for rec in records:                                                 # (check_untouched, by name for the idle stream)
        if rec["on"] == [0]:
            assert set(sc.served(rec).values()) == set(range(sc.SLOTS)), rec["t"]
            for name in ("gallery", "view_gallery", "view_q", "best_q", "best_reset", "_exit_stale", "m_crop", "boxes", "pose"):
                assert same(rec["pre"][name][sc.SLOTS:], rec["post"][name][sc.SLOTS:]), (rec["t"], name)
            idle += 1
    dropped, meta = exit_of_p2(S, records)
    p2 = [f for f in S.faces if f.name == "P2"][0]
    assert dropped == sc.P2_EXIT and meta[3] == sc.P2_EXIT + 1 and meta[4] == S.best_tick(p2)
    assert records[sc.P2_EXIT + 1]["on"] == [0]                         # queued by a tick that did not step its stream
    figures("L-clock", worst, "stream 1 sat out %d ticks; served %s; P2 dropped at tick %d, queued with frame id %d"
            % (idle, {k: len(v) for k, v in seen.items()}, dropped, meta[3]))
    assert idle == sc.TICKS // 2
