"""The scenario of tests/scenario.py has teeth: conditions on the scenario itself, checked on the CPU with the numpy
references, each printing its value.  tests/test_gpu_scenario.py relies on every one of them.

  * the aligned square of every face lies on its own texture, clear of every other face;
  * half-pixel shifts, an x/y swap, a transposed or inverted M and a B/R swap each move at least a quarter of the pixels of
    every aligned face by four times B_align or more;
  * the association reference pairs every track with its own detection by a clear margin of IoU, through the crossing;
  * the sharpest tick of every track, and of every pose bin of it, beats the runner-up by more than B_align can move a score;
  * the bare step of tests/track_ref.py, in closed loop over the truth, keeps every face until its scripted exit and drops
    it there with TRACK_OUTSIDE;
  * the flow reference, in closed loop on crops cut from the rendered frames, carries the landmarks with an error e_ref of
    at most a quarter of the smallest motion per tick.

And tests/test_gpu_scenario_rows.py, the row forms, on these:
  * scenario.rows_truth (RowTruthSource in numpy) under a full budget is scenario.slots_truth (TruthSource) exactly;
  * under each of the three row schedules the references alone (scenario.RowsReference) keep every track except P2 at its
    exit, and pass every checker of scenario.py the GPU module calls;
  * five faults of a row tick, each injected into that loop, each fail the checker named beside it."""
import math

import numpy as np
import pytest

import face_quality_ref
import flow_ref
import head_pose_ref
import mesh_ref
import scenario as sc
import stats_ref
import track_assoc_ref
import track_ref
import track_views_ref

VIEWS = sc.alignment.PoseViews()
IOU_MARGIN = 0.25


@pytest.fixture(scope="module")
def S():
    return sc.Script()


def live_ticks(S):
    return [(f, t) for f in S.faces for t in range(sc.TICKS) if f.live(t)]


# ---- geometry -----------------------------------------------------------------------------------------------------------
def test_every_aligned_square_lies_on_its_own_texture_alone(S):
    """The aligned square and one face px around it, seen from any OTHER face of the stream, lies outside that face's patch
    by at least a face px: no warp of a face ever taps another face or the patch's own edge."""
    g = np.arange(-1.0, sc.OUT + 0.01, 0.5)
    uu, vv = np.meshgrid(g, g)
    grid = np.stack([uu.ravel(), vv.ravel()], 1)
    assert sc.PATCH[0] <= -2.0 and sc.PATCH[1] >= sc.OUT + 1.0
    worst = np.inf
    for f, t in live_ticks(S):
        pts = sc.apply(f.pose(t), grid)
        for o in S.faces:
            if o is f or o.stream != f.stream or not o.rendered(t):
                continue
            q = sc.apply(sc.inverse(o.pose(t)), pts)
            out = np.maximum(np.maximum(sc.PATCH[0] - q, q - sc.PATCH[1]).max(1), 0.0)     # how far outside, face px
            worst = min(worst, float(out.min()))
    print("clearance of every aligned square from every other face: %.2f face px" % worst)
    assert worst >= 1.0


def test_head_landmarks_are_the_projected_model_and_cross_both_view_edges(S):
    head = [f for f in S.faces if f.name == "H"][0]
    idx, xyz = head_pose_ref.DEFAULT_INDICES, np.array(head_pose_ref.DEFAULT_POINTS)
    assert idx == sc.HEAD_INDICES and np.array_equal(xyz, sc.HEAD_POINTS)
    worst, bins, edge = 0.0, [], np.inf
    for t in range(sc.TICKS):
        rec = head_pose_ref.fit(head.landmarks(t)[None], None, idx, xyz)[0]
        assert rec[14] == 1.0
        worst = max(worst, float(np.abs(rec[15:18] - np.array(head.angles(t))).max()))
        bins.append(track_views_ref.bin_of(rec, VIEWS.u_edges, VIEWS.v_edges))
        yaw = head.angles(t)[0]
        assert bins[-1] == (0 if yaw < -math.radians(20) else 2 if yaw > math.radians(20) else 1)   # right, frontal, left
        edge = min(edge, min(abs(-rec[6] - e) for e in VIEWS.u_edges))
    print("head pose of the truth landmarks against the script: %.2e rad; bins %s; nearest u to an edge %.4f"
          % (worst, bins, edge))
    assert worst <= 1e-12 and set(bins) == {0, 1, 2} and edge >= 0.01


def test_the_float64_fit_is_the_one_the_similarity_reference_restates(S):
    worst = 0.0
    for f, t in live_ticks(S):
        for tmpl in (sc.TEMPLATE, sc.CROP_TEMPLATE):
            ref = stats_ref.weighted_similarity_ref(f.landmarks(t)[None], tmpl)[0]
            assert np.array_equal(ref, sc.matrix(sc.umeyama(f.landmarks(t), tmpl)).astype(np.float32)) or np.allclose(
                ref, sc.matrix(sc.umeyama(f.landmarks(t), tmpl)), rtol=2.0 ** -23, atol=0.0)
            if isinstance(f, sc.Planar):
                worst = max(worst, float(np.abs(sc.apply(sc.matrix(sc.umeyama(f.landmarks(t), tmpl)), f.landmarks(t)) - tmpl).max()))
    print("float64 fit of a planar face's truth landmarks against the template: %.2e px" % worst)
    assert worst <= 1e-10


# ---- the aligned-face bound ---------------------------------------------------------------------------------------------
def mutations(S, f, t):
    """The float64 aligned face under each fault, by name."""
    pose = f.pose(t)
    m = sc.inverse(pose)                                  # frame -> aligned: what the tracker's M_align is
    def shifted(du, dv):
        p = pose.copy()
        p[:, 2] = sc.apply(pose, [[du, dv]])[0]
        return S.aligned(f.stream, t, p)
    base = S.aligned(f.stream, t, pose)
    mt = m.copy()
    mt[:, :2] = m[:, :2].T
    return base, {
        "half a pixel in x": shifted(0.5, 0.0), "half a pixel in y": shifted(0.0, 0.5),
        "half a pixel in both": shifted(0.5, 0.5),
        "x and y swapped": base.transpose(1, 0, 2),
        "M transposed": S.aligned(f.stream, t, sc.inverse(mt)),
        "M inverted": S.aligned(f.stream, t, m),
        "B and R swapped": base[..., ::-1],
    }


def test_every_fault_moves_a_quarter_of_every_aligned_face_by_four_bounds(S):
    worst = {}
    for f, t in live_ticks(S):
        bound = sc.b_align(f.blur(t), f.scale(t))
        base, muts = mutations(S, f, t)
        for name, img in muts.items():
            share = float((np.abs(img - base).max(-1) >= 4.0 * bound).mean())
            if share < worst.get(name, (2.0,))[0]:
                worst[name] = (share, f.name, t, bound)
    for name, (share, who, t, bound) in worst.items():
        print("%-22s least share of pixels beyond 4 x B_align: %.3f (%s, tick %d, B_align %.3f)" % (name, share, who, t, bound))
    assert all(v[0] >= 0.25 for v in worst.values()), worst


def test_whole_faces_render_as_the_texture_itself(S):
    """Seen through its own pose a face that is whole is tex(u, v) at its blur: the expectation has no interpolation."""
    vv, uu = np.mgrid[0:sc.OUT, 0:sc.OUT].astype(np.float64)
    n = 0
    for f, t in live_ticks(S):
        if S.whole(f, t):
            assert np.abs(S.aligned(f.stream, t, f.pose(t)) - sc.tex(uu, vv, f.blur(t))).max() <= 1e-9
            n += 1
    assert n > 100


# ---- the closed loop on the references ------------------------------------------------------------------------------------
def crop_u8(frame, m):
    return np.clip(np.rint(mesh_ref.warp_affine_frame_ref(frame, m, sc.IN, sc.IN)), 0, 255).astype(np.uint8)


def closed_loop(S, use_flow):
    """The tracker's loop on the numpy references: track_assoc_ref at the detector's ticks, the truth through the current
    crop matrix (what scenario.TruthSource returns) into track_ref.step at those ticks and, with use_flow, flow_ref on
    crops of the rendered frames into track_ref.step on the ticks between (without it, the truth at every tick).  Returns
    one record per tick."""
    k = sc.CAP
    m_crop = np.broadcast_to(track_ref.IDENTITY, (k, 2, 3)).copy()
    boxes = np.zeros((k, 4), np.int32)
    status = np.full(k, track_ref.DEAD, np.int32)
    misses = np.zeros(k, np.int32)
    truth = S.truth()
    frames = S.frames() if use_flow else None
    prev_lm, out = None, []
    for t in range(sc.TICKS):
        rec = dict(t=t)
        if S.is_key(t):
            det, who = S.detections(t)
            rec["det_slot"], rec["iou"] = [], []
            for s in range(sc.STREAMS):
                lo, hi = s * sc.SLOTS, (s + 1) * sc.SLOTS
                before = boxes[lo:hi].copy()
                r = track_assoc_ref.associate(np.asarray(det[s], np.int32).reshape(-1, 4), None, m_crop[lo:hi], boxes[lo:hi],
                                              status[lo:hi], misses[lo:hi], None, sc.IN, sc.IN, sc.FH, sc.FW)
                m_crop[lo:hi], boxes[lo:hi], status[lo:hi], misses[lo:hi] = r["m_crop"], r["boxes"], r["status"], r["misses"]
                rec["det_slot"].append([int(v) + lo if v >= 0 else -1 for v in r["det_slot"]])
                dclip = [track_assoc_ref.clip(track_assoc_ref.square_box(b), sc.FH, sc.FW) for b in det[s]]
                for j, f in enumerate(who[s]):
                    tb = track_assoc_ref.clip(before[f.slot], sc.FH, sc.FW)
                    if track_assoc_ref.empty(tb):
                        continue                                        # a birth: no track to confuse it with
                    ious = []
                    for d in dclip:
                        i = track_assoc_ref.inter(tb, d)
                        ious.append(i / float(track_assoc_ref.area(tb) + track_assoc_ref.area(d) - i))
                    rec["iou"].append((f.name, ious[j], max([v for n, v in enumerate(ious) if n != j] + [0.0])))
        key = S.is_key(t) or not use_flow
        if key:
            p = truth[t]
            m = m_crop.astype(np.float64)
            cx = (m[:, 0, 0, None] * p[..., 0] + m[:, 0, 1, None] * p[..., 1]) + m[:, 0, 2, None]
            cy = (m[:, 1, 0, None] * p[..., 0] + m[:, 1, 1, None] * p[..., 1]) + m[:, 1, 2, None]
            empty = p[..., 0] < 0
            lm = np.stack([np.where(empty, -1.0, cx * (sc.GRID / sc.IN)), np.where(empty, -1.0, cy * (sc.GRID / sc.IN))], -1)
            r = track_ref.step(lm, np.ones((k, sc.C)), m_crop, boxes, sc.IN / sc.GRID, sc.IN / sc.GRID, sc.IN, sc.IN, sc.FH, sc.FW,
                               sc.CROP_TEMPLATE, sc.TEMPLATE)
        else:
            lm, w = np.full((k, sc.C, 2), -1.0), np.zeros((k, sc.C))
            rec["flow_lm"], rec["flags"] = lm, np.ones((k, sc.C), np.int32)
            for g in range(k):
                if track_ref.box_empty(boxes[g], sc.FH, sc.FW):
                    continue
                s = g // sc.SLOTS
                a = crop_u8(frames[S.ring_slot(s, t - 1)], m_crop[g])
                b = crop_u8(frames[S.ring_slot(s, t)], m_crop[g])
                fl = flow_ref.landmark_flow(a[None], b[None], prev_lm[g][None], m_crop[g][None], flow_ref.options())
                lm[g], w[g], rec["flags"][g] = fl[0][0], fl[1][0], fl[3][0]
            r = track_ref.step(lm, w, m_crop, boxes, 1.0, 1.0, sc.IN, sc.IN, sc.FH, sc.FW, sc.CROP_TEMPLATE, sc.TEMPLATE)
        rec.update(key=key, m_crop=m_crop.copy(), boxes=boxes.copy(), **r)
        out.append(rec)
        prev_lm = r["lm_frame"]
        m_crop, boxes, status = r["m_next"].copy(), r["boxes_next"].copy(), r["status"].copy()
    return out


@pytest.fixture(scope="module")
def bare(S):
    return closed_loop(S, False)


@pytest.fixture(scope="module")
def flowed(S):
    return closed_loop(S, True)


def check_lifetimes(S, run):
    """Every face is held from its first tick to its last, in its scripted slot, the exit is TRACK_OUTSIDE, and a slot
    without a face is dead."""
    for rec in run:
        t = rec["t"]
        for g in range(sc.CAP):
            f = S.face_in(g, t)
            want = track_ref.DEAD if f is None else track_ref.OUTSIDE if (f.last == t and t < sc.TICKS - 1) else 0
            got = int(rec["status"][g])
            assert (got & track_ref.DEAD) == want if f is None else got == want, (t, g, got, want)
        if "det_slot" in rec:
            _, who = S.detections(t)
            assert rec["det_slot"] == [[f.global_slot for f in row] for row in who], (t, rec["det_slot"])


def test_bare_step_keeps_every_face_until_its_scripted_exit(S, bare):
    check_lifetimes(S, bare)
    worst = 0.0
    truth = S.truth()
    for rec in bare:
        live = truth[rec["t"], :, 0, 0] >= 0
        assert (rec["lm_frame"][live] >= 0).all()                   # no truth landmark leaves the crop's positive quadrant
        worst = max(worst, float(np.abs(rec["lm_frame"][live] - truth[rec["t"]][live]).max()))
    print("bare step in closed loop: worst |landmark - truth| %.2e frame px" % worst)
    assert worst <= S.step_bound()


def test_association_is_unambiguous_through_the_crossing(S, bare):
    worst, least, n = np.inf, np.inf, 0
    for rec in bare:
        for _, own, other in rec.get("iou", []):
            worst, least, n = min(worst, own - other), min(least, own), n + 1
    orders = {tuple(rec["det_slot"][0]) for rec in bare if "det_slot" in rec}
    print("association: %d confirmations, least IoU with the own detection %.3f, least margin over any other %.3f; "
          "orders of stream 0's detections %s" % (n, least, worst, sorted(orders)))
    assert least >= 0.3 + IOU_MARGIN and worst >= IOU_MARGIN          # (0.3: the match_iou of TrackAssociation())
    assert orders == {(0, 1), (1, 0)}                                   # the detections swap places where the faces pass


# ---- quality --------------------------------------------------------------------------------------------------------------
def sharpness_interval(S, f, t):
    """(lo, hi, nominal) of the sharpness of the aligned face of (f, t) under any pixel error of at most B_align.
    Y is the luma in sixteenths: a pixel error e moves the quantised channel by at most 16 e + 0.5 and Y by at most that
    plus 1 (its own shift); the Laplacian has weights of absolute sum 8; and the standard deviation of a sum moves by at
    most the root mean square of what is added."""
    face = S.aligned(f.stream, t, f.pose(t)).astype(np.float32)[None]
    fmt = ("nhwc", "float32", "bgr", (1.0, 1.0, 1.0), (0.0, 0.0, 0.0))
    rec = face_quality_ref.record(face, fmt)[0]
    y = face_quality_ref.luma(face, fmt)
    e = 8.0 * (16.0 * sc.b_align(f.blur(t), f.scale(t)) + 1.5)
    assert rec[6] == 0 and rec[7] == 0 and y.min() - e / 8.0 > 16 * 16 and y.max() + e / 8.0 < 16 * 239   # exposed share 1
    std = math.sqrt(face_quality_ref.sharpness(rec) * 256.0)
    return max(std - e, 0.0) ** 2 / 256.0, (std + e) ** 2 / 256.0, std * std / 256.0


def test_the_sharpest_tick_wins_its_track_and_its_bin_by_more_than_the_bound_can_move(S):
    idx, xyz = sc.HEAD_INDICES, sc.HEAD_POINTS
    top = 0.0
    for f in S.faces:
        ticks = [t for t in range(sc.TICKS) if S.eligible(f, t)]
        iv = {t: sharpness_interval(S, f, t) for t in ticks}
        top = max(top, max(v[1] for v in iv.values()))
        front = {t: head_pose_ref.factor(head_pose_ref.fit(f.landmarks(t)[None], None, idx, xyz))[0] for t in ticks}
        assert all(v > 0.5 for v in front.values())
        b = S.best_tick(f)
        rival = max(iv[t][1] * front[t] for t in ticks if t != b)
        print("%s: best shot at tick %d, quality >= %.1f against <= %.1f of any other tick"
              % (f.name, b, iv[b][0] * front[b], rival))
        assert iv[b][0] * front[b] > rival
        bins = S.pose_bins(f, VIEWS)
        for bn, w in sorted(S.view_ticks(f, VIEWS).items()):
            others = [iv[t][1] for t in ticks if bins[t] == bn and t != w]
            print("%s: bin %d holds tick %d, sharpness >= %.1f against <= %.1f of the %d other ticks of the bin"
                  % (f.name, bn, w, iv[w][0], max(others + [0.0]), len(others)))
            assert iv[w][0] > max(others + [0.0])
    print("largest sharpness of the scenario %.1f (sharp_ref %.1f)" % (top, sc.SHARP_REF))
    assert top < sc.SHARP_REF


# ---- flow -----------------------------------------------------------------------------------------------------------------
def test_flow_reference_carries_the_landmarks_far_closer_than_they_move(S, flowed):
    check_lifetimes(S, flowed)
    truth = S.truth()
    e_ref, motion, n, points, rejected = 0.0, np.inf, 0, 0, 0
    for rec in flowed:
        t = rec["t"]
        for f in S.faces:
            pts = S.flow_checked(f, t) if f.live(t) else None
            if pts is None:
                continue
            g = f.global_slot
            m = rec["m_crop"][g].astype(np.float64)
            scale = math.hypot(m[0, 0], m[1, 0])
            rejected += int((rec["flags"][g][pts] != 0).sum())
            err = np.linalg.norm(rec["lm_frame"][g] - truth[t, g], axis=1)[pts] * scale
            move = np.linalg.norm(truth[t, g] - f.landmarks(t - 1), axis=1)[pts] * scale
            e_ref, motion, n, points = max(e_ref, float(err.max())), min(motion, float(move.min())), n + 1, points + int(pts.sum())
    print("flow in closed loop: e_ref = %.4f crop px over %d landmarks of %d face ticks (%d rejected); the smallest motion of "
          "one of them per tick is %.3f crop px; recorded E_REF %.3f" % (e_ref, points, n, rejected, motion, sc.E_REF))
    assert sc.FLOW_RADIUS == flow_ref.DEFAULTS["radius"]
    assert n >= 40 and points >= 40 * n and rejected == 0
    assert e_ref <= sc.E_REF <= motion / 4.0


# ---- the row forms ------------------------------------------------------------------------------------------------------
def test_row_truth_with_a_full_budget_is_the_truth_source_exactly(S, bare):
    """Row r of a full budget serves slot slots[r] through that slot's matrix: the same numbers through the same
    operations.  Rows in any order, inert rows among them."""
    truth = S.truth()
    n = 0
    for rec in bare:
        whole = sc.slots_truth(truth[rec["t"]], rec["m_crop"])
        assert np.array_equal(whole.view(np.uint64), np.asarray(rec_lm(rec, truth)).view(np.uint64))
        for slot in (np.arange(sc.CAP), np.array([5, -1, 0, 4, 1, -1, -1, 9])):
            m = np.where((slot >= 0)[:, None, None] & (slot < sc.CAP)[:, None, None], rec["m_crop"][np.clip(slot, 0, sc.CAP - 1)],
                         track_ref.IDENTITY)
            rows = sc.rows_truth(truth[rec["t"]], slot, m)
            for r, g in enumerate(slot):
                want = whole[g] if 0 <= g < sc.CAP else np.full((sc.C, 2), -1.0)
                assert rows[r].tobytes() == want.tobytes(), (rec["t"], r, g)
                n += 1
    assert n == 2 * sc.CAP * sc.TICKS


def rec_lm(rec, truth):
    """What closed_loop above sent its step at a tick of the bare run: the statement scenario.slots_truth restates."""
    p = truth[rec["t"]]
    m = rec["m_crop"].astype(np.float64)
    cx = (m[:, 0, 0, None] * p[..., 0] + m[:, 0, 1, None] * p[..., 1]) + m[:, 0, 2, None]
    cy = (m[:, 1, 0, None] * p[..., 0] + m[:, 1, 1, None] * p[..., 1]) + m[:, 1, 2, None]
    empty = p[..., 0] < 0
    return np.stack([np.where(empty, -1.0, cx * (sc.GRID / sc.IN)), np.where(empty, -1.0, cy * (sc.GRID / sc.IN))], -1)


ROW_RUNS = [("full", False), ("budget", False), ("budget", True), ("clock", False)]
_row_runs = {}


def row_run(S, name, smooth=False, fault=None):
    key = (name, smooth, fault)
    if key not in _row_runs:
        _row_runs[key] = sc.RowsReference(S, sc.SCHEDULES[name], smooth=smooth, fault=fault).run()
    return _row_runs[key]


def check_rows(S, name, smooth, records, ref):
    """Every checker tests/test_gpu_scenario_rows.py calls on a run of the schedule `name`, in its order."""
    worst = {}
    for rec, rref in zip(records, ref):
        sc.check_row_map(rec)
        sc.check_rows_written(rec)
        sc.check_untouched(rec)
        sc.check_flow_ready(rec)
        if rec["call"] != "flow" and not smooth:
            sc.check_truth(S, rec, rref, worst)
    if name == "budget":
        worst["wait"], worst["rows"] = sc.check_rotation(records)
    if smooth:
        worst["moved"] = sc.check_smoothing(S, records)
    return worst


@pytest.mark.parametrize("name,smooth", ROW_RUNS)
def test_references_alone_keep_every_track_under_each_row_schedule(S, name, smooth):
    """The condition before any device run: the schedule loses no track but P2 at its exit (a crop that is two ticks old
    costs P1, which moves left by 4 px a tick, a jaw point or two at the crop's left edge, never its track), and the
    reference's own run passes the checkers the device's run is held to."""
    records = row_run(S, name, smooth)
    seen = sc.check_lifetimes(S, records)
    worst = check_rows(S, name, smooth, records, records)
    lost = sum(int((rec["lm"][r] < 0).all(1).sum()) for rec in records if rec["call"] != "flow" for r in sc.served(rec)
               if not rec["status_rows"][r] & track_ref.DEAD)
    lag = max(b - a for ticks in seen.values() for a, b in zip(ticks, ticks[1:]))
    print("L-%s%s: served %s; oldest crop %d ticks; %d truth points outside a lagged crop; %s"
          % (name, " smooth" if smooth else "", {k: len(v) for k, v in seen.items()}, lag, lost, worst))
    assert lag == dict(full=1, budget=2, clock=2)[name]
    if name == "budget":
        assert worst["wait"] == 1 and set(worst["rows"]) == {sc.BUDGET}
        p2 = [f for f in S.faces if f.name == "P2"][0]
        assert seen["P2"][-1] == p2.last + 1            # the budget leaves P2 out at its scripted exit: dropped a tick later
    if smooth:
        assert worst["moved"] > 1000
    if name == "full":                                  # the flow ticks are those of closed_loop(S, True), served as rows
        assert all(rec["call"] == ("live" if S.is_key(rec["t"]) else "flow") for rec in records)


FAULT_CASES = [("rows swapped", "budget", False, "check_row_map"), ("wrong slot", "budget", False, "check_rows_written"),
               ("wrong slot", "clock", False, "check_rows_written"), ("no wait", "budget", True, "check_smoothing"),
               ("reset unserved", "budget", False, "check_untouched"), ("history kept", "budget", False, "check_flow_ready")]


@pytest.mark.parametrize("fault,name,smooth,checker", FAULT_CASES)
def test_each_fault_of_a_row_tick_fails_its_checker(S, fault, name, smooth, checker):
    with pytest.raises(AssertionError, match="^" + checker + ":") as e:
        check_rows(S, name, smooth, row_run(S, name, smooth, fault), row_run(S, name, smooth))
    print("%s under L-%s: %s" % (fault, name, e.value))


def test_a_swapped_map_and_a_wrong_slot_miss_the_truth_as_well(S):
    """Both faults are seen by check_truth too: a swapped map sends a row the truth of another face through its matrix,
    and a row written to another slot leaves that slot a crop matrix fitted to another face's landmarks."""
    good = row_run(S, "budget")
    for fault in ("rows swapped", "wrong slot"):
        bad = row_run(S, "budget", False, fault)
        with pytest.raises(AssertionError, match="^check_truth:"):
            for rec, ref in zip(bad, good):
                sc.check_truth(S, rec, ref, {})
