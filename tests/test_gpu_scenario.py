"""prediction.FaceTracker in closed loop on the GPU against the rendered ground truth of tests/scenario.py, all options on.

The landmark model is scenario.TruthSource (the truth landmarks through the tracker's current crop matrices), so everything
AFTER the network runs as shipped: association, the track step and its fits, flow, pose, the aligned and the mesh warp,
best shots, views, ids and exits -- over TICKS ticks of `update` + `step` every KEY-th tick and `step_flow` between, then
`retire(flush=True)`.  tests/test_scenario_host.py shows on the CPU that each fault this could hide would be seen.

Tracker A (weights="score", best_shot, pose, views, exits, mesh, flow, 2 streams, samples=1, no smoothing), every tick:
  * landmarks: on `step` ticks within Script.step_bound() of truth (float64 through a float32 matrix and back, derived
    there: 2.1e-12 px); on `step_flow` ticks within 1.5 x E_REF crop px, E_REF = 0.36 (measured 0.3572 by the host module),
    for the landmarks Script.flow_checked names -- the flow follows pixels, so the head, a face at the frame's edge, a tick
    after a jump of the blur and a window over the crop's border are not held against truth (the reasons are stated there);
  * both fits: M_align and M_next applied to the truth points equal the float64 Umeyama fit of the returned landmarks
    within the float32 rounding of its four numbers, 2^-24 (|a x| + |b y| + |t|); on `step` ticks of a planar face that is
    the template itself;
  * aligned and mesh faces: every pixel within B_align of the float64 rendering -- through the truth pose and the truth
    landmarks on `step` ticks, through the returned M and landmarks on `step_flow` ticks (of a face that has been whole since the last `step`:
    Script.flow_whole); a slot without a face is zero;
  * pose: yaw, pitch and roll of the head within POSE_TOL of the script on `step` ticks; the bin of every face is the
    truth's wherever the truth stayed in one bin since the last `step`;
  * identity: det_slot of every update and track_id at every tick follow the script through the crossing.
At the end: best shots, views (-1 in the bins never visited), the one exit of the face that left and the flushed rest.
Tracker B adds smooth=True: its landmarks equal tests/track_filter_ref.py, bit for bit, driven by the inputs the device
had and by its own state in closed loop, and no face is lost early.  The plain tracker has no option and takes `step` at
every tick; started from A's state it returns A's landmarks, M and status on every `step` tick, bit for bit.

Measured on an MI355X (each test prints its figures): landmarks on `step` ticks 1.71e-13 px against the bound of 2.11e-12;
on 51 `step_flow` face-ticks 0.3572 crop px (e_ref itself: the device equals the flow reference) against 0.540; both fits
0.812 of the float32 bound; the worst aligned pixel 0.884 and the worst mesh pixel 0.911 of B_align (B_align is 0.56 to
0.60 at an ordinary blur and 1.4 without blur); head pose 1.47e-15 rad against 2.82e-12; tracker B: 16170 coordinates moved
by the filter, every bit the reference's."""
import math

import numpy as np
import pytest
import torch

import scenario as sc
import track_filter_ref
import track_ref
import track_views_ref

pytestmark = pytest.mark.gpu
OUTSIDE = track_ref.OUTSIDE
Q = 16


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


def make(P, S, **kw):
    src = sc.TruthSource(S)
    tr = P.FaceTracker(src, (sc.FH, sc.FW), sc.CAP, out_size=(sc.OUT, sc.OUT), streams=sc.STREAMS, samples=1, **kw)
    src.bind(tr)
    return tr, src


def host(x):
    return x.detach().cpu().numpy()


def run(P, S, ring, follower=None, **kw):
    """The script on a tracker made with `kw`; follower: a second tracker's options -- it is given this tracker's m_crop,
    boxes and status before every `step` tick, takes `step` at every tick, and its results are recorded beside."""
    tr, src = make(P, S, **kw)
    fo = make(P, S, **follower) if follower is not None else None
    with_id = tr.best_shot is not None
    out = []
    for t in range(sc.TICKS):
        src.tick = t
        slots = [S.ring_slot(s, t) for s in range(sc.STREAMS)]
        rec = dict(t=t)
        if S.is_key(t):
            det, _ = S.detections(t)
            rec["det_slot"] = tr.update(det)[0].clone()
            if fo is not None:
                fo[0].update(det)
                for name in ("m_crop", "boxes", "status"):
                    getattr(fo[0], name).copy_(getattr(tr, name))
        rec["m_crop"], rec["boxes"] = tr.m_crop.clone(), tr.boxes.clone()
        call = tr.step if S.is_key(t) else tr.step_flow
        res = call(ring, slots, frame_id=t) if with_id else call(ring, slots)
        rec.update(aligned=res[0].clone(), M=res[1].clone(), lm=res[2].clone(), status=res[3].clone(), m_next=tr.m_crop.clone())
        if S.is_key(t):
            rec["sent"] = src.sent[t]
        elif tr.flow is not None:
            rec.update(flags=tr.flow_flags.clone(), flow_lm=tr._flow_crop_lm.clone(), flow_w=tr._flow_crop_w.clone())
        if tr.mesh is not None:
            rec["mesh"] = tr.mesh_faces.clone()
        if tr.pose is not None:
            rec["pose"] = tr.pose.clone()
        if tr.track_id is not None:
            rec["track_id"], rec["exit_head"] = tr.track_id.clone(), tr.exit_head.clone()
        if fo is not None:
            fo[1].tick = t
            r2 = fo[0].step(ring, slots)
            rec["follower"] = [x.clone() for x in r2]
        out.append(rec)
    end = {}
    if tr.best_shot is not None:
        end["best"] = [x.clone() for x in tr.best()]
    if tr.view_opts is not None:
        end["views"] = [x.clone() for x in tr.views()]
    if tr.exit_opts is not None:
        tr.retire(flush=True, frame_id=sc.TICKS)
        end["exits"] = [x.clone() for x in tr.exits()]
        end["exit_views"] = [x.clone() for x in tr.exit_views()]
        end["track_id"] = tr.track_id.clone()
    torch.cuda.synchronize()
    out = [{k: (host(v) if isinstance(v, torch.Tensor) else [host(x) for x in v] if isinstance(v, list) else v)
            for k, v in rec.items()} for rec in out]
    end = {k: ([host(x) for x in v] if isinstance(v, list) else host(v)) for k, v in end.items()}
    return tr, out, end


@pytest.fixture(scope="module")
def run_a(mods, S, ring):
    _, A, P = mods
    return run(P, S, ring, follower={}, **options(A))


fit_bound = sc.fit_bound


def pose_tol(S):
    """scenario.pose_tol on the bound of a `step` tick."""
    return sc.pose_tol(S.step_bound())


def test_tracker_a_follows_the_truth_at_every_tick(mods, S, run_a):
    _, A, P = mods
    tr, ticks, _ = run_a
    truth, ids = S.truth(), S.track_ids()
    views = tr.view_opts
    worst = dict(step=0.0, flow=0.0, fit=0.0, aligned=0.0, mesh=0.0, pose=0.0)
    n_flow = n_bins = 0
    tol_pose = pose_tol(S)
    all_bins = {f.name: S.pose_bins(f, views) for f in S.faces}
    for rec in ticks:
        t, key = rec["t"], S.is_key(rec["t"])
        if key:
            _, who = S.detections(t)
            for s in range(sc.STREAMS):
                assert rec["det_slot"][s][:len(who[s])].tolist() == [f.global_slot for f in who[s]], (t, s)
        for g in range(sc.CAP):
            f = S.face_in(g, t)
            st = int(rec["status"][g])
            if f is None:
                assert st & track_ref.DEAD and not rec["aligned"][g].any() and not rec["mesh"][g].any(), (t, g, st)
                assert (rec["lm"][g] == -1.0).all() and rec["track_id"][g] == -1, (t, g)
                continue
            assert st == (OUTSIDE if (t == f.last and t < sc.TICKS - 1) else 0), (t, f.name, st)
            assert rec["track_id"][g] == ids[f.name], (t, f.name, rec["track_id"][g])
            lm, tru = rec["lm"][g], truth[t, g]
            m_crop = rec["m_crop"][g].astype(np.float64)
            if key:
                e = float(np.abs(lm - tru).max())
                worst["step"] = max(worst["step"], e)
                assert e <= S.step_bound(), (t, f.name, e)
            else:
                pts = S.flow_checked(f, t)
                if pts is not None:
                    assert (rec["flags"][g][pts] == 0).all(), (t, f.name)
                    e = float((np.linalg.norm(lm - tru, axis=1)[pts]).max() * math.hypot(m_crop[0, 0], m_crop[1, 0]))
                    worst["flow"], n_flow = max(worst["flow"], e), n_flow + 1
                    assert e <= 1.5 * sc.E_REF, (t, f.name, e)
            ok = lm[:, 0] >= 0
            for name, tmpl in (("M", sc.TEMPLATE), ("m_next", sc.CROP_TEMPLATE)):
                if name == "m_next" and st:
                    assert np.array_equal(rec[name][g], track_ref.IDENTITY)
                    continue
                sim = sc.umeyama(lm[ok], tmpl[ok])
                got = sc.apply(rec[name][g], tru)
                d = np.abs(got - sc.apply(sc.matrix(sim), tru)) / fit_bound(sim, tru)
                if key and isinstance(f, sc.Planar):
                    d = np.maximum(d, np.abs(got - tmpl) / fit_bound(sim, tru))
                worst["fit"] = max(worst["fit"], float(d.max()))
                assert d.max() <= 1.0, (t, f.name, name, float(d.max()))
            if not key and not S.flow_whole(f, t):
                continue                      # (the face at the frame's edge: its pixels are held on `step` ticks alone)
            to_frame = f.pose(t) if key else sc.inverse(rec["M"][g])
            src_lm = tru if key else lm
            bound = sc.b_align(f.blur(t), f.scale(t))
            e = float(np.abs(rec["aligned"][g] - S.aligned(f.stream, t, to_frame)).max()) / bound
            worst["aligned"] = max(worst["aligned"], e)
            assert e <= 1.0, (t, f.name, "aligned", e)
            if ok.all():
                e = float(np.abs(rec["mesh"][g] - S.mesh_face(f.stream, t, tr.mesh, src_lm, to_frame)).max()) / bound
                worst["mesh"] = max(worst["mesh"], e)
                assert e <= 1.0, (t, f.name, "mesh", e)
            pose = rec["pose"][g]
            assert pose[14] == 1.0, (t, f.name)
            if key and isinstance(f, sc.Head):
                e = float(np.abs(pose[15:18] - np.array(f.angles(t))).max())
                worst["pose"] = max(worst["pose"], e)
                assert e <= tol_pose, (t, e)
            bins = all_bins[f.name]
            since = [bins[tt] for tt in range(max(S.last_key(t), f.first), t + 1) if tt in bins]
            if t in bins and len(set(since)) == 1:
                n_bins += 1
                assert track_views_ref.bin_of(pose, views.u_edges, views.v_edges) == bins[t], (t, f.name)
                if isinstance(f, sc.Head) and bins[t] != 1:
                    assert (pose[15] > 0) == (f.angles(t)[0] > 0), (t, pose[15])
    print("tracker A: landmarks on step ticks %.2e px (bound %.2e); on %d flow face-ticks %.4f crop px (bound %.3f); fits "
          "%.3f of the float32 bound; aligned %.3f and mesh %.3f of B_align; head pose %.2e rad (bound %.2e); %d bins checked"
          % (worst["step"], S.step_bound(), n_flow, worst["flow"], 1.5 * sc.E_REF, worst["fit"], worst["aligned"],
             worst["mesh"], worst["pose"], tol_pose, n_bins))
    assert n_flow >= 40 and n_bins >= 100


def test_tracker_a_ends_with_the_scripted_best_shots_views_and_exits(mods, S, run_a):
    tr, ticks, end = run_a
    ids = S.track_ids()
    views = tr.view_opts
    held = {f.global_slot: f for f in S.faces if f.last == sc.TICKS - 1}
    gallery, best_q, best_frame = end["best"][:3]
    view_gallery, view_q, view_frame = end["views"][:3]

    def shot(f, t):
        return S.aligned(f.stream, t, f.pose(t)), sc.b_align(f.blur(t), f.scale(t))

    for g in range(sc.CAP):
        f = held.get(g)
        if f is None:
            assert best_q[g] == -1.0 and best_frame[g] == -1 and (view_q[g] == -1.0).all() and (view_frame[g] == -1).all(), g
            continue
        assert best_frame[g] == S.best_tick(f) and best_q[g] > 0, (f.name, best_frame[g])
        exp, bound = shot(f, S.best_tick(f))
        assert np.abs(gallery[g] - exp).max() <= bound, f.name
        want = S.view_ticks(f, views)
        for b in range(views.bins):
            assert view_frame[g, b] == want.get(b, -1) and (view_q[g, b] > 0) == (b in want), (f.name, b, view_frame[g])
            if b in want:
                exp, bound = shot(f, want[b])
                assert np.abs(view_gallery[g, b] - exp).max() <= bound, (f.name, b)
    # the exits: the face that left, once, at the tick after its last; then the flush, by ascending slot
    gone = [f for f in S.faces if f.last < sc.TICKS - 1]
    (left,) = gone
    for rec in ticks:
        want = (len(gone) if rec["t"] > left.last else 0, sum(1 for f in S.faces if f.first <= rec["t"]), 0, 0)
        assert tuple(rec["exit_head"]) == want, (rec["t"], rec["exit_head"])
    faces, meta, q, m, lms, head = end["exits"]
    xv_gallery, xv_q, xv_frame = end["exit_views"][:3]
    order = [left] + [held[g] for g in sorted(held)]
    assert tuple(head) == (len(order), len(S.faces), 0, 0)
    assert (end["track_id"] == -1).all()
    for row, f in enumerate(order):
        first = row == 0
        want = [ids[f.name], f.global_slot, f.first, left.last + 1 if first else sc.TICKS, S.best_tick(f),
                OUTSIDE if first else -2, row, 0]
        assert meta[row].tolist() == want, (f.name, meta[row].tolist(), want)
        exp, bound = shot(f, S.best_tick(f))
        assert np.abs(faces[row] - exp).max() <= bound and q[row] > 0, f.name
        assert np.abs(lms[row] - f.landmarks(S.best_tick(f))).max() <= S.step_bound(), f.name
        vt = S.view_ticks(f, views)
        for b in range(views.bins):
            assert (xv_q[row, b] > 0) == (b in vt), (f.name, b)
            if b in vt:
                assert xv_frame[row, b] == vt[b], (f.name, b, xv_frame[row])
                exp, bound = shot(f, vt[b])
                assert np.abs(xv_gallery[row, b] - exp).max() <= bound, (f.name, b)
    assert ids == {"P0": 0, "P1": 1, "H": 2, "P2": 3, "P3": 4}          # the reborn slot got the next id


def test_plain_tracker_returns_the_bits_of_a_on_every_step_tick(S, run_a):
    """A tracker without any option, given A's m_crop, boxes and status before each `step` tick, returns A's landmarks, M
    and aligned faces there bit for bit, and A's status (but for the TRACK_LOW_SCORE of an empty slot); on the ticks between, where it
    takes `step` on the truth, its landmarks are the truth within the bound of a `step` tick."""
    _, ticks, _ = run_a
    truth = S.truth()
    n = 0
    for rec in ticks:
        t = rec["t"]
        aligned, m, lm, status = rec["follower"]
        if S.is_key(t):
            for a, b in ((aligned, rec["aligned"]), (m, rec["M"]), (lm, rec["lm"])):
                assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), t
            # a slot without a face has no points: with weights="score" its mean score is 0/0 and A adds TRACK_LOW_SCORE
            dead = np.array([S.face_in(g, t) is None for g in range(sc.CAP)])
            assert status.dtype == rec["status"].dtype and np.array_equal(status[~dead], rec["status"][~dead]), t
            assert np.array_equal(status[dead], rec["status"][dead] & ~track_ref.LOW_SCORE), t
            n += 1
        else:
            for g in range(sc.CAP):
                f = S.face_in(g, t)
                if f is not None and status[g] == 0:
                    assert np.abs(lm[g] - truth[t, g]).max() <= S.step_bound(), (t, f.name)
    assert n == sc.TICKS // sc.KEY


def test_tracker_b_smooths_as_the_reference_and_loses_no_face(mods, S, ring):
    _, A, P = mods
    tr, ticks, _ = run(P, S, ring, smooth=True, **options(A))
    dt = A.LandmarkFilter().time_step(None)
    state = track_filter_ref.empty_state(sc.CAP, sc.C)
    moved = 0
    for rec in ticks:
        t, key = rec["t"], S.is_key(rec["t"])
        for f in S.faces:
            if f.first == t:                                            # a birth clears the slot's history
                state[f.global_slot] = -1.0
        if key:
            lm_in, w, s = rec["sent"], np.ones((sc.CAP, sc.C)), sc.IN / sc.GRID
        else:
            lm_in, w, s = rec["flow_lm"], rec["flow_w"], 1.0
        r = track_filter_ref.step(lm_in, w, rec["m_crop"], rec["boxes"], s, s, sc.IN, sc.IN, sc.FH, sc.FW, sc.CROP_TEMPLATE,
                                  sc.TEMPLATE, state, dt)
        state = r["state"]
        for name, got in (("lm_frame", rec["lm"]), ("m_align", rec["M"]), ("m_next", rec["m_next"]), ("status", rec["status"])):
            assert got.dtype == r[name].dtype and got.tobytes() == r[name].tobytes(), (t, name)
        moved += int((r["lm_frame"] != r["lm_raw"]).sum())
        for g in range(sc.CAP):
            f = S.face_in(g, t)
            if f is not None and (t < f.last or f.last == sc.TICKS - 1):   # (the filter's lag may move the exit itself)
                assert rec["status"][g] == 0, (t, f.name)
    print("tracker B: %d coordinates moved by the filter" % moved)
    assert moved > 1000
