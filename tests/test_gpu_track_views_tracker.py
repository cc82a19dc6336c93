"""FaceTracker(views=...) on the GPU: a scenario of fourteen ticks -- a seed, `step`, `step_active` and `step_live` ticks, a
track that is lost, a rebirth in its slot by a `seed`, a tick that does not serve the reborn slot, an `update` that starts
a track, a second lost track and `retire(flush=True)` at the end -- on a synthetic ring with synthetic weights, once with
one stream and once with three.  The tracker's two view calls are wrapped: every update is compared, bit for bit and over
every view array, with tests/track_views_ref.py applied to the view state downloaded just before it and the inputs the
tracker passed (which must be the step's own returns, the tracker's pose records and its pending best-shot resets), and
every exit-views call with the restatement on the ring downloaded before it.  A second tracker without `views` runs the
same scenario first: every step output, best(), pose and exits() of the two are bit-equal on every tick.

Landmarks of random weights may all fall into one pose bin under the default edges, so the first run also observes
u = -R[2][0] of the faces that count, and the views tracker cuts u at their median (PoseViews.from_edges).

Synthetic weights lose tracks at will, so the scenario pins what it needs between the ticks, on both trackers alike: the
slots it keeps alive get their box, matrix and status back."""
import numpy as np
import pytest
import torch

import track_views_ref as vref

pytestmark = pytest.mark.gpu
RH, RW, CAP, Q = 270, 480, 9, 4
BOX = {0: (40, 30, 140, 130), 3: (200, 20, 290, 110), 4: (300, 120, 400, 220), 6: (60, 150, 150, 240)}
FAR1, FAR2 = (330, 10, 400, 80), (170, 150, 250, 230)
OUTSIDE = 16
# The landmarks of a network with synthetic weights are no face: a model of 17 arbitrary points on every fourth landmark
# spreads the fitted rotations (tests/test_gpu_head_pose.py uses the same device).
MODEL17 = (list(range(0, 68, 4)), np.random.default_rng(5).uniform(-100.0, 100.0, (17, 3)).tolist())
SHARP_REF, MIN_EXPOSED = 1e6, 0.25


@pytest.fixture(scope="module")
def mods():
    import flm_amd  # noqa: F401
    from flm_amd import _lib, alignment, prediction
    _lib.load()
    return _lib, alignment, prediction


@pytest.fixture(scope="module")
def ring():
    rng = np.random.default_rng(31)
    return torch.from_numpy(rng.integers(0, 256, (8, RH, RW, 3), dtype=np.uint8)).cuda()


@pytest.fixture(scope="module")
def model():
    from flm_amd.networks import LANDMARKS_MODELS
    from flm_amd.weights import synth_fcn8_weights
    m = LANDMARKS_MODELS["fcn_8"](68, input_height=64, input_width=64, dtype="bf16")
    m.load_weights(synth_fcn8_weights(68, seed=2))
    return m


def view_bits(x):
    return x.view(torch.int64) if x.dtype == torch.float64 else x.view(torch.int32) if x.dtype == torch.float32 else x


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(view_bits(a), view_bits(b))


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[x.dtype.itemsize])


def as_bytes(t, lead):
    """A tensor [*lead, face...] as uint8 [*lead, face_bytes] on the host."""
    return t.contiguous().view(torch.uint8).reshape(tuple(t.shape[:lead]) + (-1,)).cpu().numpy()


def host(t):
    return None if t is None else t.detach().cpu().numpy().copy()


def views_state(tr):
    return dict(view_q=host(tr.view_q), view_frame=host(tr.view_frame), view_gallery=as_bytes(tr.view_gallery, 2),
                view_m=host(tr.view_M), view_lm=host(tr.view_landmarks), view_pose=host(tr.view_pose))


def ring_state(tr):
    return dict(x_view_q=host(tr.exit_view_q), x_view_frame=host(tr.exit_view_frame),
                x_view_gallery=as_bytes(tr.exit_view_gallery, 2), x_view_m=host(tr.exit_view_M),
                x_view_lm=host(tr.exit_view_landmarks), x_view_pose=host(tr.exit_view_pose))


def assert_same_arrays(got, want, what):
    for k in want:
        assert got[k].shape == want[k].shape and np.array_equal(bits(got[k]), bits(want[k])), (k, what)


def play(tr, A, ring, streams, on_tick):
    """The scenario on one tracker.  on_tick(t, how, res, served): after every tick; res: the step's returns (None for a
    bare retire), served: the global slots of its rows (-1: an inert row)."""
    keep = {}

    def pin():
        for slot, box in keep.items():
            b = torch.tensor([box], dtype=torch.int32, device="cuda")
            m, st = A.track_seed_device(b, (64, 64), (RH, RW))
            tr.boxes[slot], tr.m_crop[slot], tr.status[slot] = b[0], m[0], st[0]

    def tick(t, how, **kw):
        fid = 100 + t
        fi = [(3 * t + 2 * i + 1) % 8 for i in range(streams)]
        fi = fi[0] if streams == 1 and how == "step" else fi
        if how == "step":
            res = tr.step(ring, fi, frame_id=fid)
            served = list(range(CAP))
        elif how == "active":
            res = tr.step_active(ring, fi, frame_id=fid, **kw)
            served = res[4].tolist()
        elif how == "live":
            res = tr.step_live(ring, fi, frame_id=fid, **kw)
            served = res[4].tolist()
        else:
            assert tr.retire(frame_id=fid, **kw) is tr.exit_head
            res, served = None, []
        on_tick(t, how, res, served)
        return served

    all_streams = list(range(streams))
    tr.seed(list(BOX), list(BOX.values()))                             # tick 0: four tracks begin
    tick(0, "step")
    keep.update(BOX)
    pin()
    tick(1, "step")
    pin()
    served = tick(2, "active", active=all_streams[:2] if streams > 1 else [0])      # three streams: slot 6 is not served
    assert (6 in served) == (streams == 1)
    pin()
    tick(3, "live", budget=CAP)
    pin()
    tr.boxes[3], tr.status[3] = 0, OUTSIDE                             # tick 4: the track of slot 3 is lost
    del keep[3]
    tick(4, "step")
    pin()
    tr.seed([3], [FAR2])                                               # tick 5: a rebirth in its slot; the tick does not serve it
    if streams == 1:
        served = tick(5, "live", budget=1)
    else:
        served = tick(5, "active", active=[0, 2])
    assert 3 not in served and int(tr._best_reset[3]) == 1
    keep[3] = FAR2
    pin()
    served = tick(6, "step")                                           # tick 6: the reborn slot's first served step
    pin()
    dets = [BOX[0], FAR1]                                              # tick 7: an update starts a track in a free slot of stream 0
    det_slot, _, _ = tr.update(dets if streams == 1 else [dets] + [None] * (streams - 1))
    new = int(det_slot.reshape(-1)[1])
    assert det_slot.reshape(-1)[0] == 0 and new >= 0 and new not in keep
    tick(7, "step")
    keep[new] = FAR1
    pin()
    tick(8, "live", budget=2)                                          # live slots beyond the budget sit the tick out
    pin()
    tick(9, "active", active=all_streams)
    pin()
    tick(10, "step")
    pin()
    tr.boxes[4], tr.status[4] = 0, OUTSIDE                             # tick 11: a second track is lost
    del keep[4]
    tick(11, "live", budget=CAP)
    pin()
    tick(12, "step")
    pin()
    tick(13, "retire", flush=True)                                     # the end of the video
    return keep


@pytest.mark.parametrize("streams", [1, 3])
def test_views_over_a_scenario(mods, ring, model, streams, monkeypatch):
    L, A, P = mods
    pose = A.HeadPose(model=A.HeadModel(*MODEL17))
    mk = lambda **kw: P.FaceTracker(model, (RH, RW), CAP, best_shot=A.BestShot(sharp_ref=SHARP_REF, min_exposed=MIN_EXPOSED),
                                    weights="score", associate=A.TrackAssociation(square=False), streams=streams, pose=pose,
                                    exits=Q, **kw)
    # ---- the first run: a tracker without views; what it returns, and the u of the faces that count
    plain, record, us = mk(), [], []

    def on_plain(t, how, res, served):
        if res is not None:
            status = res[3].cpu().numpy()
            p = plain.pose.cpu().numpy()
            for r, g in enumerate(served):
                if g >= 0 and status[r] == 0 and p[g, 14] == 1.0:
                    us.append(float(-p[g, 6]))
        record.append(dict(res=None if res is None else [x.clone() for x in res], best=[x.clone() for x in plain.best()],
                           pose=plain.pose.clone(), exits=[x.clone() for x in plain.exits()],
                           state=[getattr(plain, n).clone() for n in ("m_crop", "boxes", "status", "_best_reset", "track_id")]))

    with pytest.raises(ValueError, match="views"):
        plain.views()
    play(plain, A, ring, streams, on_plain)
    print("u of the", len(us), "faces that count:", np.round(np.sort(us), 3).tolist())
    assert len(us) >= 4, "the scenario has too few faces with status 0 and an ok pose"
    edge = float(np.median(us))
    opts = A.PoseViews.from_edges((edge,), sharp_ref=SHARP_REF, min_exposed=MIN_EXPOSED)
    assert opts.bins == 2

    # ---- the second run: the same scenario with views, the two view calls wrapped
    tr = mk(views=opts)
    real_update, real_exit = A.track_views_update_device, A.track_exit_views_device
    log, exit_log, now = [], [], {}

    def spy_update(faces, rec, lm, pose_t, view_q, view_frame, view_gallery, take, frame_id, **kw):
        assert view_q is tr.view_q and view_frame is tr.view_frame and view_gallery is tr.view_gallery and pose_t is tr.pose
        assert kw["view_m"] is tr.view_M and kw["view_lm"] is tr.view_landmarks and kw["view_pose"] is tr.view_pose
        assert kw["opts"] is opts
        state = views_state(tr)
        inp = dict(faces=as_bytes(faces, 1), rec=host(rec), lm=host(lm), pose=host(pose_t), w=host(kw["weights"]),
                   status=host(kw["status"]), reset=host(kw["reset"]), m=host(kw["m"]), slot=host(kw["slot"]))
        ins = dict(faces=faces, rec=rec, lm=lm, m=kw["m"], status=kw["status"], reset=kw["reset"], slot=kw["slot"])
        before = {k: None if v is None else v.clone() for k, v in ins.items()}
        pose_before = pose_t.clone()
        out = real_update(faces, rec, lm, pose_t, view_q, view_frame, view_gallery, take, frame_id, **kw)
        want = vref.update(state, inp["faces"], inp["rec"], inp["lm"], inp["pose"], frame_id, opts.u_edges, opts.v_edges,
                           w=inp["w"], status=inp["status"], reset=inp["reset"], m=inp["m"], slot=inp["slot"],
                           sharp_ref=SHARP_REF, min_exposed=MIN_EXPOSED)
        assert np.array_equal(host(take), want), (frame_id, host(take), want)
        assert_same_arrays(views_state(tr), state, ("update", frame_id))
        for k, v in ins.items():                                       # the inputs are unchanged
            assert v is None or same(v, before[k]), k
        assert same(pose_t, pose_before)
        now.update(frame_id=frame_id, faces=faces, lm=lm, m=kw["m"], status=kw["status"], slot=kw["slot"], reset=inp["reset"],
                   take=want)
        return out

    def spy_exit(exit_row, view_q, view_frame, view_gallery, x_view_q, x_view_frame, x_view_gallery, **kw):
        assert exit_row is tr.exit_row and view_q is tr.view_q and x_view_q is tr.exit_view_q
        state, ring_before = views_state(tr), ring_state(tr)
        rows = host(exit_row)
        want = {k: v.copy() for k, v in ring_before.items()}
        vref.exit_views(state, want, rows)
        out = real_exit(exit_row, view_q, view_frame, view_gallery, x_view_q, x_view_frame, x_view_gallery, **kw)
        got = ring_state(tr)
        assert_same_arrays(got, want, ("exit", rows.tolist()))
        assert_same_arrays(views_state(tr), state, "the views are inputs of the exit call")
        for t_, row in enumerate(rows):
            if row >= 0:                                               # the views the ended slot held
                assert np.array_equal(bits(got["x_view_q"][row]), bits(state["view_q"][t_]))
                full = state["view_q"][t_] >= 0.0
                assert np.array_equal(got["x_view_gallery"][row][full], state["view_gallery"][t_][full])
                exit_log.append(dict(slot=t_, row=int(row), filled=int(full.sum()), track=int(tr.exit_meta[row, 0]),
                                     q=state["view_q"][t_].tolist()))
        return out

    monkeypatch.setattr(A, "track_views_update_device", spy_update)
    monkeypatch.setattr(A, "track_exit_views_device", spy_exit)
    filled_bins, first_served = set(), {}

    def on_views(t, how, res, served):
        ref = record[t]
        if res is not None:
            assert len(res) == len(ref["res"])
            for a, b in zip(res, ref["res"]):                          # the step's returns: the bits of a tracker without views
                assert same(a, b), (t, how)
            # what the tracker passed to the view update is what the step returns, its pose and its pending resets
            assert now["frame_id"] == 100 + t and same(now["faces"], res[0]) and same(now["m"], res[1])
            assert same(now["lm"].contiguous(), res[2]) and same(now["status"], res[3])
            assert (now["slot"] is None) == (how == "step") and (how == "step" or same(now["slot"], res[4]))
            for r, g in enumerate(served):
                if g >= 0:
                    first_served.setdefault(g, []).append((t, int(now["reset"][r]), int(now["take"][r])))
            filled_bins.update(int(v) for v in now["take"] if v >= 0)
            print("tick", t, how, "served", served, "take", now["take"].tolist(), "reset", now["reset"].tolist())
        for a, b in zip(tr.best(), ref["best"]):
            assert same(a, b), (t, how)
        for a, b in zip(tr.exits(), ref["exits"]):
            assert same(a, b), (t, how)
        assert same(tr.pose, ref["pose"]), (t, how)
        for n, b in zip(("m_crop", "boxes", "status", "_best_reset", "track_id"), ref["state"]):
            assert same(getattr(tr, n), b), (n, t, how)

    assert tr.view_q is None
    play(tr, A, ring, streams, on_views)
    assert len(record) == 14 and tr.exit_head.tolist() == plain.exit_head.tolist()
    # ---- a reborn slot's first served step starts from empty bins: tick 6 serves slot 3 with its reset pending
    t6 = [e for e in first_served[3] if e[0] == 6]
    assert t6 and t6[0][1] == 1, first_served[3]
    assert [e for e in first_served[3] if e[0] == 5] == []             # tick 5 did not serve it
    # ---- the tensors handed out
    vg, vq, vf, vm, vl, vp = tr.views()
    assert vg is tr.view_gallery and vq is tr.view_q and vp is tr.view_pose and tuple(vq.shape) == (CAP, 2)
    assert tuple(vg.shape) == (CAP, 2) + tuple(tr.gallery.shape[1:]) and vg.dtype == tr.gallery.dtype
    xg, xq, xf, xm, xl, xp = tr.exit_views()
    assert xg is tr.exit_view_gallery and xq is tr.exit_view_q and tuple(xq.shape) == (Q, 2)
    assert tuple(xg.shape) == (Q, 2) + tuple(tr.gallery.shape[1:]) and tuple(xl.shape) == (Q, 2, 68, 2)
    print("bins filled:", sorted(filled_bins), "exits:", exit_log)
    assert len(filled_bins) >= 2, filled_bins
    assert any(e["filled"] >= 2 for e in exit_log), exit_log
