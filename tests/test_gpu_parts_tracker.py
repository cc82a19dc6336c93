"""FaceTracker(parts=..., openness=...) on the GPU, in the configuration of tests/test_gpu_track_flow.py (its fixtures and
helpers are used as they are): 2 streams x 2 slots, bf16 fcn_8 at 64x64 with synthetic weights, the translated 1080p
ring.  Through `step`, `step_flow`, `step_active`, `step_live` and `step_flow_live`:
  * with every option on, everything the calls return and every state tensor the tracker had before equals, bit for bit,
    that of a tracker made without the two options;
  * `part_faces`, `part_M` and `part_ok` equal the stand-alone call on the returned landmarks, `openness` equals the
    stand-alone call at the rows' slots, and `open_state` equals tests/parts_ref.py run over the same ticks;
  * a slot that sits a tick out keeps its `open_state` and its pending reset."""
import numpy as np
import pytest
import torch

import parts_ref as ref
import test_gpu_track_flow as base
from test_gpu_track_flow import frames, mods, model, ring  # noqa: F401  (fixtures)
from test_gpu_track_flow import CAP, LARGE, RH, RW, SMALL, STREAMS, same

pytestmark = pytest.mark.gpu
SPS = CAP // STREAMS
SMALL4 = SMALL + [(1200, 700, 1328, 828)]                     # a face for slot 3 too
LARGE4 = LARGE + [(1136, 636, 1392, 892)]
STATE = base.STATE + ("misses", "slot_age", "_best_reset", "flow_frame", "flow_ready", "mesh_faces", "view_q", "view_frame",
                      "view_gallery", "view_M", "view_landmarks", "view_pose", "track_id", "born_frame", "exit_row",
                      "exit_head", "exit_faces", "exit_meta", "exit_q", "exit_M", "exit_landmarks", "exit_rec",
                      "exit_view_q", "exit_view_frame", "exit_view_gallery", "exit_view_M", "exit_view_landmarks",
                      "exit_view_pose", "live_cursor", "live_counts", "flow_cursor", "flow_counts", "flow_err", "flow_flags",
                      "flow_fb")


def u64(a):
    return np.ascontiguousarray(a).view(np.uint64)


def ticks(ring_):
    """(name, the call, the boxes pinned before it, the ring slot of each stream)."""
    return [
        ("step", lambda t, kw: t.step(ring_, [0, 0], **kw), SMALL4, [0, 0]),
        ("step_flow", lambda t, kw: t.step_flow(ring_, [1, 1], **kw), LARGE4, [1, 1]),
        ("step_active", lambda t, kw: t.step_active(ring_, [None, 2], [1], **kw), SMALL4, [0, 2]),
        ("step_live", lambda t, kw: t.step_live(ring_, [0, 0], 3, **kw), SMALL4, [0, 0]),
        ("step_flow_live", lambda t, kw: t.step_flow_live(ring_, [1, 1], 3, **kw), LARGE4, [1, 1]),
    ]


def test_every_other_output_and_state_keeps_its_bits_with_all_options_on(mods, model, ring):
    _, A, P = mods
    every = dict(smooth=True, weights="score", best_shot=True, pose=True, views=True, exits=8, mesh=True,
                 flow=A.LandmarkFlow(levels=3))
    tr, plain = base.make(P, model, parts=True, openness=True, **every), base.make(P, model, **every)
    assert plain.parts is None and plain.open_opts is None and plain.openness is None and plain.part_faces is None
    assert isinstance(tr.parts, A.FaceParts) and isinstance(tr.open_opts, A.Openness)
    for t in (tr, plain):
        t.seed(list(range(CAP)), SMALL4)
    assert not hasattr(plain, "_part_buf") and not hasattr(plain, "_open_reset")       # nothing new is allocated
    for i, (name, call, boxes, _) in enumerate(ticks(ring)):
        for t in (tr, plain):
            base.pin(A, t, boxes)
        kw = dict(dt=0.04, frame_id=10 + i)
        got, want = call(tr, kw), call(plain, kw)
        assert len(got) == len(want) and all(same(a, b) for a, b in zip(got, want)), name
        for k in STATE:
            a, b = getattr(tr, k, None), getattr(plain, k, None)
            assert (a is None) == (b is None), (name, k)
            if a is not None:
                assert same(a, b), (name, k)
        n = int(got[0].shape[0])
        assert tuple(tr.part_faces.shape) == (n, 3, 32, 48, 3) and tr.part_faces.data_ptr() == tr._part_buf.data_ptr()
        assert tuple(tr.part_ok.shape) == (n, 3) and tuple(tr.part_M.shape) == (n, 3, 2, 3)
        assert tuple(tr.openness.shape) == (CAP, 3, 4) and tuple(tr.open_state.shape) == (CAP, 3, 8)
    assert bool((tr.open_state[..., 5] > 0).any())              # some measure of some face was read


def test_parts_and_openness_equal_the_stand_alone_calls(mods, model, ring):
    _, A, P = mods
    opts = A.Openness.default(68, min_closed=0.0, max_closed=10.0)
    tr = base.make(P, model, parts=True, openness=opts, best_shot=True, pose=True, mesh=True, flow=A.LandmarkFlow(levels=3))
    tr.seed(list(range(CAP)), SMALL4)
    th = dict(close_below=opts.close_below, open_above=opts.open_above, min_closed=0.0, max_closed=10.0)
    state_h = np.tile(np.array(ref.STATE_EMPTY), (CAP, 3, 1))
    rec_h = np.tile(np.array([-1.0, -1.0, 0.0, -1.0]), (CAP, 3, 1))
    reset_h = np.ones(CAP, np.int32)
    assert np.array_equal(tr._open_reset.cpu().numpy(), reset_h)
    assert np.array_equal(u64(tr.open_state.cpu().numpy()), u64(state_h)) and np.array_equal(u64(tr.openness.cpu().numpy()), u64(rec_h))
    warped = False
    for i, (name, call, boxes, fi) in enumerate(ticks(ring)):
        base.pin(A, tr, boxes)
        before = tr.boxes.clone().cpu().numpy()
        res = call(tr, dict(frame_id=10 + i))
        sl = (res[4] if len(res) > 4 else torch.arange(CAP, dtype=torch.int32)).cpu().numpy()
        n = len(sl)
        # ---- the parts: the stand-alone call on the returned landmarks, with the rows' ring slots and boxes
        idx = np.array([fi[s // SPS] if s >= 0 else 0 for s in sl], np.int32)
        bx = np.array([before[s] if s >= 0 else (0, 0, 0, 0) for s in sl], np.int32)
        m = torch.empty((n, 3, 2, 3), dtype=torch.float32, device="cuda")
        ok = torch.empty((n, 3), dtype=torch.int32, device="cuda")
        want = A.warp_parts_frames_device(ring, res[2], tr.parts, frame_index_dev=torch.from_numpy(idx).cuda(),
                                          boxes_dev=torch.from_numpy(bx).cuda(), affines_out=m, ok_out=ok)
        assert same(tr.part_faces, want) and same(tr.part_M, m) and same(tr.part_ok, ok), name
        m2, ok2 = A.part_affines_device(res[2], tr.parts)
        assert same(m, m2) and same(ok, ok2), name
        live = ok.bool().any(dim=1) & torch.from_numpy(sl >= 0).cuda()
        if bool(live.any()):
            warped = warped or bool((tr.part_faces[live] != 0).any())
        # ---- the openness: the stand-alone call at the slots, and the state of the reference
        alone = A.face_openness_device(res[2], opts).cpu().numpy()
        got = tr.openness.cpu().numpy()
        for r, s in enumerate(sl):
            if s >= 0:
                assert np.array_equal(u64(got[s]), u64(alone[r])), (name, r, s)
        ref.openness(res[2].cpu().numpy(), None, opts.measures, opts.min_width, th, slot=sl, rec=rec_h, state=state_h,
                     reset=reset_h, dt=opts.dt, status=res[3].cpu().numpy(), frame_id=10 + i)
        assert np.array_equal(u64(got), u64(rec_h)), name
        assert np.array_equal(u64(tr.open_state.cpu().numpy()), u64(state_h)), name
        assert np.array_equal(tr._open_reset.cpu().numpy(), reset_h), name
    assert warped and state_h[..., 5].max() > 0


def test_a_slot_that_sits_a_tick_out_keeps_state_and_pending_reset(mods, model, ring):
    _, A, P = mods
    tr = base.make(P, model, openness=True, parts=True)
    tr.seed(list(range(CAP)), SMALL4)
    res = tr.step_live(ring, [0, 0], 3)
    served = [int(s) for s in res[4].cpu().tolist() if s >= 0]
    left = sorted(set(range(CAP)) - set(served))
    assert len(served) == 3 and len(left) == 1
    reset = tr._open_reset.cpu().numpy()
    assert (reset[served] == 0).all() and reset[left[0]] == 1
    st = tr.open_state.cpu().numpy()
    assert (st[left[0]] == ref.STATE_EMPTY).all() and (tr.openness.cpu().numpy()[left[0]] == [-1.0, -1.0, 0.0, -1.0]).all()
    snap_state, snap_rec = tr.open_state.clone(), tr.openness.clone()
    tr.open_state[left[0]] = 5.0                                 # a mark the pending reset must wipe
    res = tr.step_live(ring, [0, 0], 3)                          # the waiting slot is served first
    served2 = [int(s) for s in res[4].cpu().tolist() if s >= 0]
    assert left[0] in served2
    assert int(tr._open_reset[left[0]]) == 0 and not bool((tr.open_state[left[0]] == 5.0).all())
    out = sorted(set(range(CAP)) - set(served2))                 # whoever sat this tick out kept every bit
    for s in out:
        assert same(tr.open_state[s], snap_state[s]) and same(tr.openness[s], snap_rec[s])
    # a birth through update resets the slot's state with the next tick that serves it
    tr2 = base.make(P, model, openness=True)
    tr2.update([None, [list(SMALL4[0])]])
    assert tr2._open_reset.cpu().tolist() == [0, 0, 1, 0]


def test_tracker_rejects_what_it_cannot_use(mods, model):
    _, A, P = mods
    with pytest.raises(ValueError):
        P.FaceTracker(model, (RH, RW), CAP, parts="eyes")
    with pytest.raises(ValueError):
        P.FaceTracker(model, (RH, RW), CAP, openness=0.2)
    t = P.FaceTracker(model, (RH, RW), CAP, parts=False, openness=False)
    assert t.parts is None and t.open_opts is None
    t = P.FaceTracker(model, (RH, RW), CAP, openness=True)
    t.step(torch.zeros((1, RH, RW, 3), dtype=torch.uint8, device="cuda"), 0, frame_id=5)    # frame_id without best_shot
    with pytest.raises(ValueError, match="frame_id goes with best_shot"):
        P.FaceTracker(model, (RH, RW), CAP).step(torch.zeros((1, RH, RW, 3), dtype=torch.uint8, device="cuda"), 0, frame_id=5)
