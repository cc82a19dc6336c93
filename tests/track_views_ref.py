"""numpy restatement of the pose-binned best shots as include/flm.h ("pose-binned best shots") states them: the bin of a
face, flm_track_views_update and flm_track_exit_views.  The quality arithmetic is that of tests/face_quality_ref.py.  What
the device must equal bit for bit.  No device, no library.

    bin_of(pose_row, u_edges, v_edges)                       -> the bin, or -1 for a face that is not binned
    new_state(n_slots, bins, face_shape, dtype, c)           -> dict of the in/out arrays
    update(state, faces, rec, lm, pose, frame_id, ...)       -> edits `state` in place, returns take int32 [N]
    exit_views(state, ring, exit_row)                        -> edits `ring` in place
"""
import numpy as np

import face_quality_ref as qref

f32, f64 = np.float32, np.float64
POSE_REC = 18


def bin_of(pose_row, u_edges, v_edges):
    ok = pose_row[14] == 1.0
    u, v = -f64(pose_row[6]), f64(pose_row[7])
    if not ok or np.isnan(u) or np.isnan(v):
        return -1
    iu = sum(1 for e in u_edges if u >= f64(e))
    iv = sum(1 for e in v_edges if v >= f64(e))
    return iv * (len(u_edges) + 1) + iu


def n_bins(u_edges, v_edges):
    return (len(u_edges) + 1) * (len(v_edges) + 1)


def new_state(n_slots, bins, face_shape, dtype, c, fill=None):
    """The tracker-side state; fill: None for the empty state, or a byte every array is filled with."""
    s = dict(view_q=np.full((n_slots, bins), -1.0, f64), view_frame=np.full((n_slots, bins), -1, np.int64),
             view_gallery=np.zeros((n_slots, bins) + tuple(face_shape), dtype),
             view_m=np.zeros((n_slots, bins, 2, 3), f32), view_lm=np.full((n_slots, bins, c, 2), -1.0, f64),
             view_pose=np.zeros((n_slots, bins, POSE_REC), f64))
    if fill is not None:
        for v in s.values():
            v.view(np.uint8)[...] = fill
    return s


def update(state, faces, rec, lm, pose, frame_id, u_edges, v_edges, w=None, status=None, reset=None, m=None, slot=None,
           sharp_ref=100.0, min_exposed=0.5):
    """One flm_track_views_update on `state` (in place); -> take int32 [N].  Arrays of `state` that are None are not
    written (the optional view_m, view_lm, view_pose)."""
    n = rec.shape[0]
    n_slots = state["view_q"].shape[0]
    q, ok = qref.quality(rec, lm, w, None, status, sharp_ref, min_exposed)
    take = np.full(n, -1, np.int32)
    for r in range(n):
        g = r if slot is None else int(slot[r])
        if not 0 <= g < n_slots:
            continue
        if reset is not None and reset[r] != 0:
            state["view_q"][g, :] = -1.0
        b = bin_of(pose[g], u_edges, v_edges)
        if not ok[r] or b < 0 or not q[r] > state["view_q"][g, b]:
            continue
        take[r] = b
        state["view_q"][g, b] = q[r]
        state["view_frame"][g, b] = frame_id
        state["view_gallery"][g, b] = faces[r]
        if state.get("view_m") is not None:
            state["view_m"][g, b] = m[r]
        if state.get("view_lm") is not None:
            state["view_lm"][g, b] = lm[r]
        if state.get("view_pose") is not None:
            state["view_pose"][g, b] = pose[g]
    return take


def exit_views(state, ring, exit_row):
    """flm_track_exit_views: `ring` holds x_view_q, x_view_frame, x_view_gallery and the optional x_view_m, x_view_lm,
    x_view_pose (None: not given), `state` their sources."""
    q_rows = ring["x_view_q"].shape[0]
    for t in range(len(exit_row)):
        row = int(exit_row[t])
        if not 0 <= row < q_rows:
            continue
        ring["x_view_q"][row] = state["view_q"][t]
        ring["x_view_frame"][row] = state["view_frame"][t]
        for b in range(state["view_q"].shape[1]):
            if not state["view_q"][t, b] >= 0.0:
                continue
            ring["x_view_gallery"][row, b] = state["view_gallery"][t, b]
            for name in ("view_m", "view_lm", "view_pose"):
                if ring.get("x_" + name) is not None:
                    ring["x_" + name][row, b] = state[name][t, b]
