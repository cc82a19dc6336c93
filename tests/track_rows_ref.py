"""flm_track_gather_streams, flm_track_step_rows and flm_track_best_update_rows of include/flm.h ("rows") in plain numpy:
a loop over the rows around tests/track_ref.py, tests/track_filter_ref.py and tests/face_quality_ref.py, one face at a
time, plus the two rules the rows add -- a row whose dt is not > 0 and finite has no history, and an inert row (a slot
outside [0, n_slots)) writes its compact outputs and nothing else.  What the three calls must equal bit for bit.
"""
import numpy as np

import face_quality_ref as qref
import track_filter_ref as fref
import track_ref

f64, f32 = np.float64, np.float32
DEAD = track_ref.DEAD


def gather_streams(active, s, k, m_crop, boxes, frame_idx_stream=None, dt_stream=None, best_q=None, reset=None):
    """flm_track_gather_streams -> dict(slot, m, boxes, frame_index, dt, best_q, reset (each present with its input),
    reset_global: `reset` after the call, or None).  The inputs are not modified."""
    active = [int(v) for v in active]
    n = len(active) * k
    out = dict(slot=np.full(n, -1, np.int32), m=np.tile(track_ref.IDENTITY, (n, 1, 1)).astype(f32),
               boxes=np.zeros((n, 4), np.int32), frame_index=np.zeros(n, np.int32),
               dt=None if dt_stream is None else np.zeros(n, f64),
               best_q=None if best_q is None else np.full(n, -1.0, f64),
               reset=None if reset is None else np.zeros(n, np.int32),
               reset_global=None if reset is None else np.array(reset, np.int32))
    for a, sid in enumerate(active):
        if not 0 <= sid < s:
            continue
        for j in range(k):
            r, g = a * k + j, sid * k + j
            out["slot"][r] = g
            out["m"][r] = m_crop[g]
            out["boxes"][r] = boxes[g]
            if frame_idx_stream is not None:
                out["frame_index"][r] = frame_idx_stream[sid]
            if dt_stream is not None:
                out["dt"][r] = dt_stream[sid]
            if best_q is not None:
                out["best_q"][r] = best_q[g]
            if reset is not None:
                out["reset"][r] = reset[g]
                out["reset_global"][g] = 0
    return out


def dt_ok(dt):
    return bool(dt > 0.0 and np.isfinite(dt))


def step_rows(lm, w, m_crop_c, boxes_c, slot, sx, sy, in_h, in_w, fh, fw, tmpl_crop, tmpl_align, m_next, boxes_next, status,
              state=None, dt=None, filt=None, **limits):
    """flm_track_step_rows.  lm [N,C,2], w None or [N,C], m_crop_c, boxes_c, slot [N]; m_next, boxes_next, status and
    state (None without `filt`) are the GLOBAL tensors, not modified; dt: a scalar or [N]; filt: None or a dict of
    min_cutoff, beta, d_cutoff.  -> dict(lm_frame, m_align (None without tmpl_align), lm_raw (None without filt),
    status_rows, and the new global m_next, boxes_next, status, state)."""
    lm = np.asarray(lm, f64)
    n, c = lm.shape[:2]
    n_slots = len(status)
    out = dict(lm_frame=np.full((n, c, 2), -1.0, f64),
               m_align=None if tmpl_align is None else np.tile(track_ref.IDENTITY, (n, 1, 1)).astype(f32),
               lm_raw=None if filt is None else np.full((n, c, 2), -1.0, f64), status_rows=np.full(n, DEAD, np.int32),
               m_next=np.array(m_next, f32), boxes_next=np.array(boxes_next, np.int32), status=np.array(status, np.int32),
               state=None if filt is None else np.array(state, f64))
    for r in range(n):
        g = int(slot[r])
        if not 0 <= g < n_slots:
            continue                                        # inert: the compact outputs above, nothing global
        one = slice(r, r + 1)
        wr = None if w is None else np.asarray(w, f64)[one]
        if filt is None:
            res = track_ref.step(lm[one], wr, m_crop_c[one], boxes_c[one], sx, sy, in_h, in_w, fh, fw, tmpl_crop, tmpl_align,
                                 **limits)
        else:
            dtr = f64(dt if np.ndim(dt) == 0 else dt[r])
            st = out["state"][g:g + 1]
            if not dt_ok(dtr):                              # the one new rule: no point of the row has a history
                st, dtr = fref.empty_state(1, c), f64(1.0)
            res = fref.step(lm[one], wr, m_crop_c[one], boxes_c[one], sx, sy, in_h, in_w, fh, fw, tmpl_crop, tmpl_align, st,
                            dtr, **filt, **limits)
            out["state"][g] = res["state"][0]
            out["lm_raw"][r] = res["lm_raw"][0]
        out["lm_frame"][r] = res["lm_frame"][0]
        if tmpl_align is not None:
            out["m_align"][r] = res["m_align"][0]
        out["status_rows"][r] = out["status"][g] = res["status"][0]
        out["m_next"][g] = res["m_next"][0]
        out["boxes_next"][g] = res["boxes_next"][0]
    return out


def best_update_rows(state, faces, rec, lm, slot, best_q_c, frame_id, w=None, factor=None, status_rows=None, reset_c=None,
                     m=None, sharp_ref=100.0, min_exposed=0.5, with_m=True, with_lm=True, with_rec=True):
    """flm_track_best_update_rows on `state` (the dict of face_quality_ref.new_state over n_slots, in place); -> taken
    bool [N].  with_m, with_lm, with_rec: whether best_m, best_lm, best_rec were given."""
    n = rec.shape[0]
    n_slots = len(state["best_q"])
    q, ok = qref.quality(rec, lm, w, factor, status_rows, sharp_ref, min_exposed)
    taken = np.zeros(n, bool)
    for r in range(n):
        g = int(slot[r])
        if not 0 <= g < n_slots:
            continue
        prev = f64(-1.0) if (reset_c is not None and reset_c[r] != 0) else f64(best_q_c[r])
        if ok[r] and q[r] > prev:
            taken[r] = True
            state["gallery"][g] = faces[r]
            state["best_q"][g] = q[r]
            state["best_frame"][g] = frame_id
            if m is not None and with_m:
                state["best_m"][g] = m[r]
            if with_lm:
                state["best_lm"][g] = lm[r]
            if with_rec:
                state["best_rec"][g] = rec[r]
        else:
            state["best_q"][g] = prev
    return taken
