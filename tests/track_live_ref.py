"""flm_track_gather_live of include/flm.h in plain numpy: a loop over the slots in the cyclic order of the contract, one
slot at a time.  The call has only integer work and one float64 add per slot, so the device must equal this bit for bit.
"""
import numpy as np

import track_ref

f64, f32 = np.float64, np.float32


def box_empty(b, fh, fw):
    """The clip of flm_landmarks_to_frame, and the DEAD test of flm_track_step on it."""
    x0, y0, x1, y1 = [int(v) for v in b]
    cx0, cy0 = min(max(x0, 0), fw), min(max(y0, 0), fh)
    cx1, cy1 = min(max(x1, 0), fw), min(max(y1, 0), fh)
    return cx1 - cx0 <= 0 or cy1 - cy0 <= 0


def good(d):
    return bool(d > 0.0 and np.isfinite(d))


def gather_live(m_crop, boxes, s, k, fh, fw, n, stream_on=None, frame_idx_stream=None, dt_stream=None, dt=None,
                best_q=None, reset=None, age=None, cursor=None):
    """flm_track_gather_live -> dict(slot, m, boxes, frame_index, counts; dt, best_q, reset, each present with its input
    (age, best_q, reset); reset_global, age_global, cursor_global: the in/out tensors after the call, or None).  cursor: None
    or an integer.  The inputs are not modified."""
    total = s * k
    out = dict(slot=np.full(n, -1, np.int32), m=np.tile(track_ref.IDENTITY, (n, 1, 1)).astype(f32),
               boxes=np.zeros((n, 4), np.int32), frame_index=np.zeros(n, np.int32),
               dt=None if age is None else np.zeros(n, f64),
               best_q=None if best_q is None else np.full(n, -1.0, f64),
               reset=None if reset is None else np.zeros(n, np.int32),
               reset_global=None if reset is None else np.array(reset, np.int32),
               age_global=None if age is None else np.array(age, f64), cursor_global=None)
    c0 = 0 if cursor is None or not 0 <= int(cursor) < total else int(cursor)
    on = lambda g: stream_on is None or stream_on[g // k] != 0
    eligible = [g for g in [(c0 + p) % total for p in range(total)] if on(g) and not box_empty(boxes[g], fh, fw)]
    served = eligible[:n]
    for r, g in enumerate(served):
        i = g // k
        out["slot"][r] = g
        out["m"][r] = m_crop[g]
        out["boxes"][r] = boxes[g]
        if frame_idx_stream is not None:
            out["frame_index"][r] = frame_idx_stream[i]
        if best_q is not None:
            out["best_q"][r] = best_q[g]
        if reset is not None:
            out["reset"][r] = reset[g]
            out["reset_global"][g] = 0
    if age is not None:
        row = {g: r for r, g in enumerate(served)}
        live = set(eligible)
        for g in range(total):
            if not on(g):
                continue
            d = f64(dt if dt_stream is None else dt_stream[g // k])
            if g in row:
                with np.errstate(invalid="ignore", over="ignore"):
                    out["dt"][row[g]] = d + f64(age[g]) if good(d) else d
                out["age_global"][g] = 0.0
            elif g in live:
                with np.errstate(invalid="ignore", over="ignore"):
                    out["age_global"][g] = f64(age[g]) + d if good(d) else np.nan
            else:
                out["age_global"][g] = 0.0
    e = len(eligible)
    nxt = (served[-1] + 1) % total if e > n else c0
    out["counts"] = np.array([e, len(served), e - len(served), nxt], np.int32)
    if cursor is not None:
        out["cursor_global"] = nxt
    return out
