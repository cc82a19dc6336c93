"""The numpy restatement of flm_track_gather_flow, flm_landmark_flow_rows and flm_track_flow_history_put (include/flm.h,
"the flow tick on rows").  The forward pass of a point is tests/flow_ref.py's flow_point; the backward pass of the
forward-backward check is stated here: exact integers for everything summed over a window, Python floats (IEEE float64,
one operation per operator, nothing fused) for the closed form, in the order the header writes.  The device equals this
bit for bit."""
import math

import numpy as np

import flow_ref
from flow_ref import LOW_TEXTURE, NO_HISTORY, NOT_FINITE, sample

FB = 64
QUIET_NAN = np.uint64(0x7ff8000000000000)


def backward(prev, cur, qx, qy, o):
    """The backward pass: "for l = levels-1 down to 0" of flm_landmark_flow with the two images exchanged, from p0' = q
    in crop px (no matrix).  prev, cur: the level lists of the two crops -> (q'x, q'y, flags: LOW_TEXTURE / NOT_FINITE)."""
    r, levels = o["radius"], o["levels"]
    n = (2 * r + 1) ** 2
    jj, ii = np.meshgrid(np.arange(-r, r + 1, dtype=np.float64), np.arange(-r, r + 1, dtype=np.float64), indexing="ij")
    flags = 0
    bx = by = 0.0
    for l in range(levels - 1, -1, -1):
        s = float(1 << l)
        px, py = (qx + 0.5) / s - 0.5, (qy + 0.5) / s - 0.5
        if l == levels - 1:
            bx, by = px, py
        P, Q = cur[l], prev[l]                       # exchanged: the window is taken from the current image
        T = sample(P, px + ii, py + jj)
        gx = sample(P, px + (ii + 1.0), py + jj) - sample(P, px + (ii - 1.0), py + jj)
        gy = sample(P, px + ii, py + (jj + 1.0)) - sample(P, px + ii, py + (jj - 1.0))
        A, B, C = float(int((gx * gx).sum())), float(int((gx * gy).sum())), float(int((gy * gy).sum()))
        det = A * C - B * B
        e = (((A + C) - math.sqrt((A - C) * (A - C) + 4.0 * B * B)) / 2.0) / (float(n) * 4194304.0)
        if not e >= o["min_eig"]:
            if l == 0:
                flags |= LOW_TEXTURE
        else:
            for _ in range(o["max_iter"]):
                D = T - sample(Q, bx + ii, by + jj)
                sx, sy = float(int((D * gx).sum())), float(int((D * gy).sum()))
                with np.errstate(all="ignore"):
                    dx = float(np.float64(2.0 * (C * sx - B * sy)) / np.float64(det))
                    dy = float(np.float64(2.0 * (A * sy - B * sx)) / np.float64(det))
                bx, by = bx + dx, by + dy
                if not (-flow_ref.REACH <= bx <= flow_ref.REACH and -flow_ref.REACH <= by <= flow_ref.REACH):
                    return bx, by, flags | NOT_FINITE
                if dx * dx + dy * dy < o["eps"] * o["eps"]:
                    break
        if l > 0:
            bx, by = 2.0 * bx + 0.5, 2.0 * by + 0.5
    return bx, by, flags


def _p0(m, x, y):
    mm = [[float(v) for v in row] for row in np.asarray(m, np.float32)]
    return (mm[0][0] * x + mm[0][1] * y) + mm[0][2], (mm[1][0] * x + mm[1][1] * y) + mm[1][2]


def rows_point(prev, cur, m, x, y, o, max_fb):
    """One point of flm_landmark_flow_rows -> (qx, qy, err, fb2, flags) before the output rule."""
    qx, qy, err, flags = flow_ref.flow_point(prev, cur, m, x, y, o)
    if flags or not max_fb > 0.0:
        return qx, qy, err, -1.0, flags
    bx, by, bflags = backward(prev, cur, qx, qy, o)
    if bflags & NOT_FINITE:
        return qx, qy, err, -1.0, FB
    p0x, p0y = _p0(m, float(x), float(y))
    ex, ey = bx - p0x, by - p0y
    fb2 = ex * ex + ey * ey
    if bflags & LOW_TEXTURE or not fb2 <= max_fb * max_fb:
        return qx, qy, err, fb2, FB
    return qx, qy, err, fb2, 0


def landmark_flow_rows(prev_crops, cur_crops, slot, lm_prev, m, o, max_fb=0.0, w_prev=None):
    """prev_crops, cur_crops uint8 [N,H,W(,3)]; slot int32 [N]; lm_prev float64 [n_slots,C,2] frame px and w_prev None or
    float64 [n_slots,C], read at the slot; m float32 [N,2,3] -> (lm [N,C,2], w [N,C], err int32 [N,C], fb float64 [N,C],
    flags int32 [N,C]) as flm_landmark_flow_rows writes them."""
    lm_prev = np.asarray(lm_prev, np.float64)
    n_slots, c = lm_prev.shape[:2]
    n = len(slot)
    lm = np.full((n, c, 2), -1.0)
    wt = np.zeros((n, c))
    err = np.full((n, c), -1, np.int32)
    fb = np.full((n, c), -1.0)
    flags = np.full((n, c), NO_HISTORY, np.int32)
    yp, yc = flow_ref.luma(prev_crops), flow_ref.luma(cur_crops)
    for r in range(n):
        g = int(slot[r])
        if not 0 <= g < n_slots:
            continue
        pp, pc = flow_ref.pyramid(yp[r], o["levels"]), flow_ref.pyramid(yc[r], o["levels"])
        for i in range(c):
            qx, qy, e, f2, fl = rows_point(pp, pc, m[r], lm_prev[g, i, 0], lm_prev[g, i, 1], o, max_fb)
            err[r, i], fb[r, i], flags[r, i] = e, f2, fl
            if fl == 0:
                lm[r, i] = (qx, qy)
                wt[r, i] = 1.0 if w_prev is None else w_prev[g, i]
    return lm, wt, err, fb, flags


def box_empty(b, fh, fw):
    x0, y0, x1, y1 = [int(v) for v in b]
    cx0, cx1 = min(max(x0, 0), fw), min(max(x1, 0), fw)
    cy0, cy1 = min(max(y0, 0), fh), min(max(y1, 0), fh)
    return cx1 - cx0 <= 0 or cy1 - cy0 <= 0


def gather_flow(a):
    """flm_track_gather_flow on a dict of numpy arrays under the names of include/flm.h (s, k, fh, fw, n, dt; stream_on,
    frame_idx_stream, dt_stream, best_q, reset, age, cursor: each an array or None; m_crop, boxes, flow_frame,
    flow_ready).  Returns a dict of every tensor the call writes: the in/out ones as they are afterwards (copies) and the
    compact ones."""
    s, k, fh, fw, n = a["s"], a["k"], a["fh"], a["fw"], a["n"]
    ns = s * k
    opt = lambda name: None if a.get(name) is None else np.array(a[name], copy=True)
    reset, age, cursor, ready = opt("reset"), opt("age"), opt("cursor"), np.array(a["flow_ready"], copy=True)
    on_of = lambda i: a.get("stream_on") is None or a["stream_on"][i] != 0
    c0 = 0 if cursor is None else int(cursor[0])
    if not 0 <= c0 < ns:
        c0 = 0
    out = dict(slot_c=np.full(n, -1, np.int32), m_c=np.tile(np.array([[1, 0, 0], [0, 1, 0]], np.float32), (n, 1, 1)),
               boxes_c=np.zeros((n, 4), np.int32), frame_idx_c=np.zeros(n, np.int32), prev_frame_idx_c=np.zeros(n, np.int32))
    if age is not None:
        out["dt_c"] = np.zeros(n)
    if a.get("best_q") is not None:
        out["best_q_c"] = np.full(n, -1.0)
    if reset is not None:
        out["reset_c"] = np.zeros(n, np.int32)
    n_live = n_elig = 0
    last = 0
    for p in range(ns):
        g = (c0 + p) % ns
        i = g // k
        if not on_of(i):
            continue
        live = not box_empty(a["boxes"][g], fh, fw)
        elig = live and a["flow_ready"][g] != 0
        served = elig and n_elig < n
        d, good = 0.0, False
        if age is not None:
            d = float(a["dt_stream"][i]) if a.get("dt_stream") is not None else float(a["dt"])
            good = d > 0.0 and math.isfinite(d)
        if served:
            r = n_elig
            out["slot_c"][r] = g
            out["m_c"][r] = a["m_crop"][g]
            out["boxes_c"][r] = a["boxes"][g]
            out["frame_idx_c"][r] = 0 if a.get("frame_idx_stream") is None else a["frame_idx_stream"][i]
            out["prev_frame_idx_c"][r] = a["flow_frame"][g]
            if "best_q_c" in out:
                out["best_q_c"][r] = a["best_q"][g]
            if reset is not None:
                out["reset_c"][r] = reset[g]
                reset[g] = 0
            if age is not None:
                with np.errstate(all="ignore"):
                    out["dt_c"][r] = np.float64(d) + age[g] if good else d
                age[g] = 0.0
            if r == n - 1:
                last = g
        elif age is not None:
            if not live:
                age[g] = 0.0
            elif good:
                with np.errstate(all="ignore"):
                    age[g] = age[g] + np.float64(d)
            else:
                age.view(np.uint64)[g] = QUIET_NAN
        ready[g] = 0
        n_live += int(live)
        n_elig += int(elig)
    served = min(n_elig, n)
    nxt = c0
    if n_elig > n:
        nxt = (last + 1) % ns
    out["counts"] = np.array([n_live, n_elig, served, n_elig - served, n_live - n_elig, nxt], np.int32)
    if cursor is not None:
        cursor[0] = nxt
    out.update(flow_ready=ready)
    for name, v in (("reset", reset), ("age", age), ("cursor", cursor)):
        if v is not None:
            out[name] = v
    return out


def history_put(slot, status_rows, frame_idx_c, flow_frame, flow_ready, lm_rows=None, hist_lm=None, w_rows=None, hist_w=None):
    """flm_track_flow_history_put -> (hist_lm, hist_w, flow_frame, flow_ready) afterwards (copies; None where not given)."""
    cp = lambda x: None if x is None else np.array(x, copy=True)
    hist_lm, hist_w, flow_frame, flow_ready = cp(hist_lm), cp(hist_w), cp(flow_frame), cp(flow_ready)
    for r, g in enumerate(slot):
        if not 0 <= g < len(flow_ready):
            continue
        if status_rows[r] != 0:
            flow_ready[g] = 0
            continue
        if lm_rows is not None:
            hist_lm[g] = lm_rows[r]
            if w_rows is not None:
                hist_w[g] = w_rows[r]
        flow_frame[g] = frame_idx_c[r]
        flow_ready[g] = 1
    return hist_lm, hist_w, flow_frame, flow_ready
