"""The tracking arithmetic of include/flm.h ("tracking") in plain numpy float64, restated line by line: every operation
is one IEEE add, multiply, divide, sqrt, floor or ceil on float64 scalars or arrays (numpy fuses nothing), float32 only
where the header writes (float).  What flm_track_seed, flm_landmarks_from_crop and flm_track_step must equal bit for bit.
"""
import numpy as np

f64, f32 = np.float64, np.float32
DEAD, FEW_POINTS, LOW_SCORE, SCALE, OUTSIDE = 1, 2, 4, 8, 16
IDENTITY = np.array([[1, 0, 0], [0, 1, 0]], f32)


def box_empty(box, fh, fw):
    """The clip of flm_landmarks_to_frame."""
    x0, y0, x1, y1 = [int(v) for v in box]
    cx0, cx1 = min(max(x0, 0), fw), min(max(x1, 0), fw)
    cy0, cy1 = min(max(y0, 0), fh), min(max(y1, 0), fh)
    return cx1 - cx0 <= 0 or cy1 - cy0 <= 0


def seed(boxes, in_h, in_w, fh, fw):
    """flm_track_seed: int32 [K,4] -> (float32 [K,2,3], int32 [K])."""
    boxes = np.asarray(boxes, np.int32).reshape(-1, 4)
    m = np.zeros((len(boxes), 2, 3), f32)
    status = np.zeros(len(boxes), np.int32)
    for f, (x0, y0, x1, y1) in enumerate(boxes.tolist()):
        if box_empty((x0, y0, x1, y1), fh, fw):
            m[f], status[f] = IDENTITY, DEAD
            continue
        sx = f64(in_w) / f64(x1 - x0)
        sy = f64(in_h) / f64(y1 - y0)
        m[f] = [[f32(sx), 0, f32((f64(0.5) - f64(x0)) * sx - f64(0.5))],
                [0, f32(sy), f32((f64(0.5) - f64(y0)) * sy - f64(0.5))]]
    return m, status


def back(m, x, y):
    """back() of the header: (x, y) float64 scalars or arrays in the matrix's target space -> (xf, yf, det) through
    the float32 [2,3] matrix m widened to float64."""
    m = np.asarray(m, f32).astype(f64)
    m00, m01, m02, m10, m11, m12 = m.reshape(6)
    with np.errstate(all="ignore"):
        det = m00 * m11 - m01 * m10
        u = x - m02
        v = y - m12
        xf = (m11 * u - m01 * v) / det
        yf = (m00 * v - m10 * u) / det
    return xf, yf, det


def landmarks_from_crop(lm, m, sx, sy):
    """flm_landmarks_from_crop: lm float64 [K,C,2] on the output grid, m float32 [K,2,3] -> float64 [K,C,2]."""
    lm = np.asarray(lm, f64)
    out = np.full(lm.shape, -1.0, f64)
    for f in range(lm.shape[0]):
        x, y = lm[f, :, 0], lm[f, :, 1]
        with np.errstate(all="ignore"):
            xf, yf, det = back(m[f], x * f64(sx), y * f64(sy))
            if not np.isfinite(det) or det == 0.0:
                continue
            bad = (x < 0) | (y < 0) | (xf < 0) | (yf < 0) | ~np.isfinite(xf) | ~np.isfinite(yf)
        out[f, :, 0] = np.where(bad, -1.0, xf)
        out[f, :, 1] = np.where(bad, -1.0, yf)
    return out


def fit(p, w, t):
    """flm_similarity_from_landmarks_weighted with sx = sy = 1 for one face: p [C,2], w [C] (None: ones), t [C,2]
    -> (float32 [2,3], cnt, W)."""
    c = p.shape[0]
    w = np.ones(c, f64) if w is None else np.asarray(w, f64)
    idx = [i for i in range(c) if p[i, 0] >= 0.0 and p[i, 1] >= 0.0 and w[i] > 0.0]
    mpx = mpy = mqx = mqy = wsum = f64(0)
    with np.errstate(all="ignore"):
        for i in idx:
            mpx = mpx + w[i] * p[i, 0]
            mpy = mpy + w[i] * p[i, 1]
            mqx = mqx + w[i] * t[i, 0]
            mqy = mqy + w[i] * t[i, 1]
            wsum = wsum + w[i]
        a, b, tx, ty = f64(1), f64(0), f64(0), f64(0)
        if len(idx) >= 2:
            mpx, mpy, mqx, mqy = mpx / wsum, mpy / wsum, mqx / wsum, mqy / wsum
            sa = sb = var = f64(0)
            for i in idx:
                px, py = p[i, 0] - mpx, p[i, 1] - mpy
                qx, qy = t[i, 0] - mqx, t[i, 1] - mqy
                sa = sa + w[i] * (px * qx + py * qy)
                sb = sb + w[i] * (px * qy - py * qx)
                var = var + w[i] * (px * px + py * py)
            if var > 0.0:
                a = sa / var
                b = sb / var
                tx = mqx - (a * mpx - b * mpy)
                ty = mqy - (b * mpx + a * mpy)
        m = np.array([[f32(a), f32(-b), f32(tx)], [f32(b), f32(a), f32(ty)]], f32)
    return m, len(idx), wsum


def _cl(t):
    return int(min(max(t, f64(-2.0 ** 30)), f64(2.0 ** 30)))


def step(lm, w, m_crop, boxes, sx, sy, in_h, in_w, fh, fw, tmpl_crop, tmpl_align=None, min_points=2, min_score=0.0,
         min_side=0.0, max_side=np.inf):
    """flm_track_step -> dict(lm_frame, m_align (None without tmpl_align), m_next, boxes_next, status)."""
    lm = np.asarray(lm, f64)
    k, c = lm.shape[:2]
    boxes = np.asarray(boxes, np.int32).reshape(k, 4)
    lm_frame = landmarks_from_crop(lm, m_crop, sx, sy)
    m_align = None if tmpl_align is None else np.zeros((k, 2, 3), f32)
    m_next = np.zeros((k, 2, 3), f32)
    boxes_next = np.zeros((k, 4), np.int32)
    status = np.zeros(k, np.int32)
    for f in range(k):
        dead = box_empty(boxes[f], fh, fw)
        if dead:
            lm_frame[f] = -1.0
        wf = None if w is None else np.asarray(w, f64)[f]
        if tmpl_align is not None:
            m_align[f] = fit(lm_frame[f], wf, tmpl_align)[0]
        mn, cnt, wsum = fit(lm_frame[f], wf, tmpl_crop)
        st = DEAD if dead else 0
        if cnt < min_points:
            st |= FEW_POINTS
        with np.errstate(all="ignore"):
            if w is not None and not (f64(wsum) / f64(cnt) >= min_score):
                st |= LOW_SCORE
            a, b = f64(mn[0, 0]), f64(mn[1, 0])
            side = f64(in_w) / np.sqrt(a * a + b * b)
        if not (side >= min_side and side <= max_side):
            st |= SCALE
        ex, ey = f64(in_w - 1), f64(in_h - 1)
        cx, cy, det = back(mn, ex / f64(2), ey / f64(2))
        if not (np.isfinite(det) and det != 0.0 and 0.0 <= cx <= f64(fw - 1) and 0.0 <= cy <= f64(fh - 1)):
            st |= OUTSIDE
        status[f] = st
        if st:
            m_next[f] = IDENTITY
            continue
        m_next[f] = mn
        corners = [back(mn, x, y)[:2] for x, y in ((f64(0), f64(0)), (ex, f64(0)), (f64(0), ey), (ex, ey))]
        mnx, mny = corners[0]
        mxx, mxy = corners[0]
        for x, y in corners[1:]:
            mnx = x if x < mnx else mnx
            mny = y if y < mny else mny
            mxx = x if x > mxx else mxx
            mxy = y if y > mxy else mxy
        boxes_next[f] = [_cl(np.floor(mnx)), _cl(np.floor(mny)), _cl(np.ceil(mxx) + f64(1)), _cl(np.ceil(mxy) + f64(1))]
    return dict(lm_frame=lm_frame, m_align=m_align, m_next=m_next, boxes_next=boxes_next, status=status)


def apply(m, pts):
    """pts [C,2] through the float32 [2,3] matrix m, in float64 (for the tests' own geometry, not part of the contract)."""
    m = np.asarray(m, f32).astype(f64)
    return pts @ m[:, :2].T + m[:, 2]
