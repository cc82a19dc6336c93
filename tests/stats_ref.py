"""CPU restatements for the landmark-record tests (TEST INFRASTRUCTURE ONLY): the record of include/flm.h
(x, y, score, var_x, var_y, cov_xy) in float64 on oracle/decode_ref.py's chain for hsum, x and y, and the weighted
similarity fit as sequential float64 sums in landmark order."""
import numpy as np

from oracle import decode_ref

REC = 6


def topn_record_ref(hmi, n_points, thresh, order=None):
    """One map [H,W] float32 -> the six record values of the top-n mode.  x, y come from decode_ref.get_average_xy_ref
    itself; hsum is its float32 chain (ascending (value, flat index) order = list ranks n-1 .. 0) repeated for the
    score; the moments are the second walk in the same order.  `order`: the map's stable argsort, when the caller
    already has it."""
    h, w = hmi.shape
    if order is None:
        order = hmi.argsort(axis=None, kind="stable")
    ind = order[-n_points:]
    with np.errstate(all="ignore"):
        x, y = decode_ref.get_average_xy_ref(hmi, n_points, thresh, order)
        hsum = np.float32(0)
        for i in ind:
            hsum = np.float32(hsum + hmi.flat[i])
        score = float(np.float32(hsum / np.float32(n_points)))
    if np.float32(hsum / np.float32(n_points)) <= thresh:
        return [-1.0, -1.0, score, -1.0, -1.0, 0.0]
    x, y = float(x), float(y)
    vxx = vyy = vxy = 0.0
    for i in ind:
        hv = float(hmi.flat[i])
        dx, dy = float(i % w) - x, float(i // w) - y
        vxx += hv * (dx * dx)
        vyy += hv * (dy * dy)
        vxy += hv * (dx * dy)
    hs = float(hsum)
    return [x, y, score, vxx / hs, vyy / hs, vxy / hs]


def all_pixel_record_ref(hmi, thresh):
    """One map [H,W] float32 -> (record, score of numpy's float32 sum).  float64 sums throughout; hsum is rounded to
    float32 once, as the device rounds it, before the divisions.  The second value is float32(np.sum(hmi)) / float32(H*W),
    what utils/metrics.py:60,78 computes."""
    h, w = hmi.shape
    d = hmi.astype(np.float64)
    cols = np.arange(w, dtype=np.float64)[None, :]
    rows = np.arange(h, dtype=np.float64)[:, None]
    hsum = np.float32(d.sum())
    score = float(np.float32(hsum / np.float32(h * w)))
    score_np = float(np.float32(np.sum(hmi) / np.float32(h * w)))
    if np.float32(hsum / np.float32(h * w)) <= thresh:
        return [-1.0, -1.0, score, -1.0, -1.0, 0.0], score_np
    hs = float(hsum)
    x, y = float((d * cols).sum()) / hs, float((d * rows).sum()) / hs
    var_x = max(0.0, float((d * cols * cols).sum()) / hs - x * x)
    var_y = max(0.0, float((d * rows * rows).sum()) / hs - y * y)
    cov = float((d * cols * rows).sum()) / hs - x * y
    return [x, y, score, var_x, var_y, cov], score_np


def records_ref(y, n_points, thresh, orders=None):
    """[N,H,W,L] float32 -> float64 [N,L,6] (and, in all-pixel mode, the [N,L] numpy-sum scores)."""
    n, h, w, l = y.shape
    out = np.zeros((n, l, REC), np.float64)
    score_np = np.zeros((n, l), np.float64)
    for f in range(n):
        for c in range(l):
            hmi = np.ascontiguousarray(y[f, :, :, c])
            if n_points < 1:
                out[f, c], score_np[f, c] = all_pixel_record_ref(hmi, thresh)
            else:
                out[f, c] = topn_record_ref(hmi, n_points, thresh, None if orders is None else orders[f][c])
    return (out, score_np) if n_points < 1 else out


def stable_orders(y):
    """The stable argsort of every map of [N,H,W,L], computed once for all n_points."""
    n, h, w, l = y.shape
    return [[np.ascontiguousarray(y[f, :, :, c]).argsort(axis=None, kind="stable") for c in range(l)] for f in range(n)]


def weighted_similarity_ref(lm, tmpl, weights=None, scale=(1.0, 1.0)):
    """include/flm.h, flm_similarity_from_landmarks_weighted, term by term: lm [N,K,2], tmpl [K,2], weights [N,K] or
    None (all ones) -> float32 [N,2,3]."""
    n, k, _ = lm.shape
    out = np.zeros((n, 2, 3), np.float32)
    for f in range(n):
        p = [[(v if v < 0.0 else v * s) for v, s in zip((float(lm[f, i, 0]), float(lm[f, i, 1])), scale)] for i in range(k)]
        w = [1.0 if weights is None else float(weights[f, i]) for i in range(k)]
        ok = [i for i in range(k) if p[i][0] >= 0.0 and p[i][1] >= 0.0 and w[i] > 0.0]
        a, b, tx, ty = 1.0, 0.0, 0.0, 0.0
        if len(ok) >= 2:
            mpx = mpy = mqx = mqy = wsum = 0.0
            for i in ok:
                mpx += w[i] * p[i][0]; mpy += w[i] * p[i][1]
                mqx += w[i] * float(tmpl[i, 0]); mqy += w[i] * float(tmpl[i, 1])
                wsum += w[i]
            mpx /= wsum; mpy /= wsum; mqx /= wsum; mqy /= wsum
            sa = sb = var = 0.0
            for i in ok:
                px, py = p[i][0] - mpx, p[i][1] - mpy
                qx, qy = float(tmpl[i, 0]) - mqx, float(tmpl[i, 1]) - mqy
                sa += w[i] * (px * qx + py * qy)
                sb += w[i] * (px * qy - py * qx)
                var += w[i] * (px * px + py * py)
            if var > 0.0:
                a, b = sa / var, sb / var
                tx = mqx - (a * mpx - b * mpy)
                ty = mqy - (b * mpx + a * mpy)
        out[f] = [[a, -b, tx], [b, a, ty]]
    return out


def similarity_case(seed=31):
    """The meaning check's data: landmarks that are an exact similarity of the 68-point template (true M maps them onto
    it), 10 of them displaced by 40 px and given weight 1e-6.  Returns (lm [1,68,2], template, weights [1,68], true M)."""
    from flm_amd import alignment
    rng = np.random.default_rng(seed)
    tm = alignment.canonical_template(68, 256, 256)
    s, th, tx, ty = 1.25, 0.3, 12.0, -7.0
    a, b = s * np.cos(th), s * np.sin(th)
    m = np.array([[a, -b, tx], [b, a, ty]], np.float64)
    inv = np.linalg.inv(np.array([[a, -b], [b, a]]))
    lm = (tm - np.array([tx, ty])) @ inv.T + 60.0        # (+60: every coordinate positive; folded into the true tx, ty)
    m[:, 2] -= m[:, :2] @ np.array([60.0, 60.0])
    bad = rng.choice(68, 10, replace=False)
    ang = rng.uniform(0, 2 * np.pi)
    lm[bad] += 40.0 * np.array([np.cos(ang), np.sin(ang)])
    w = np.ones((1, 68), np.float64)
    w[0, bad] = 1e-6
    return lm[None], tm, w, m
