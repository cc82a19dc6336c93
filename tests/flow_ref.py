"""The numpy restatement of flm_flow_pyramid and flm_landmark_flow (include/flm.h, "landmark flow"): exact integers for
everything summed over a window, Python floats (IEEE float64, one operation per operator, nothing fused) for the closed
form, in the order the header writes.  The device equals this bit for bit."""
import math

import numpy as np

NO_HISTORY, LOW_TEXTURE, RESIDUAL, OUTSIDE, MOVED, NOT_FINITE = 1, 2, 4, 8, 16, 32
REACH = 1048576.0
DEFAULTS = dict(levels=4, radius=7, max_iter=10, eps=0.03, min_eig=0.5, max_err=12.0, max_move=64.0)


def options(**kw):
    o = dict(DEFAULTS)
    o.update(kw)
    return o


def luma(img):
    """uint8 [...,H,W] or [...,H,W,3] (B,G,R) -> uint8 [...,H,W]."""
    img = np.asarray(img)
    if img.ndim >= 3 and img.shape[-1] == 3:
        v = img.astype(np.int64)
        return ((1868 * v[..., 0] + 9617 * v[..., 1] + 4899 * v[..., 2] + 8192) >> 14).astype(np.uint8)
    return img.astype(np.uint8)


def pyramid(y, levels):
    """uint8 [H,W] luma -> the list of its levels."""
    out = [np.ascontiguousarray(y, np.uint8)]
    for _ in range(1, levels):
        a = out[-1].astype(np.int64)
        h, w = a.shape[0] // 2, a.shape[1] // 2
        a = a[:2 * h, :2 * w]
        out.append(((a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2] + 2) >> 2).astype(np.uint8))
    return out


def pyramid_bytes(h, w, levels):
    return sum((h >> l) * (w >> l) for l in range(levels))


def pyramid_flat(crops, levels):
    """uint8 [N,H,W] or [N,H,W,3] -> uint8 [N, pyramid_bytes]: what flm_flow_pyramid writes."""
    ys = luma(crops)
    return np.stack([np.concatenate([lv.reshape(-1) for lv in pyramid(y, levels)]) for y in ys])


def sample(img, x, y):
    """S(I, x, y) for float64 arrays x, y of one shape -> int64."""
    hl, wl = img.shape
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    fx, fy = np.floor(x), np.floor(y)
    ix, iy = fx.astype(np.int64), fy.astype(np.int64)
    ax, ay = ((x - fx) * 32.0).astype(np.int64), ((y - fy) * 32.0).astype(np.int64)
    x0, x1 = np.clip(ix, 0, wl - 1), np.clip(ix + 1, 0, wl - 1)
    y0, y1 = np.clip(iy, 0, hl - 1), np.clip(iy + 1, 0, hl - 1)
    im = img.astype(np.int64)
    return ((32 - ax) * (32 - ay) * im[y0, x0] + ax * (32 - ay) * im[y0, x1] + (32 - ax) * ay * im[y1, x0]
            + ax * ay * im[y1, x1])


def _in_reach(x, y):
    return -REACH <= x <= REACH and -REACH <= y <= REACH     # (a NaN fails)


def flow_point(prev, cur, m, x, y, o):
    """prev, cur: the level lists of the two crops; m float32 [2,3]; (x, y) in frame px -> (qx, qy, err, flags), q the
    guess where the point stopped (-1,-1 before p0 exists)."""
    x, y = float(x), float(y)
    if not (x >= 0.0 and y >= 0.0 and math.isfinite(x) and math.isfinite(y)):
        return -1.0, -1.0, -1, NO_HISTORY
    mm = [[float(v) for v in row] for row in np.asarray(m, np.float32)]
    with np.errstate(all="ignore"):
        p0x = float((np.float64(mm[0][0]) * x + np.float64(mm[0][1]) * y) + np.float64(mm[0][2]))
        p0y = float((np.float64(mm[1][0]) * x + np.float64(mm[1][1]) * y) + np.float64(mm[1][2]))
    if not _in_reach(p0x, p0y):
        return p0x, p0y, -1, NOT_FINITE
    r, levels = o["radius"], o["levels"]
    n = (2 * r + 1) ** 2
    jj, ii = np.meshgrid(np.arange(-r, r + 1, dtype=np.float64), np.arange(-r, r + 1, dtype=np.float64), indexing="ij")
    flags = 0
    h, w = prev[0].shape
    qx = qy = 0.0
    T = None
    for l in range(levels - 1, -1, -1):
        s = float(1 << l)
        px, py = (p0x + 0.5) / s - 0.5, (p0y + 0.5) / s - 0.5
        if l == levels - 1:
            qx, qy = px, py
        P, Q = prev[l], cur[l]
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
                D = T - sample(Q, qx + ii, qy + jj)
                bx, by = float(int((D * gx).sum())), float(int((D * gy).sum()))
                with np.errstate(all="ignore"):
                    dx = float(np.float64(2.0 * (C * bx - B * by)) / np.float64(det))
                    dy = float(np.float64(2.0 * (A * by - B * bx)) / np.float64(det))
                qx, qy = qx + dx, qy + dy
                if not _in_reach(qx, qy):
                    return qx, qy, -1, flags | NOT_FINITE
                if dx * dx + dy * dy < o["eps"] * o["eps"]:
                    break
        if l > 0:
            qx, qy = 2.0 * qx + 0.5, 2.0 * qy + 0.5
    err = int(np.abs(T - sample(cur[0], qx + ii, qy + jj)).sum())
    if not float(err) / (float(n) * 1024.0) <= o["max_err"]:
        flags |= RESIDUAL
    if not (0.0 <= qx <= float(w - 1) and 0.0 <= qy <= float(h - 1)):
        flags |= OUTSIDE
    mx, my = qx - p0x, qy - p0y
    if not mx * mx + my * my <= o["max_move"] * o["max_move"]:
        flags |= MOVED
    return qx, qy, err, flags


def landmark_flow(prev_crops, cur_crops, lm_prev, m, o, w_prev=None):
    """prev_crops, cur_crops uint8 [K,H,W] or [K,H,W,3]; lm_prev float64 [K,C,2] frame px; m float32 [K,2,3] ->
    (lm float64 [K,C,2] crop px, w float64 [K,C], err int32 [K,C], flags int32 [K,C]) as flm_landmark_flow writes them."""
    lm_prev = np.asarray(lm_prev, np.float64)
    k, c = lm_prev.shape[:2]
    lm = np.full((k, c, 2), -1.0)
    wt = np.zeros((k, c))
    err = np.full((k, c), -1, np.int32)
    flags = np.zeros((k, c), np.int32)
    yp, yc = luma(prev_crops), luma(cur_crops)
    for f in range(k):
        pp, pc = pyramid(yp[f], o["levels"]), pyramid(yc[f], o["levels"])
        for i in range(c):
            qx, qy, e, fl = flow_point(pp, pc, m[f], lm_prev[f, i, 0], lm_prev[f, i, 1], o)
            err[f, i], flags[f, i] = e, fl
            if fl == 0:
                lm[f, i] = (qx, qy)
                wt[f, i] = 1.0 if w_prev is None else w_prev[f, i]
    return lm, wt, err, flags


def texture(h, w, seed):
    """The multi-scale texture of the tests: Gaussian-filtered noise at sigma 1.5, 4 and 10, summed, in 0..255 float64."""
    from scipy.ndimage import gaussian_filter
    rng = np.random.default_rng(seed)
    t = np.zeros((h, w))
    for sigma in (1.5, 4.0, 10.0):
        g = gaussian_filter(rng.standard_normal((h, w)), sigma, mode="wrap")
        t += g / g.std()
    t -= t.min()
    return t * (255.0 / t.max())


def shifted(tex, dx, dy):
    """The texture moved by (dx, dy): out(y, x) = tex(y - dy, x - dx), cubic, as uint8."""
    from scipy.ndimage import map_coordinates
    h, w = tex.shape
    yy, xx = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    out = map_coordinates(tex, [yy - dy, xx - dx], order=3, mode="nearest")
    return np.clip(np.rint(out), 0, 255).astype(np.uint8)
