"""A numpy restatement of flm_head_pose (include/flm.h, "head pose"): np.float64 scalars, one operation per written
operator, every sum a Python loop in model order.  No np.dot, no np.sum."""
import numpy as np

f64 = np.float64
REC = 18
H = f64(0.7071067811865476)

# the default model of alignment.HeadModel.default(68), restated: landmark, X, Y, Z
DEFAULT_INDICES = [30, 8, 36, 45, 48, 54]
DEFAULT_POINTS = [[0.0, 0.0, 0.0], [0.0, 330.0, 65.0], [-225.0, -170.0, 135.0], [225.0, -170.0, 135.0],
                  [-150.0, 150.0, 125.0], [150.0, 150.0, 125.0]]


def not_ok(cnt):
    r = np.zeros(REC, f64)
    r[0] = r[4] = r[8] = 1.0
    r[10] = r[11] = -1.0
    r[13] = cnt
    return r


def _pos(v):
    return bool(np.isfinite(v) and v > 0.0)


def _norm(a):
    return np.sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2])


def fit_one(lm, w, idx, xyz, min_volume=1e-6, info=None):
    """lm float64 [C,2]; w None or float64 [C]; idx int [P]; xyz float64 [P,3] -> the record, float64 [18].
    info (a dict) receives vol."""
    c = lm.shape[0]
    pts = []
    for p in range(len(idx)):
        i = int(idx[p])
        if not 0 <= i < c:
            continue
        x, y = f64(lm[i, 0]), f64(lm[i, 1])
        wt = f64(1.0) if w is None else f64(w[i])
        if not (x >= 0.0 and y >= 0.0 and wt > 0.0):
            continue
        pts.append((f64(xyz[p, 0]), f64(xyz[p, 1]), f64(xyz[p, 2]), x, y, wt))
    cnt = len(pts)
    with np.errstate(all="ignore"):
        W = f64(0.0)
        s = [f64(0.0)] * 5
        for q in pts:
            W = W + q[5]
            for j in range(5):
                s[j] = s[j] + q[5] * q[j]
        mean = [v / W for v in s]
        a = {}
        for u, v in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2), (0, 3), (1, 3), (2, 3), (0, 4), (1, 4), (2, 4)):
            t = f64(0.0)
            for q in pts:
                t = t + q[5] * ((q[u] - mean[u]) * (q[v] - mean[v]))
            a[u, v] = t
        a00, a01, a02, a11, a12, a22 = a[0, 0], a[0, 1], a[0, 2], a[1, 1], a[1, 2], a[2, 2]
        bx = [a[0, 3], a[1, 3], a[2, 3]]
        by = [a[0, 4], a[1, 4], a[2, 4]]
        c00 = a11 * a22 - a12 * a12
        c01 = a02 * a12 - a01 * a22
        c02 = a01 * a12 - a02 * a11
        c11 = a00 * a22 - a02 * a02
        c12 = a01 * a02 - a00 * a12
        c22 = a00 * a11 - a01 * a01
        det = (a00 * c00 + a01 * c01) + a02 * c02
        vol = det / ((a00 * a11) * a22)
        if info is not None:
            info["vol"] = vol
        ck = [[c00, c01, c02], [c01, c11, c12], [c02, c12, c22]]
        I = [((ck[k][0] * bx[0] + ck[k][1] * bx[1]) + ck[k][2] * bx[2]) / det for k in range(3)]
        J = [((ck[k][0] * by[0] + ck[k][1] * by[1]) + ck[k][2] * by[2]) / det for k in range(3)]
        nI, nJ = _norm(I), _norm(J)
        sc = np.sqrt(nI * nJ)
        i_ = [I[k] / nI for k in range(3)]
        j_ = [J[k] / nJ for k in range(3)]
        e = [i_[k] + j_[k] for k in range(3)]
        f = [i_[k] - j_[k] for k in range(3)]
        ne, nf = _norm(e), _norm(f)
        e = [e[k] / ne for k in range(3)]
        f = [f[k] / nf for k in range(3)]
        r1 = [(e[k] + f[k]) * H for k in range(3)]
        r2 = [(e[k] - f[k]) * H for k in range(3)]
        r3 = [r1[1] * r2[2] - r1[2] * r2[1], r1[2] * r2[0] - r1[0] * r2[2], r1[0] * r2[1] - r1[1] * r2[0]]
        se = f64(0.0)
        for q in pts:
            X = [q[k] - mean[k] for k in range(3)]
            xp, yp = q[3] - mean[3], q[4] - mean[4]
            ex = sc * ((r1[0] * X[0] + r1[1] * X[1]) + r1[2] * X[2]) - xp
            ey = sc * ((r2[0] * X[0] + r2[1] * X[1]) + r2[2] * X[2]) - yp
            se = se + q[5] * (ex * ex + ey * ey)
        rms = np.sqrt(se / W)
        ok = (cnt >= 4 and all(_pos(v) for v in (W, det, nI, nJ, ne, nf)) and bool(vol >= min_volume)
              and all(bool(np.isfinite(v)) for v in r1 + r2 + r3 + [sc, rms]))
        if not ok:
            return not_ok(cnt)
        yaw = np.arctan2(-r3[0], r3[2])
        pitch = np.arcsin(np.fmin(np.fmax(r3[1], f64(-1.0)), f64(1.0)))
        roll = np.arctan2(-r1[1], r2[1])
    return np.array(r1 + r2 + r3 + [sc, mean[3], mean[4], rms, f64(cnt), f64(1.0), yaw, pitch, roll], f64)


def fit(lm, w, idx, xyz, min_volume=1e-6):
    """lm float64 [N,C,2]; w None or float64 [N,C] -> float64 [N,18]."""
    lm = np.asarray(lm, f64)
    xyz = np.asarray(xyz, f64)
    return np.stack([fit_one(lm[r], None if w is None else np.asarray(w, f64)[r], idx, xyz, min_volume)
                     for r in range(lm.shape[0])]) if lm.shape[0] else np.zeros((0, REC), f64)


def factor(rec, min_frontal=0.0):
    """factor_out of the records: (ok && R[2][2] >= min_frontal) ? R[2][2] : 0.0."""
    rec = np.asarray(rec, f64)
    return np.where((rec[:, 14] == 1.0) & (rec[:, 8] >= f64(min_frontal)), rec[:, 8], f64(0.0))


def angles_of(rec):
    """yaw, pitch, roll of the R of records, by numpy's atan2 / asin: float64 [N,3]."""
    rec = np.asarray(rec, f64)
    return np.stack([np.arctan2(-rec[:, 6], rec[:, 8]), np.arcsin(np.clip(rec[:, 7], -1.0, 1.0)),
                     np.arctan2(-rec[:, 1], rec[:, 4])], axis=1)


def rotation(yaw, pitch, roll):
    """Rz(roll) Rx(pitch) Ry(yaw) in the model frame of the header (X right, Y down, Z away)."""
    cy, sy, cp, sp, cr, sr = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    rx = np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
    rz = np.array([[cr, -sr, 0], [sr, cr, 0], [0, 0, 1]])
    return rz @ rx @ ry


def project(xyz, r, scale, tx, ty):
    """The model under R, scaled and moved: float64 [P,2] (scaled orthography: Z is dropped)."""
    q = np.asarray(xyz, f64) @ r.T
    return np.stack([scale * q[:, 0] + tx, scale * q[:, 1] + ty], axis=1)
