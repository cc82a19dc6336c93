"""include/flm.h, "face parts" and "openness and blink state", restated in numpy float64 scalars: one IEEE operation per
written operator, in the written order, every sum sequential from 0.0.  The kernels of csrc/flm_parts.hip and the host
program tests/native/parts_host.cpp must equal these functions bit for bit.  Shared cases for the tests live here too."""
import numpy as np

f64 = np.float64
REC, STATE = 4, 8
STATE_EMPTY = (0.0, 0.0, 0.0, -1.0, 0.0, 0.0, -1.0, 0.0)
DBL_MAX = np.finfo(np.float64).max


# ---- parts ----------------------------------------------------------------------------------------------------------------
def part_fit(lm, w, idx, tmpl):
    """lm float64 [C,2], w float64 [C] or None, idx: the part's landmark numbers in order, tmpl float64 [n,2] ->
    (float32 [2,3], ok)."""
    c = lm.shape[0]
    pts = []
    for i, j in enumerate(idx):
        j = int(j)
        if 0 <= j < c:
            x, y, wt = f64(lm[j, 0]), f64(lm[j, 1]), (f64(1.0) if w is None else f64(w[j]))
        else:
            x, y, wt = f64(-1.0), f64(-1.0), f64(0.0)
        if x >= 0.0 and y >= 0.0 and wt > 0.0:
            pts.append((x, y, wt, f64(tmpl[i, 0]), f64(tmpl[i, 1])))
    a, b, tx, ty, ok = f64(1.0), f64(0.0), f64(0.0), f64(0.0), False
    with np.errstate(all="ignore"):
        if len(pts) >= 2:
            mpx = mpy = mqx = mqy = wsum = f64(0.0)
            for x, y, wt, qx, qy in pts:
                mpx = mpx + wt * x
                mpy = mpy + wt * y
                mqx = mqx + wt * qx
                mqy = mqy + wt * qy
                wsum = wsum + wt
            mpx, mpy, mqx, mqy = mpx / wsum, mpy / wsum, mqx / wsum, mqy / wsum
            sa = sb = var = f64(0.0)
            for x, y, wt, tqx, tqy in pts:
                px, py = x - mpx, y - mpy
                qx, qy = tqx - mqx, tqy - mqy
                sa = sa + wt * (px * qx + py * qy)
                sb = sb + wt * (px * qy - py * qx)
                var = var + wt * (px * px + py * py)
            if var > 0.0:
                a, b = sa / var, sb / var
                tx = mqx - (a * mpx - b * mpy)
                ty = mqy - (b * mpx + a * mpy)
                ok = True
        return np.array([[a, -b, tx], [b, a, ty]], np.float64).astype(np.float32), ok


def part_affines(lm, w, parts):
    """lm [K,C,2], w [K,C] or None, parts: a list of (indices, template [n,2]) -> (float32 [K,R,2,3], int32 [K,R])."""
    k, r = lm.shape[0], len(parts)
    aff, ok = np.zeros((k, r, 2, 3), np.float32), np.zeros((k, r), np.int32)
    for f in range(k):
        for j, (idx, tmpl) in enumerate(parts):
            aff[f, j], o = part_fit(lm[f], None if w is None else w[f], idx, np.asarray(tmpl, np.float64))
            ok[f, j] = 1 if o else 0
    return aff, ok


# ---- openness -------------------------------------------------------------------------------------------------------------
def _point(lm, w, j):
    c = lm.shape[0]
    j = int(j)
    if not 0 <= j < c:
        return f64(-1.0), f64(-1.0), False
    x, y = f64(lm[j, 0]), f64(lm[j, 1])
    wt = f64(1.0) if w is None else f64(w[j])
    return x, y, bool(x >= 0.0 and y >= 0.0 and wt > 0.0)


def _dist(a, b):
    dx, dy = a[0] - b[0], a[1] - b[1]
    return np.sqrt(dx * dx + dy * dy)


def open_record(lm, w, measure, min_width):
    """lm [C,2], w [C] or None, measure ((a, b), ((u, l), ...)) -> float64 [4]."""
    (wa, wb), pairs = measure
    with np.errstate(all="ignore"):
        a, b = _point(lm, w, wa), _point(lm, w, wb)
        ends = [(_point(lm, w, u), _point(lm, w, l)) for u, l in pairs]
        if not (a[2] and b[2] and all(u[2] and l[2] for u, l in ends)):
            return np.array([-1.0, -1.0, 0.0, -1.0], np.float64)
        dw = _dist(a, b)
        s = f64(0.0)
        for u, l in ends:
            s = s + _dist(u, l)
        o = (s / f64(len(pairs))) / dw
        ok = bool(dw >= f64(min_width)) and bool(-DBL_MAX <= o <= DBL_MAX)
        return np.array([o if ok else -1.0, dw, 1.0 if ok else 0.0, s], np.float64)


def state_step(st, ok, o, status, dt, th, frame_id):
    """One tick of one measure's state, in place.  th: dict(close_below, open_above, min_closed, max_closed)."""
    dt = f64(dt)
    if not ok or status != 0 or not (dt > 0.0 and dt <= DBL_MAX):
        return
    st[5] = st[5] + dt
    if st[0] == 0.0:
        if o < th["close_below"]:
            st[0] = 1.0
            st[1] = 0.0
            st[4] = st[4] + dt
        else:
            st[1] = st[1] + dt
    elif o > th["open_above"]:
        d = st[1] + dt
        st[3] = d
        if th["min_closed"] <= d <= th["max_closed"]:
            st[2] = st[2] + f64(1.0)
            st[6] = f64(frame_id)
        st[0] = 0.0
        st[1] = 0.0
    else:
        st[1] = st[1] + dt
        st[4] = st[4] + dt


def openness(lm, w, measures, min_width, th=None, slot=None, rec=None, state=None, reset=None, dt=None, status=None,
             frame_id=0):
    """The whole call on the host, in place on rec [N or n_slots,G,4], state [.,G,8] and reset [.] (each a numpy array;
    rec None without slot: a new one).  dt: a number or [N]; status: [N] or None.  Returns rec."""
    n, g = lm.shape[0], len(measures)
    if rec is None:
        rec = np.zeros((n, g, REC), np.float64)
    for r in range(n):
        s = r
        if slot is not None:
            s = int(slot[r])
            if not 0 <= s < rec.shape[0]:
                continue
        do_reset = state is not None and reset[s] != 0
        for m in range(g):
            rr = open_record(lm[r], None if w is None else w[r], measures[m], min_width)
            rec[s, m] = rr
            if state is not None:
                if do_reset:
                    state[s, m] = STATE_EMPTY
                state_step(state[s, m], rr[2] == 1.0, rr[0], 0 if status is None else int(status[r]),
                           dt[r] if np.ndim(dt) else dt, th, frame_id)
        if do_reset:
            reset[s] = 0
    return rec


# ---- shared cases ---------------------------------------------------------------------------------------------------------
DEFAULT_MEASURES = (((36, 39), ((37, 41), (38, 40))), ((42, 45), ((43, 47), (44, 46))),
                    ((60, 64), ((61, 67), (62, 66), (63, 65))))
EXTRA_MEASURES = (((0, 16), ((8, 27),)), ((48, 54), ((50, 58), (51, 57), (52, 56), (49, 59))))   # V = 1 and V = 4
DEFAULT_TH = dict(close_below=0.18, open_above=0.22, min_closed=0.03, max_closed=0.5)


def custom_parts(ph, pw):
    """A set whose indices are non-contiguous and out of order (one repeats across parts, one lies outside a 68-point
    face): brows + nose tip, and a jaw-to-eye triangle."""
    rng = np.random.default_rng(5)
    a = [30, 17, 26, 21, 22, 19, 24]
    b = [45, 8, 36, 30, 200]
    return [(np.array(a), rng.uniform(1.0, [pw - 2.0, ph - 2.0], (len(a), 2))),
            (np.array(b), rng.uniform(1.0, [pw - 2.0, ph - 2.0], (len(b), 2)))]


def face_landmarks(k, fh, fw, seed, template):
    """K faces of 68 landmarks inside an fh x fw frame -- the template under a random similarity plus noise -- and
    weights, with the degenerate faces the contract names at fixed rows (where K allows): row 1 rejected points and
    zero / NaN weights, row 2 a single participating point, row 3 coincident points, row 4 a NaN coordinate."""
    rng = np.random.default_rng(seed)
    c = template.shape[0]
    t = template - template.mean(axis=0)
    t = t / np.abs(t).max()
    lm = np.zeros((k, c, 2), np.float64)
    for f in range(k):
        s = rng.uniform(0.15, 0.3) * min(fh, fw)
        th = rng.uniform(-0.5, 0.5)
        rot = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
        centre = np.array([rng.uniform(0.35, 0.65) * fw, rng.uniform(0.35, 0.65) * fh])
        lm[f] = np.abs(t @ rot.T * s + centre + rng.normal(0, 0.4, (c, 2)))
    w = rng.uniform(0.2, 1.0, (k, c))
    if k > 1:
        lm[1, 36:40] = -1.0
        w[1, 42] = 0.0
        w[1, 43] = np.nan
        w[1, 50:55] = 0.0
    if k > 2:
        lm[2, :] = -1.0
        lm[2, 37] = [40.0, 30.0]
        lm[2, 60] = [50.0, 60.0]
    if k > 3:
        lm[3, 36:48] = lm[3, 36]
        lm[3, 48:68] = [33.25, 44.5]
    if k > 4:
        lm[4, 44, 0] = np.nan
        lm[4, 62, 1] = np.nan
    return lm, w


def openness_landmarks(n, seed, min_width=4.0):
    """N faces of 68 landmarks for the openness records: random eyes and mouths, and at fixed rows a missing point, a
    width just below and just above min_width, NaN coordinates, a zero weight."""
    rng = np.random.default_rng(seed)
    lm = rng.uniform(5.0, 400.0, (n, 68, 2))
    w = rng.uniform(0.1, 1.0, (n, 68))
    if n > 1:
        lm[1, 37] = -1.0
    if n > 2:   # dw of measure 0 one ulp below min_width (from x = 0, so that the sum does not round it away), of measure
        # 1 exactly min_width, the least width that is read
        lm[2, 36], lm[2, 39] = [0.0, 50.0], [np.nextafter(min_width, 0.0), 50.0]
        lm[2, 42], lm[2, 45] = [200.0, 50.0], [200.0 + min_width, 50.0]
    if n > 3:
        lm[3, 38, 0] = np.nan
        lm[3, 64, 1] = np.nan
    if n > 4:
        w[4, 46] = 0.0
        w[4, 61] = np.nan
    if n > 5:   # a width of zero: o = x / 0
        lm[5, 60] = lm[5, 64]
    return lm, w


def eye_script():
    """Twelve ticks of openness values for six slots, and the events a reader counts by hand at dt = 0.04 with
    min_closed = 0.05, max_closed = 0.2 (run starts at 0 on the closing tick and the opening tick adds its own dt, so a
    closure seen closed on c served ticks lasts d = c * dt):
      slot 0: closed on ticks 3,4,5, open at 6 -> d = 0.12: one event
      slot 1: closed on tick 3 alone -> d = 0.04 < min_closed: none
      slot 2: closed on ticks 2..8, open at 9 -> d = 0.28 > max_closed: none
      slot 3: closed on 3,4,5 with a not-ok tick at 4 (the state waits) -> d = 0.08: one event
      slot 4: closed on 3,4,5 with a reset at tick 5 (the slot starts over, open, and closes again at 5; opens at 6 ->
              d = 0.04): none
      slot 5: open throughout: none"""
    o = np.full((12, 6), 0.3)
    o[3:6, 0] = 0.1
    o[3, 1] = 0.1
    o[2:9, 2] = 0.1
    o[3:6, 3] = 0.1
    o[3:6, 4] = 0.1
    not_ok = {(4, 3)}
    resets = {(5, 4)}
    events = [1, 0, 0, 1, 0, 0]
    return o, not_ok, resets, events


def eye_landmarks(o_row, not_ok_slots):
    """68-point faces whose three default measures read exactly-representable openness near o: width 64 px, every pair
    64*o px apart (rounded to 1/64 px so all distances are exact)."""
    n = len(o_row)
    lm = np.full((n, 68, 2), -1.0)
    for s in range(n):
        h = np.round(64.0 * o_row[s] * 64.0) / 64.0
        for (a, b), pairs in DEFAULT_MEASURES:
            x0 = 100.0 + a
            lm[s, a], lm[s, b] = [x0, 200.0], [x0 + 64.0, 200.0]
            for i, (u, l) in enumerate(pairs):
                lm[s, u], lm[s, l] = [x0 + 16.0 * (i + 1), 200.0], [x0 + 16.0 * (i + 1), 200.0 + h]
        if s in not_ok_slots:
            lm[s, 36] = -1.0
            lm[s, 42] = -1.0
            lm[s, 60] = -1.0
    return lm
