"""Sequences of frames for the filtered track step, made by running tests/track_filter_ref.py in a closed loop: the
landmarks of step t are synthetic frame points seen through the crop the reference itself placed at step t-1, so the
inputs of every step and its seven expected outputs come from one pass.  Shared by the host and the GPU tests.

Steps are numbered from 1.  What happens on the way (faces by k: 1 face is PLAIN, 3 are PLAIN, DEAD, LOST, more cycle
through PLAIN, ROLLED, DEAD, LOST, SMALL):
  every step    the points move by a few px and carry 0.3 px of noise
  step 2        in every face some points are rejected; half of them return at step 3, the others at step 4
  step 3        a LOST face shows a centre right of the frame: FLM_TRACK_OUTSIDE, an empty box
                before it, one state entry of face 0 is poisoned with NaN
  step 4        the LOST faces are re-seeded: state refilled with -1, a new box and its seeded matrix
  DEAD faces have an empty box throughout.
"""
import numpy as np

import track_filter_ref
import track_ref

f32, f64 = np.float32, np.float64
IN, GRID, FH, FW = 64, 72, 270, 480
SC = IN / GRID
DT = 1.0 / 30.0
PLAIN, ROLLED, DEAD, LOST, SMALL = range(5)


def kinds_of(k):
    return {1: [PLAIN], 3: [PLAIN, DEAD, LOST]}.get(k) or [i % 5 for i in range(k)]


def template(c, h, w):
    from flm_amd import alignment
    return alignment.canonical_template(c, h, w)


def pose(tmpl, scale, deg, cx, cy):
    th = np.deg2rad(deg)
    r = scale * np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
    return (tmpl - (IN - 1) / 2.0) @ r.T + np.array([cx, cy])


def seed_box(cx, cy, side):
    x0, y0 = int(cx - side / 2), int(cy - side / 2)
    return [x0, y0, x0 + int(side), y0 + int(side)]


def poisoned(c):
    """(point, entry) of face 0 whose state is set to NaN before step 3: a point that is not rejected then."""
    return (c - 1, 2)


def rejected_at(c, t):
    """The points rejected at step t: every fourth from 1 at steps 2 and 3, every fourth from 3 at step 2 alone."""
    idx = []
    if t in (2, 3):
        idx += list(range(1, c, 4))
    if t == 2:
        idx += list(range(3, c, 4))
    return [i for i in idx if i != c - 1] if c > 1 else ([0] if t == 2 else [])


def sequence(k, c, weighted, steps=5, seed=0, filt=None, **limits):
    """-> dict(k, c, tc, ta, kinds, steps=[dict(lm, w, m_crop, boxes, state, exp=dict of the seven outputs)]): the inputs
    of every step as the closed loop of the reference has them (with the re-seed and the poisoned entry applied), and
    what the step must write."""
    filt = dict(track_filter_ref.DEFAULTS if filt is None else filt)
    rng = np.random.default_rng(1000 * k + 10 * c + seed)
    kinds = kinds_of(k)
    tc, ta = template(c, IN, IN), template(c, 112, 112)
    scale = rng.uniform(0.8, 1.6, k)
    deg = rng.uniform(-10, 10, k)
    cx, cy = rng.uniform(140, 340, k), rng.uniform(90, 180, k)
    vel = rng.uniform(-3, 3, (k, 2))                              # px per frame
    spin = rng.uniform(-1.5, 1.5, k)                              # degrees per frame
    for f, kind in enumerate(kinds):
        if kind == ROLLED:
            deg[f] = rng.uniform(25, 40) * (1 if f % 2 else -1)
        elif kind == SMALL:
            scale[f] = 0.5
    boxes = np.array([seed_box(cx[f], cy[f], 1.25 * IN * scale[f]) for f in range(k)], np.int32)
    for f, kind in enumerate(kinds):
        if kind == DEAD:
            boxes[f] = [[FW + 5, 10, FW + 85, 90], [0, 0, 0, 0], [-90, -90, -10, -10]][f % 3]
    m_crop, _ = track_ref.seed(boxes, IN, IN, FH, FW)
    state = track_filter_ref.empty_state(k, c)
    out = []
    for t in range(1, steps + 1):
        if t == 3:
            i, e = poisoned(c)
            state = state.copy()
            state[0, i, e] = np.nan
        if t == 4:
            state, boxes, m_crop = state.copy(), boxes.copy(), m_crop.copy()
            for f, kind in enumerate(kinds):
                if kind == LOST:
                    state[f] = -1.0
                    boxes[f] = seed_box(cx[f] + 3 * vel[f, 0], cy[f] + 3 * vel[f, 1], 1.25 * IN * scale[f])
                    m_crop[f] = track_ref.seed(boxes[f:f + 1], IN, IN, FH, FW)[0][0]
        lm = np.zeros((k, c, 2), f64)
        for f, kind in enumerate(kinds):
            x, y = cx[f] + (t - 1) * vel[f, 0], cy[f] + (t - 1) * vel[f, 1]
            if kind == LOST and t == 3:
                x = FW + 20.0                                     # (to the right: every coordinate stays positive)
            pts = pose(tc, scale[f], deg[f] + (t - 1) * spin[f], x, y) + rng.normal(0, 0.3, (c, 2))
            lm[f] = track_ref.apply(m_crop[f], pts) / SC
            lm[f, rejected_at(c, t), (t + f) % 2] = -1.0
        w = None
        if weighted:
            w = rng.uniform(0.05, 1.0, (k, c))
            if c >= 5:
                bad = [0.0, np.nan, -0.5][:3 if c >= 16 else 1]      # each leaves its point out of the fit
                for f in range(k):
                    w[f, rng.permutation(c)[:len(bad)]] = bad
        exp = track_filter_ref.step(lm, w, m_crop, boxes, SC, SC, IN, IN, FH, FW, tc, ta, state, DT, **filt, **limits)
        out.append(dict(lm=lm, w=w, m_crop=m_crop, boxes=boxes, state=state, exp=exp))
        m_crop, boxes, state = exp["m_next"], exp["boxes_next"], exp["state"]
    return dict(k=k, c=c, tc=tc, ta=ta, kinds=kinds, steps=out)
