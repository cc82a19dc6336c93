"""flm_track_step_filtered of include/flm.h in plain numpy float64, on top of tests/track_ref.py: the raw points are
track_ref.landmarks_from_crop's, the filter below restates the header line by line (every operation one IEEE float64
operation on arrays, numpy fuses nothing), and the two fits, the status tests and the box are track_ref.step's own, run on
the filtered points.  What the filtered step must equal bit for bit.
"""
import numpy as np

import track_ref

f64, f32 = np.float64, np.float32
TWO_PI = f64(6.283185307179586)
DEFAULTS = dict(min_cutoff=1.0, beta=15.0, d_cutoff=1.0)


def empty_state(*shape):
    """A state without history: every entry -1."""
    return np.full(tuple(shape) + (6,), -1.0, f64)


def one_euro(raw, state, side, dt, min_cutoff=1.0, beta=15.0, d_cutoff=1.0):
    """The filter of the header for any number of points at once: raw [...,2] frame px ((-1,-1) = rejected), state
    [...,6] = (xh, yh, vx, vy, xr, yr), side [...] (or a scalar) the crop side in frame px -> (out [...,2], state')."""
    raw, state = np.asarray(raw, f64), np.asarray(state, f64)
    side, dt = np.asarray(side, f64), f64(dt)
    min_cutoff, beta, d_cutoff = f64(min_cutoff), f64(beta), f64(d_cutoff)
    one = f64(1.0)
    x, y = raw[..., 0], raw[..., 1]
    xh, yh, vx, vy, xr, yr = [state[..., j] for j in range(6)]
    rejected = x < 0.0                                   # (the back-projection writes exactly (-1,-1))
    with np.errstate(all="ignore"):
        history = (xh >= 0.0) & (yh >= 0.0) & np.isfinite(state).all(-1)
        rx = (x - xr) / dt
        ry = (y - yr) / dt
        ad = one / (one + (one / (TWO_PI * d_cutoff)) / dt)
        vx1 = ad * rx + (one - ad) * vx
        vy1 = ad * ry + (one - ad) * vy
        fc = min_cutoff + beta * (np.sqrt(vx1 * vx1 + vy1 * vy1) / side)
        a = one / (one + (one / (TWO_PI * fc)) / dt)
        xh1 = a * x + (one - a) * xh
        yh1 = a * y + (one - a) * yh
        use = history & np.isfinite(xh1) & np.isfinite(yh1) & np.isfinite(vx1) & np.isfinite(vy1)
    zero = np.zeros_like(x)
    ox, oy = np.where(use, xh1, x), np.where(use, yh1, y)
    new = np.stack([ox, oy, np.where(use, vx1, zero), np.where(use, vy1, zero), x, y], -1)
    gone = np.broadcast_to(np.array([-1.0, -1.0, 0.0, 0.0, -1.0, -1.0]), new.shape)
    new = np.where(rejected[..., None], gone, new)
    out = np.where(rejected[..., None], f64(-1.0), np.stack([ox, oy], -1))
    return out, new


def crop_side(m_crop, in_w):
    """side of the header for every face: m_crop float32 [K,2,3] -> float64 [K]."""
    m = np.asarray(m_crop, f32).astype(f64)
    with np.errstate(all="ignore"):
        return f64(in_w) / np.sqrt(m[:, 0, 0] * m[:, 0, 0] + m[:, 1, 0] * m[:, 1, 0])


def step(lm, w, m_crop, boxes, sx, sy, in_h, in_w, fh, fw, tmpl_crop, tmpl_align, state, dt, min_cutoff=1.0, beta=15.0,
         d_cutoff=1.0, **limits):
    """flm_track_step_filtered -> dict(lm_frame, m_align, m_next, boxes_next, status, state, lm_raw); `state` [K,C,6] is
    not modified."""
    lm = np.asarray(lm, f64)
    k = lm.shape[0]
    boxes = np.asarray(boxes, np.int32).reshape(k, 4)
    raw = track_ref.landmarks_from_crop(lm, m_crop, sx, sy)
    for f in range(k):
        if track_ref.box_empty(boxes[f], fh, fw):
            raw[f] = -1.0
    out, new = one_euro(raw, state, crop_side(m_crop, in_w)[:, None], dt, min_cutoff, beta, d_cutoff)
    # steps 2 to 5 of flm_track_step on `out`: under the identity matrix and unit scales track_ref.step's own
    # back-projection returns a point that is not rejected as it came (x*1 - 0, (1*u - 0*v)/1), and (-1,-1) as (-1,-1)
    eye = np.broadcast_to(track_ref.IDENTITY, (k, 2, 3))
    r = track_ref.step(out, w, eye, boxes, 1.0, 1.0, in_h, in_w, fh, fw, tmpl_crop, tmpl_align, **limits)
    assert np.array_equal(r["lm_frame"].view(np.uint64), out.view(np.uint64))
    r.update(state=new, lm_raw=raw)
    return r
