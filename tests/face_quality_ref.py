"""numpy restatement of flm_face_quality and flm_track_best_update as include/flm.h ("the best shot of a track") states
them: int64 sums, and float32 / float64 operations one at a time.  What the device must equal bit for bit.

    record(faces, fmt, dark=16, bright=239)          -> int64 [K,8]
    quality(rec, lm, w, factor, status, opts)        -> (q float64 [K], eligible bool [K])
    best_update(state, faces, rec, ...)              -> edits the dict `state` in place, returns taken bool [K]

`faces` is the stored tensor in the format's own layout; bfloat16 comes as its uint16 BITS (numpy has no such type), as
tests/aligned_format_ref.py hands it out.  No device, no library.
"""
import numpy as np

from aligned_format_ref import _as_format

f32, f64 = np.float32, np.float64
REC = 8


def to_f32(x, dtype):
    """The stored elements as float32: exact for every type."""
    x = np.asarray(x)
    if dtype == "bfloat16":
        assert x.dtype == np.uint16
        return (x.astype(np.uint32) << 16).view(f32)
    assert x.dtype == np.dtype(dtype)
    return x.astype(f32)


def quantise(xf, bias, inv):
    """xf float32 [...,3] by output channel -> int64 p in [0, 4080]: t = xf - bias, v = t * inv, rint(v * 16)."""
    with np.errstate(all="ignore"):
        t = (xf - bias).astype(f32)
        v = (t * inv).astype(f32)
        r = np.rint((v * f32(16.0)).astype(f32))
        r = np.where(np.isnan(r), f32(0.0), r)
        return np.clip(r, 0.0, 4080.0).astype(np.int64)


def luma_of(p, reverse):
    """p int64 [...,3] by OUTPUT channel -> Y; source channel s = reverse ? 2-c : c, and B, G, R are s = 0, 1, 2."""
    b, g, r = (p[..., 2], p[..., 1], p[..., 0]) if reverse else (p[..., 0], p[..., 1], p[..., 2])
    return (1868 * b + 9617 * g + 4899 * r + 8192) >> 14


def luma(faces, fmt):
    layout, dtype, reverse, scale, bias = _as_format(fmt)
    x = to_f32(faces, dtype)
    assert x.ndim == 4
    if layout == "nchw":
        x = x.transpose(0, 2, 3, 1)
    assert x.shape[3] == 3
    with np.errstate(all="ignore"):
        inv = (f32(1.0) / scale).astype(f32)
    return luma_of(quantise(x, bias, inv), reverse)


def laplacian(y):
    """Y int64 [K,h,w] -> L int64 [K,max(h-2,0),max(w-2,0)] over the interior pixels."""
    k, h, w = y.shape
    if h < 3 or w < 3:
        return np.zeros((k, max(h - 2, 0), max(w - 2, 0)), np.int64)
    return y[:, :-2, 1:-1] + y[:, 2:, 1:-1] + y[:, 1:-1, :-2] + y[:, 1:-1, 2:] - 4 * y[:, 1:-1, 1:-1]


def record(faces, fmt, dark=16, bright=239):
    y = luma(faces, fmt)
    k, h, w = y.shape
    lap = laplacian(y)
    rec = np.zeros((k, REC), np.int64)
    rec[:, 0] = h * w
    rec[:, 1] = y.sum(axis=(1, 2))
    rec[:, 2] = (y * y).sum(axis=(1, 2))
    rec[:, 3] = max(h - 2, 0) * max(w - 2, 0)
    rec[:, 4] = lap.sum(axis=(1, 2))
    rec[:, 5] = (lap * lap).sum(axis=(1, 2))
    rec[:, 6] = (y < 16 * dark).sum(axis=(1, 2))
    rec[:, 7] = (y > 16 * bright).sum(axis=(1, 2))
    return rec


def sharpness(rec_row):
    """The header's mu, var, sharp for one record (float64, one operation each)."""
    with np.errstate(all="ignore"):
        nl = f64(int(rec_row[3]))
        mu = f64(int(rec_row[4])) / nl
        m2 = f64(int(rec_row[5])) / nl
        var = m2 - mu * mu
        return np.fmax(var / f64(256.0), f64(0.0))


def quality(rec, lm, w=None, factor=None, status=None, sharp_ref=100.0, min_exposed=0.5):
    """-> (q float64 [K], eligible bool [K]).  lm float64 [K,C,2]; w None or float64 [K,C]; factor None or float64 [K];
    status None or int32 [K]."""
    k = rec.shape[0]
    q, ok = np.zeros(k, f64), np.zeros(k, bool)
    with np.errstate(all="ignore"):
        for i in range(k):
            n_pix, n_lap, n_dark, n_bright = [int(rec[i, j]) for j in (0, 3, 6, 7)]
            s = np.fmin(sharpness(rec[i]) / f64(sharp_ref), f64(1.0))
            e = f64(n_pix - n_dark - n_bright) / f64(n_pix)
            wbar = f64(1.0)
            if w is not None:
                total, n = f64(0.0), 0
                for j in range(lm.shape[1]):
                    if lm[i, j, 0] == -1.0 and lm[i, j, 1] == -1.0:
                        continue
                    total = total + f64(w[i, j])
                    n += 1
                wbar = total / f64(n) if n else f64(0.0)
            f = f64(1.0) if factor is None else f64(factor[i])
            qi = ((s * e) * wbar) * f
            q[i] = qi
            ok[i] = bool((status is None or status[i] == 0) and n_lap > 0 and e >= f64(min_exposed) and not np.isnan(qi)
                         and qi >= 0.0)
    return q, ok


def new_state(faces_like, k, c):
    """The tracker-side state of flm_track_best_update for K slots; `faces_like` gives the gallery's dtype and shape."""
    g = np.zeros_like(faces_like)
    return dict(gallery=g, best_q=np.full(k, -1.0, f64), best_frame=np.full(k, -1, np.int64),
              best_m=np.zeros((k, 2, 3), f32), best_lm=np.full((k, c, 2), -1.0, f64), best_rec=np.zeros((k, REC), np.int64))


def best_update(state, faces, rec, lm, frame_id, w=None, factor=None, status=None, reset=None, m=None, sharp_ref=100.0,
                min_exposed=0.5):
    """One flm_track_best_update on `state` (in place); -> taken bool [K]."""
    k = rec.shape[0]
    q, ok = quality(rec, lm, w, factor, status, sharp_ref, min_exposed)
    taken = np.zeros(k, bool)
    for i in range(k):
        prev = f64(-1.0) if (reset is not None and reset[i] != 0) else state["best_q"][i]
        if ok[i] and q[i] > prev:
            taken[i] = True
            state["gallery"][i] = faces[i]
            state["best_q"][i] = q[i]
            state["best_frame"][i] = frame_id
            if m is not None:
                state["best_m"][i] = m[i]
            state["best_lm"][i] = lm[i]
            state["best_rec"][i] = rec[i]
        else:
            state["best_q"][i] = prev
    return taken


def box_blur(img):
    """A 3x3 box blur of a float32 [h,w,3] image, edges replicated (the tests' blurred copies)."""
    p = np.pad(np.asarray(img, f32), ((1, 1), (1, 1), (0, 0)), mode="edge")
    h, w = img.shape[:2]
    acc = np.zeros_like(img, dtype=np.float64)
    for dy in range(3):
        for dx in range(3):
            acc += p[dy:dy + h, dx:dx + w]
    return (acc / 9.0).astype(f32)
