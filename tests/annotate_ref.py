"""numpy restatement of flm_frames_annotate and flm_bgr_to_yuv (include/flm.h, "frame annotation"): per frame the regions,
the union of the mosaic's cells -- each averaged from the ORIGINAL frame --, then the outlines of all faces, then the marks
of all faces.  A BGR form on [F,H,W,3] rings and an NV12 form on the raw [F,rows,pitch] slot bytes.  Sequential, face by
face: it shares no code and no order of evaluation with the kernels."""
from fractions import Fraction

import numpy as np

LIM = 2 ** 30
DEFAULT_MARGIN = (0.1, 0.35, 0.1, 0.1)
DISC = [(dx, dy) for dy in range(-2, 3) for dx in range(-2, 3) if dx * dx + dy * dy <= 5]
_K = {"bt601": (Fraction(299, 1000), Fraction(114, 1000)), "bt709": (Fraction(2126, 10000), Fraction(722, 10000))}


def _round(q):
    """round-half-away of an exact fraction (no coefficient lies on a tie)."""
    n = (abs(q) * 2 + 1) // 2
    return int(n if q >= 0 else -n)


def yuv_coefficients(matrix):
    """round(exact x 2^16) of the limited-range forward matrix, rows Y, U, V over (B, G, R), from Kr and Kb in exact
    arithmetic: Y = 16 + 219/255 * (Kr R + Kg G + Kb B); U = 128 + 224/255 * (B - Y') / (2 (1 - Kb)); V likewise with R, Kr."""
    kr, kb = _K[matrix]
    kg = 1 - kr - kb
    ys, cs = Fraction(219, 255) * 65536, Fraction(224, 255) * 65536
    y = [kb * ys, kg * ys, kr * ys]
    u = [(1 - kb) / (2 * (1 - kb)) * cs, -kg / (2 * (1 - kb)) * cs, -kr / (2 * (1 - kb)) * cs]
    v = [-kb / (2 * (1 - kr)) * cs, -kg / (2 * (1 - kr)) * cs, (1 - kr) / (2 * (1 - kr)) * cs]
    return [[_round(c) for c in row] for row in (y, u, v)]


def bgr_to_yuv(bgr, matrix):
    """uint8 [...,3] (B,G,R) -> uint8 [...,3] (Y,U,V): int32 arithmetic with an arithmetic shift, as flm_bgr_to_yuv."""
    cy, cu, cv = yuv_coefficients(matrix)
    p = np.asarray(bgr).astype(np.int64)
    dot = lambda c: (c[0] * p[..., 0] + c[1] * p[..., 1] + c[2] * p[..., 2] + (1 << 15)) >> 16
    y = np.clip(16 + dot(cy), 16, 235)
    u = np.clip(128 + dot(cu), 16, 240)
    v = np.clip(128 + dot(cv), 16, 240)
    return np.stack([y, u, v], -1).astype(np.uint8)


def accepted(x, y):
    return bool(x >= 0 and y >= 0 and x <= LIM and y <= LIM)


def _coord(v):
    return int(min(max(np.float64(v), np.float64(-LIM)), np.float64(LIM)))


def region(points, margin=DEFAULT_MARGIN):
    """R of one face: points float64 [C,2]."""
    pts = [(np.float64(x), np.float64(y)) for x, y in np.asarray(points, np.float64).reshape(-1, 2) if accepted(x, y)]
    if not pts:
        return (0, 0, 0, 0)
    mnx, mny = min(p[0] for p in pts), min(p[1] for p in pts)
    mxx, mxy = max(p[0] for p in pts), max(p[1] for p in pts)
    side = max(mxx - mnx, mxy - mny)
    m = [np.float64(v) for v in margin]
    return (_coord(np.floor(mnx - m[0] * side)), _coord(np.floor(mny - m[1] * side)),
            _coord(np.ceil(mxx + m[2] * side) + np.float64(1.0)), _coord(np.ceil(mxy + m[3] * side) + np.float64(1.0)))


def regions(lm, margin=DEFAULT_MARGIN):
    lm = np.asarray(lm, np.float64)
    return np.array([region(face, margin) for face in lm], np.int32).reshape(len(lm), 4)


def _clip(r, fw, fh):
    return (max(r[0], 0), max(r[1], 0), min(r[2], fw), min(r[3], fh))


def _faces(lm, frame_idx, nframes, fh, fw, margin):
    """(R, [(face, frame, R, P) for the faces that take part])."""
    reg = regions(lm, margin)
    fi = np.zeros(len(reg), np.int64) if frame_idx is None else np.asarray(frame_idx, np.int64)
    part = []
    for k, r in enumerate(reg.tolist()):
        p = _clip(r, fw, fh)
        if p[2] > p[0] and p[3] > p[1] and 0 <= fi[k] < nframes:
            part.append((k, int(fi[k]), tuple(r), p))
    return reg, part


def _cells(part, frame, s):
    cells = set()
    for _, f, _, p in part:
        if f == frame:
            for cy in range(p[1] // s, (p[3] - 1) // s + 1):
                for cx in range(p[0] // s, (p[2] - 1) // s + 1):
                    cells.add((cx, cy))
    return sorted(cells)


def _outline(r, p, t):
    """The pixels of P on the outline of R, as (xs, ys) index arrays."""
    ys, xs = np.mgrid[p[1]:p[3], p[0]:p[2]]
    on = (xs < r[0] + t) | (xs >= r[2] - t) | (ys < r[1] + t) | (ys >= r[3] - t)
    return xs[on], ys[on]


def _marks(points, fw, fh):
    """The pixels of the discs of the accepted points, clipped to the frame, as (xs, ys) index arrays."""
    px = [(int(x) + dx, int(y) + dy) for x, y in np.asarray(points, np.float64).reshape(-1, 2) if accepted(x, y)
          for dx, dy in DISC]
    px = [(x, y) for x, y in px if 0 <= x < fw and 0 <= y < fh]
    return np.array([x for x, _ in px], np.int64), np.array([y for _, y in px], np.int64)


def annotate_bgr(frames, lm, frame_idx=None, marks=1, box=0, redact=0, margin=DEFAULT_MARGIN, mark_bgr=(0, 255, 0),
                 box_bgr=(0, 255, 0)):
    """frames uint8 [F,H,W,3] -> (the annotated copy, regions int32 [K,4])."""
    frames = np.asarray(frames)
    nf, fh, fw = frames.shape[:3]
    out = frames.copy()
    reg, part = _faces(lm, frame_idx, nf, fh, fw, margin)
    if redact:
        s = redact
        for f in range(nf):
            for cx, cy in _cells(part, f, s):
                blk = frames[f, cy * s:min((cy + 1) * s, fh), cx * s:min((cx + 1) * s, fw)].astype(np.int64)
                n = blk.shape[0] * blk.shape[1]
                out[f, cy * s:cy * s + blk.shape[0], cx * s:cx * s + blk.shape[1]] = (blk.sum((0, 1)) + (n >> 1)) // n
    if box:
        for _, f, r, p in part:
            xs, ys = _outline(r, p, box)
            out[f, ys, xs] = box_bgr
    if marks:
        for k, f, _, _ in part:
            xs, ys = _marks(lm[k], fw, fh)
            out[f, ys, xs] = mark_bgr
    return out, reg


def annotate_nv12(ring, fh, fw, uv_row, matrix, lm, frame_idx=None, marks=1, box=0, redact=0, margin=DEFAULT_MARGIN,
                  mark_bgr=(0, 255, 0), box_bgr=(0, 255, 0)):
    """ring uint8 [F,rows,pitch], luma rows 0..fh-1 and U,V rows from `uv_row` of every slot, both at the ring's pitch ->
    (the annotated copy, regions).  Only bytes of the two planes' fw columns can change."""
    ring = np.asarray(ring)
    nf = ring.shape[0]
    out = ring.copy()
    reg, part = _faces(lm, frame_idx, nf, fh, fw, margin)

    def paint(f, xy, yuv):
        xs, ys = xy
        out[f, ys, xs] = yuv[0]
        out[f, uv_row + (ys >> 1), xs & ~1] = yuv[1]
        out[f, uv_row + (ys >> 1), (xs & ~1) + 1] = yuv[2]

    if redact:
        s = redact
        for f in range(nf):
            for cx, cy in _cells(part, f, s):
                x0, y0, x1, y1 = cx * s, cy * s, min((cx + 1) * s, fw), min((cy + 1) * s, fh)
                n = (x1 - x0) * (y1 - y0)
                m = n // 4
                out[f, y0:y1, x0:x1] = (int(ring[f, y0:y1, x0:x1].astype(np.int64).sum()) + (n >> 1)) // n
                uv = ring[f, uv_row + y0 // 2:uv_row + y1 // 2, x0:x1].astype(np.int64)
                out[f, uv_row + y0 // 2:uv_row + y1 // 2, x0:x1:2] = (int(uv[:, 0::2].sum()) + (m >> 1)) // m
                out[f, uv_row + y0 // 2:uv_row + y1 // 2, x0 + 1:x1:2] = (int(uv[:, 1::2].sum()) + (m >> 1)) // m
    if box:
        yuv = bgr_to_yuv(np.array(box_bgr, np.uint8), matrix)
        for _, f, r, p in part:
            paint(f, _outline(r, p, box), yuv)
    if marks:
        yuv = bgr_to_yuv(np.array(mark_bgr, np.uint8), matrix)
        for k, f, _, _ in part:
            paint(f, _marks(lm[k], fw, fh), yuv)
    return out, reg
