"""numpy restatement of the mesh of the piecewise-affine warp (include/flm.h, "shape-normalised faces"): the triangle map,
the anchors' frame positions and the per-(face, triangle) affines, float64 in the stated operation order (numpy neither
reorders nor fuses), plus `warp_mesh_ref`, the warp itself on a copy of the per-sample restatement of the frame-warp
tests (tests/test_gpu_frames.py).  No device, no library.
"""
import numpy as np

from oracle.warp_ref import fma

f32 = np.float32
f64 = np.float64
NO_TRI = 255


def edge(ax, ay, bx, by, qx, qy):
    """E_ab(q) = (bx-ax)*(qy-ay) - (by-ay)*(qx-ax): two products, one subtraction."""
    u = (bx - ax) * (qy - ay)
    v = (by - ay) * (qx - ax)
    return u - v


def mesh_map_ref(points, tris, h, w):
    """uint8 [h,w]: the lowest triangle whose three edge functions at the integer point are >= 0, 255 if none is."""
    pts = np.asarray(points, f64)
    qy, qx = np.mgrid[0:h, 0:w].astype(f64)
    out = np.full((h, w), NO_TRI, np.uint8)
    for t in range(len(tris) - 1, -1, -1):          # descending, so that the lowest index is written last
        (ax, ay), (bx, by), (cx, cy) = pts[tris[t][0]], pts[tris[t][1]], pts[tris[t][2]]
        inside = (edge(ax, ay, bx, by, qx, qy) >= 0) & (edge(bx, by, cx, cy, qx, qy) >= 0) & (edge(cx, cy, ax, ay, qx, qy) >= 0)
        out[inside] = t
    return out


def anchor_source_ref(m, d):
    """M^-1 d in float64 from the float32 M: m [K,2,3] float32, d [A,2] float64 -> [K,A,2]."""
    m = np.asarray(m, f32).astype(f64)
    m00, m01, m02 = m[:, 0, 0, None], m[:, 0, 1, None], m[:, 0, 2, None]
    m10, m11, m12 = m[:, 1, 0, None], m[:, 1, 1, None], m[:, 1, 2, None]
    with np.errstate(all="ignore"):
        det = m00 * m11 - m01 * m10
        i00, i01, i10, i11 = m11 / det, -m01 / det, -m10 / det, m00 / det
        tx, ty = d[None, :, 0] - m02, d[None, :, 1] - m12
        return np.stack([i00 * tx + i01 * ty, i10 * tx + i11 * ty], -1)


def mesh_sources_ref(lm, m, points, n_anchors):
    """The frame position of every mesh vertex of every face, float64 [K,P,2]: landmarks, then anchors."""
    pts = np.asarray(points, f64)
    c = pts.shape[0] - n_anchors
    lm = np.asarray(lm, f64)
    assert lm.shape[1] == c
    return np.concatenate([lm, anchor_source_ref(m, pts[c:])], 1)


def mesh_affines_ref(lm, m, points, tris, n_anchors, min_det=1e-6):
    """float32 [K,T,2,3]: the forward matrix frame px -> aligned px of every (face, triangle); the face's M where
    !(fabs(det) >= min_det)."""
    pts = np.asarray(points, f64)
    tris = np.asarray(tris)
    m = np.asarray(m, f32)
    s = mesh_sources_ref(lm, m, pts, n_anchors)                    # [K,P,2]
    s0, s1, s2 = s[:, tris[:, 0]], s[:, tris[:, 1]], s[:, tris[:, 2]]   # [K,T,2]
    d0, d1, d2 = pts[tris[:, 0]][None], pts[tris[:, 1]][None], pts[tris[:, 2]][None]
    with np.errstate(all="ignore"):
        e1x, e1y = s1[..., 0] - s0[..., 0], s1[..., 1] - s0[..., 1]
        e2x, e2y = s2[..., 0] - s0[..., 0], s2[..., 1] - s0[..., 1]
        g1x, g1y = d1[..., 0] - d0[..., 0], d1[..., 1] - d0[..., 1]
        g2x, g2y = d2[..., 0] - d0[..., 0], d2[..., 1] - d0[..., 1]
        det = e1x * e2y - e1y * e2x
        a00 = (g1x * e2y - g2x * e1y) / det
        a01 = (g2x * e1x - g1x * e2x) / det
        a10 = (g1y * e2y - g2y * e1y) / det
        a11 = (g2y * e1x - g1y * e2x) / det
        a02 = d0[..., 0] - (a00 * s0[..., 0] + a01 * s0[..., 1])
        a12 = d0[..., 1] - (a10 * s0[..., 0] + a11 * s0[..., 1])
        aff = np.stack([np.stack([a00, a01, a02], -1), np.stack([a10, a11, a12], -1)], -2).astype(f32)
        ok = np.abs(det) >= min_det                                 # False for a NaN
    return np.where(ok[..., None, None], aff, m[:, None]).astype(f32)


# ---- the warp: a copy of the per-sample restatement of tests/test_gpu_frames.py ------------------------------------------
def inverse_ref(m):
    """warp_inverse on arrays of matrices [...,2,3] float32 -> six float32 arrays."""
    m = np.asarray(m, f32)
    m00, m01, m02, m10, m11, m12 = m[..., 0, 0], m[..., 0, 1], m[..., 0, 2], m[..., 1, 0], m[..., 1, 1], m[..., 1, 2]
    with np.errstate(all="ignore"):
        det = fma(m00, m11, -(m01 * m10))
        idet = f32(1.0) / det
        i00, i01, i10, i11 = m11 * idet, -m01 * idet, -m10 * idet, m00 * idet
        return i00, i01, -fma(i00, m02, i01 * m12), i10, i11, -fma(i10, m02, i11 * m12)


def sample_ref(src, inv, xd, yd):
    """One bilinear sample per destination coordinate; `inv` may hold one value per pixel."""
    i00, i01, i02, i10, i11, i12 = inv
    hs, ws = src.shape[:2]
    xs = fma(i00, xd, fma(i01, yd, i02))
    ys = fma(i10, xd, fma(i11, yd, i12))
    xs = np.minimum(np.maximum(xs, f32(0)), f32(ws - 1))
    ys = np.minimum(np.maximum(ys, f32(0)), f32(hs - 1))
    xf, yf = np.floor(xs), np.floor(ys)
    fx, fy = (xs - xf).astype(f32), (ys - yf).astype(f32)
    x0, y0 = xf.astype(np.int64), yf.astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, ws - 1), np.minimum(y0 + 1, hs - 1)
    p00, p01 = src[y0, x0].astype(f32), src[y0, x1].astype(f32)
    p10, p11 = src[y1, x0].astype(f32), src[y1, x1].astype(f32)
    top = fma(fx[..., None], p01 - p00, p00)
    bot = fma(fx[..., None], p11 - p10, p10)
    return fma(fy[..., None], bot - top, top)


def _warp_per_pixel(frame, inv, hd, wd, s):
    yd0, xd0 = np.mgrid[0:hd, 0:wd]
    xd0, yd0 = xd0.astype(f32), yd0.astype(f32)
    acc = None
    for i in range(s):
        for j in range(s):
            xd = xd0 if s == 1 else (xd0 + f32(2 * j + 1 - s) / f32(2 * s)).astype(f32)
            yd = yd0 if s == 1 else (yd0 + f32(2 * i + 1 - s) / f32(2 * s)).astype(f32)
            v = sample_ref(frame, inv, xd, yd)
            acc = v if acc is None else (acc + v).astype(f32)
    return acc if s == 1 else (acc * (f32(1.0) / f32(s * s))).astype(f32)


def warp_affine_frame_ref(frame, m, hd, wd, s=1):
    """One face of flm_warp_affine_frames from one BGR frame: float32 [hd,wd,3]."""
    return _warp_per_pixel(frame, inverse_ref(np.asarray(m, f32)), hd, wd, s)


def warp_mesh_ref(frame, lm, m, points, tris, n_anchors, hd, wd, s=1, min_det=1e-6):
    """One face of flm_warp_mesh_frames from one BGR frame, float32 [hd,wd,3] NHWC BGR: the triangle of every pixel from
    the map at the pixel's centre, that triangle's affine inverted as warp_inverse inverts it, the s x s samples of the
    frame warps; 0 where the map has no triangle."""
    tmap = mesh_map_ref(points, tris, hd, wd)
    aff = mesh_affines_ref(np.asarray(lm, f64)[None], np.asarray(m, f32)[None], points, tris, n_anchors, min_det)[0]
    inv_t = inverse_ref(aff)                                       # six [T] arrays
    idx = np.where(tmap == NO_TRI, 0, tmap).astype(np.int64)
    out = _warp_per_pixel(frame, tuple(v[idx] for v in inv_t), hd, wd, s)
    out[tmap == NO_TRI] = 0
    return out
