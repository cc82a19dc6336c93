"""The cases tests/test_flow_native_host.py and tests/test_gpu_flow.py run against tests/flow_ref.py: two crops, the
matrix, the previous landmarks in frame px and the options of one flm_landmark_flow call each.  Every case is built from a
seed; the reference answer of a case is computed once (`expected`) and shared."""
import functools

import numpy as np

import flow_ref


def _rot(deg, scale, tx, ty):
    a = np.deg2rad(deg)
    return np.array([[scale * np.cos(a), -scale * np.sin(a), tx], [scale * np.sin(a), scale * np.cos(a), ty]], np.float32)


def _to_frame(m, pts):
    """Crop px -> frame px under the float32 matrix m (a float64 inverse: the points only have to land near pts)."""
    a = np.asarray(m, np.float64)
    inv = np.linalg.inv(a[:, :2])
    return (pts - a[:, 2]) @ inv.T


def _points(rng, c, h, w, r):
    """c points in crop px: interior, integer positions, fraction 31/32, within the radius of each border, the corners."""
    b = min(10, (min(h, w) - 1) // 2)
    pts = np.stack([rng.uniform(b, w - 1 - b, c), rng.uniform(b, h - 1 - b, c)], axis=1)
    special = [(12.0, 13.0), (float(w // 2), float(h // 2)), (20.0 + 31 / 32, 17.0 + 31 / 32), (w - 12 - 1 / 32, 11 + 31 / 32),
               (r - 2.5, h / 2), (w - 1 - (r - 2.5), h / 2), (w / 2, r - 3.0), (w / 2, h - 1 - (r - 3.0)),
               (0.0, 0.0), (w - 1.0, 0.0), (0.0, h - 1.0), (w - 1.0, h - 1.0), (0.25, h - 1.0), (w - 1.0, 0.5)]
    n = min(c, len(special))
    idx = rng.permutation(c)[:n]
    pts[idx] = np.asarray(special[:n])
    return pts


def make(name, k, c, h, w, ch, levels, radius, seed, shift=(1.25, -0.75), m=None, weights=False, rejected=True, zero=None,
         coarse_flat=None, **opts):
    rng = np.random.default_rng(seed)
    o = flow_ref.options(levels=levels, radius=radius, **opts)
    prev = np.zeros((k, h, w, ch), np.uint8)
    cur = np.zeros_like(prev)
    for f in range(k):
        tex = flow_ref.texture(h, w, seed * 100 + f)
        a, b = flow_ref.shifted(tex, 0.0, 0.0), flow_ref.shifted(tex, *shift)
        if f == zero:
            a[:], b[:] = 0, 0
        if f == coarse_flat:    # blocks of 2x2 in a checkerboard: level 1 is a checkerboard, level 2 and above are flat
            yy, xx = np.mgrid[:h, :w]
            a = ((((xx % 4) < 2) ^ ((yy % 4) < 2)) * 255).astype(np.uint8)
            b = np.roll(a, 1, axis=1)
        if ch == 1:
            prev[f, ..., 0], cur[f, ..., 0] = a, b
        else:                   # colours whose luma is the texture up to rounding, channel by channel different
            for j, g in enumerate((0.8, 1.0, 1.1)):
                prev[f, ..., j] = np.clip(a * g, 0, 255).astype(np.uint8)
                cur[f, ..., j] = np.clip(b * g, 0, 255).astype(np.uint8)
    if m is None:
        mats = np.tile(np.array([[1, 0, 0], [0, 1, 0]], np.float32), (k, 1, 1))
    else:
        mats = np.stack([m(f) for f in range(k)]).astype(np.float32)
    lm = np.stack([_to_frame(mats[f], _points(rng, c, h, w, radius)) for f in range(k)])
    if rejected:                # (-1,-1), a NaN, an infinity, a negative coordinate: NO_HISTORY each
        bad = [(-1.0, -1.0), (np.nan, 3.0), (np.inf, 5.0), (4.0, -0.5)]
        for j, b in enumerate(bad[:max(1, c // 5)]):
            lm[(j * 7) % k, (j * 3 + 1) % c] = b
    wt = rng.uniform(0.05, 1.0, (k, c)) if weights else None
    if ch == 1:
        prev, cur = prev[..., 0], cur[..., 0]
    return dict(name=name, prev=np.ascontiguousarray(prev), cur=np.ascontiguousarray(cur), m=mats,
                lm=np.ascontiguousarray(lm), w=wt, opts=o, ch=ch, hw=(h, w))


@functools.lru_cache(maxsize=None)
def cases():
    rot = lambda f: _rot(7.0 + 3 * f, 0.5 + 0.05 * f, 9.0 - f, 4.0 + 2 * f)
    return (
        make("k1_c5_luma", 1, 5, 64, 64, 1, 3, 7, 1),
        make("k3_c68_bgr", 3, 68, 64, 64, 3, 3, 7, 2, weights=True, zero=1),
        make("k9_c68_luma_r3", 9, 68, 64, 64, 1, 3, 3, 3, shift=(3.3, -2.6), zero=4, coarse_flat=7),
        make("k3_c5_32x48_two_levels", 3, 5, 32, 48, 3, 2, 7, 4, shift=(-0.5, 1.0)),
        make("k3_c68_rotated_m", 3, 68, 64, 64, 1, 3, 7, 5, m=rot, weights=True),
        make("k1_c68_one_iteration", 1, 68, 64, 64, 3, 3, 7, 6, shift=(3.3, -2.6), max_iter=1),
        make("k3_c5_gates", 3, 5, 64, 64, 1, 3, 3, 7, shift=(3.3, -2.6), max_move=1.0, max_err=0.5, min_eig=0.0),
        make("k1_c5_one_level_odd", 1, 5, 9, 7, 3, 1, 2, 8, shift=(0.5, 0.0), rejected=False),
    )


@functools.lru_cache(maxsize=None)
def expected(i):
    """(pyr_prev, pyr_cur, lm, w, err, flags) of case i by flow_ref, computed once."""
    c = cases()[i]
    lv = c["opts"]["levels"]
    return (flow_ref.pyramid_flat(c["prev"], lv), flow_ref.pyramid_flat(c["cur"], lv)) + \
        flow_ref.landmark_flow(c["prev"], c["cur"], c["lm"], c["m"], c["opts"], c["w"])
