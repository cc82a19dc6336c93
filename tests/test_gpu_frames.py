"""GPU parity of the frame-space tail: flm_landmarks_to_frame, flm_warp_affine_frames, prediction.align_frames.

Bars: the landmark mapping (three float64 operations on both sides) is bit-exact; the one-sample warp is the same bits
as flm_warp_affine on the face's frame and within 1 ULP of oracle/warp_ref.py (the bar of tests/test_gpu_align.py);
the s x s sample means are held to the bound derived in `mean_bound`; the similarity fit is bit-exact against
`similarity_ref` as in tests/test_gpu_stream.py.  The restatements of the new arithmetic live in this file.
"""
import numpy as np
import pytest
import torch

from oracle import warp_ref
from oracle.warp_ref import fma

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.fixture(scope="module")
def mods():
    import flm_amd  # noqa: F401
    from flm_amd import _lib, alignment, prediction
    _lib.load()
    return alignment, prediction


# ---- restatements ------------------------------------------------------------------------------------------------
def clip_box(b, fh, fw):
    cx0, cx1 = min(max(int(b[0]), 0), fw), min(max(int(b[2]), 0), fw)
    cy0, cy1 = min(max(int(b[1]), 0), fh), min(max(int(b[3]), 0), fh)
    return cx0, cy0, cx1 - cx0, cy1 - cy0


def landmarks_to_frame_ref(lm, boxes, gh, gw, fh, fw):
    out = np.full(lm.shape, -1.0, np.float64)
    for f in range(lm.shape[0]):
        cx0, cy0, cw, ch = clip_box(boxes[f], fh, fw)
        if cw <= 0 or ch <= 0:
            continue
        sx, sy = np.float64(cw) / np.float64(gw), np.float64(ch) / np.float64(gh)
        for i in range(lm.shape[1]):
            x, y = lm[f, i]
            if x < 0.0 or y < 0.0:
                continue
            out[f, i, 0] = np.float64(cx0) + x * sx
            out[f, i, 1] = np.float64(cy0) + y * sy
    return out


def sample_ref(src, inv, xd, yd):
    """One bilinear sample per destination coordinate: warp_kernel's arithmetic (csrc/flm_misc.hip) restated."""
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
    return fma(fy[..., None], bot - top, top), xs, ys


def inverse_ref(m):
    m00, m01, m02, m10, m11, m12 = [f32(v) for v in np.asarray(m, f32).reshape(-1)]
    det = fma(m00, m11, -(m01 * m10))
    idet = f32(1.0) / det
    i00, i01, i10, i11 = m11 * idet, -m01 * idet, -m10 * idet, m00 * idet
    return i00, i01, -fma(i00, m02, i01 * m12), i10, i11, -fma(i10, m02, i11 * m12)


def warp_frames_ref(frames, idx, boxes, m, hd, wd, s):
    """flm_warp_affine_frames restated: s x s samples at xd + (2j+1-s)/(2s), yd + (2i+1-s)/(2s), added in float32 in
    row-major order from the first, times 1/(s*s)."""
    nf, fh, fw = frames.shape[:3]
    out = np.zeros((m.shape[0], hd, wd, 3), f32)
    yd0, xd0 = np.mgrid[0:hd, 0:wd]
    xd0, yd0 = xd0.astype(f32), yd0.astype(f32)
    for f in range(m.shape[0]):
        fi = 0 if idx is None else int(idx[f])
        if not 0 <= fi < nf:
            continue
        if boxes is not None:
            _, _, cw, ch = clip_box(boxes[f], fh, fw)
            if cw <= 0 or ch <= 0:
                continue
        inv = inverse_ref(m[f])
        acc = None
        for i in range(s):
            for j in range(s):
                xd = xd0 if s == 1 else (xd0 + f32(2 * j + 1 - s) / f32(2 * s)).astype(f32)
                yd = yd0 if s == 1 else (yd0 + f32(2 * i + 1 - s) / f32(2 * s)).astype(f32)
                v = sample_ref(frames[fi], inv, xd, yd)[0]
                acc = v if acc is None else (acc + v).astype(f32)
        out[f] = acc if s == 1 else (acc * (f32(1.0) / f32(s * s))).astype(f32)
    return out


def mean_bound(s):
    """Each sample is within 1 ULP of its restatement (ulp(255) = 2^-16); a one-ULP difference in an addend can move
    each of the s*s-1 float32 additions by one ULP of the running sum (<= 2^-12 below 4096): bound on the mean."""
    return (s * s * 2.0 ** -16 + (s * s - 1) * 2.0 ** -12) / (s * s)


def ulp_diff(a, b):
    ai = a.view(np.int32).astype(np.int64)
    bi = b.view(np.int32).astype(np.int64)
    ai = np.where(ai < 0, -(ai & 0x7fffffff), ai)
    bi = np.where(bi < 0, -(bi & 0x7fffffff), bi)
    return np.abs(ai - bi)


def frame_sims(rng, n, fh, fw, hd, wd):
    """Similarity matrices frame px -> aligned px around random frame points: strong down-scales (a 400 px face to
    the aligned size and beyond), near-unit scales, rotations; centres near the border send samples out of the frame."""
    m = np.zeros((n, 2, 3), f32)
    for i in range(n):
        s = float(rng.choice([0.06, 0.12, 0.28, 0.6, 1.0, 1.7]))
        th = rng.uniform(-np.pi, np.pi)
        cx, cy = rng.uniform(-0.1 * fw, 1.1 * fw), rng.uniform(-0.1 * fh, 1.1 * fh)
        a, b = s * np.cos(th), s * np.sin(th)
        m[i] = [[a, -b, wd / 2 - (a * cx - b * cy)], [b, a, hd / 2 - (b * cx + a * cy)]]
    return m


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


# ---- 1. landmarks -------------------------------------------------------------------------------------------------
def test_landmarks_to_frame_bit_exact(mods):
    A, _ = mods
    rng = np.random.default_rng(31)
    fh, fw, gh, gw = 1080, 1920, 264, 264
    boxes = np.array([[100, 120, 356, 376], [900, 400, 1300, 800],         # inside the frame
                      [-40, 300, 160, 500], [1800, 300, 2000, 500],        # out on the left, on the right
                      [500, -60, 700, 140], [500, 980, 700, 1180],         # out at the top, at the bottom
                      [-80, -80, 120, 120], [1850, 1000, 2050, 1200],      # corners
                      [2000, 100, 2200, 300], [300, -300, 500, -100],      # entirely outside
                      [0, 0, 1920, 1080], [700, 700, 700, 900]], np.int32)  # the whole frame; zero width
    k = boxes.shape[0]
    lm = rng.uniform(0, 263, (k, 68, 2))
    lm[0, 5] = [-1, -1]
    lm[2, 0] = [-1, -1]
    lm[3, 67] = [-1, 12.5]           # one negative coordinate rejects the point
    lm[4, 11] = [7.25, -1]
    lm[5, :] = -1
    exp = landmarks_to_frame_ref(lm, boxes, gh, gw, fh, fw)
    lmd, bd = dev(lm), dev(boxes)
    got = A.landmarks_to_frame_device(lmd, bd, (gh, gw), (fh, fw))
    assert got.dtype == torch.float64 and got.is_cuda and got.data_ptr() != lmd.data_ptr()
    assert np.array_equal(got.cpu().numpy(), exp)
    assert torch.equal(lmd, dev(lm))                                  # the input is left alone
    for f in (8, 9, 11):
        assert (exp[f] == -1).all()
    assert (exp[0, 5] == -1).all() and (exp[3, 67] == -1).all() and (exp[4, 11] == -1).all() and (exp[5] == -1).all()
    assert exp[2, 1, 0] == 0.0 + lm[2, 1, 0] * (160.0 / 264.0)       # the clipped region, not the box
    # rectangular grid and a non-square frame region, another class count
    lm2 = rng.uniform(0, 100, (3, 5, 2))
    b2 = np.array([[10, 20, 90, 70], [-5, -5, 40, 30], [60, 50, 200, 100]], np.int32)
    got2 = A.landmarks_to_frame_device(dev(lm2), dev(b2), (104, 136), (90, 120)).cpu().numpy()
    assert np.array_equal(got2, landmarks_to_frame_ref(lm2, b2, 104, 136, 90, 120))
    # in place
    r = A.landmarks_to_frame_device(lmd, bd, (gh, gw), (fh, fw), out=lmd)
    assert r.data_ptr() == lmd.data_ptr() and np.array_equal(lmd.cpu().numpy(), exp)
    with pytest.raises(ValueError):
        A.landmarks_to_frame_device(lmd, bd[:3], (gh, gw), (fh, fw))
    with pytest.raises(ValueError):
        A.landmarks_to_frame_device(lmd, bd.to(torch.int64), (gh, gw), (fh, fw))
    with pytest.raises(ValueError):
        A.landmarks_to_frame_device(lmd, bd, (gh, gw), (fh, fw), out=torch.empty((k, 68, 2), dtype=torch.float32, device="cuda"))
    assert tuple(A.landmarks_to_frame_device(lmd[:0], bd[:0], (gh, gw), (fh, fw)).shape) == (0, 68, 2)


# ---- 2. one sample per pixel ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 40, 52, 33, 47), (4, 61, 77, 30, 34), (3, 90, 120, 112, 112),
                                   (2, 64, 80, 256, 256), (2, 40, 52, 48, 60)])
def test_warp_frames_equals_warp_affine_small(mods, shape):
    """Small frames; (33,47): pixel count not a multiple of 4; (30,34): of 4, not of 64; 112x112; 256x256; (48,60) on a
    40x52 frame with the identity: every column from fw-1 on is xs = fw-1 exactly (the x0 = fw-1 pair)."""
    A, _ = mods
    nf, fh, fw, hd, wd = shape
    rng = np.random.default_rng(hd * 1000 + wd)
    frames = rng.integers(0, 256, (nf, fh, fw, 3), dtype=np.uint8)
    k = 11
    idx = rng.integers(0, nf, k).astype(np.int32)                  # slots out of order, repeated
    m = frame_sims(rng, k, fh, fw, hd, wd)
    m[0] = [[1, 0, 0], [0, 1, 0]]
    m[1] = [[1, 0, wd - fw], [0, 1, hd - fh]]                      # shifted identity: the last pixel is (fw-1, fh-1)
    fd, md, idd = dev(frames), dev(m), dev(idx)
    got = A.warp_frames_device(fd, md, hd, wd, frame_index_dev=idd)
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (k, hd, wd, 3)
    same = A.warp_device(fd[idd.long()].contiguous(), md, hd, wd)   # device against device: the same bits
    assert torch.equal(got, same)
    exp = warp_frames_ref(frames, idx, None, m, hd, wd, 1)
    u = ulp_diff(got.cpu().numpy(), exp)
    print("warp_frames %s: %d of %d values differ from the restatement, max %d ULP" % (shape, int((u > 0).sum()), u.size, int(u.max())))
    assert u.max() <= 1
    assert np.array_equal(exp, warp_ref.warp_affine_ref(frames[idx], m, hd, wd))   # the two restatements agree
    if wd >= fw:
        xs = sample_ref(frames[0], inverse_ref(m[0]), *[v.astype(f32) for v in np.mgrid[0:hd, 0:wd][::-1]])[1]
        assert (xs == fw - 1).sum() >= hd                           # the x0 = fw-1 case is in the data
    # no frame_index: every face reads slot 0
    got0 = A.warp_frames_device(fd, md, hd, wd)
    assert torch.equal(got0, A.warp_device(fd[:1].expand(k, -1, -1, -1).contiguous(), md, hd, wd))


def test_warp_frames_1080p_ring(mods):
    A, _ = mods
    rng = np.random.default_rng(33)
    nf, fh, fw, hd, wd = 8, 1080, 1920, 112, 112
    frames = rng.integers(0, 256, (nf, fh, fw, 3), dtype=np.uint8)
    k = 12
    idx = np.array([7, 0, 3, 3, 5, 1, 6, 2, 4, 7, 0, 5], np.int32)
    m = frame_sims(rng, k, fh, fw, hd, wd)
    m[0] = [[1, 0, wd - fw], [0, 1, hd - fh]]                      # the frame's last corner, x0 = fw-1 included
    fd, md, idd = dev(frames), dev(m), dev(idx)
    got = A.warp_frames_device(fd, md, hd, wd, frame_index_dev=idd)
    same = torch.cat([A.warp_device(fd[int(idx[f])][None], md[f:f + 1], hd, wd) for f in range(k)], 0)
    assert torch.equal(got, same)
    u = ulp_diff(got.cpu().numpy(), warp_frames_ref(frames, idx, None, m, hd, wd, 1))
    print("warp_frames 1080p: max %d ULP" % int(u.max()))
    assert u.max() <= 1
    assert got[0, -1, -1].tolist() == frames[7, -1, -1].astype(np.float32).tolist()


def test_warp_frames_zero_fill(mods):
    """A slot outside the ring or a clipped box without pixels gives zeros; the neighbours are what they are alone."""
    A, _ = mods
    rng = np.random.default_rng(34)
    nf, fh, fw, hd, wd = 3, 60, 80, 30, 34
    frames = rng.integers(1, 256, (nf, fh, fw, 3), dtype=np.uint8)       # no zero pixel: a zero output is the fill
    k = 7
    idx = np.array([0, -1, 2, 3, 1, 1, 2], np.int32)                      # faces 1, 3: outside [0, 3)
    boxes = np.array([[5, 5, 40, 40], [5, 5, 40, 40], [10, 10, 50, 50], [0, 0, 20, 20],
                      [90, 10, 120, 40], [-30, -30, 0, 10], [60, 40, 100, 80]], np.int32)   # faces 4, 5: empty
    m = frame_sims(rng, k, fh, fw, hd, wd)
    fd, md = dev(frames), dev(m)
    for s in (1, 2, 4):
        out = torch.full((k, hd, wd, 3), 777.0, dtype=torch.float32, device="cuda")
        r = A.warp_frames_device(fd, md, hd, wd, frame_index_dev=dev(idx), boxes_dev=dev(boxes), samples=s, out=out)
        assert r.data_ptr() == out.data_ptr()
        for f in (1, 3, 4, 5):
            assert not out[f].any(), (s, f)
        ok = [0, 2, 6]
        alone = A.warp_frames_device(fd, md[ok].contiguous(), hd, wd, frame_index_dev=dev(idx[ok]), samples=s)
        assert torch.equal(out[ok], alone) and (alone != 0).all()
    # without boxes only the ring slot decides
    nb = A.warp_frames_device(fd, md, hd, wd, frame_index_dev=dev(idx))
    assert not nb[1].any() and not nb[3].any() and nb[4].any() and nb[5].any()
    with pytest.raises(ValueError):
        A.warp_frames_device(fd, md, hd, wd, frame_index_dev=dev(idx[:3]))
    with pytest.raises(ValueError):
        A.warp_frames_device(fd, md, hd, wd, samples=3)
    with pytest.raises(ValueError):
        A.warp_frames_device(fd, md, hd, wd, out=torch.empty((k, hd, wd, 3), dtype=torch.float64, device="cuda"))
    assert tuple(A.warp_frames_device(fd, md[:0], hd, wd).shape) == (0, hd, wd, 3)


# ---- 3. s x s samples per pixel ------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [2, 4])
@pytest.mark.parametrize("shape", [(3, 61, 77, 33, 47), (2, 200, 240, 112, 112)])
def test_warp_frames_sample_grid(mods, s, shape):
    A, _ = mods
    nf, fh, fw, hd, wd = shape
    rng = np.random.default_rng(35 + s)
    frames = rng.integers(0, 256, (nf, fh, fw, 3), dtype=np.uint8)
    k = 9
    idx = rng.integers(0, nf, k).astype(np.int32)
    m = frame_sims(rng, k, fh, fw, hd, wd)
    m[0] = [[1, 0, 0], [0, 1, 0]]
    got = A.warp_frames_device(dev(frames), dev(m), hd, wd, frame_index_dev=dev(idx), samples=s).cpu().numpy()
    exp = warp_frames_ref(frames, idx, None, m, hd, wd, s)
    d = np.abs(got.astype(np.float64) - exp.astype(np.float64))
    print("warp_frames samples=%d %s: max |diff| %.3g (bound %.3g), %d of %d values differ, max %d ULP"
          % (s, shape, d.max(), mean_bound(s), int((d > 0).sum()), d.size, int(ulp_diff(got, exp).max())))
    assert d.max() <= mean_bound(s)
    # the sample mean is not the single sample: on a strong down-scale the two differ by whole grey levels
    one = warp_frames_ref(frames, idx, None, m, hd, wd, 1)
    assert np.abs(exp - one).max() > 1.0


def test_warp_frames_constant_colour_and_single_sample(mods):
    A, _ = mods
    rng = np.random.default_rng(37)
    nf, fh, fw, hd, wd = 2, 70, 90, 40, 44
    col = np.array([17, 133, 251], np.uint8)
    frames = np.broadcast_to(col, (nf, fh, fw, 3)).copy()
    k = 6
    m = frame_sims(rng, k, fh, fw, hd, wd)
    idx = dev(rng.integers(0, nf, k).astype(np.int32))
    for s in (1, 2, 4):
        got = A.warp_frames_device(dev(frames), dev(m), hd, wd, frame_index_dev=idx, samples=s).cpu().numpy()
        assert np.array_equal(got, np.broadcast_to(col.astype(f32), got.shape)), s
    # samples=1 with every optional argument in use is still flm_warp_affine's bits
    noisy = dev(rng.integers(0, 256, (nf, fh, fw, 3), dtype=np.uint8))
    boxes = dev(np.tile(np.array([[5, 5, 60, 60]], np.int32), (k, 1)))
    got = A.warp_frames_device(noisy, dev(m), hd, wd, frame_index_dev=idx, boxes_dev=boxes, samples=1)
    assert torch.equal(got, A.warp_device(noisy[idx.long()].contiguous(), dev(m), hd, wd))


# ---- 4. end to end -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stream():
    from flm_amd.weights import synth_fcn8_weights
    rng = np.random.default_rng(41)
    frames = rng.integers(0, 256, (2, 1080, 1920, 3), dtype=np.uint8)
    # detector boxes of 96 ... 400 px; the last of slot 1 pokes out of the frame's right and bottom edges
    faces = [[[100, 120, 300, 360], [900, 400, 1296, 700], [1500, 60, 1596, 170]],
             [[40, 500, 420, 900], [1000, 200, 1180, 420], [1700, 850, 1960, 1100]]]
    return frames, faces, synth_fcn8_weights(68, seed=2)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_align_frames_end_to_end(mods, stream, dtype):
    A, P = mods
    from flm_amd.networks import LANDMARKS_MODELS
    frames, faces, params = stream
    model = LANDMARKS_MODELS["fcn_8"](68, input_height=256, input_width=256, dtype=dtype)
    model.load_weights(params)
    ring = dev(frames)
    slots = [1, 0]                                                    # entry 0 lives in ring slot 1
    aligned, m, lm, boxes_dev = P.align_frames(ring, faces, model, out_size=(112, 112), frame_index=slots)
    for t in (aligned, m, lm, boxes_dev):
        assert isinstance(t, torch.Tensor) and t.is_cuda
    k = 6
    assert tuple(aligned.shape) == (k, 112, 112, 3) and aligned.dtype == torch.float32
    assert tuple(m.shape) == (k, 2, 3) and m.dtype == torch.float32
    assert tuple(lm.shape) == (k, 68, 2) and lm.dtype == torch.float64
    boxes = np.asarray([b for f in faces for b in P.face_boxes(f)], np.int32)
    assert np.array_equal(boxes_dev.cpu().numpy(), boxes)
    sides = boxes[:, 2] - boxes[:, 0]
    assert sides.min() >= 96 and sides.max() <= 400 and boxes[5, 2] > 1920 and boxes[5, 3] > 1080
    # landmarks: the decode of the crops, taken to the frame
    crops, _, bdev, idev = P.crop_frames_device(ring, faces, 256, 256, frame_index=slots, return_device=True)
    assert np.array_equal(idev.cpu().numpy(), np.array([1, 1, 1, 0, 0, 0], np.int32)) and torch.equal(bdev, boxes_dev)
    crops_plain, _ = P.crop_frames_device(ring, faces, 256, 256, frame_index=slots)
    assert torch.equal(crops, crops_plain)
    grid = model.forward_device(crops, "landmarks", n_points=4).clone()
    assert torch.equal(lm, A.landmarks_to_frame_device(grid, bdev, (264, 264), (1080, 1920)))
    lm_np = lm.cpu().numpy()
    assert np.array_equal(lm_np, landmarks_to_frame_ref(grid.cpu().numpy(), boxes, 264, 264, 1080, 1920))
    # the fit: float64 sums in landmark order on both sides, rounded to float32 once
    tm = A.canonical_template(68, 112, 112)
    m_np = m.cpu().numpy()
    assert np.array_equal(m_np, warp_ref.similarity_ref(lm_np, tm))
    # the warp: one bilinear sampling of the frame, within 1 ULP of the restatement
    al = aligned.cpu().numpy()
    for f in range(k):
        exp = warp_ref.warp_affine_ref(frames[[1, 1, 1, 0, 0, 0][f]][None], m_np[f:f + 1], 112, 112)[0]
        assert ulp_diff(al[f], exp).max() <= 1, f
    # the fit is the least-squares similarity: the mapped landmarks lie no further from the template (in squares, the
    # quantity the fit minimises) than under the plain box-to-aligned-square scaling, a similarity too
    valid = (lm_np >= 0).all(-1)
    assert valid.mean() > 0.5
    mapped = np.einsum("nij,nkj->nki", m_np[:, :, :2].astype(np.float64), lm_np) + m_np[:, None, :, 2]
    before = (lm_np - boxes[:, None, :2]) * (112.0 / sides)[:, None, None]
    r_after = (((mapped - tm) ** 2).sum(-1) * valid).sum(1)
    r_before = (((before - tm) ** 2).sum(-1) * valid).sum(1)
    print("align_frames %s: squared residual per face after the fit %s, before %s" % (dtype, np.round(r_after, 2), np.round(r_before, 2)))
    assert (r_after <= r_before + 1e-3).all()
    # in-frame boxes: truncated to integers these are detect_marks_batch's marks (float32 there, float64 here: an
    # integer boundary may be stepped).  Same three faces as one batch on both sides: a face's bf16 landmarks depend
    # on the batch it sits in beyond four faces (tests/test_gpu_stream.py), and a top-4 pick on synthetic weights
    # moves by tens of pixels with them
    marks = P.detect_marks_batch(frames[1], model, faces[0], n_points=4)
    lm3 = P.align_frames(ring, faces[:1], model, out_size=(112, 112), frame_index=[1])[2].cpu().numpy()
    assert (lm3 >= 0).all()
    mine = np.maximum(lm3, 0).astype(np.int64)
    step = np.abs(marks.astype(np.int64) - mine)
    print("align_frames %s vs detect_marks_batch: %d of %d integer coordinates differ, max %d" % (dtype, int((step > 0).sum()), step.size, int(step.max())))
    assert step.max() <= 1
    # sample grids through the same entry point, and a list of frames stacked once
    a4 = P.align_frames([ring[0], ring[1]], faces, model, out_size=(112, 112), frame_index=slots, samples=4)
    assert torch.equal(a4[1], m) and torch.equal(a4[2], lm)
    assert torch.equal(a4[0], A.warp_frames_device(ring, m, 112, 112, frame_index_dev=idev, boxes_dev=bdev, samples=4))
    # no faces: shapes only, nothing launched
    e = P.align_frames(ring, [[], []], model, out_size=(96, 80))
    assert [tuple(t.shape) for t in e[:3]] == [(0, 96, 80, 3), (0, 2, 3), (0, 68, 2)] and all(t.is_cuda for t in e)
    with pytest.raises(ValueError):
        P.align_frames(ring, faces, model, frame_index=[0, 2])


# ---- 5. what the frame-space path is for ------------------------------------------------------------------------
def test_frame_space_alignment_sees_beyond_the_crop(mods):
    """A frame that is one colour inside the face box and another outside, an M rotated by 30 degrees: the corners of the
    aligned square map outside the box.  Warping the crop can only return the inside colour there (its edge clamp);
    warping the frame returns what the frame holds."""
    A, P = mods
    fh, fw, side, oh = 300, 400, 128, 112
    x0, y0 = 140, 90
    inside, outside = np.array([40, 90, 200], np.uint8), np.array([220, 30, 10], np.uint8)
    frame = np.broadcast_to(outside, (1, fh, fw, 3)).copy()
    frame[0, y0:y0 + side, x0:x0 + side] = inside
    box = np.array([[x0, y0, x0 + side, y0 + side]], np.int32)
    th = np.deg2rad(30.0)

    def rot_about(scale, cx, cy):      # source (cx, cy) -> aligned centre, scaled and rotated
        a, b = scale * np.cos(th), scale * np.sin(th)
        return np.array([[[a, -b, oh / 2 - (a * cx - b * cy)], [b, a, oh / 2 - (b * cx + a * cy)]]], f32)

    m_frame = rot_about(oh / side, x0 + side / 2, y0 + side / 2)
    m_crop = rot_about(oh / 256, 128.0, 128.0)                   # the same geometry in the 256x256 crop's pixels
    fd = dev(frame)
    crops = P.crop_faces_device(fd[0], None, 256, 256, boxes_dev=dev(box))
    crop_space = A.warp_device(crops, dev(m_crop), oh, oh).cpu().numpy()[0]
    assert np.abs(crop_space - inside.astype(f32)).max() <= 1.0  # (the fixed-point resize may round a level)
    got = A.warp_frames_device(fd, dev(m_frame), oh, oh, boxes_dev=dev(box)).cpu().numpy()
    exp = warp_frames_ref(frame, None, box, m_frame, oh, oh, 1)
    assert ulp_diff(got, exp).max() <= 1
    yd, xd = np.mgrid[0:oh, 0:oh]
    _, xs, ys = sample_ref(frame[0], inverse_ref(m_frame[0]), xd.astype(f32), yd.astype(f32))
    far_out = (xs < x0 - 1) | (xs > x0 + side) | (ys < y0 - 1) | (ys > y0 + side)      # both taps outside the box
    well_in = (xs > x0) & (xs < x0 + side - 2) & (ys > y0) & (ys < y0 + side - 2)
    assert far_out.sum() > 500 and well_in.sum() > 5000
    assert (got[0][far_out] == outside.astype(f32)).all()
    assert (got[0][well_in] == inside.astype(f32)).all()
    assert (got[0, 0, 0] == outside.astype(f32)).all() and (crop_space[0, 0] != outside.astype(f32)).all()
