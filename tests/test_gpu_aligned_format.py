"""GPU parity of the aligned-face formats: flm_warp_affine_fmt, flm_warp_affine_frames_fmt, and the `fmt=` /
`aligned_format=` arguments above them.

The yardstick is the EXISTING float32 call on the same inputs (tests/test_gpu_align.py and tests/test_gpu_frames.py pin
it to the oracle): the expected value is tests/aligned_format_ref.convert of its output, and the comparison is exact --
raw bits for the 8- and 16-bit types, np.array_equal for float32.  No tolerance, no excluded value: the inputs hold no
NaN, so the restatement leaves nothing undetermined.  Every destination sits between guard bytes that must survive.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import aligned_format_ref as ref
from oracle import warp_ref

pytestmark = pytest.mark.gpu
f32 = np.float32
GUARD = 256          # bytes on either side of a destination; keeps the destination's own 16-byte alignment
FILL = 0xA5


@pytest.fixture(scope="module")
def mods():
    import flm_amd  # noqa: F401
    from flm_amd import _lib, alignment, prediction
    _lib.load()
    return alignment, prediction


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def formats(A):
    """Every (layout, type, reverse) combination, 16 in all, with scale and bias that differ by channel so that a channel
    mix-up shows.  uint8: channel 1 halves (exact .5 ties on integer v: half-even against half-away), channel 2 reaches
    both clamps.  16-bit types twice: the matcher normalisation, and scale (1000, 1, 2^-22) -- 255000 overflows float16
    to inf, 255 * 2^-22 is a float16 subnormal."""
    out = []
    for layout in ("nhwc", "nchw"):
        for ch in ("bgr", "rgb"):
            out.append(A.AlignedFormat(layout, "float32", ch, (1.0 / 127.5, 0.5, 2.0), (-1.0, 0.25, -3.0)))
            out.append(A.AlignedFormat(layout, "uint8", ch, (1.0, 0.5, 1.5), (0.0, 0.0, -20.0)))
            for dt in ("float16", "bfloat16"):
                out.append(A.AlignedFormat(layout, dt, ch, (1.0 / 127.5,) * 3, (-1.0,) * 3))
                out.append(A.AlignedFormat(layout, dt, ch, (1000.0, 1.0, 2.0 ** -22), (0.0, -3.0, 0.0)))
    assert len({(f.layout, f.dtype, f.channels) for f in out}) == 16
    return out


def guarded(fmt, n, h, w, offset_elems=0):
    """(raw uint8 buffer, destination view, byte offset of the view): GUARD bytes of FILL before and after."""
    nbytes = fmt.nbytes(n, h, w)
    off = GUARD + offset_elems * fmt.itemsize
    raw = torch.full((off + nbytes + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    return raw, raw[off:off + nbytes].view(fmt.torch_dtype).view(fmt.shape(n, h, w)), off


def result_bits(t):
    """The bits of a result tensor as numpy: bfloat16 and float16 as uint16, float32 as float32, uint8 as it is."""
    t = t.contiguous()
    if t.dtype in (torch.float16, torch.bfloat16):
        return t.view(torch.int16).cpu().numpy().view(np.uint16)
    return t.cpu().numpy()


def check(fmt, raw, out, off, base_f32, what):
    """out (a view into raw at byte `off`) against convert(base), exactly; the bytes around it untouched."""
    exp = ref.convert(base_f32, fmt)
    got = result_bits(out)
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    if fmt.dtype == "float32":
        same = np.array_equal(got, exp)
    else:
        same = np.array_equal(got, ref.bits(exp))
    if not same:
        bad = np.argwhere(got != ref.bits(exp) if fmt.dtype != "float32" else got != exp)
        raise AssertionError("%s %r: %d of %d elements differ, first at %s: got %r, expected %r"
                             % (what, fmt, len(bad), got.size, bad[0], got[tuple(bad[0])], exp[tuple(bad[0])]))
    r = raw.cpu().numpy()
    nbytes = out.numel() * out.element_size()
    assert (r[:off] == FILL).all(), "%s %r: bytes BEFORE the destination were written" % (what, fmt)
    assert (r[off + nbytes:] == FILL).all(), "%s %r: bytes AFTER the destination were written" % (what, fmt)
    return exp


# ---- 1. frames call ---------------------------------------------------------------------------------------------------
FH, FW = 135, 240


@pytest.fixture(scope="module")
def ring():
    """A 2 x 135 x 240 ring and six faces: rotation with scale; a translation whose samples leave the frame (edge
    clamp); a mirrored 3x shrink (negative determinant); a pure integer translation (v is an exact uint8 value); a slot
    outside the ring and a box that is empty after clipping (both zero faces)."""
    rng = np.random.default_rng(20261017)
    frames = rng.integers(0, 256, (2, FH, FW, 3), dtype=np.uint8)
    a, b = 0.6 * np.cos(0.5), 0.6 * np.sin(0.5)
    cx, cy = 120.0, 67.0
    m = np.array([[[a, -b, 40 - (a * cx - b * cy)], [b, a, 30 - (b * cx + a * cy)]],
                  [[1, 0, 40], [0, 1, 30]],
                  [[1 / 3, 0, 0], [0, -1 / 3, 45]],
                  [[1, 0, -7], [0, 1, -5]],
                  [[1, 0, 0], [0, 1, 0]],
                  [[0.8, 0, 3], [0, 0.8, 2]]], f32)
    assert np.linalg.det(m[2, :, :2].astype(np.float64)) < 0
    idx = np.array([0, 1, 1, 0, 5, 1], np.int32)
    boxes = np.array([[60, 20, 180, 120], [0, 0, 120, 135], [0, 0, 240, 135], [7, 5, 119, 117],
                      [10, 10, 90, 90], [300, 10, 340, 50]], np.int32)
    return frames, m, idx, boxes


_BASE = {}


def frames_base(A, ring, hd, wd, s):
    """The existing float32 call, once per (size, samples), shared by every format."""
    key = (hd, wd, s)
    if key not in _BASE:
        frames, m, idx, boxes = ring
        t = A.warp_frames_device(dev(frames), dev(m), hd, wd, frame_index_dev=dev(idx), boxes_dev=dev(boxes), samples=s)
        _BASE[key] = t.cpu().numpy()
        _BASE[key].setflags(write=False)
    return _BASE[key]


@pytest.mark.parametrize("hd,wd,s", [(112, 112, 1), (33, 47, 1), (33, 47, 2), (33, 47, 4), (8, 8, 1), (5, 3, 1)])
def test_frames_call_every_format(mods, ring, hd, wd, s):
    """112x112: whole waves, aligned planes; 33x47 = 1551 pixels: a ragged tail, faces and planes that are only
    element-aligned, a pixel count that is no multiple of 4; 8x8: exactly one wave; 5x3: less than one."""
    A, _ = mods
    frames, m, idx, boxes = ring
    base = frames_base(A, ring, hd, wd, s)
    assert not base[4].any() and not base[5].any() and base[0].any()          # the two zero faces are in the data
    if s == 1 and hd >= 8:
        assert np.array_equal(base[3], frames[0, 5:5 + hd, 7:7 + wd].astype(f32))   # the integer translation is exact
    fd, md, idd, bd = dev(frames), dev(m), dev(idx), dev(boxes)
    k = m.shape[0]
    seen = {"tie": 0, "lo": 0, "hi": 0, "inf": 0, "sub": 0}
    for fmt in formats(A):
        raw, out, off = guarded(fmt, k, hd, wd)
        r = A.warp_frames_device(fd, md, hd, wd, frame_index_dev=idd, boxes_dev=bd, samples=s, out=out, fmt=fmt)
        assert r.data_ptr() == out.data_ptr() and r.dtype == fmt.torch_dtype and tuple(r.shape) == fmt.shape(k, hd, wd)
        exp = check(fmt, raw, out, off, base, "frames %dx%d samples=%d" % (hd, wd, s))
        # the edge cases the formats were chosen for are really in the data
        if fmt.dtype == "uint8" and fmt.layout == "nhwc" and fmt.channels == "bgr":
            u1 = base[3, ..., 1].astype(np.float64) * 0.5
            seen["tie"] += int(((u1 % 1.0) == 0.5).sum())
            u2 = (base[..., 2] * f32(1.5)).astype(f32) + f32(-20.0)
            seen["lo"] += int((u2 < -0.5).sum())
            seen["hi"] += int((u2 > 255.5).sum())
            if s == 1 and hd >= 8:      # ties where half-even and half-away part: 0.5 -> 0, 2.5 -> 2
                ties = (u1 % 1.0) == 0.5
                assert (np.rint(u1[ties]) != np.floor(u1[ties] + 0.5)).any()
                assert np.array_equal(exp[3, ..., 1][ties], np.rint(u1[ties]).astype(np.uint8))
        if fmt.dtype == "float16" and fmt.scale[0] == 1000.0 and fmt.layout == "nhwc":
            seen["inf"] += int(np.isinf(exp).sum())
            tiny = np.abs(exp.astype(np.float64))
            seen["sub"] += int(((tiny > 0) & (tiny < 2.0 ** -14)).sum())
    if hd * wd >= 64:
        assert seen["lo"] > 0 and seen["hi"] > 0, seen
        assert seen["inf"] > 0 and seen["sub"] > 0, seen
        if s == 1:
            assert seen["tie"] > 0, seen


# ---- 2. crop call -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("u8", [True, False])
@pytest.mark.parametrize("hd,wd", [(64, 64), (33, 47), (7, 9)])
def test_crop_call_every_format(mods, u8, hd, wd):
    """uint8 and float32 sources [3,40,56,3] (the float32 one with negative values and values near 1e5); 64x64 is the
    domain of the float32 call's row kernel (wd % 64 == 0), which the formatted call must match all the same."""
    A, _ = mods
    rng = np.random.default_rng(1000 * hd + wd + int(u8))
    n, hs, ws = 3, 40, 56
    src = rng.integers(0, 256, (n, hs, ws, 3), dtype=np.uint8)
    if not u8:
        src = ((src.astype(f32) - f32(100.0)) * f32(640.0)).astype(f32)
        assert src.min() < -6e4 and src.max() > 9.9e4
    a, b = 1.3 * np.cos(-0.4), 1.3 * np.sin(-0.4)
    m = np.array([[[a, -b, 5], [b, a, 12]],
                  [[1, 0, 20], [0, 1, -15]],                         # samples leave the crop on two sides
                  [[wd / ws, 0, 0], [0, hd / hs, 0]]], f32)
    sd, md = dev(src), dev(m)
    base = A.warp_device(sd, md, hd, wd).cpu().numpy()
    for fmt in formats(A):
        raw, out, off = guarded(fmt, n, hd, wd)
        r = A.warp_device(sd, md, hd, wd, out=out, fmt=fmt)
        assert r.data_ptr() == out.data_ptr()
        check(fmt, raw, out, off, base, "crop u8=%s %dx%d" % (u8, hd, wd))
    # a new destination when none is given
    fmt = A.AlignedFormat.matcher("bfloat16")
    got = A.warp_device(sd, md, hd, wd, fmt=fmt)
    assert got.dtype == torch.bfloat16 and tuple(got.shape) == (n, 3, hd, wd) and got.is_cuda
    assert np.array_equal(result_bits(got), ref.convert(base, fmt))


def test_crop_single_column_source(mods):
    """A uint8 source one column wide has no pixel pair to read: the channel-by-channel path, same contract."""
    A, _ = mods
    rng = np.random.default_rng(5)
    src = rng.integers(0, 256, (2, 9, 1, 3), dtype=np.uint8)
    m = np.array([[[1, 0, 2], [0, 0.7, 0.5]], [[0.5, 0, 0], [0, 1.5, -2]]], f32)
    base = A.warp_device(dev(src), dev(m), 10, 13).cpu().numpy()
    for fmt in (A.AlignedFormat.matcher("float16"), A.AlignedFormat("nhwc", "uint8", "rgb", (1, 0.5, 1.5), (0, 0, -20))):
        raw, out, off = guarded(fmt, 2, 10, 13)
        A.warp_device(dev(src), dev(m), 10, 13, out=out, fmt=fmt)
        check(fmt, raw, out, off, base, "one-column crop")


# ---- 3. sliced destination --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout,dtype", [("nhwc", "uint8"), ("nchw", "float16")])
def test_sliced_destination(mods, ring, layout, dtype):
    """The destination starts ONE ELEMENT into a larger buffer: 112x112 would take 16-byte stores by its size, the
    address says otherwise.  Exact result, and the element before and the bytes after are untouched."""
    A, _ = mods
    frames, m, idx, boxes = ring
    hd = wd = 112
    base = frames_base(A, ring, hd, wd, 1)
    fmt = (A.AlignedFormat(layout, dtype, "rgb", (1.0, 0.5, 1.5), (0.0, 0.0, -20.0)) if dtype == "uint8"
           else A.AlignedFormat.matcher(dtype))
    raw, out, off = guarded(fmt, m.shape[0], hd, wd, offset_elems=1)
    assert out.data_ptr() % 16 == fmt.itemsize and out.is_contiguous()
    A.warp_frames_device(dev(frames), dev(m), hd, wd, frame_index_dev=dev(idx), boxes_dev=dev(boxes), out=out, fmt=fmt)
    check(fmt, raw, out, off, base, "sliced frames")
    # the crop call into the same kind of view
    src = frames[:, :40, :56].copy()
    mc = m[[0, 3]].copy()
    basec = A.warp_device(dev(src), dev(mc), hd, wd).cpu().numpy()
    raw, out, off = guarded(fmt, 2, hd, wd, offset_elems=1)
    A.warp_device(dev(src), dev(mc), hd, wd, out=out, fmt=fmt)
    check(fmt, raw, out, off, basec, "sliced crop")


# ---- 4. identity format -----------------------------------------------------------------------------------------------
def ulp_diff(a, b):
    ai = a.view(np.int32).astype(np.int64)
    bi = b.view(np.int32).astype(np.int64)
    ai = np.where(ai < 0, -(ai & 0x7fffffff), ai)
    bi = np.where(bi < 0, -(bi & 0x7fffffff), bi)
    return np.abs(ai - bi)


def test_identity_format_is_the_existing_call(mods, ring, golden_dir):
    """flm_image_format_init's defaults (float32, NHWC, BGR, scale 1, bias 0): the values of the existing calls, and on
    the scikit-image golden set the bars tests/test_gpu_align.py holds the existing call to."""
    A, _ = mods
    from flm_amd import _lib
    lib = _lib.load()
    cf = _lib.ImageFormat()
    lib.flm_image_format_init(C.byref(cf))
    assert A.AlignedFormat().struct().struct_size == cf.struct_size
    gold = np.load(os.path.join(golden_dir, "warp_golden.npz"))
    imgs = gold["imgs"]
    mg = np.ascontiguousarray(gold["mats"][:, :2, :].astype(f32))
    sd, md = dev(imgs), dev(mg)
    n, hs, ws = imgs.shape[:3]
    out = torch.empty((n, 40, 44, 3), dtype=torch.float32, device="cuda")
    _lib.check(lib.flm_warp_affine_fmt(_lib.stream_ptr(), _lib.ptr(sd), int(imgs.dtype == np.uint8), n, hs, ws,
                                       _lib.ptr(md), _lib.ptr(out), 40, 44, C.byref(cf)), "flm_warp_affine_fmt")
    got = out.cpu().numpy()
    assert np.array_equal(got, A.warp_device(sd, md, 40, 44).cpu().numpy())
    assert np.array_equal(got, A.warp_device(sd, md, 40, 44, fmt=A.AlignedFormat()).cpu().numpy())
    u = ulp_diff(got, warp_ref.warp_affine_ref(imgs, mg, 40, 44))
    d = np.abs(got - gold["warped"]).max()
    print("identity format on the golden set: max %d ULP from the restatement, %.3g grey levels from scikit-image" % (int(u.max()), d))
    assert u.max() <= 1
    assert d < 2 * 255 * 1.2e-5                      # the bound of test_warp_vs_skimage_golden, derived there
    # the frames call, every sample count, zero faces included
    frames, m, idx, boxes = ring
    for hd, wd, s in ((112, 112, 1), (33, 47, 1), (33, 47, 2), (33, 47, 4)):
        g = A.warp_frames_device(dev(frames), dev(m), hd, wd, frame_index_dev=dev(idx), boxes_dev=dev(boxes), samples=s,
                                 fmt=A.AlignedFormat())
        assert g.dtype == torch.float32 and np.array_equal(g.cpu().numpy(), frames_base(A, ring, hd, wd, s)), (hd, wd, s)
    # float32 crops too
    srcf = (imgs.astype(f32) - f32(31.5)) * f32(3.25)
    assert np.array_equal(A.warp_device(dev(srcf), md, 33, 47, fmt=A.AlignedFormat()).cpu().numpy(),
                          A.warp_device(dev(srcf), md, 33, 47).cpu().numpy())


# ---- 5. end to end ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_model():
    from flm_amd.networks import LANDMARKS_MODELS
    from flm_amd.weights import synth_fcn8_weights
    model = LANDMARKS_MODELS["fcn_8"](68, input_height=64, input_width=96, dtype="bf16")
    model.load_weights(synth_fcn8_weights(68, seed=2))
    return model


@pytest.mark.parametrize("weights", [None, "score"])
def test_end_to_end(mods, ring, small_model, weights):
    A, P = mods
    frames = ring[0]
    faces = [[[20, 10, 110, 100], [130, 30, 230, 125]], [[60, 20, 150, 120]]]
    fd = dev(frames)
    fmt = A.AlignedFormat.matcher("float16")
    plain = P.align_frames(fd, faces, small_model, out_size=(112, 112), weights=weights)
    formed = P.align_frames(fd, faces, small_model, out_size=(112, 112), weights=weights, aligned_format=fmt)
    assert len(plain) == len(formed) == (4 if weights is None else 5)
    assert formed[0].dtype == torch.float16 and tuple(formed[0].shape) == (3, 3, 112, 112) and formed[0].is_cuda
    assert np.array_equal(result_bits(formed[0]), ref.bits(ref.convert(plain[0].cpu().numpy(), fmt)))
    for a, b in zip(plain[1:], formed[1:]):          # M, landmarks, boxes (, weights): bit for bit
        assert a.dtype == b.dtype and torch.equal(a, b)
    assert plain[0].abs().max() > 0
    # no faces: an empty tensor of the format's dtype and shape
    e = P.align_frames(fd, [[], []], small_model, out_size=(96, 80), weights=weights, aligned_format=fmt)
    assert tuple(e[0].shape) == (0, 3, 96, 80) and e[0].dtype == torch.float16 and e[0].is_cuda
    # prediction.align, numpy in and numpy out
    crops = P.crop_frames_device(fd, faces, 64, 96)[0].cpu().numpy()
    p0 = P.align(crops, small_model, out_size=(112, 112), weights=weights)
    for f in (fmt, A.AlignedFormat("nhwc", "uint8", "rgb")):
        p1 = P.align(crops, small_model, out_size=(112, 112), weights=weights, aligned_format=f)
        assert len(p0) == len(p1) and all(isinstance(x, np.ndarray) for x in p1)
        assert p1[0].dtype == f.numpy_dtype and p1[0].shape == f.shape(3, 112, 112)
        assert np.array_equal(ref.bits(p1[0]), ref.bits(ref.convert(p0[0], f)))
        for a, b in zip(p0[1:], p1[1:]):
            assert a.dtype == b.dtype and np.array_equal(a, b)
    with pytest.raises(ValueError):
        P.align(crops, small_model, aligned_format=A.AlignedFormat.matcher("bfloat16"))
    # tensors in: bfloat16 comes back as a tensor
    t = P.align(dev(crops), small_model, out_size=(112, 112), weights=weights, aligned_format=A.AlignedFormat.matcher("bfloat16"))
    assert t[0].dtype == torch.bfloat16 and np.array_equal(result_bits(t[0]), ref.convert(p0[0], A.AlignedFormat.matcher("bfloat16")))
