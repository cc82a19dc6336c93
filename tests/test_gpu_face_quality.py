"""GPU parity of flm_face_quality against tests/face_quality_ref.py (the header's arithmetic in numpy: int64 sums, float32
operations one at a time): the record of every face, bit for bit, over the four pixel types x both layouts x both channel
orders x {the matcher's scale and bias, the identity}, over face sizes that hit one Laplacian pixel, no interior, no
multiple of the tile, more columns than a workgroup has threads and the matcher's own size, for 1, 3 and 17 faces, on
aligned buffers and on a slice that starts one element into a larger buffer (the path without 16-byte loads); then the
extremes (the 0 / 255 checkerboard, every kind of float bit pattern), the exposure levels, and every argument error."""
import ctypes as C

import numpy as np
import pytest
import torch

import aligned_format_ref as fref
import face_quality_ref as ref

pytestmark = pytest.mark.gpu
f32 = np.float32
SIZES = [(3, 3), (1, 5), (2, 7), (113, 37), (5, 300), (112, 112)]
KS = [1, 3, 17]
DTYPES = ["float32", "float16", "bfloat16", "uint8"]
MATCHER = ((1.0 / 127.5,) * 3, (-1.0,) * 3)
IDENTITY = ((1.0,) * 3, (0.0,) * 3)
UNEVEN = ((0.5, 2.0, -1.0), (3.0, -10.0, 255.0))     # per-channel values, a negative scale among them


@pytest.fixture(scope="module")
def mods():
    import flm_amd  # noqa: F401
    from flm_amd import _lib, alignment, prediction
    _lib.load()
    return _lib, alignment, prediction


@pytest.fixture(scope="module")
def images():
    """float32 BGR NHWC faces, 17 of every size, made once: noise over a gradient, so that the sums differ by face."""
    rng = np.random.default_rng(11)
    out = {}
    for h, w in SIZES:
        base = rng.uniform(0, 255, (17, h, w, 3))
        ramp = np.linspace(0.2, 1.0, 17)[:, None, None, None]
        out[(h, w)] = (base * ramp).astype(f32)
    return out


def upload(stored, dtype, offset=0):
    """The stored numpy faces as a CUDA tensor of their type; offset: that many elements into a larger buffer."""
    a = np.ascontiguousarray(stored)
    t = torch.from_numpy(a.view(np.int16) if dtype == "bfloat16" else a)
    if offset:
        buf = torch.empty(t.numel() + offset + 3, dtype=t.dtype).cuda()
        buf[offset:offset + t.numel()] = t.flatten().cuda()
        d = buf[offset:offset + t.numel()].view(t.shape)
        assert d.data_ptr() % 16 == offset * d.element_size() % 16
    else:
        d = t.cuda()
    return d.view(torch.bfloat16) if dtype == "bfloat16" else d


def same(got, exp):
    got = got.cpu().numpy()
    assert got.dtype == np.int64 and got.shape == exp.shape
    return np.array_equal(got, exp)


@pytest.mark.parametrize("layout", ["nhwc", "nchw"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_record_matches_the_reference(mods, images, dtype, layout):
    L, A, P = mods
    n = 0
    for channels in ("bgr", "rgb"):
        for scale, bias in (MATCHER, IDENTITY):
            fmt = A.AlignedFormat(layout, dtype, channels, scale, bias)
            for (h, w), img in images.items():
                stored = fref.convert(img, fmt)
                exp = ref.record(stored, fmt)
                assert exp[0, 3] == max(h - 2, 0) * max(w - 2, 0)
                for k in KS:
                    for offset in (0, 1):
                        got = A.face_quality_device(upload(stored[:k], dtype, offset), fmt)
                        assert same(got, exp[:k]), (fmt, h, w, k, offset, got.cpu().numpy(), exp[:k])
                        n += 1
    assert n == 2 * 2 * len(SIZES) * len(KS) * 2


def test_records_tell_faces_apart(images):
    """(the cases hold what they promise: every face of a size has its own record, and the sizes hit what they name)"""
    fmt = ("nhwc", "float32", "bgr") + IDENTITY
    for (h, w), img in images.items():
        rec = ref.record(img, fmt)
        assert len({tuple(r) for r in rec.tolist()}) == 17
    assert ref.record(images[(3, 3)], fmt)[0, 3] == 1
    assert ref.record(images[(1, 5)], fmt)[0, 3] == 0 and ref.record(images[(2, 7)], fmt)[0, 3] == 0
    assert 113 % 8 and 37 % 128 and 300 > 256


def test_uneven_scale_and_bias_per_channel(mods, images):
    L, A, P = mods
    for dtype in ("float32", "float16"):
        fmt = A.AlignedFormat("nchw", dtype, "rgb", *UNEVEN)
        stored = fref.convert(images[(113, 37)][:3], fmt)
        assert same(A.face_quality_device(upload(stored, dtype), fmt), ref.record(stored, fmt))


def test_checkerboard(mods):
    L, A, P = mods
    h, w = 112, 112
    yy, xx = np.mgrid[0:h, 0:w]
    a = np.where((yy + xx) % 2 == 0, 255, 0).astype(np.uint8)
    face = np.repeat(a[None, :, :, None], 3, axis=3)
    fmt = A.AlignedFormat("nhwc", "uint8")
    exp = ref.record(face, fmt)
    assert exp[0, 5] == 110 * 110 * (4 * 4080) ** 2 and exp[0, 4] == 0
    assert same(A.face_quality_device(upload(face, "uint8"), fmt), exp)
    rec, sc = P.face_quality(face, fmt)                                  # the numpy entry point
    assert isinstance(rec, np.ndarray) and np.array_equal(rec, exp) and sc[0, 0] == (4 * 255.0) ** 2


@pytest.mark.parametrize("dtype", ["float32", "float16", "bfloat16"])
def test_float_faces_of_any_bits(mods, dtype):
    """Random bit patterns: NaNs, both infinities, subnormals and values far outside [0, 255] among ordinary ones."""
    L, A, P = mods
    rng = np.random.default_rng(3)
    k, h, w = 3, 37, 53
    if dtype == "float32":
        raw = rng.integers(0, 2 ** 32, (k, h, w, 3), dtype=np.uint64).astype(np.uint32).view(f32)
        raw[0, :4, :4] = [np.nan, np.inf, -np.inf]
        raw[1, 5:9, 5:9] = [1e30, -1e30, 300.0]
    else:
        raw = rng.integers(0, 2 ** 16, (k, h, w, 3), dtype=np.uint64).astype(np.uint16)
        nan, inf, ninf = (0x7e00, 0x7c00, 0xfc00) if dtype == "float16" else (0x7fc0, 0x7f80, 0xff80)
        raw[0, :4, :4] = [nan, inf, ninf]
        if dtype == "float16":
            raw = raw.view(np.float16)
    # ordinary values too, so that not every pixel clamps
    plain = rng.uniform(0, 255, (h, w, 3)).astype(f32)
    if dtype == "bfloat16":
        raw[2] = fref.bf16_bits(plain)
    else:
        raw[2] = plain.astype(raw.dtype)
    xf = ref.to_f32(raw, dtype)
    assert np.isnan(xf).any() and np.isposinf(xf).any() and np.isneginf(xf).any() and (np.abs(xf[np.isfinite(xf)]) > 1e4).any()
    for layout in ("nhwc", "nchw"):
        stored = raw if layout == "nhwc" else np.ascontiguousarray(raw.transpose(0, 3, 1, 2))
        for scale, bias in (IDENTITY, MATCHER):
            fmt = A.AlignedFormat(layout, dtype, "bgr", scale, bias)
            exp = ref.record(stored, fmt)
            assert same(A.face_quality_device(upload(stored, dtype), fmt), exp), (fmt, exp)


def test_exposure_levels(mods, images):
    L, A, P = mods
    img = images[(113, 37)][:3]
    fmt = A.AlignedFormat("nhwc", "float32")
    seen = set()
    for dark, bright in ((16, 239), (0, 255), (255, 0), (100, 101), (60, 200)):
        exp = ref.record(img, fmt, dark, bright)
        got = A.face_quality_device(upload(img, "float32"), fmt, A.QualityOptions(dark, bright))
        assert same(got, exp), (dark, bright)
        seen.add((int(exp[2, 6]), int(exp[2, 7])))
    assert len(seen) == 5
    out = torch.full((3, 8), -7, dtype=torch.int64, device="cuda")
    assert A.face_quality_device(upload(img, "float32"), fmt, out=out) is out and same(out, ref.record(img, fmt))
    # the default format: None is float32 NHWC BGR
    assert same(A.face_quality_device(upload(img, "float32")), ref.record(img, fmt))
    rec, sc = P.face_quality(upload(img, "float32"))
    assert rec.is_cuda and sc.is_cuda and tuple(sc.shape) == (3, 4) and same(rec, ref.record(img, fmt))


def test_argument_errors(mods):
    L, A, P = mods
    lib = L.load()
    faces = torch.zeros((2, 8, 8, 3), dtype=torch.float32, device="cuda")
    rec = torch.full((2, 8), -7, dtype=torch.int64, device="cuda")

    def fmt_struct(**kw):
        f = L.ImageFormat()
        lib.flm_image_format_init(C.byref(f))
        for key, v in kw.items():
            if key in ("scale", "bias"):
                for c in range(3):
                    getattr(f, key)[c] = v[c]
            else:
                setattr(f, key, v)
        return f

    def call(faces_p=L.ptr(faces), k=2, h=8, w=8, fmt=None, opts=None, rec_p=L.ptr(rec)):
        rc = lib.flm_face_quality(L.stream_ptr(), faces_p, k, h, w, None if fmt is None else C.byref(fmt),
                                  None if opts is None else C.byref(opts), rec_p)
        return rc, lib.flm_last_error().decode()

    small = L.QualityOpts.make()
    small.struct_size = 4
    ARG, SHAPE = -1, -2
    for kw, code, word in [
            (dict(faces_p=None), ARG, "null"), (dict(rec_p=None), ARG, "null"),
            (dict(fmt=fmt_struct(struct_size=4)), ARG, "struct_size"), (dict(fmt=fmt_struct(layout=7)), ARG, "layout"),
            (dict(fmt=fmt_struct(type=9)), ARG, "pixel type"), (dict(fmt=fmt_struct(reverse_channels=3)), ARG, "reverse_channels"),
            (dict(fmt=fmt_struct(scale=(float("nan"), 1.0, 1.0))), ARG, "finite"),
            (dict(fmt=fmt_struct(scale=(1.0, 1.0, 0.0))), ARG, "scale != 0"),
            (dict(faces_p=C.c_void_p(faces.data_ptr() + 2)), ARG, "4-byte"),
            (dict(opts=L.QualityOpts.make(dark=256)), ARG, "[0, 255]"), (dict(opts=L.QualityOpts.make(bright=-1)), ARG, "[0, 255]"),
            (dict(opts=small), ARG, "struct_size"),
            (dict(k=0), SHAPE, "1 <= k <= 65535"), (dict(k=65536), SHAPE, "1 <= k <= 65535"),
            (dict(h=0), SHAPE, "h, w >= 1"), (dict(w=-1), SHAPE, "h, w >= 1"), (dict(h=13378, w=13378), SHAPE, "h*w*3*4 < 2^31")]:
        rc, msg = call(**kw)
        assert rc == code and word in msg, (kw, rc, msg)
    torch.cuda.synchronize()
    assert (rec == -7).all()                     # nothing was launched
    rc, msg = call()
    assert rc == 0
    assert rec.cpu().numpy()[:, 0].tolist() == [64, 64]
