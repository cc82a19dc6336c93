"""CPU-side checks of the aligned-face formats (flm_image_format, flm_warp_affine_fmt, flm_warp_affine_frames_fmt,
alignment.AlignedFormat, the `fmt=` / `aligned_format=` arguments): the defaults, the size query, every argument check
(each answers before any launch, so without a GPU), the Python validation, that `None` still reaches the old symbols, the
numpy restatement against torch's own conversions, and the build hygiene of csrc/flm_warp_fmt.hip."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import flm_amd  # noqa: F401
from flm_amd import _lib, alignment, prediction
from flm_amd.alignment import AlignedFormat

import aligned_format_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "face-landmark-detector_amd", "csrc")
P = C.c_void_p(0x1000)        # never dereferenced: every call below is rejected before a launch
FULL = 1080 * 1920 * 3


def err():
    return _lib.load().flm_last_error().decode()


def fresh(**kw):
    f = _lib.ImageFormat()
    _lib.load().flm_image_format_init(C.byref(f))
    for k, v in kw.items():
        if k in ("scale", "bias"):
            for c in range(3):
                getattr(f, k)[c] = v[c]
        else:
            setattr(f, k, v)
    return f


def crop_call(fmt, src=P, m=P, dst=P, n=1, hs=40, ws=56, hd=112, wd=112, u8=1):
    return _lib.load().flm_warp_affine_fmt(None, src, u8, n, hs, ws, m, dst, hd, wd, None if fmt is None else C.byref(fmt))


def frames_call(fmt, frames=P, m=P, dst=P, stride=FULL, nf=8, fh=1080, fw=1920, k=1, hd=112, wd=112, samples=1):
    return _lib.load().flm_warp_affine_frames_fmt(None, frames, stride, nf, fh, fw, None, None, m, k, dst, hd, wd, samples,
                                                 None if fmt is None else C.byref(fmt))


# ---- the C ABI ----------------------------------------------------------------------------------------------------------
def test_exports_and_init_defaults():
    lib = C.CDLL(_lib.LIB_PATH)
    for name in ("flm_image_format_init", "flm_image_format_bytes", "flm_warp_affine_fmt", "flm_warp_affine_frames_fmt"):
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTS
    assert _lib.load().flm_abi_version() == 2          # purely additive
    f = fresh()
    assert f.struct_size == C.sizeof(_lib.ImageFormat) == 40
    assert (f.layout, f.type, f.reverse_channels) == (_lib.LAYOUT_NHWC, _lib.PIX_F32, 0)
    assert list(f.scale) == [1.0, 1.0, 1.0] and list(f.bias) == [0.0, 0.0, 0.0]
    assert (_lib.LAYOUT_NHWC, _lib.LAYOUT_NCHW) == (0, 1)
    assert (_lib.PIX_F32, _lib.PIX_F16, _lib.PIX_BF16, _lib.PIX_U8) == (0, 1, 2, 3)
    hdr = open(os.path.join(ROOT, "include", "flm.h")).read()
    assert "FLM_LAYOUT_NHWC = 0, FLM_LAYOUT_NCHW = 1" in hdr
    assert "FLM_PIX_F32 = 0, FLM_PIX_F16 = 1, FLM_PIX_BF16 = 2, FLM_PIX_U8 = 3" in hdr


def test_format_bytes():
    lib = _lib.load()
    for layout in (0, 1):
        for t, es in ((_lib.PIX_F32, 4), (_lib.PIX_F16, 2), (_lib.PIX_BF16, 2), (_lib.PIX_U8, 1)):
            assert lib.flm_image_format_bytes(C.byref(fresh(layout=layout, type=t)), 505, 112, 112) == 505 * 112 * 112 * 3 * es
            assert lib.flm_image_format_bytes(C.byref(fresh(layout=layout, type=t)), 3, 33, 47) == 3 * 33 * 47 * 3 * es
    assert lib.flm_image_format_bytes(C.byref(fresh(type=_lib.PIX_F32)), 65535, 4096, 4096) == 65535 * 4096 * 4096 * 12  # 64-bit
    assert lib.flm_image_format_bytes(None, 1, 8, 8) == 0
    bad = [fresh(layout=2), fresh(layout=-1), fresh(type=4), fresh(type=-1), fresh(reverse_channels=2),
           fresh(reverse_channels=-1), fresh(scale=(1, float("nan"), 1)), fresh(scale=(float("inf"), 1, 1)),
           fresh(bias=(0, 0, float("-inf"))), fresh(bias=(float("nan"), 0, 0)), fresh(struct_size=39), fresh(struct_size=0)]
    for f in bad:
        assert lib.flm_image_format_bytes(C.byref(f), 1, 8, 8) == 0
    for n, h, w in ((0, 8, 8), (1, 0, 8), (1, 8, 0), (-1, 8, 8)):
        assert lib.flm_image_format_bytes(C.byref(fresh()), n, h, w) == 0
    # a larger struct_size (a newer caller) is fine, as with flm_forward_opts
    assert lib.flm_image_format_bytes(C.byref(fresh(struct_size=64)), 1, 8, 8) == 8 * 8 * 3 * 4


def test_argument_checks_answer_without_a_gpu():
    ok = fresh(layout=_lib.LAYOUT_NCHW, type=_lib.PIX_F16, reverse_channels=1)
    for call in (crop_call, frames_call):
        # null pointers, null format -> FLM_ERR_ARG
        assert call(None) == -1 and "format" in err()
        for kw in ({"m": None}, {"dst": None}, {"src": None} if call is crop_call else {"frames": None}):
            assert call(ok, **kw) == -1, kw
            assert "null" in err()
        # the format itself
        assert call(fresh(layout=2)) == -1 and "layout" in err()
        assert call(fresh(layout=-1)) == -1 and "layout" in err()
        assert call(fresh(type=4)) == -1 and "type" in err()
        assert call(fresh(type=-3)) == -1 and "type" in err()
        assert call(fresh(reverse_channels=2)) == -1 and "reverse_channels" in err()
        assert call(fresh(reverse_channels=-1)) == -1 and "reverse_channels" in err()
        for kw in ({"scale": (1, float("nan"), 1)}, {"scale": (float("inf"), 1, 1)}, {"bias": (0, 0, float("-inf"))},
                   {"bias": (float("nan"), 0, 0)}):
            assert call(fresh(**kw)) == -1, kw
            assert "finite" in err()
        assert call(fresh(struct_size=39)) == -1 and "struct_size" in err()
        assert call(fresh(struct_size=0)) == -1 and "struct_size" in err()
        # a destination that is not aligned to its element
        assert call(fresh(type=_lib.PIX_F16), dst=C.c_void_p(0x1001)) == -1 and "aligned" in err()
        assert call(fresh(type=_lib.PIX_F32), dst=C.c_void_p(0x1002)) == -1 and "aligned" in err()
        # the aligned-size limit counts float32 bytes whatever the type
        for t in (_lib.PIX_F32, _lib.PIX_U8):
            assert call(fresh(type=t), hd=16384, wd=16384) == -2 and "hd*wd*3*4 < 2^31" in err()
        assert call(ok, hd=0) == -2 and "hd, wd >= 1" in err()
        assert call(ok, wd=-4) == -2 and "hd, wd >= 1" in err()
    # the crop call's own limits
    assert crop_call(ok, n=0) == -2 and "1 <= n <= 65535" in err()
    assert crop_call(ok, n=65536) == -2 and "1 <= n <= 65535" in err()
    assert crop_call(ok, hs=0) == -2 and "hs, ws >= 1" in err()
    assert crop_call(ok, hs=16384, ws=16384) == -2 and "hs*ws*3*4 < 2^31" in err()
    # the frames call's own limits: those of flm_warp_affine_frames
    assert frames_call(ok, k=0) == -2 and "1 <= k <= 65535" in err()
    assert frames_call(ok, k=65536) == -2 and "1 <= k <= 65535" in err()
    assert frames_call(ok, stride=1080 * 3, fw=1) == -2 and "fw >= 2" in err()
    assert frames_call(ok, stride=FULL - 1) == -2 and "frame_stride >= fh*fw*3" in err()
    assert frames_call(ok, stride=1 << 32, nf=1, fh=32768, fw=21846) == -2 and "fh*fw*3 < 2^31" in err()
    assert frames_call(ok, nf=0) == -2 and "nframes >= 1" in err()
    for s in (3, 0, 8, -1):
        assert frames_call(ok, samples=s) == -1, s
        assert "samples" in err()


# ---- AlignedFormat ------------------------------------------------------------------------------------------------------
def test_aligned_format_object():
    f = AlignedFormat()
    assert (f.layout, f.dtype, f.channels, f.scale, f.bias) == ("nhwc", "float32", "bgr", (1.0, 1.0, 1.0), (0.0, 0.0, 0.0))
    assert f.torch_dtype == torch.float32 and f.numpy_dtype == np.float32 and f.shape(5, 7, 9) == (5, 7, 9, 3)
    s, init = f.struct(), fresh()
    assert bytes(s) == bytes(init)                                    # what flm_image_format_init gives
    m = AlignedFormat.matcher()
    assert (m.layout, m.dtype, m.channels) == ("nchw", "float16", "rgb")
    assert m.scale == (1 / 127.5,) * 3 and m.bias == (-1.0,) * 3
    assert m.torch_dtype == torch.float16 and m.shape(505, 112, 112) == (505, 3, 112, 112) and m.nbytes(505, 112, 112) == 505 * 3 * 112 * 112 * 2
    ms = m.struct()
    assert (ms.layout, ms.type, ms.reverse_channels) == (1, 1, 1)
    assert list(ms.scale) == [np.float32(1 / 127.5)] * 3 and list(ms.bias) == [-1.0] * 3
    assert _lib.load().flm_image_format_bytes(C.byref(ms), 505, 112, 112) == m.nbytes(505, 112, 112)
    b = AlignedFormat.matcher("bfloat16")
    assert b.torch_dtype == torch.bfloat16 and b.numpy_dtype is None and b.struct().type == _lib.PIX_BF16
    assert AlignedFormat("NCHW", torch.uint8, "RGB").key() == AlignedFormat("nchw", "uint8", "rgb").key()
    assert AlignedFormat(dtype=np.float16).dtype == "float16" and AlignedFormat(dtype=torch.bfloat16).dtype == "bfloat16"
    assert AlignedFormat(scale=2, bias=-1).scale == (2.0, 2.0, 2.0)
    assert AlignedFormat("nchw", "uint8") == AlignedFormat("nchw", "uint8") != AlignedFormat("nhwc", "uint8")
    assert "nchw" in repr(m) and "float16" in repr(m)
    for kw in ({"layout": "chwn"}, {"layout": 1}, {"dtype": "float64"}, {"dtype": "int8"}, {"dtype": torch.int32},
               {"channels": "gbr"}, {"channels": None}, {"scale": (1, 1)}, {"bias": (0, 0, 0, 0)}, {"scale": "abc"},
               {"scale": (1, float("nan"), 1)}, {"bias": (0, float("inf"), 0)}, {"scale": (1e39, 1, 1)}, {"scale": None}):
        with pytest.raises(ValueError):
            AlignedFormat(**kw)
    with pytest.raises(ValueError):
        AlignedFormat.matcher("int8")


def test_wrappers_reject_bad_arguments_on_the_host():
    src = torch.zeros((2, 16, 20, 3), dtype=torch.uint8)
    m = torch.zeros((2, 2, 3), dtype=torch.float32)
    fmt = AlignedFormat.matcher()
    for bad in ("nchw", 1, {"layout": "nchw"}):
        with pytest.raises(ValueError, match="AlignedFormat"):
            alignment.warp_device(src, m, 8, 8, fmt=bad)
        with pytest.raises(ValueError, match="AlignedFormat"):
            alignment.warp_frames_device(src, m, 8, 8, fmt=bad)
        with pytest.raises(ValueError, match="AlignedFormat"):
            alignment.align_device(src, None, None, 8, 8, fmt=bad)
        with pytest.raises(ValueError, match="AlignedFormat"):
            prediction.align(np.zeros((2, 16, 20, 3), np.uint8), landmarks=np.zeros((2, 68, 2)), aligned_format=bad)
        with pytest.raises(ValueError, match="AlignedFormat"):
            prediction.align_frames(src, [[], []], None, aligned_format=bad)
    # out= against the format's dtype and shape
    with pytest.raises(ValueError, match="out must be a float16"):        # the float32 NHWC tensor of the plain call
        alignment.warp_device(src, m, 8, 8, out=torch.empty((2, 8, 8, 3), dtype=torch.float32), fmt=fmt)
    with pytest.raises(ValueError, match="out must be a float16"):        # right type, NHWC shape
        alignment.warp_device(src, m, 8, 8, out=torch.empty((2, 8, 8, 3), dtype=torch.float16), fmt=fmt)
    with pytest.raises(ValueError, match="out must be a float16"):
        alignment.warp_device(src, m, 8, 8, out=torch.empty((2, 3, 8, 9), dtype=torch.float16), fmt=fmt)
    with pytest.raises(ValueError, match="out must be a float16"):
        alignment.warp_device(src, m, 8, 8, out=np.empty((2, 3, 8, 8), np.float16), fmt=fmt)
    with pytest.raises(ValueError, match="CUDA"):                        # right in every way but on the host
        alignment.warp_device(src, m, 8, 8, out=torch.empty((2, 3, 8, 8), dtype=torch.float16), fmt=fmt)
    with pytest.raises(ValueError):
        alignment._format_out(AlignedFormat("nhwc", "uint8"), torch.empty((2, 8, 8, 3), dtype=torch.int8), 2, 8, 8, "cpu")
    # numpy has no bfloat16: said before any device work
    with pytest.raises(ValueError, match="bfloat16"):
        prediction.align(np.zeros((2, 16, 20, 3), np.uint8), landmarks=np.zeros((2, 68, 2)),
                         aligned_format=AlignedFormat.matcher("bfloat16"))


# ---- None reaches the old symbols -----------------------------------------------------------------------------------------
class _OnDevice(torch.Tensor):
    """A host tensor that answers is_cuda = True, so the wrappers' checks pass and the stubbed library is reached."""
    is_cuda = property(lambda self: True)


class _StubLib:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("flm_"):
            raise AttributeError(name)

        def call(*args):
            self.calls.append((name, len(args)))
            return 0
        return call


def test_no_format_reaches_the_old_symbols(monkeypatch):
    stub = _StubLib()
    monkeypatch.setattr(_lib, "load", lambda: stub)
    monkeypatch.setattr(_lib, "stream_ptr", lambda: None)
    frames = torch.zeros((2, 16, 20, 3), dtype=torch.uint8).as_subclass(_OnDevice)
    m = torch.zeros((3, 2, 3), dtype=torch.float32).as_subclass(_OnDevice)
    out = alignment.warp_frames_device(frames, m, 8, 8)
    assert stub.calls == [("flm_warp_affine_frames", 14)] and out.dtype == torch.float32 and tuple(out.shape) == (3, 8, 8, 3)
    alignment.warp_frames_device(frames, m, 8, 8, fmt=None, samples=2)
    assert stub.calls[-1] == ("flm_warp_affine_frames", 14)
    src = torch.zeros((3, 16, 20, 3), dtype=torch.uint8)
    alignment.warp_device(src, m, 8, 8)
    assert stub.calls[-1] == ("flm_warp_affine", 10)
    alignment.warp_device(src, m, 8, 8, fmt=None)
    assert stub.calls[-1] == ("flm_warp_affine", 10)
    lm = torch.zeros((3, 68, 2), dtype=torch.float64)
    tm = torch.zeros((68, 2), dtype=torch.float64)
    alignment.align_device(src, lm, tm, 8, 8)
    assert [c[0] for c in stub.calls[-2:]] == ["flm_similarity_from_landmarks_scaled", "flm_warp_affine"]
    # and with a format, the new ones: one more argument
    fmt = AlignedFormat.matcher()
    out = alignment.warp_frames_device(frames, m, 8, 8, fmt=fmt)
    assert stub.calls[-1] == ("flm_warp_affine_frames_fmt", 15) and out.dtype == torch.float16 and tuple(out.shape) == (3, 3, 8, 8)
    out = alignment.warp_device(src, m, 8, 8, fmt=fmt)
    assert stub.calls[-1] == ("flm_warp_affine_fmt", 11) and out.dtype == torch.float16 and tuple(out.shape) == (3, 3, 8, 8)
    # the entry points hand the argument down unchanged
    seen = []
    monkeypatch.setattr(_lib, "require_gpu", lambda: torch.device("cpu"))
    monkeypatch.setattr(alignment, "align_device",
                        lambda *a, **kw: (seen.append(kw.get("fmt", "absent")), (torch.zeros(1), torch.zeros(1)))[1])
    crops = np.zeros((3, 16, 20, 3), np.uint8)
    prediction.align(crops, landmarks=np.zeros((3, 68, 2)))
    prediction.align(crops, landmarks=np.zeros((3, 68, 2)), aligned_format=fmt)
    assert seen == [None, fmt]


# ---- the restatement itself ------------------------------------------------------------------------------------------------
def test_numpy_restatement_matches_torch_conversions():
    rng = np.random.default_rng(3)
    u = np.concatenate([rng.normal(0, 1, 4000), rng.normal(0, 1e-6, 2000), rng.uniform(-70000, 70000, 2000),
                        np.array([0.5, 1.5, 2.5, -0.5, 254.5, 255.5, 65504, 65520, 65519.99, 2.0 ** -24, 2.0 ** -25, 6.0e-8])]).astype(np.float32)
    assert np.array_equal(ref.bf16_bits(u), torch.from_numpy(u).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16))
    with np.errstate(over="ignore"):
        assert np.array_equal(u.astype(np.float16).view(np.uint16),
                              torch.from_numpy(u).to(torch.float16).view(torch.int16).numpy().view(np.uint16))
    assert np.rint(np.float32([0.5, 1.5, 2.5, 3.5])).tolist() == [0, 2, 2, 4]
    v = rng.integers(0, 256, (2, 5, 7, 3)).astype(np.float32)
    fmt = AlignedFormat("nchw", "uint8", "rgb", (1, 0.5, 1.5), (0, 0, -20))
    e = ref.convert(v, fmt)
    assert e.shape == (2, 3, 5, 7) and e.dtype == np.uint8
    assert e[1, 0, 2, 3] == v[1, 2, 3, 2]                                        # output channel 0 = source channel 2
    assert e[0, 2, 4, 6] == np.clip(np.rint(v[0, 4, 6, 0] * 1.5 - 20), 0, 255)   # output channel 2 = source 0, clamped
    assert np.array_equal(ref.convert(v, AlignedFormat()), v)
    t = torch.from_numpy(v)
    chain = t.permute(0, 3, 1, 2).flip(1).mul(np.float32(1 / 127.5)).add(-1.0).to(torch.float16)
    assert np.array_equal(ref.bits(ref.convert(v, AlignedFormat.matcher())), chain.contiguous().view(torch.int16).numpy().view(np.uint16))


# ---- build hygiene -----------------------------------------------------------------------------------------------------
def test_warp_fmt_source_compiles_without_scratch(tmp_path):
    """The method of tests/test_frames_host.py for csrc/flm_warp_fmt.hip: built by build.py, compiles for gfx950 with the
    build's flags, holds a kernel for every source kind and sample count, none has a private segment, none needs more
    than 128 registers (four waves per SIMD)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("_flm_build", os.path.join(ROOT, "face-landmark-detector_amd", "build.py"))
    bld = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bld)
    assert "flm_warp_fmt.hip" in bld.SOURCES
    assert "-ffp-contract=off" in bld.FLAGS
    out = str(tmp_path / "flm_warp_fmt.s")
    cmd = [bld._hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off",
           *bld.FILE_FLAGS.get("flm_warp_fmt.hip", []), "-I", os.path.join(ROOT, "include"), "-I", CSRC, "-S",
           "--cuda-device-only", os.path.join(CSRC, "flm_warp_fmt.hip"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    text = open(out).read()
    kernels = {}
    for m in re.finditer(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)", text):
        kernels[m.group(1)] = (int(m.group(2)), int(m.group(3)))
    print(kernels)
    for s in (1, 2, 4):                                   # uint8 pixel pairs: crops and ring frames, per sample count
        assert sum("warp_fmt_u8_kernelILi%dE" % s in k for k in kernels) == 8, s     # 2 layouts x 4 types
    for u8 in (0, 1):                                     # float32 crops; uint8 crops one column wide
        assert sum("warp_fmt_any_kernelILb%dE" % u8 in k for k in kernels) == 8, u8
    assert len(kernels) == 40
    bad = {k: v for k, v in kernels.items() if v[0] != 0}
    assert not bad, "kernels with a private segment (scratch): %s" % bad
    assert all(v[1] <= 128 for v in kernels.values()), kernels       # four waves per SIMD at the least
