"""CPU-side checks of the NV12 frame source (flm_frames_to_bgr, flm_crop_resize_frames_src, flm_warp_affine_frames_src,
alignment.FrameFormat): the symbols exist, every argument check answers before any launch (so without a GPU), the new
source compiles for gfx950 without a private segment, the numpy reference has the properties include/flm.h states, and
the Python wrappers reject what they cannot run."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import flm_amd  # noqa: F401
from flm_amd import _lib, alignment, prediction

import nv12_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "face-landmark-detector_amd", "csrc")
NEW = ("flm_frame_format_init", "flm_frame_format_bytes", "flm_frames_to_bgr", "flm_crop_resize_frames_src",
       "flm_warp_affine_frames_src")


def test_library_exports_the_nv12_entry_points():
    lib = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTS
    assert _lib.load().flm_abi_version() == 2          # purely additive


def fmt(pixel=_lib.FRAME_NV12, matrix=0, y_pitch=0, uv_pitch=0, uv_offset=0):
    f = _lib.FrameFormat()
    _lib.load().flm_frame_format_init(C.byref(f))
    f.pixel, f.matrix, f.y_pitch, f.uv_pitch, f.uv_offset = pixel, matrix, y_pitch, uv_pitch, uv_offset
    return f


def test_frame_format_init_and_bytes():
    lib = _lib.load()
    f = _lib.FrameFormat()
    lib.flm_frame_format_init(C.byref(f))
    assert f.struct_size == C.sizeof(_lib.FrameFormat) == 32
    assert (f.pixel, f.matrix, f.y_pitch, f.uv_pitch, f.uv_offset) == (_lib.FRAME_BGR24, 0, 0, 0, 0)
    assert lib.flm_frame_format_bytes(C.byref(f), 1080, 1920) == 1080 * 1920 * 3
    assert lib.flm_frame_format_bytes(C.byref(f), 5, 7) == 105          # BGR frames may be odd
    # NV12: uv_offset + (fh/2 - 1)*uv_pitch + fw, defaults resolved
    assert lib.flm_frame_format_bytes(C.byref(fmt()), 1080, 1920) == 1080 * 1920 * 3 // 2
    assert lib.flm_frame_format_bytes(C.byref(fmt()), 2, 2) == 6
    assert lib.flm_frame_format_bytes(C.byref(fmt(y_pitch=2048)), 1080, 1920) == 2048 * 1080 + 539 * 2048 + 1920
    assert lib.flm_frame_format_bytes(C.byref(fmt(y_pitch=80, uv_pitch=96, uv_offset=56 * 80)), 48, 64) == 56 * 80 + 23 * 96 + 64
    for fh, fw, g in ((48, 64, dict(y_pitch=80, uv_offset=56 * 80)), (6, 4, dict(y_pitch=7, uv_pitch=5, uv_offset=45))):
        yp = g.get("y_pitch", fw)
        assert lib.flm_frame_format_bytes(C.byref(fmt(**g)), fh, fw) == nv12_ref.slot_bytes_needed(
            fh, fw, yp, g.get("uv_offset", yp * fh), g.get("uv_pitch", yp))
    # rejected: 0
    for bad, fh, fw in ((fmt(), 1079, 1920), (fmt(), 1080, 1919), (fmt(), 0, 2), (fmt(y_pitch=63), 48, 64),
                        (fmt(uv_pitch=62), 48, 64), (fmt(y_pitch=80, uv_offset=48 * 80 - 1), 48, 64),
                        (fmt(pixel=2), 48, 64), (fmt(matrix=2), 48, 64), (fmt(pixel=_lib.FRAME_BGR24, y_pitch=64), 48, 64),
                        (fmt(pixel=_lib.FRAME_BGR24), 0, 64)):
        assert lib.flm_frame_format_bytes(C.byref(bad), fh, fw) == 0
    short = fmt()
    short.struct_size = 16
    assert lib.flm_frame_format_bytes(C.byref(short), 48, 64) == 0
    assert lib.flm_frame_format_bytes(None, 48, 64) == 0


def test_argument_checks_answer_without_a_gpu():
    lib = _lib.load()
    p = C.c_void_p(0x1000)        # never dereferenced: every call below is rejected before a launch
    err = lambda: lib.flm_last_error().decode()
    fh, fw = 1080, 1920
    full = fh * fw * 3 // 2
    ok = fmt()
    r = C.byref

    def to_bgr(src, frames=p, out=p, stride=full, nf=8, fh=fh, fw=fw):
        return lib.flm_frames_to_bgr(None, frames, stride, nf, fh, fw, src, out)

    def crop(src, frames=p, boxes=p, idx=p, out=p, stride=full, nf=8, fh=fh, fw=fw, k=1, oh=256, ow=256):
        return lib.flm_crop_resize_frames_src(None, frames, stride, nf, fh, fw, boxes, idx, k, out, oh, ow, src)

    def warp(src, frames=p, m=p, dst=p, stride=full, nf=8, fh=fh, fw=fw, k=1, hd=112, wd=112, samples=1, f=None):
        return lib.flm_warp_affine_frames_src(None, frames, stride, nf, fh, fw, None, None, m, k, dst, hd, wd, samples, f, src)

    # null pointers -> FLM_ERR_ARG
    assert to_bgr(r(ok), frames=None) == -1 and to_bgr(r(ok), out=None) == -1 and to_bgr(None) == -1
    assert crop(r(ok), frames=None) == -1 and crop(r(ok), boxes=None) == -1 and crop(r(ok), idx=None) == -1
    assert crop(r(ok), out=None) == -1 and crop(None) == -1
    assert warp(r(ok), frames=None) == -1 and warp(r(ok), m=None) == -1 and warp(r(ok), dst=None) == -1 and warp(None) == -1
    # unknown pixel / matrix, short struct -> FLM_ERR_ARG
    short = fmt()
    short.struct_size = C.sizeof(_lib.FrameFormat) - 4
    for call in (to_bgr, crop, warp):
        assert call(r(fmt(pixel=2))) == -1 and "pixel" in err()
        assert call(r(fmt(pixel=-1))) == -1
        assert call(r(fmt(matrix=2))) == -1 and "matrix" in err()
        assert call(r(fmt(pixel=_lib.FRAME_BGR24, matrix=7))) == -1
        assert call(r(short)) == -1 and "struct_size" in err()
    assert to_bgr(r(fmt(pixel=_lib.FRAME_BGR24))) == -1          # nothing to convert
    # the image format and samples of the warp, as flm_warp_affine_frames_fmt answers them
    bad_fmt = alignment.AlignedFormat().struct()
    bad_fmt.layout = 5
    assert warp(r(ok), f=r(bad_fmt)) == -1 and "layout" in err()
    f16 = alignment.AlignedFormat.matcher().struct()
    assert warp(r(ok), dst=C.c_void_p(0x1001), f=r(f16)) == -1 and "aligned" in err()
    assert warp(r(ok), dst=C.c_void_p(0x1002)) == -1             # fmt NULL is float32: 4-byte elements
    for s in (3, 0, 8, -1):
        assert warp(r(ok), samples=s) == -1 and "samples" in err()
    # everything else -> FLM_ERR_SHAPE, the limit named
    for call in (to_bgr, crop, warp):
        for a, b in ((1079, 1920), (1080, 1919), (0, 1920), (1080, 0), (-2, 1920)):
            assert call(r(ok), fh=a, fw=b) == -2 and "even" in err(), (a, b)
        assert call(r(fmt(y_pitch=1919))) == -2 and "y_pitch >= fw" in err()
        assert call(r(fmt(y_pitch=2048, uv_pitch=1918)), stride=1 << 23) == -2 and "uv_pitch >= fw" in err()
        assert call(r(fmt(y_pitch=2048, uv_offset=2048 * 1080 - 1)), stride=1 << 23) == -2 and "uv_offset >= y_pitch*fh" in err()
        assert call(r(ok), stride=full - 1) == -2 and "frame_stride >= flm_frame_format_bytes" in err()
        assert call(r(fmt(y_pitch=2048)), stride=2048 * 1080 + 539 * 2048 + 1919) == -2 and "frame_stride" in err()
        assert call(r(ok), fh=32768, fw=65536, stride=1 << 40) == -2 and "slot bytes < 2^31" in err()
        assert call(r(fmt(y_pitch=2048, uv_offset=1 << 31)), stride=1 << 40) == -2 and "slot bytes < 2^31" in err()
        assert call(r(ok), nf=0) == -2 and "nframes >= 1" in err()
    for call in (crop, warp):
        assert call(r(ok), k=0) == -2 and "1 <= k <= 65535" in err()
        assert call(r(ok), k=65536) == -2 and "1 <= k <= 65535" in err()
        # a BGR24 source is the dense ring: the pitch fields must be 0, and the limits are those of the BGR calls
        assert call(r(fmt(pixel=_lib.FRAME_BGR24, y_pitch=1920 * 3)), stride=fh * fw * 3) == -2 and "dense" in err()
        assert call(r(fmt(pixel=_lib.FRAME_BGR24, uv_offset=8)), stride=fh * fw * 3) == -2 and "dense" in err()
    assert crop(r(ok), oh=0) == -2 and "oh, ow >= 1" in err()
    assert crop(r(ok), oh=32768, ow=32768) == -2 and "oh*ow*3 < 2^31" in err()
    assert warp(r(ok), hd=16384, wd=16384) == -2 and "hd*wd*3*4 < 2^31" in err()
    assert warp(r(ok), hd=0) == -2
    bgr = fmt(pixel=_lib.FRAME_BGR24)
    assert warp(r(bgr), stride=fh * fw * 3 - 1) == -2 and "frame_stride >= fh*fw*3" in err()
    assert warp(r(bgr), stride=fh * fw * 3 - 1, f=r(f16)) == -2 and "frame_stride >= fh*fw*3" in err()
    assert warp(r(bgr), stride=1080 * 3, fw=1) == -2 and "fw >= 2" in err()
    assert crop(r(bgr), stride=fh * fw * 3 - 1) == -2


def test_nv12_source_compiles_without_scratch(tmp_path):
    """The method of tests/test_frames_host.py for csrc/flm_frames_nv12.hip: built by build.py, compiles for gfx950 with
    the build's flags, no kernel has a private segment, and the warps keep four waves per SIMD (128 registers)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("_flm_build", os.path.join(ROOT, "face-landmark-detector_amd", "build.py"))
    bld = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bld)
    assert "flm_frames_nv12.hip" in bld.SOURCES
    assert "-ffp-contract=off" in bld.FLAGS
    out = str(tmp_path / "flm_frames_nv12.s")
    cmd = [bld._hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off",
           *bld.FILE_FLAGS.get("flm_frames_nv12.hip", []), "-I", os.path.join(ROOT, "include"), "-I", CSRC, "-S",
           "--cuda-device-only", os.path.join(CSRC, "flm_frames_nv12.hip"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    text = open(out).read()
    kernels = {}
    for m in re.finditer(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)", text):
        kernels[m.group(1)] = (int(m.group(2)), int(m.group(3)))
    print(kernels)
    assert any("frames_to_bgr_kernel" in k for k in kernels)
    assert any("crop_resize_nv12_kernel" in k for k in kernels)
    for s, unr in ((1, 4), (2, 2), (4, 1)):
        for layout in (0, 1):
            for typ in (0, 1, 2, 3):
                tag = "warp_nv12_kernelILi%dELi%dELi%dELi%dE" % (s, unr, layout, typ)
                assert any(tag in k for k in kernels), tag
    bad = {k: v for k, v in kernels.items() if v[0] != 0}
    assert not bad, "kernels with a private segment (scratch): %s" % bad
    assert all(v[1] <= 128 for v in kernels.values()), kernels


# ---- the reference ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("matrix", ["bt601", "bt709"])
def test_reference_grey_points_and_saturation(matrix):
    g = lambda y, u=128, v=128: nv12_ref.yuv_to_bgr(y, u, v, matrix).tolist()
    assert g(16) == [0, 0, 0] and g(235) == [255, 255, 255]
    assert g(0) == [0, 0, 0] and g(15) == [0, 0, 0] and g(255) == [255, 255, 255]      # below black, above white
    assert g(126) == [128, 128, 128]
    # the clamps at both ends, per channel
    assert g(128, 255, 128)[0] == 255 and g(128, 0, 128)[0] == 0
    assert g(128, 128, 255)[2] == 255 and g(128, 128, 0)[2] == 0
    assert g(200, 0, 0)[1] == 255 and g(40, 255, 255)[1] == 0
    # all (Y,U,V) on a coarse lattice plus the extremes: the accumulator bound of include/flm.h (asserted in the reference)
    ax = np.unique(np.concatenate([np.arange(0, 256, 5), [15, 16, 17, 127, 128, 129, 234, 235, 236, 255]]))
    y, u, v = np.meshgrid(ax, ax, ax, indexing="ij")
    out = nv12_ref.yuv_to_bgr(y, u, v, matrix)
    assert out.dtype == np.uint8 and out.shape == y.shape + (3,)
    cy, cub, cug, cvg, cvr = nv12_ref.COEF[matrix]
    worst = max(abs(239 * cy + 127 * cub), abs(-128 * cub), abs(239 * cy - 128 * cvg - 128 * cug), abs(127 * cvg + 127 * cug),
                abs(239 * cy + 127 * cvr), abs(-128 * cvr)) + (1 << 19)
    assert worst <= 573636921 < 2 ** 31


def test_reference_constants():
    assert nv12_ref.COEF["bt601"] == tuple(int(round(c * 2 ** 20)) for c in (1.164, 2.018, -0.391, -0.813, 1.596))
    kr, kb = 0.2126, 0.0722
    kg = 1.0 - kr - kb
    sy, sc = 255.0 / 219.0, 255.0 / 224.0
    exact = (sy, 2 * (1 - kb) * sc, -2 * kb * (1 - kb) / kg * sc, -2 * kr * (1 - kr) / kg * sc, 2 * (1 - kr) * sc)
    assert nv12_ref.COEF["bt709"] == tuple(int(round(c * 2 ** 20)) for c in exact)


def test_reference_addressing_and_forward_transform():
    rng = np.random.default_rng(5)
    fh, fw, pitch, uv_row, rows = 6, 8, 11, 7, 12
    bgr = rng.integers(0, 256, (fh, fw, 3), dtype=np.uint8)
    y, uv = nv12_ref.bgr_to_nv12(bgr, "bt709")
    assert y.shape == (fh, fw) and uv.shape == (fh // 2, fw)
    slot = nv12_ref.pack_slot(y, uv, pitch, uv_row, rows, rng)
    out = nv12_ref.nv12_to_bgr_ref(slot.reshape(-1), fh, fw, pitch, uv_row * pitch, pitch, "bt709")
    for yy in range(fh):
        for xx in range(fw):
            exp = nv12_ref.yuv_to_bgr(y[yy, xx], uv[yy // 2, xx & ~1], uv[yy // 2, (xx & ~1) + 1], "bt709")
            assert (out[yy, xx] == exp).all()
    # the junk in the padding does not matter, and the reference reads no byte past flm_frame_format_bytes
    n = nv12_ref.slot_bytes_needed(fh, fw, pitch, uv_row * pitch, pitch)
    assert (nv12_ref.nv12_to_bgr_ref(slot.reshape(-1)[:n], fh, fw, pitch, uv_row * pitch, pitch, "bt709") == out).all()
    # a grey frame comes back grey, and a flat colour within the rounding of two 8-bit conversions
    flat = np.broadcast_to(np.array([40, 120, 200], np.uint8), (fh, fw, 3))
    for mtx in ("bt601", "bt709"):
        yf, uvf = nv12_ref.bgr_to_nv12(flat, mtx)
        back = nv12_ref.nv12_to_bgr_ref(nv12_ref.pack_slot(yf, uvf, fw, fh, fh * 3 // 2).reshape(-1), fh, fw, fw, fh * fw, fw, mtx)
        assert np.abs(back.astype(int) - flat.astype(int)).max() <= 3


# ---- Python ---------------------------------------------------------------------------------------------------------
class _Model:
    n_classes, input_height, input_width, output_height, output_width = 68, 64, 96, 72, 104


def test_frame_format_class():
    F = alignment.FrameFormat
    assert F.bgr().pixel == "bgr" and F.bgr() == F("bgr") and F.bgr().struct().pixel == _lib.FRAME_BGR24
    n = F.nv12(48, 64, matrix="bt709", uv_row=56)
    assert (n.pixel, n.height, n.width, n.matrix, n.uv_row) == ("nv12", 48, 64, "bt709", 56)
    assert F.nv12(48, 64).uv_row == 48 and F.nv12(48, 64).matrix == "bt601"
    assert n == F.nv12(48, 64, "bt709", 56) and n != F.nv12(48, 64, "bt601", 56) and hash(n) == hash(F.nv12(48, 64, "bt709", 56))
    ring = torch.zeros((3, 84, 80), dtype=torch.uint8)
    s = n.struct(ring)
    assert (s.struct_size, s.pixel, s.matrix, s.y_pitch, s.uv_pitch, s.uv_offset) == (32, 1, 1, 80, 80, 56 * 80)
    for bad in (dict(height=47, width=64), dict(height=48, width=63), dict(height=0, width=64), dict(height=48, width=64, uv_row=47),
                dict(height=48, width=64, matrix="bt2020"), dict(height=48, width=64, matrix=None)):
        with pytest.raises(ValueError):
            F.nv12(**bad)
    with pytest.raises(ValueError):
        F("i420")


def test_python_wrappers_reject_bad_arguments_on_the_host():
    F = alignment.FrameFormat
    nv = F.nv12(48, 64, uv_row=56)
    faces = [[(10, 10, 40, 40)], [(20, 20, 50, 50)]]
    ring = torch.zeros((2, 84, 80), dtype=torch.uint8)
    m = torch.zeros((2, 2, 3), dtype=torch.float32)
    bad_rings = [[ring[0], ring[1]],                                   # a list of frames
                 ring[0],                                              # wrong rank
                 torch.zeros((2, 48, 64, 3), dtype=torch.uint8),       # a BGR ring
                 ring.to(torch.float32),                               # wrong type
                 torch.zeros((2, 79, 80), dtype=torch.uint8),          # too few rows for 24 U,V rows from row 56
                 torch.zeros((2, 84, 62), dtype=torch.uint8),          # pitch shorter than the width
                 ring]                                                 # host memory
    for bad in bad_rings:
        with pytest.raises(ValueError):
            prediction.align_frames(bad, faces, _Model(), frame_format=nv)
        with pytest.raises(ValueError):
            prediction.crop_frames_device(bad, faces, 64, 96, frame_format=nv)
        with pytest.raises(ValueError):
            alignment.warp_frames_device(bad, m, 112, 112, src=nv)
        with pytest.raises(ValueError):
            prediction.frames_to_bgr_device(bad, nv)
    with pytest.raises(ValueError):      # not a FrameFormat
        prediction.align_frames(ring, faces, _Model(), frame_format="nv12")
    with pytest.raises(ValueError):
        prediction.crop_frames_device(ring, faces, 64, 96, frame_format="nv12")
    with pytest.raises(ValueError):
        alignment.warp_frames_device(ring, m, 112, 112, src="nv12")
    with pytest.raises(ValueError):      # nothing to convert
        prediction.frames_to_bgr_device(torch.zeros((2, 48, 64, 3), dtype=torch.uint8), F.bgr())
    with pytest.raises(ValueError):
        prediction.frames_to_bgr_device(ring, None)
    with pytest.raises(ValueError):      # a BGR format wants the BGR ring
        alignment.warp_frames_device(ring, m, 112, 112, src=F.bgr())
