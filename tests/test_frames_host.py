"""CPU-side checks of the frame-space tail (flm_landmarks_to_frame, flm_warp_affine_frames, prediction.align_frames):
the symbols exist, every argument check answers before any launch (so without a GPU), the new source compiles for
gfx950 without a private segment, and the Python wrappers reject what they cannot run."""
import ctypes as C
import os
import re
import subprocess

import pytest
import torch

import flm_amd  # noqa: F401
from flm_amd import _lib, alignment, prediction

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "face-landmark-detector_amd", "csrc")


def test_library_exports_the_frame_entry_points():
    lib = C.CDLL(_lib.LIB_PATH)
    for name in ("flm_landmarks_to_frame", "flm_warp_affine_frames"):
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTS
    assert _lib.load().flm_abi_version() == 2          # purely additive


def test_argument_checks_answer_without_a_gpu():
    lib = _lib.load()
    p = C.c_void_p(0x1000)        # never dereferenced: every call below is rejected before a launch
    err = lambda: lib.flm_last_error().decode()
    full = 1080 * 1920 * 3
    # null pointers -> FLM_ERR_ARG
    assert lib.flm_landmarks_to_frame(None, None, p, 1, 68, 264, 264, 1080, 1920, p) == -1
    assert lib.flm_landmarks_to_frame(None, p, None, 1, 68, 264, 264, 1080, 1920, p) == -1
    assert lib.flm_landmarks_to_frame(None, p, p, 1, 68, 264, 264, 1080, 1920, None) == -1
    assert lib.flm_warp_affine_frames(None, None, full, 8, 1080, 1920, None, None, p, 1, p, 112, 112, 1) == -1
    assert lib.flm_warp_affine_frames(None, p, full, 8, 1080, 1920, None, None, None, 1, p, 112, 112, 1) == -1
    assert lib.flm_warp_affine_frames(None, p, full, 8, 1080, 1920, None, None, p, 1, None, 112, 112, 1) == -1
    # sizes outside the kernels' reach -> FLM_ERR_SHAPE, the limit named
    assert lib.flm_landmarks_to_frame(None, p, p, 0, 68, 264, 264, 1080, 1920, p) == -2
    assert lib.flm_landmarks_to_frame(None, p, p, 1, 68, 0, 264, 1080, 1920, p) == -2
    assert lib.flm_warp_affine_frames(None, p, full, 8, 1080, 1920, None, None, p, 0, p, 112, 112, 1) == -2
    assert "1 <= k <= 65535" in err()
    assert lib.flm_warp_affine_frames(None, p, full, 8, 1080, 1920, None, None, p, 65536, p, 112, 112, 1) == -2
    assert "1 <= k <= 65535" in err()
    assert lib.flm_warp_affine_frames(None, p, 1080 * 3, 8, 1080, 1, None, None, p, 1, p, 112, 112, 1) == -2
    assert "fw >= 2" in err()
    assert lib.flm_warp_affine_frames(None, p, full - 1, 8, 1080, 1920, None, None, p, 1, p, 112, 112, 1) == -2
    assert "frame_stride >= fh*fw*3" in err()
    assert lib.flm_warp_affine_frames(None, p, 1 << 32, 1, 32768, 21846, None, None, p, 1, p, 112, 112, 1) == -2
    assert "fh*fw*3 < 2^31" in err()                   # 32768 * 21846 * 3 = 2^31 + 98304
    assert lib.flm_warp_affine_frames(None, p, full, 0, 1080, 1920, None, None, p, 1, p, 112, 112, 1) == -2
    assert "nframes >= 1" in err()
    assert lib.flm_warp_affine_frames(None, p, full, 8, 1080, 1920, None, None, p, 1, p, 16384, 16384, 1) == -2
    assert "hd*wd*12 < 2^31" in err()
    # samples other than 1, 2, 4 -> FLM_ERR_ARG
    for s in (3, 0, 8, -1):
        assert lib.flm_warp_affine_frames(None, p, full, 8, 1080, 1920, None, None, p, 1, p, 112, 112, s) == -1, s
        assert "samples" in err()


def test_frames_source_compiles_without_scratch(tmp_path):
    """Same method as tests/test_build_hygiene.py, for the source that file's fixed list does not name: no kernel of
    flm_frames.hip has a private segment (the 4x4 sample grid holds 64 gathered dwords per pixel in registers)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("_flm_build", os.path.join(ROOT, "face-landmark-detector_amd", "build.py"))
    bld = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bld)
    assert "flm_frames.hip" in bld.SOURCES
    assert "-ffp-contract=off" in bld.FLAGS
    out = str(tmp_path / "flm_frames.s")
    cmd = [bld._hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off",
           *bld.FILE_FLAGS.get("flm_frames.hip", []), "-I", os.path.join(ROOT, "include"), "-I", CSRC, "-S",
           "--cuda-device-only", os.path.join(CSRC, "flm_frames.hip"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    text = open(out).read()
    kernels = {}
    for m in re.finditer(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)", text):
        kernels[m.group(1)] = (int(m.group(2)), int(m.group(3)))
    print(kernels)
    assert any("landmarks_to_frame_kernel" in k for k in kernels)
    for s in (1, 2, 4):
        assert any("warp_frames_kernelILi%dE" % s in k for k in kernels), s
    bad = {k: v for k, v in kernels.items() if v[0] != 0}
    assert not bad, "kernels with a private segment (scratch): %s" % bad
    assert all(v[1] <= 128 for v in kernels.values()), kernels       # four waves per SIMD at the least


class _Model:
    n_classes, input_height, input_width, output_height, output_width = 68, 256, 256, 264, 264


def test_python_wrappers_reject_bad_arguments_on_the_host():
    faces = [[(10, 10, 100, 100)], [(20, 20, 90, 90)]]
    ring = torch.zeros((2, 64, 96, 3), dtype=torch.uint8)
    with pytest.raises(ValueError):      # wrong dtype
        prediction.align_frames(ring.to(torch.float32), faces, _Model())
    with pytest.raises(ValueError):      # wrong rank
        prediction.align_frames(ring[0], faces, _Model())
    with pytest.raises(ValueError):      # not BGR triples
        prediction.align_frames(torch.zeros((2, 64, 96, 4), dtype=torch.uint8), faces, _Model())
    with pytest.raises(ValueError):      # slot outside the ring
        prediction.align_frames(ring, faces, _Model(), frame_index=[0, 2])
    with pytest.raises(ValueError):      # one slot per entry
        prediction.align_frames(ring, faces, _Model(), frame_index=[0])
    with pytest.raises(ValueError):      # more entries than ring slots, no explicit index
        prediction.align_frames(ring, faces + faces, _Model())
    with pytest.raises(ValueError):
        prediction.align_frames(ring, faces, _Model(), samples=3)
    with pytest.raises(ValueError):      # a list of frames of different sizes
        prediction.align_frames([ring[0], ring[1, :32]], faces, _Model())
    with pytest.raises(ValueError):      # host memory
        prediction.align_frames(ring, faces, _Model())
    lm = torch.zeros((2, 68, 2), dtype=torch.float64)
    boxes = torch.zeros((2, 4), dtype=torch.int32)
    m = torch.zeros((2, 2, 3), dtype=torch.float32)
    with pytest.raises(ValueError):
        alignment.landmarks_to_frame_device(lm.to(torch.float32), boxes, (264, 264), (64, 96))
    with pytest.raises(ValueError):
        alignment.landmarks_to_frame_device(lm[0], boxes, (264, 264), (64, 96))
    with pytest.raises(ValueError):      # host memory
        alignment.landmarks_to_frame_device(lm, boxes, (264, 264), (64, 96))
    with pytest.raises(ValueError):
        alignment.warp_frames_device(ring.to(torch.float32), m, 112, 112)
    with pytest.raises(ValueError):
        alignment.warp_frames_device(ring[0], m, 112, 112)
    with pytest.raises(ValueError):      # host memory
        alignment.warp_frames_device(ring, m, 112, 112)
