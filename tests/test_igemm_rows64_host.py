"""Launcher side of the 64-row tiles of the fp32 position-major implicit GEMM, on the host (no GPU):
tests/native/igemm_rows64_host.cpp sweeps 1..130 faces on 2x2, 4x4 and 8x8 maps with fc6's 7x7 filter and checks, with
csrc/flm_igemm_args.h as the library compiles it, that every output row belongs to exactly one tile, that a tile's tap mask
is the pixel-by-pixel one, that the position search is never worse than map order, and that the list-schedule model gives
69 tap-units for 128-row tiles and at most 62 for 64-row tiles at 64 faces on the 8x8 map.  The program is built with the
host's address and undefined-behaviour sanitizers.  The knob that forces a form is checked through the library's C ABI."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rows64_tiles_masks_search_and_schedule_model_on_the_host(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    exe = str(tmp_path / "igemm_rows64_host")
    cmd = [hipcc, "-x", "hip", "--cuda-host-only", "--offload-arch=gfx950", "-O1", "-g", "-std=c++17",
           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "face-landmark-detector_amd", "csrc"),
           os.path.join(ROOT, "tests", "native", "igemm_rows64_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert " 0 failures" in r.stdout


def test_rows64_kernel_fits_three_workgroups_per_cu(tmp_path):
    """The 64-row form is built for three workgroups per CU: at most 168 registers (512 / 3, in granules of 8) and no scratch
    (its 48 KiB of LDS are a launch argument).  The compile line of tests/test_build_hygiene.py."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    csrc = os.path.join(ROOT, "face-landmark-detector_amd", "csrc")
    out = str(tmp_path / "flm_igemm.s")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                        "-I", csrc, "-S", "--cuda-device-only", os.path.join(csrc, "flm_igemm.hip"), "-o", out],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    found = {}
    for m in re.finditer(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)",
                         open(out).read()):
        if "igemm_kernel" in m.group(1) and m.group(1).endswith("Li64EEEvNS_9IgemmArgsE"):
            found[m.group(1)] = (int(m.group(2)), int(m.group(3)))
    assert len(found) == 2, found                       # position-major, with and without the ReLU
    for name, (scratch, vgpr) in found.items():
        assert scratch == 0 and vgpr <= 168, (name, scratch, vgpr)


def test_f32_fc6_rows_knob():
    """"f32_fc6_rows": documented in the knob comment of include/flm.h, starts at 0 (the model decides), takes 64 and 128,
    rejects everything else and keeps its value then."""
    from flm_amd import _lib
    src = open(os.path.join(ROOT, "include", "flm.h")).read()
    text = src[src.index("/* A/B performance knobs"):src.index("int flm_set_tuning")]
    assert re.search(r'"f32_fc6_rows"\s+rows per tile', text) and re.search(r"0\s+\*\s+\(default\)", text)
    lib = _lib.load()
    v = C.c_int(-1)
    with _lib.tuning("f32_fc6_rows"):
        for val in (64, 128, 0):
            assert lib.flm_set_tuning(b"f32_fc6_rows", val) == 0
            assert lib.flm_get_tuning(b"f32_fc6_rows", C.byref(v)) == 0 and v.value == val
        assert lib.flm_set_tuning(b"f32_fc6_rows", 64) == 0
        for bad in (1, 32, 96, 256, -64):
            assert lib.flm_set_tuning(b"f32_fc6_rows", bad) != 0 and b"f32_fc6_rows" in lib.flm_last_error()
            assert lib.flm_get_tuning(b"f32_fc6_rows", C.byref(v)) == 0 and v.value == 64
