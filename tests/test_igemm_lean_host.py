"""Launcher side of the fp32 implicit GEMM's lean set-up, on the host (no GPU): tests/native/igemm_lean_host.cpp checks
the multiply-shift row split of csrc/flm_igemm_args.h against integer division over the whole range of rows a launch
may have, and the launcher's claim "every tile sees every filter tap" (IgemmArgs::all_taps) against tap masks worked
out pixel by pixel for a few thousand layer geometries."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fastdiv_and_all_taps_on_the_host(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    exe = str(tmp_path / "igemm_lean_host")
    cmd = [hipcc, "-x", "hip", "--cuda-host-only", "--offload-arch=gfx950", "-O1", "-std=c++17",
           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "face-landmark-detector_amd", "csrc"),
           os.path.join(ROOT, "tests", "native", "igemm_lean_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
