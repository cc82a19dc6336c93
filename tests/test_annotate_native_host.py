"""The integer pieces of flm_frames_annotate on the host (no GPU): tests/native/annotate_host.cpp runs
csrc/flm_annotate_dev.h -- the header the kernels of csrc/flm_annotate.hip and flm_bgr_to_yuv are built from -- over all
2^24 colours and both matrices (against a restatement whose coefficients come from Kr and Kb, and through the round trip
of csrc/flm_nv12_dev.h, which stays within 2 per channel), over regions at the extremes of the contract (coordinates 0 and
2^30, margins 0 and 4, one point, every point rejected, NaN, inf, -0.0), and over the cell range and the ownership
predicate of every pair of small boxes on a small grid.  The program is built without contraction, as the library is, and
with the host's address and undefined-behaviour sanitizers; it is run directly."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_annotate_arithmetic_on_the_host(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    exe = str(tmp_path / "annotate_host")
    cmd = [hipcc, "-x", "hip", "--cuda-host-only", "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-ffp-contract=off",
           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "face-landmark-detector_amd", "csrc"),
           os.path.join(ROOT, "tests", "native", "annotate_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert " 0 failures" in r.stdout
    assert "worst |difference| per channel = " in r.stdout
