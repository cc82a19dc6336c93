"""The vocabulary of argument checks on the host (no GPU): tests/native/api_checks_host.cpp includes
csrc/flm_api_checks.h -- the header the extern "C" entry points of csrc/flm_api*.hip state their checks in -- and pins
ranges_overlap at its edges (adjacent, one byte in, nested, zero-length), the two overlap shapes (null entries skipped, the
first pair in array order named, the message formed from the caller's phrasing), the option-struct head (NULL gives the
defaults, struct_size one byte short, reserved = 1) and the integer range.  Built with the host's address and
undefined-behaviour sanitizers and run as its own process; it links nothing of the library."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_api_checks_on_the_host(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    exe = str(tmp_path / "api_checks_host")
    cmd = [hipcc, "-x", "hip", "--cuda-host-only", "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Wall",
           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "face-landmark-detector_amd", "csrc"),
           os.path.join(ROOT, "tests", "native", "api_checks_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "0 failures" in r.stdout
