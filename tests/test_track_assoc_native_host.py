"""The integer pieces of flm_track_associate on the host (no GPU): tests/native/track_assoc_host.cpp runs
csrc/flm_track_assoc_dev.h -- the header the kernel of csrc/flm_track_assoc.hip is built from -- over boxes at the
extremes of the contract (coordinates at +-2^28, frames of 1 x 2^30 and 32768 x 32768, empty, inverted and one-pixel
boxes) and compares every result with an __int128 / long-double restatement.  The program is built with the host's
address and undefined-behaviour sanitizers, so a signed overflow in the header ends it: this is where one is caught."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_track_assoc_pieces_on_the_host(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    exe = str(tmp_path / "track_assoc_host")
    cmd = [hipcc, "-x", "hip", "--cuda-host-only", "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-ffp-contract=off",
           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "face-landmark-detector_amd", "csrc"),
           os.path.join(ROOT, "tests", "native", "track_assoc_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert " 0 failures" in r.stdout
