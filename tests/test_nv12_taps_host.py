"""The NV12 tap code on the host (no GPU): tests/native/nv12_taps_host.cpp runs csrc/flm_nv12_dev.h -- the header the
kernels of csrc/flm_frames_nv12.hip are built from -- over every clamped source position of 2x2 ... 4x8 frames, dense
and with padded pitches and a U,V offset, in a heap buffer of exactly flm_frame_format_bytes, and compares each result
with a convert-then-index restatement.  The program is built with the host's address and undefined-behaviour
sanitizers, so a load outside the slot ends it: this is where an out-of-slot read is caught."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_nv12_taps_on_the_host(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    exe = str(tmp_path / "nv12_taps_host")
    cmd = [hipcc, "-x", "hip", "--cuda-host-only", "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-ffp-contract=off",
           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "face-landmark-detector_amd", "csrc"),
           os.path.join(ROOT, "tests", "native", "nv12_taps_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "0 failures" in r.stdout
