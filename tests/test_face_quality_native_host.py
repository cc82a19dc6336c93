"""The per-pixel pieces of flm_face_quality on the host (no GPU): tests/native/quality_host.cpp runs
csrc/flm_quality_dev.h -- the header the kernel of csrc/flm_quality.hip is built from -- over all 2^24 uint8 (B, G, R)
triples (Y in [0, 4080] and equal to a wide-integer restatement) and over every one of the 65,536 binary16 and bfloat16
bit patterns through the de-normalise and quantise step, with the matcher's scale and bias and with the identity (a NaN
gives 0, the infinities clamp, every result equals a long-double restatement rounded once per operation).  The program
is built with the host's address and undefined-behaviour sanitizers and run directly."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_quality_pieces_on_the_host(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    exe = str(tmp_path / "quality_host")
    cmd = [hipcc, "-x", "hip", "--cuda-host-only", "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-ffp-contract=off",
           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "face-landmark-detector_amd", "csrc"),
           os.path.join(ROOT, "tests", "native", "quality_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert " 0 failures" in r.stdout
