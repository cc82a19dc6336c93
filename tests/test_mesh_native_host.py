"""The mesh arithmetic of the piecewise-affine warp on the host (no GPU): tests/native/mesh_host.cpp runs
csrc/flm_mesh_dev.h -- the header the kernels of csrc/flm_mesh.hip are built from -- over seeded meshes and faces and over
the extremes of the contract (collapsed, collinear and NaN landmarks, coordinates at 0 and 2^15, a pixel exactly on a
shared edge and on a shared vertex, a determinant on either side of min_det) and compares with a long-double
restatement: the map must be equal, the affines within 1 ULP of float32.  The program is built without contraction, as
the library is, and with the host's address and undefined-behaviour sanitizers."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mesh_arithmetic_on_the_host(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    exe = str(tmp_path / "mesh_host")
    cmd = [hipcc, "-x", "hip", "--cuda-host-only", "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-ffp-contract=off",
           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "face-landmark-detector_amd", "csrc"),
           os.path.join(ROOT, "tests", "native", "mesh_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert " 0 failures" in r.stdout
