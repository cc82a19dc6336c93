"""The arithmetic of flm_flow_pyramid and flm_landmark_flow on the host (no GPU): tests/native/flow_host.cpp runs
csrc/flm_flow_dev.h -- the header the flow kernels are built from -- over the cases of tests/flow_cases.py
and must equal tests/flow_ref.py bit for bit: both pyramids byte for byte, every landmark as its uint64 bits, every err
and every flag.  The program is built without contraction, as the library is, and with the host's address and
undefined-behaviour sanitizers."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import flow_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_flow_arithmetic_on_the_host_equals_the_reference(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    exe = str(tmp_path / "flow_host")
    cmd = [hipcc, "-x", "hip", "--cuda-host-only", "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-ffp-contract=off",
           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "face-landmark-detector_amd", "csrc"),
           os.path.join(ROOT, "tests", "native", "flow_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    cases = flow_cases.cases()
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        # the program takes one face per case: the faces of a case become cases of their own
        faces = [(c, k) for c in cases for k in range(c["lm"].shape[0])]
        f.write(struct.pack("<i", len(faces)))
        for c, k in faces:
            o, (h, w) = c["opts"], c["hw"]
            f.write(struct.pack("<8i", h, w, c["ch"], o["levels"], o["radius"], o["max_iter"], c["lm"].shape[1], 0))
            f.write(struct.pack("<4d", o["eps"], o["min_eig"], o["max_err"], o["max_move"]))
            f.write(np.ascontiguousarray(c["m"][k], np.float32).tobytes())
            f.write(np.ascontiguousarray(c["lm"][k], np.float64).tobytes())
            f.write(c["prev"][k].tobytes())
            f.write(c["cur"][k].tobytes())
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert " 0 failures" in r.stdout
    got = open(fout, "rb").read()
    off = 0
    rec = np.dtype([("lm", "<u8", 2), ("err", "<i4"), ("flags", "<i4")])
    for i, c in enumerate(cases):
        pp, pc, lm, _, err, flags = flow_cases.expected(i)
        for k in range(lm.shape[0]):
            for want in (pp[k], pc[k]):
                assert got[off:off + want.size] == want.tobytes(), (c["name"], k, "pyramid")
                off += want.size
            pts = np.frombuffer(got, rec, lm.shape[1], off)
            off += rec.itemsize * lm.shape[1]
            assert (pts["flags"] == flags[k]).all(), (c["name"], k, pts["flags"], flags[k])
            assert (pts["err"] == err[k]).all(), (c["name"], k)
            assert (pts["lm"] == np.ascontiguousarray(lm[k]).view(np.uint64)).all(), (c["name"], k)
    assert off == len(got)
