"""The flow tick on rows on the host (no GPU): tests/native/flow_rows_host.cpp runs csrc/flm_flow_rows_dev.h -- the header
the kernels of csrc/flm_flow_rows.hip are built from -- over the cases of tests/flow_rows_cases.py and must equal
tests/flow_rows_ref.py bit for bit: every landmark, weight and fb as its uint64 bits, every err and flag; every tensor the
gather and the put write.  The program is built without contraction, as the library is, and with the host's address and
undefined-behaviour sanitizers.  The occlusion case's own condition is asserted on the reference."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import flow_rows_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GATHER_INOUT = (("reset", np.int32), ("age", np.float64), ("cursor", np.int32), ("flow_ready", np.int32))
GATHER_OUT = (("slot_c", np.int32), ("m_c", np.float32), ("boxes_c", np.int32), ("frame_idx_c", np.int32),
              ("prev_frame_idx_c", np.int32), ("dt_c", np.float64), ("best_q_c", np.float64), ("reset_c", np.int32),
              ("counts", np.int32))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32, 1: np.uint8}[a.dtype.itemsize])


def test_the_occlusion_case_is_one_only_the_backward_pass_judges():
    only_fb, passed = rc.occlusion_holds()
    assert only_fb >= 5 and passed >= 5, (only_fb, passed)


@pytest.fixture(scope="module")
def answer(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    tmp = tmp_path_factory.mktemp("flow_rows")
    exe = str(tmp / "flow_rows_host")
    cmd = [hipcc, "-x", "hip", "--cuda-host-only", "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-ffp-contract=off",
           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "face-landmark-detector_amd", "csrc"),
           os.path.join(ROOT, "tests", "native", "flow_rows_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    fin, fout = str(tmp / "in.bin"), str(tmp / "out.bin")
    raw = lambda a, t: np.ascontiguousarray(a, t).tobytes()
    with open(fin, "wb") as f:
        f.write(struct.pack("<i", len(rc.cases()) + len(rc.gather_cases()) + len(rc.put_cases())))
        for c in rc.cases():
            o, (h, w) = c["opts"], c["hw"]
            f.write(struct.pack("<11i", 1, h, w, c["ch"], o["levels"], o["radius"], o["max_iter"], c["lm"].shape[1],
                                len(c["slot"]), c["n_slots"], int(c["w"] is not None)))
            f.write(struct.pack("<5d", o["eps"], o["min_eig"], o["max_err"], o["max_move"], c["max_fb"]))
            f.write(raw(c["m"], np.float32) + raw(c["slot"], np.int32) + raw(c["lm"], np.float64))
            if c["w"] is not None:
                f.write(raw(c["w"], np.float64))
            f.write(c["prev"].tobytes() + c["cur"].tobytes())
        for a in rc.gather_cases():
            has = [int(a[k] is not None) for k in ("stream_on", "frame_idx_stream", "dt_stream", "best_q", "reset", "age", "cursor")]
            f.write(struct.pack("<13i", 2, a["s"], a["k"], a["fh"], a["fw"], a["n"], *has))
            f.write(struct.pack("<d", a["dt"]))
            for k, t in (("stream_on", np.int32), ("frame_idx_stream", np.int32), ("dt_stream", np.float64),
                         ("m_crop", np.float32), ("boxes", np.int32), ("best_q", np.float64), ("reset", np.int32),
                         ("age", np.float64), ("cursor", np.int32), ("flow_frame", np.int32), ("flow_ready", np.int32)):
                if a[k] is not None:
                    f.write(raw(a[k], t))
        for a in rc.put_cases():
            f.write(struct.pack("<6i", 3, len(a["slot"]), len(a["flow_ready"]), a["c"], int(a["lm_rows"] is not None),
                                int(a["w_rows"] is not None)))
            for k, t in (("slot", np.int32), ("status_rows", np.int32), ("frame_idx_c", np.int32), ("lm_rows", np.float64),
                         ("hist_lm", np.float64), ("w_rows", np.float64), ("hist_w", np.float64), ("flow_frame", np.int32),
                         ("flow_ready", np.int32)):
                if a[k] is not None:
                    f.write(raw(a[k], t))
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert " 0 failures" in r.stdout
    got = open(fout, "rb").read()
    # cut the answer into its records
    off, flows, gathers, puts = 0, [], [], []
    rec = np.dtype([("d", "<u8", 4), ("err", "<i4"), ("flags", "<i4")])
    for c in rc.cases():
        cnt = len(c["slot"]) * c["lm"].shape[1]
        flows.append(np.frombuffer(got, rec, cnt, off).reshape(len(c["slot"]), -1))
        off += rec.itemsize * cnt
    for i in range(len(rc.gather_cases())):
        want, rec_out = rc.gather_expected(i), {}
        for name, t in GATHER_INOUT + GATHER_OUT:
            if name in want:
                cnt = want[name].size
                rec_out[name] = np.frombuffer(got, t, cnt, off).reshape(want[name].shape)
                off += cnt * np.dtype(t).itemsize
        gathers.append(rec_out)
    for i in range(len(rc.put_cases())):
        rec_out = []
        for want, t in zip(rc.put_expected(i), (np.float64, np.float64, np.int32, np.int32)):
            if want is None:
                rec_out.append(None)
                continue
            rec_out.append(np.frombuffer(got, t, want.size, off).reshape(want.shape))
            off += want.size * np.dtype(t).itemsize
        puts.append(rec_out)
    assert off == len(got)
    return flows, gathers, puts


@pytest.mark.parametrize("i", range(len(rc.cases())), ids=[c["name"] for c in rc.cases()])
def test_rows_flow_on_the_host_equals_the_reference(answer, i):
    lm, w, err, fb, flags = rc.expected(i)
    pts = answer[0][i]
    assert (pts["flags"] == flags).all(), (pts["flags"], flags)
    assert (pts["err"] == err).all()
    assert (pts["d"][..., :2] == bits(lm)).all()
    assert (pts["d"][..., 2] == bits(w)).all()
    assert (pts["d"][..., 3] == bits(fb)).all()


@pytest.mark.parametrize("i", range(len(rc.gather_cases())), ids=[c["name"] for c in rc.gather_cases()])
def test_gather_on_the_host_equals_the_reference(answer, i):
    want, got = rc.gather_expected(i), answer[1][i]
    assert set(want) == set(got)
    for name, v in want.items():
        assert np.array_equal(bits(got[name]), bits(v)), (name, got[name], v)


@pytest.mark.parametrize("i", range(len(rc.put_cases())), ids=[c["name"] for c in rc.put_cases()])
def test_put_on_the_host_equals_the_reference(answer, i):
    for name, got, want in zip(("hist_lm", "hist_w", "flow_frame", "flow_ready"), answer[2][i], rc.put_expected(i)):
        assert (got is None) == (want is None), name
        if want is not None:
            assert np.array_equal(bits(got), bits(want)), name
