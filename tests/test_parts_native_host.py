"""The arithmetic of flm_part_affines / flm_warp_parts_frames and flm_face_openness on the host (no GPU):
tests/native/parts_host.cpp runs csrc/flm_parts_dev.h -- the header the kernels of csrc/flm_parts.hip are built from --
over the cases of tests/parts_ref.py and must equal that restatement bit for bit: every matrix as its uint32 bits, every
record and every state as uint64 bits.  The program is built without contraction, as the library is, and with the host's
address and undefined-behaviour sanitizers."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import flm_amd  # noqa: F401
from flm_amd import alignment

import parts_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fit_cases():
    tm = alignment.canonical_template(68, 96, 128)
    lm, w = ref.face_landmarks(7, 96, 128, 3, tm)
    dp = alignment.FaceParts.default(68, (17, 23))
    parts = [dp.part(r) for r in range(len(dp))] + ref.custom_parts(17, 23)
    return [(lm[f], ww, idx, t) for f in range(lm.shape[0]) for ww in (None, w[f]) for idx, t in parts]


def _rec_cases():
    lm, w = ref.openness_landmarks(9, 4)
    ms = ref.DEFAULT_MEASURES + ref.EXTRA_MEASURES
    return [(lm[r], ww, m, 4.0) for r in range(lm.shape[0]) for ww in (None, w[r]) for m in ms]


def _seq_cases():
    o, not_ok, resets, _ = ref.eye_script()
    th = dict(ref.DEFAULT_TH, min_closed=0.05, max_closed=0.2)
    seqs = []
    for s in range(o.shape[1]):
        seqs.append((th, list(ref.STATE_EMPTY), [(0 if (t, s) in not_ok else 1, 0, 1 if (t, s) in resets else 0,
                                                   float(o[t, s]), 0.04, 100 + t) for t in range(o.shape[0])]))
    rng = np.random.default_rng(8)
    for _ in range(6):   # random walks: every branch, odd dt (a zero, a NaN and an inf among them), statuses, resets
        ticks = []
        for t in range(60):
            dt = float(rng.choice([0.01, 0.033, 0.1, 0.0, np.nan, np.inf, 1e-9], p=[0.3, 0.3, 0.25, 0.04, 0.04, 0.03, 0.04]))
            ticks.append((int(rng.random() < 0.85), int(rng.choice([0, 0, 0, 8])), int(rng.random() < 0.05),
                          float(rng.choice([0.05, 0.17, 0.18, 0.2, 0.22, 0.23, 0.4])), dt, int(rng.integers(-5, 2 ** 40))))
        seqs.append((ref.DEFAULT_TH, [7.0] * 8 if _ % 2 else list(ref.STATE_EMPTY), ticks))
    return seqs


def test_parts_arithmetic_on_the_host_equals_the_reference(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    exe = str(tmp_path / "parts_host")
    cmd = [hipcc, "-x", "hip", "--cuda-host-only", "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-ffp-contract=off",
           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "face-landmark-detector_amd", "csrc"),
           os.path.join(ROOT, "tests", "native", "parts_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    fits, recs, seqs = _fit_cases(), _rec_cases(), _seq_cases()
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<i", len(fits)))
        for lm, w, idx, t in fits:
            f.write(struct.pack("<4i", lm.shape[0], len(idx), int(w is not None), 0))
            f.write(np.asarray(idx, np.int32).tobytes())
            f.write(np.ascontiguousarray(t, np.float64).tobytes())
            f.write(np.ascontiguousarray(lm, np.float64).tobytes())
            if w is not None:
                f.write(np.ascontiguousarray(w, np.float64).tobytes())
        f.write(struct.pack("<i", len(recs)))
        for lm, w, ((a, b), pairs), mw in recs:
            f.write(struct.pack("<8i", lm.shape[0], int(w is not None), a, b, len(pairs), 0, 0, 0))
            up = [u for u, _ in pairs] + [0] * (4 - len(pairs))
            lo = [l for _, l in pairs] + [0] * (4 - len(pairs))
            f.write(struct.pack("<8i", *(up + lo)))
            f.write(struct.pack("<d", mw))
            f.write(np.ascontiguousarray(lm, np.float64).tobytes())
            if w is not None:
                f.write(np.ascontiguousarray(w, np.float64).tobytes())
        f.write(struct.pack("<i", len(seqs)))
        for th, st, ticks in seqs:
            f.write(struct.pack("<2i", len(ticks), 0))
            f.write(struct.pack("<4d", th["close_below"], th["open_above"], th["min_closed"], th["max_closed"]))
            f.write(struct.pack("<8d", *st))
            for ok, status, reset, o, dt, fid in ticks:
                f.write(struct.pack("<4i2dq", ok, status, reset, 0, o, dt, fid))
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert " 0 failures" in r.stdout
    got = open(fout, "rb").read()
    off = 0
    seen_ok = set()
    for i, (lm, w, idx, t) in enumerate(fits):
        m, ok = ref.part_fit(lm, w, idx, np.asarray(t, np.float64))
        assert got[off:off + 24] == m.tobytes(), ("fit", i)
        assert struct.unpack_from("<i", got, off + 24)[0] == int(ok), ("fit ok", i)
        seen_ok.add(bool(ok))
        off += 28
    assert seen_ok == {True, False}
    seen_ok = set()
    for i, (lm, w, m, mw) in enumerate(recs):
        want = ref.open_record(lm, w, m, mw)
        assert got[off:off + 32] == want.tobytes(), ("record", i, np.frombuffer(got, np.float64, 4, off), want)
        seen_ok.add(want[2])
        off += 32
    assert seen_ok == {0.0, 1.0}
    events = []
    for i, (th, st, ticks) in enumerate(seqs):
        st = np.array(st, np.float64)
        for j, (ok, status, reset, o, dt, fid) in enumerate(ticks):
            if reset:
                st[:] = ref.STATE_EMPTY
            ref.state_step(st, bool(ok), np.float64(o), status, dt, th, fid)
            assert got[off:off + 64] == st.tobytes(), ("state", i, j, np.frombuffer(got, np.float64, 8, off), st)
            off += 64
        events.append(st[2])
    assert off == len(got)
    assert events[:6] == [float(v) for v in ref.eye_script()[3]]      # the hand count
