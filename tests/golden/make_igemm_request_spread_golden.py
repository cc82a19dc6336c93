"""Generate tests/golden/igemm_request_spread_golden.npz: what the fp32 forward held, bit for bit, with the operand
requests of the implicit GEMM's k-step in (A, B) pairs behind every fourth MFMA (the placement before the requests were
dealt one per MFMA; csrc/flm_igemm.hip, FLM_IGEMM_VAR bits 7-8 = 2 rebuilds it).

Run on a GPU with a library of that placement:
    python tests/golden/make_igemm_request_spread_golden.py [path to libflm_hip.so]

Per case of tests/igemm_spread_cases.py: "<case>/landmarks" the float32 landmarks, "<case>/<name>" the SHA-1 of every
named workspace tensor (20 uint8; the tensors themselves run to megabytes).  Recorded results only.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
import flm_amd  # noqa: E402,F401
from flm_amd import _lib  # noqa: E402
import igemm_spread_cases as cases  # noqa: E402

if len(sys.argv) > 1:
    _lib.LIB_PATH = os.path.abspath(sys.argv[1])
out = {}
for case in cases.CASES:
    got = cases.run_case(case)
    cid = cases.case_id(case)
    out[cid + "/landmarks"] = got.pop("landmarks").cpu().numpy()
    for k, t in got.items():
        out[cid + "/" + k] = cases.digest(t)
    print(cid, sorted(got), flush=True)
dst = os.environ.get("OUT", os.path.join(HERE, "igemm_request_spread_golden.npz"))
np.savez(dst, **out)
print("wrote", dst, os.path.getsize(dst), "bytes")
