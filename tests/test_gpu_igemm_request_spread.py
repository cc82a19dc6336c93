"""The operand requests of the fp32 implicit GEMM's k-step, dealt one per MFMA (csrc/flm_igemm.hip, FLM_STEP2).

Only WHERE a step's eight buffer_load ... lds requests (six in the 64-row form) stand among the MFMAs behind the step's
barrier changed: the same requests fill the same stages and are waited for at the same barrier, no arithmetic moved.  The
placement is chosen at compile time (FLM_IGEMM_VAR bits 7-8), so the two cannot run in one library; the reference is what
a library with the earlier placement held, recorded by tests/golden/make_igemm_request_spread_golden.py: the landmarks
themselves, and the SHA-1 of every workspace tensor (equal digests = equal bits; the tensors run to megabytes).  Every
tensor of the forward must be equal bit for bit (torch.equal)."""
import os

import numpy as np
import pytest
import torch

import igemm_spread_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "igemm_request_spread_golden.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("case", cases.CASES, ids=cases.case_id)
def test_f32_forward_keeps_every_bit(golden, case):
    got = cases.run_case(case)
    cid = cases.case_id(case)
    names = sorted(k[len(cid) + 1:] for k in golden if k.startswith(cid + "/"))
    assert sorted(got) == names                                     # nothing recorded goes unchecked, nothing new unrecorded
    if case[0] == "fcn_8":
        assert set(cases.NAMES) <= set(names)
    lm = got.pop("landmarks").cpu()
    assert torch.isfinite(lm).all()
    exp = torch.from_numpy(golden[cid + "/landmarks"])
    assert torch.equal(lm, exp), float((lm - exp).abs().max())
    for k, t in got.items():
        assert torch.isfinite(t).all(), k
        assert float(t.abs().max()) > 0.0, k
        assert torch.equal(torch.from_numpy(cases.digest(t)), torch.from_numpy(golden[cid + "/" + k])), k
