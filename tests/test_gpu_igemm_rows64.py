"""The 64-row tiles of the fp32 position-major implicit GEMM (csrc/flm_igemm.hip, template BMT; knob "f32_fc6_rows").

The 64-row form keeps the k-step, the k order and the three accumulator sets of the 128-row form and cuts the third-level
groups on the same dense (chunk, tap) index, so an output is the same sum in the same order whichever form computes it:
fc6, fc7 and the landmarks must be equal bit for bit (torch.equal) with the knob forced to 64 and to 128.  With the knob
at 0 the launcher's schedule model chooses; which form ran is read back through flm_debug_query("igemm_posmajor_rows")."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from flm_amd import _lib
    return _lib.load()


def _model_and_faces(n, h, w):
    from flm_amd.networks import LANDMARKS_MODELS
    from flm_amd.weights import synth_fcn8_weights
    model = LANDMARKS_MODELS["fcn_8"](68, input_height=h, input_width=w)
    model.load_weights(synth_fcn8_weights(68, seed=2))
    xd = torch.from_numpy(np.random.default_rng(1000 * n + h).integers(0, 256, (n, h, w, 3), dtype=np.uint8)).cuda()
    return model, xd


# (faces, H, W); fc6's map is H/32 x W/32.
#   (64, 64, 64)    2x2 map, a 64-row tile is one position            (65, 64, 64)   partial last tile
#   (64, 128, 128)  4x4 map, positions with different tap sets       (32, 128, 128) two positions per tile, posperm active
#   (17, 256, 256)  8x8 map, tiles straddle positions, above the split-K brackets
#   (3, 256, 256)   split-K bracket: the slices are chosen from the 128-row grid and stay
@pytest.mark.parametrize("n,h,w", [(64, 64, 64), (64, 128, 128), (32, 128, 128), (17, 256, 256), (65, 64, 64), (3, 256, 256)])
def test_fcn8_f32_rows64_keeps_every_bit(lib, n, h, w):
    from flm_amd import _lib
    model, xd = _model_and_faces(n, h, w)
    got = {}
    with _lib.tuning("f32_fc6_rows"):
        for rows in (64, 128):
            _lib.check(lib.flm_set_tuning(b"f32_fc6_rows", rows), "set_tuning")
            lm = model.forward_device(xd, "landmarks", n_points=4).clone()
            torch.cuda.synchronize()
            assert lib.flm_debug_query(b"igemm_posmajor_rows", 0) == rows      # the forced form is the one that ran
            got[rows] = {"fc6": model.intermediate("fc6", n, "landmarks", 4).clone(),
                         "fc7": model.intermediate("fc7", n, "landmarks", 4).clone(), "landmarks": lm}
    for k in ("fc6", "fc7", "landmarks"):
        assert torch.isfinite(got[64][k]).all(), k
        assert torch.equal(got[64][k], got[128][k]), (k, float((got[64][k] - got[128][k]).abs().max()))
    assert float(got[64]["fc6"].abs().max()) > 0.0


@pytest.mark.parametrize("n,h,w,rows", [(64, 256, 256, 64), (128, 64, 64, 128)])
def test_default_form_is_the_models_choice(lib, n, h, w, rows):
    from flm_amd import _lib
    model, xd = _model_and_faces(n, h, w)
    with _lib.tuning(f32_fc6_rows=0):
        model.forward_device(xd, "landmarks", n_points=4)
        torch.cuda.synchronize()
        assert lib.flm_debug_query(b"igemm_posmajor_rows", 0) == rows
