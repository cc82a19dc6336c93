"""The lean set-up and write-out of the fp32 implicit GEMM (csrc/flm_igemm.hip, template LEAN; knob "f32_lean_tile").

Only the path into and out of the k-loop differs from the plain form (LEAN = false): rows are taken apart with multiply-shift
constants, the tap mask is the full set where the launcher proves every tap in bounds for every tile, full tiles are
stored without per-element tests.  The k-loop, the summation tree and the write-out's arithmetic are the same, so
knob 0 against knob 1 must agree bit for bit (torch.equal) on every tensor of the forward."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

_NAMES = ("f1", "f2", "f3", "f4", "f5", "fc6", "fc7", "score5", "fuse4", "seg_feats")


@pytest.fixture(scope="module")
def lib():
    from flm_amd import _lib
    return _lib.load()


def _both_knobs(lib, run):
    """run() under f32_lean_tile = 0 and = 1; the value on entry is restored whatever happens."""
    from flm_amd import _lib
    got = {}
    with _lib.tuning("f32_lean_tile"):
        for knob in (0, 1):
            _lib.check(lib.flm_set_tuning(b"f32_lean_tile", knob), "set_tuning")
            got[knob] = run()
    return got


# 1 face 32x32: a tile spans whole maps, h5 = 1, split-K bracket; 5 faces 96x160: neither square nor a power of two (the
# multiply-shift constants are not shifts); 20 faces: above the split-K brackets, partial last tiles; 2 faces 256x256:
# the real geometry inside the split-K bracket
@pytest.mark.parametrize("n,h,w", [(1, 32, 32), (3, 64, 64), (5, 96, 160), (20, 64, 64), (2, 256, 256)])
def test_fcn8_f32_lean_tile_keeps_every_bit(lib, n, h, w):
    from flm_amd.networks import LANDMARKS_MODELS
    from flm_amd.weights import synth_fcn8_weights
    model = LANDMARKS_MODELS["fcn_8"](68, input_height=h, input_width=w)
    model.load_weights(synth_fcn8_weights(68, seed=2))
    xd = torch.from_numpy(np.random.default_rng(100 * n + h).integers(0, 256, (n, h, w, 3), dtype=np.uint8)).cuda()

    def run():
        lm = model.forward_device(xd, "landmarks", n_points=4).clone()
        probs = model.forward_device(xd, "probs").clone()
        torch.cuda.synchronize()
        out = {k: model.intermediate(k, n, "probs").clone() for k in _NAMES}
        out["probs"], out["landmarks"] = probs, lm
        return out

    got = _both_knobs(lib, run)
    for k in got[0]:
        assert torch.isfinite(got[1][k]).all(), k
        assert torch.equal(got[0][k], got[1][k]), (k, float((got[0][k] - got[1][k]).abs().max()))


# strides, the residual add and the ReLU6 clamp in the write-out
@pytest.mark.parametrize("name,synth", [("fcn_8_resnet50", "synth_resnet50_weights"), ("fcn_8_vgg", "synth_vgg_weights"),
                                        ("fcn_8_mobilenet", "synth_mobilenet_weights")])
def test_other_encoders_f32_lean_tile_keeps_every_bit(lib, name, synth):
    from flm_amd import weights
    from flm_amd.networks import LANDMARKS_MODELS
    n, h, w = 2, 64, 64
    model = LANDMARKS_MODELS[name](68, input_height=h, input_width=w)
    model.load_weights(getattr(weights, synth)(68, seed=5))
    xd = torch.from_numpy(np.random.default_rng(9).integers(0, 256, (n, h, w, 3), dtype=np.uint8)).cuda()

    def run():
        probs = model.forward_device(xd, "probs").clone()
        torch.cuda.synchronize()
        return probs

    got = _both_knobs(lib, run)
    assert torch.isfinite(got[1]).all()
    assert torch.equal(got[0], got[1]), float((got[0] - got[1]).abs().max())
