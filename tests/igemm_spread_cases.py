"""Cases and runner shared by tests/test_gpu_igemm_request_spread.py and tests/golden/make_igemm_request_spread_golden.py.

A case is (model name, weight synthesiser, seed, faces, H, W).  run_case() does one fp32 forward to landmarks
(n_points = 4) and returns the landmarks and every named workspace tensor the model's layout holds."""
import hashlib

import numpy as np

NAMES = ("f1", "f2", "f3", "f4", "f5", "fc6", "fc7", "score5", "fuse4", "seg_feats")

# fcn_8, fc6's map is H/32 x W/32:
#   64x64 x 1    one tile per layer beyond enc2, the 8-slice split-K bracket of fc6 / fc7 / enc4 / enc5
#   64x64 x 3    the same bracket, every layer beyond enc3 one partial tile (fc6: 3 faces x 4 positions = 12 rows)
#   64x64 x 20   above every split-K bracket; 80 rows of fc6: a full 64-row tile and a partial one, tiles straddle positions
#   96x64 x 2    a 3x2 map: not square, the row-major layers take the guarded set-up (tiles are not two whole map rows)
#   256x256 x 2  the real geometry: the pooled layers on the lean path with all taps proven in bounds
# the other encoders (strides, residual adds, ReLU6 in the write-out) at 64x64 x 2
CASES = [
    ("fcn_8", "synth_fcn8_weights", 2, 1, 64, 64),
    ("fcn_8", "synth_fcn8_weights", 2, 3, 64, 64),
    ("fcn_8", "synth_fcn8_weights", 2, 20, 64, 64),
    ("fcn_8", "synth_fcn8_weights", 2, 2, 96, 64),
    ("fcn_8", "synth_fcn8_weights", 2, 2, 256, 256),
    ("fcn_8_vgg", "synth_vgg_weights", 5, 2, 64, 64),
    ("fcn_8_mobilenet", "synth_mobilenet_weights", 5, 2, 64, 64),
    ("fcn_8_resnet50", "synth_resnet50_weights", 5, 2, 64, 64),
]


def case_id(case):
    name, _, _, n, h, w = case
    return "%s-%dx%d-b%d" % (name, h, w, n)


def digest(t):
    """SHA-1 of a tensor's bytes as 20 uint8: equal digests = equal bits."""
    return np.frombuffer(hashlib.sha1(t.contiguous().cpu().numpy().tobytes()).digest(), dtype=np.uint8).copy()


def run_case(case):
    import torch
    from flm_amd import weights
    from flm_amd.networks import LANDMARKS_MODELS
    name, synth, seed, n, h, w = case
    model = LANDMARKS_MODELS[name](68, input_height=h, input_width=w)
    model.load_weights(getattr(weights, synth)(68, seed=seed))
    xd = torch.from_numpy(np.random.default_rng(1000 * n + h).integers(0, 256, (n, h, w, 3), dtype=np.uint8)).cuda()
    lm = model.forward_device(xd, "landmarks", n_points=4).clone()
    torch.cuda.synchronize()
    out = {"landmarks": lm}
    for k in NAMES:
        try:
            out[k] = model.intermediate(k, n, "landmarks", 4).clone()
        except KeyError:
            if name == "fcn_8":
                raise
    return out
