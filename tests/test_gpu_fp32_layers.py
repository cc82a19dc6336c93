"""The exact-fp32 configuration, layer by layer, and every class-tile count through a whole forward.

(1) Teacher-forced fp32 gate (tests/bf16_gate.py with dtype="f32"): every layer of the vanilla fcn_8 -- f1 .. f5, fc6, fc7,
    score5, fuse4, seg_feats, logits -- gets the DEVICE's own input, read back through model.intermediate, and must land
    within `slack` of the tensor's maximum of the float64 evaluation of that input in the fp32 path's arithmetic
    (oracle/fcn_bf16_ref.py layer_f32_ref: raw float32 kernels, BatchNorm and bias as the packer's float32-stored scale
    and shift, nothing rounded to bf16).  slack = min(2e-5, max(4 x e32, 2^-23)); e32 is measured on the reference alone,
    per layer and input: the float32-accumulating evaluation of the same input against the float64 one.  Nothing is
    stored rounded, so there is no flip count.  Class pad columns of score5 / fuse4 / seg_feats must be exact zeros; the
    probabilities are held at the suite's 1e-5 to the softmax of the oracle's logits from the device's seg_feats.
    Shapes, the smallest that reach each launch form: 1 x 32 x 32 (a 1 x 1 f5: fc6 is all padding but its centre tap,
    inside the split-K bracket); 3 x 96 x 160 (ragged tiles in every layer, a 3 x 5 fc6 map, multiply-shift constants
    that are not shifts), also with f32_lean_tile = 0 and with f32_two_level = 0; 2 x 64 x 512 (wide rows); 20 x 64 x 64
    (above the split-K brackets, partial last tiles).  The 256 x 256 geometry stays with tests/test_gpu_forward.py and
    tests/test_gpu_baseline_configs.py.

(2) Every class-tile count through a whole forward.  launch_convt dispatches on MT = ceil(C / 16) to twelve generic
    instantiations (fp32 G = 4 MT, bf16 G = 2 MT); fcn_8 at 3 x 64 x 96 -- up5 has 36 positions, up4 105, up3 351: a
    partial 64-position tile in every launch -- runs C = 1, 17, 36, 64, 65, 84, 96 in both types: the teacher-forced gate
    of the type; logits where C % 4 == 0; probabilities that sum to 1 within 1e-5; a class map that never names a class
    >= C and equals the argmax of the oracle's probabilities except where the oracle's top two are within 2e-6, on fewer
    than 1e-3 of the pixels; landmarks (n_points = 4) bit-equal to flm_decode of the probabilities output.  The oracle of
    the class-map rule is the teacher-forced one -- the float64 softmax of the type's logits arithmetic on the device's
    own seg_feats: the bf16 network is another function than the float64 fcn_ref network, and the device's seg_feats is
    what its argmax kernel was handed.  fcn_32 at 2 x 64 x 96, C = 17, 64, 96: fp32 against fcn32_predict_ref at 1e-5,
    bf16 through the free-running rounding-oracle gate of tests/test_gpu_forward.py.

Reference-side values and what the kernels measured on an MI355X.  e32: the float32 CPU evaluation's largest error against
float64 on the same input, of the tensor's maximum (range over the four shapes); "error": the kernels' largest
|got - exact64| with the slack = 4 x e32 it was gated against, at the shape where the two came closest; then the same
for 3 x 96 x 160 with f32_two_level = 0 (one fmaf chain of K per output), and the closest approach over the seven class
counts of (2) in fp32 and in bf16 (there: beyond the half step).

    layer      e32 (reference)   error / slack (kernels)           f32_two_level = 0      C = 1 .. 96, fp32             bf16
    f1         1.6 .. 2.2e-07    1.6e-07 / 6.3e-07  (1x32x32)      2.1e-07 / 8.6e-07      2.2e-07 / 8.1e-07  (C=96)     1.6e-08 / 5.1e-07  (C=64)
    f2         3.0 .. 3.6e-07    1.8e-07 / 1.3e-06  (3x96x160)     9.5e-07 / 1.3e-06      1.6e-07 / 1.1e-06  (C=17)     7.5e-08 / 5.7e-07  (C=64)
    f3         3.0 .. 3.9e-07    2.1e-07 / 1.2e-06  (20x64x64)     4.9e-07 / 1.3e-06      1.9e-07 / 1.2e-06  (C=96)     7.5e-08 / 6.1e-07  (C=65)
    f4         2.8 .. 4.6e-07    1.9e-07 / 1.1e-06  (2x64x512)     4.6e-07 / 1.4e-06      1.9e-07 / 1.0e-06  (C=36)     2.9e-08 / 7.1e-07  (C=84)
    f5         2.5e-07 .. 1e-06  1.5e-07 / 1.0e-06  (20x64x64)     3.8e-07 / 7.4e-07      1.7e-07 / 7.7e-07  (C=84)     8.4e-09 / 8.5e-07  (C=17)
    fc6        2.3 .. 4.1e-07    1.5e-07 / 9.3e-07  (20x64x64)     5.7e-07 / 1.6e-06      1.5e-07 / 7.9e-07  (C=17)     3.5e-08 / 6.6e-07  (C=17)
    fc7        2.8 .. 4.8e-07    1.6e-07 / 1.1e-06  (3x96x160)     3.7e-07 / 9.6e-07      1.7e-07 / 9.8e-07  (C=84)     4.2e-08 / 6.2e-07  (C=1)
    score5     2.7 .. 3.5e-07    1.9e-07 / 1.1e-06  (20x64x64)     2.9e-07 / 1.3e-06      2.1e-07 / 1.0e-06  (C=96)     1.7e-07 / 4.7e-07  (C=17)
    fuse4      3.9 .. 5.7e-07    2.3e-07 / 2.1e-06  (2x64x512)     5.2e-07 / 1.9e-06      2.2e-07 / 1.1e-06  (C=1)      1.7e-07 / 6.0e-07  (C=17)
    seg_feats  1.5 .. 4.4e-07    1.7e-07 / 6.0e-07  (1x32x32)      2.7e-07 / 1.2e-06      1.8e-07 / 9.5e-07  (C=17)     2.3e-07 / 6.2e-07  (C=96)
    logits     3.7 .. 7.3e-07    3.5e-07 / 1.7e-06  (20x64x64)     3.7e-07 / 1.9e-06      3.3e-07 / 8.1e-07  (C=36)     4.1e-07 / 7.4e-07  (C=64)
    probs      max-abs error 2.4 .. 5.0e-07 (two_level = 0: 6.3e-07; class counts 2.3 .. 6.7e-07) against the bar of 1e-5

The default kernels use 0.11 to 0.28 of their allowance at every layer and shape; the 2e-5 cap never binds.  f32_lean_tile
= 0 gives the bits of the default (the same figures).  f32_two_level = 0 PASSES the same gate, as a valid fp32 evaluation
must; it comes closest at f2 (K = 576 in one chain: 0.72 of the allowance).  The class map of every count equals the
oracle's argmax on all 22,464 pixels (at most 1.8e-4 of the oracle's pixels have a top-2 gap below 2e-6; the free-running
float64 oracle on the same inputs: at most 1.8e-4 too), no class >= C is named, and the landmarks are the decode of the
probabilities bit for bit.  fcn_32: fp32 probabilities 0.7 .. 1.8e-07 from the oracle; bf16 mean distance to the rounding
oracle, kernels / reference pair: C = 17 5.8e-5 / 5.4e-5, C = 64 6.5e-6 / 1.2e-5, C = 96 9.55e-6 / 9.57e-6.

Fault injection (scratch builds, not committed; wrong values only).  (a) The softmax's class mask of the generic layouts
off by one in bf16 (FLM_CVALID as `16 m + 4 q + e < C + 1` in the maximum and the sum): the probabilities of bf16 C = 17
are 3.7e-2 off and sum to 1 within 9.6e-2 only, C = 1 0.96 off, fcn_32 C = 17 sums to 1 within 7.6e-2 -- while every layer up to the
logits passes.  (b) The far-far tap of phase 0 zeroed in pack_convt_kernel for the generic layouts with MT >= 3: the
integer up5 check fails at its second grid for C = 36, 48, 52, 64, 65, 80, 84, 96, and the forwards of those counts fail
at fuse4 (0.14 .. 0.30 of the maximum against slacks near 1e-6), seg_feats, logits and probabilities in both types,
fcn_32 at C = 64, 96 with 1.6e-2 .. 1.9e-2.  The suite as it stood before these tests (120 GPU tests) passes with both
faults in the build: it ran no generic class count in bf16 and none with MT >= 3.  (Its fp32 cases at C = 5 and 21 and
its 68-class cases hold the probabilities at 1e-5, so the same two faults placed in fp32 at those counts would have
been caught there; that was not run.)
"""
import numpy as np
import pytest
import torch

from bf16_gate import check_layers

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def flm():
    import flm_amd
    from flm_amd import _lib
    _lib.load()
    return flm_amd


_WEIGHTS = {}


def _weights(c, fcn32=False):
    from flm_amd.weights import synth_fcn32_weights, synth_fcn8_weights
    if (c, fcn32) not in _WEIGHTS:
        _WEIGHTS.clear()                       # one class count at a time: 470 MB of float32 each
        _WEIGHTS[(c, fcn32)] = (synth_fcn32_weights if fcn32 else synth_fcn8_weights)(c, seed=2)
    return _WEIGHTS[(c, fcn32)]


def _forward_and_gate(model, params, crops, dtype, label, logits=True):
    n = crops.shape[0]
    xd = torch.from_numpy(crops).cuda()
    probs = model.forward_device(xd, "probs").cpu().numpy()
    lg = model.forward_device(xd, "logits").cpu().numpy() if logits else None
    torch.cuda.synchronize()
    if logits:
        for k in ("f5", "fc7", "seg_feats"):   # the two forwards wrote the same bits into their workspaces
            assert torch.equal(model.intermediate(k, n, "probs"), model.intermediate(k, n, "logits")), k
    reports = check_layers(model, params, crops, n, "probs", logits=lg, probs=probs, label=label, dtype=dtype)
    return xd, probs, reports


FP32_CASES = [(1, 32, 32, None), (3, 96, 160, None), (2, 64, 512, None), (20, 64, 64, None),
              (3, 96, 160, "f32_lean_tile"), (3, 96, 160, "f32_two_level")]


@pytest.mark.parametrize("n,h,w,knob_off", FP32_CASES)
def test_fp32_layers_teacher_forced(flm, n, h, w, knob_off):
    from flm_amd import _lib
    from flm_amd.networks import LANDMARKS_MODELS
    params = _weights(68)
    model = LANDMARKS_MODELS["fcn_8"](68, input_height=h, input_width=w)
    model.load_weights(params)
    crops = np.random.default_rng(100 + h + w).integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    with _lib.tuning(**({knob_off: 0} if knob_off else {})):
        _forward_and_gate(model, params, crops, "f32", "fp32 %dx%dx%d%s" % (n, h, w, " %s=0" % knob_off if knob_off else ""))


# ---- every class-tile count through a whole forward --------------------------------------------------------------

FCN8_CLASS_COUNTS = [1, 17, 36, 64, 65, 84, 96]


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("c", FCN8_CLASS_COUNTS)
def test_fcn8_generic_class_counts(flm, c, dtype):
    from flm_amd.networks import LANDMARKS_MODELS
    from flm_amd.utils.metrics import decode_device
    from oracle import fcn_bf16_ref as B
    n, h, w = 3, 64, 96
    params = _weights(c)
    model = LANDMARKS_MODELS["fcn_8"](c, input_height=h, input_width=w, dtype=dtype)
    model.load_weights(params)
    crops = np.random.default_rng(300 + c).integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    label = "%s C=%d %dx%dx%d" % (dtype, c, n, h, w)
    xd, probs, _ = _forward_and_gate(model, params, crops, dtype, label, logits=(c % 4 == 0))
    assert probs.shape == (n, (h + 8) * (w + 8), c) and np.isfinite(probs).all()
    assert np.abs(probs.sum(-1) - 1).max() < 1e-5
    # class map: the argmax of the oracle's probabilities from the device's own seg_feats, except at the oracle's ties
    cm = model.forward_device(xd, "classmap").cpu().numpy()
    torch.cuda.synchronize()
    seg = model.intermediate("seg_feats", n, "classmap").cpu().numpy().astype(np.float64)
    assert cm.min() >= 0 and cm.max() < c, (cm.min(), cm.max())
    pr = B.softmax_ref(B.layer_bf16_ref("logits", seg, params, fp32=(dtype == "f32"))[0]).reshape(n, h + 8, w + 8, c)
    diff = cm != pr.argmax(-1)
    srt = np.sort(pr, axis=-1)
    gap = srt[..., -1] - srt[..., -2] if c > 1 else np.ones(pr.shape[:3])
    print("%s class map: %d of %d pixels differ from the oracle's argmax; %.3g of the oracle's pixels have a top-2 gap below 2e-6"
          % (label, diff.sum(), diff.size, (gap < 2e-6).mean()))
    assert (gap < 2e-6).mean() < 1e-3, "the inputs sit on ties: pick another seed"
    if diff.any():
        assert gap[diff].max() < 2e-6, ("class map differs away from ties", float(gap[diff].max()))
    assert diff.mean() < 1e-3
    # landmarks: these counts have no candidate path -- the decode of the probabilities, bit for bit
    lm = model.forward_device(xd, "landmarks", n_points=4)
    exp = decode_device(torch.from_numpy(probs).cuda().view(n, h + 8, w + 8, c), n_points=4)
    torch.cuda.synchronize()
    assert torch.equal(lm, exp) or np.array_equal(lm.cpu().numpy(), exp.cpu().numpy(), equal_nan=True), label


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("c", [17, 64, 96])
def test_fcn32_generic_class_counts(flm, c, dtype):
    """The 64 x 64 stride-32 transposed conv on the generic class layouts."""
    from flm_amd.networks import LANDMARKS_MODELS
    from oracle import fcn_ref
    from test_gpu_forward import _gate_against_the_rounding_oracle
    n, h, w = 2, 64, 96
    params = _weights(c, fcn32=True)
    model = LANDMARKS_MODELS["fcn_32"](c, input_height=h, input_width=w, dtype=dtype)
    model.load_weights(params)
    img = np.random.default_rng(400 + c).integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    got = model.forward_device(torch.from_numpy(img).cuda(), "probs").cpu().numpy()
    assert got.shape == (n, (h + 32) * (w + 32), c) and np.isfinite(got).all()
    assert np.abs(got.sum(-1) - 1).max() < 1e-5
    if dtype == "f32":
        exp = fcn_ref.fcn32_predict_ref(np.stack([fcn_ref.get_image_array_ref(im) for im in img]), params)
        err = np.abs(got - exp).max()
        print("fcn_32 f32 C=%d: probabilities max-abs error %.3g (bar 1e-5)" % (c, err))
        assert err <= 1e-5, (c, err)
    else:
        _gate_against_the_rounding_oracle("fcn_32 C=%d %s" % (c, (n, h, w)), got, img, params, "vanilla", True)
