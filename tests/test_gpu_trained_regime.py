"""Every BatchNorm epilogue under a trained checkpoint's statistics: negative, zero, large and small folded scales.

Every other GPU test builds its network from the synth weights (flm_amd/weights.py), whose folded scale gamma / sqrt(var + 1e-3)
is a positive number between 0.4 and 2.1.  Under a positive scale an epilogue that takes the 2x2 maximum before the affine,
or that drops the sign of the scale, gives the right bits (tests/test_trained_regime_host.py asserts that equality on the
oracle and that the same epilogues fail the gate below by five to seven decades under this regime): no GPU test could
see a sign-dependent regression in flm_enc1.hip, flm_conv3_halo.hip, flm_igemm.hip (igemm_kernel and its LEAN form,
splitk_reduce*), flm_igemm_bf16.hip (128- and 256-row tiles, LDS-DMA and mfma16 forms), flm_mobile.hip (mb_conv1, depthwise,
the pointwise pair, rn_conv1) or the residual epilogue.  Here the three BatchNorm encoders run on tests/trained_regime.py's
transform of their synth sets (68 classes; vanilla seed 2, MobileNet 5, ResNet50 6), loaded through model.load_weights so
that the library's own pack folds them: per layer, channels c % 4 == 1 have a negative gamma, c % 16 == 6 gamma = 0 with
beta = +0.5 / -0.5 / +6.5 in turn, c % 8 == 3 a running variance of 1e-4 .. 1e-2 (|scale| 9.5 .. 30 x gamma), c % 8 == 7 one of
16 .. 100 (0.10 .. 0.25 x gamma), the upper half of the last two negated as well.

(a) Vanilla fcn_8, teacher-forced through tests/bf16_gate.py check_layers, criteria unchanged: slack = min(2e-5, max(4 x e32,
    2^-23)) with e32 from the reference alone; in bf16 the half step and the flip count; pad columns zero; probabilities at
    1e-5.  f1 .. f5, the head, logits and probs, in both types at 1 x 32 x 32 (fp32: the affine of enc3 .. enc5 happens in
    splitk_reduce*), 3 x 96 x 160 and 20 x 64 x 64; fp32 at 3 x 96 x 160 also with f32_lean_tile = 0 and with f32_two_level = 0.
(b) MobileNet and ResNet50 fcn_8, encoder layers only (head=False), at 1 x 32 x 32 and 3 x 64 x 96 in both types: ReLU6 with
    negative and zero scales, the shortcut BatchNorm with no ReLU, the residual add on negative-scale channels, the strided
    1x1 convs.  At 3 x 64 x 96 in fp32 also f32_lean_tile = 0: every act<i> the default's bit for bit.
(c) Every "same bits" knob of the bf16 BatchNorm layers on the vanilla model: f1 .. f5 must be the default run's bit for
    bit.  What the launchers' conditions select (flm_igemm.hip launch_igemm, flm_conv3_halo.hip launch_conv3_halo_bf16,
    flm_igemm_bf16.hip launch_igemm_bf16_big):
      the halo kernel takes enc2 (the only 64-channel 3x3 input) when n (h/32)(w/32) 2 >= 1024, or when forced (knob 2) on
      any f1 map of whole 16 x 16 tiles; the 256-row tiles take a stride-1 layer without split-K when ceil(M / 256) x
      ceil(cout / 256) >= 192 and cout > 128, or when forced (2): then also enc2 on the 256 x 128 shape.  In bf16 enc3 (two
      64-element chunks per tap) never splits K; enc4 / enc5 split at all three shapes below unless noted.
      3 x 96 x 160   default: 128-row tiles everywhere (enc2: 90 halo tiles; enc3: 12 tiles of 256 rows).  bf16_conv3_halo = 2
                     puts enc2 on the halo kernel, bf16_big_tiles = 2 enc2 on 256 x 128 and enc3 on 256 x 256 tiles.
      20 x 64 x 64   the same selections (160 halo tiles; enc3: 20 tiles).
      48 x 128 x 128 added: the smallest batch of 128 x 128 faces at which the DEFAULT takes the halo kernel (enc2, 1536
                     tiles) and the 256 x 256 tiles (enc3, 192 tiles); bf16_big_tiles = 2 adds enc4 (no split-K at 48
                     faces), bf16_conv3_halo = 0 / bf16_big_tiles = 0 take them away.
    bf16_group_n, bf16_lds_dma and bf16_mfma16 act on the 256-row tiles only and bf16_halo_mfma16 on the halo kernel only:
    alone they select nothing at the two small shapes, so each also runs together with the knob that forces its kernel.
    bf16_group_n = 8 is capped at the layer's count of N tiles, which is 1 for every BatchNorm layer of this model (cout <=
    256): it regroups fc6 / fc7 only and proves nothing about a BatchNorm epilogue at any shape; it runs because the
    launch arithmetic it feeds (launch_big_t) is the one these layers go through.
(d) The zero class, exactly: in every case of (a) and (b), for every layer without a shortcut input, the device's zero-gamma
    channels equal act(float32(beta)) at every pixel (bf16: its rounding) -- fmaf(acc, 0, shift) has no rounding.
(e) Free running through the public path: model.predict in fp32 at 2 x 64 x 96 on the three encoders against
    fcn_ref.fcn8_predict_ref in float64 (Keras's unfused BatchNorm: shares no fold with the packer) at the suite's 1e-5;
    bf16 on the vanilla model through tests/test_gpu_forward.py's gate against the rounding oracle.

No wrong kernel is run on the GPU: what the gate catches is shown on the oracle, in tests/test_trained_regime_host.py.

Measured on an MI355X (one run; the bars are the formulas above, not these figures).  Per encoder, type and layer group: the
reference-side e32 range over the group's layers and the case's shapes; the kernels' largest error (bf16: beyond the half
step) against the slack it was gated with, at the layer and shape where the two came closest; for bf16 the flip count
against its allowance where that came closest.

    encoder   type layer group                        e32 (reference)       error / slack (kernels)
    vanilla   f32  f1                                 1.4e-07 .. 2.4e-07    1.4e-07 / 5.6e-07  (1x32x32)
    vanilla   f32  f2                                 3.0e-07 .. 4.5e-07    2.3e-07 / 1.5e-06  (3x96x160)
    vanilla   f32  f3                                 3.1e-07 .. 4.0e-07    1.9e-07 / 1.2e-06  (1x32x32)
    vanilla   f32  f4                                 2.5e-07 .. 3.9e-07    2.1e-07 / 1.2e-06  (3x96x160)
    vanilla   f32  f5                                 2.2e-07 .. 4.9e-07    2.4e-07 / 9.6e-07  (3x96x160)
    vanilla   f32  fc6                                2.8e-07 .. 3.1e-07    1.6e-07 / 1.1e-06  (20x64x64)
    vanilla   f32  fc7                                2.4e-07 .. 5.4e-07    1.7e-07 / 1.1e-06  (20x64x64)
    vanilla   f32  score5                             2.4e-07 .. 5.9e-07    2.3e-07 / 1.1e-06  (20x64x64)
    vanilla   f32  fuse4                              4.6e-07 .. 5.6e-07    1.7e-07 / 1.8e-06  (3x96x160)
    vanilla   f32  seg_feats                          2.5e-07 .. 4.2e-07    2.0e-07 / 1.0e-06  (3x96x160)
    vanilla   f32  logits                             3.5e-07 .. 5.3e-07    3.4e-07 / 1.4e-06  (1x32x32)
    vanilla   f32  f1 .. f5, f32_two_level = 0        2.3e-07 .. 3.8e-07    1.2e-06 / 1.5e-06  (f2, 3x96x160; f1 2.3e-07 / 9.6e-07, f3 5.2e-07 / 1.4e-06, f4 4.2e-07 / 1.2e-06, f5 2.7e-07 / 9.3e-07)
    vanilla   bf16 f1                                 1.1e-07 .. 1.5e-07    1.3e-08 / 4.5e-07  (20x64x64)   flips 9 / 40 allowed of 737280 (3x96x160)
    vanilla   bf16 f2                                 1.6e-07 .. 2.1e-07    4.1e-08 / 8.3e-07  (20x64x64)   flips 28 / 72 allowed of 655360 (20x64x64)
    vanilla   bf16 f3                                 1.7e-07 .. 2.2e-07    4.7e-08 / 6.9e-07  (3x96x160)   flips 19 / 48 allowed of 327680 (20x64x64)
    vanilla   bf16 f4                                 1.7e-07 .. 2.3e-07    5.3e-08 / 6.9e-07  (3x96x160)   flips 5 / 8 allowed of 81920 (20x64x64)
    vanilla   bf16 f5                                 2.3e-07 .. 4.9e-07    4.6e-08 / 9.0e-07  (20x64x64)   flips 2 / 8 allowed of 20480 (20x64x64)
    vanilla   bf16 fc6                                1.2e-07 .. 2.3e-07    4.2e-08 / 8.2e-07  (3x96x160)   flips 11 / 32 allowed of 184320 (3x96x160)
    vanilla   bf16 fc7                                1.3e-07 .. 2.9e-07    2.9e-08 / 5.3e-07  (3x96x160)   flips 18 / 44 allowed of 184320 (3x96x160)
    vanilla   bf16 score5                             1.8e-07 .. 2.9e-07    2.1e-07 / 8.4e-07  (20x64x64)
    vanilla   bf16 fuse4                              1.8e-07 .. 2.2e-07    1.8e-07 / 8.8e-07  (20x64x64)
    vanilla   bf16 seg_feats                          8.3e-08 .. 2.1e-07    2.4e-07 / 5.5e-07  (20x64x64)
    vanilla   bf16 logits                             1.6e-07 .. 2.1e-07    3.1e-07 / 7.9e-07  (3x96x160)
    mobilenet f32  conv1 (3x3 s2)                     1.9e-07 .. 3.3e-07    2.9e-07 / 7.5e-07  (conv1, 1x32x32)
    mobilenet f32  depthwise s1                       6.2e-08 .. 3.0e-07    1.6e-07 / 6.3e-07  (conv_dw_3, 1x32x32)
    mobilenet f32  pointwise 1 (pixel pairs)          2.9e-07 .. 3.5e-07    2.8e-07 / 1.1e-06  (conv_pw_1, 1x32x32)
    mobilenet f32  depthwise s2                       1.3e-07 .. 3.4e-07    1.9e-07 / 5.8e-07  (conv_dw_4, 1x32x32)
    mobilenet f32  pointwise 2..13                    3.7e-07 .. 1.6e-06    3.6e-07 / 1.6e-06  (conv_pw_2, 3x64x96)
    mobilenet bf16 conv1 (3x3 s2)                     1.9e-07 .. 3.3e-07    3.5e-08 / 1.3e-06  (conv1, 3x64x96)            flips 5 / 20 allowed of 147456 (conv1, 3x64x96)
    mobilenet bf16 depthwise s1                       5.8e-08 .. 2.7e-07    3.6e-08 / 7.1e-07  (conv_dw_3, 1x32x32)        flips 2 / 8 allowed of 147456 (conv_dw_3, 3x64x96)
    mobilenet bf16 pointwise 1 (pixel pairs)          1.7e-07 .. 2.5e-07    4.0e-09 / 1.0e-06  (conv_pw_1, 3x64x96)        flips 2 / 12 allowed of 294912 (conv_pw_1, 3x64x96)
    mobilenet bf16 depthwise s2                       1.3e-07 .. 3.3e-07    2.7e-08 / 1.2e-06  (conv_dw_4, 3x64x96)        flips 2 / 12 allowed of 36864 (conv_dw_4, 3x64x96)
    mobilenet bf16 pointwise 2..13                    1.5e-07 .. 7.6e-07    1.3e-07 / 1.9e-06  (conv_pw_13, 3x64x96)       flips 2 / 8 allowed of 147456 (conv_pw_2, 3x64x96)
    resnet50  f32  conv1 (7x7 s2)                     3.6e-07 .. 4.4e-07    3.6e-07 / 1.4e-06  (conv1, 1x32x32)
    resnet50  f32  branch1 (shortcut 1x1, no ReLU)    3.2e-07 .. 3.3e-07    2.6e-07 / 1.3e-06  (res2a_branch1, 3x64x96)
    resnet50  f32  branch2a 1x1                       2.1e-07 .. 1.2e-06    2.6e-07 / 1.4e-06  (res3c_branch2a, 1x32x32)
    resnet50  f32  branch2b 3x3                       2.0e-07 .. 9.2e-07    2.5e-07 / 8.7e-07  (res5c_branch2b, 3x64x96)
    resnet50  f32  branch2c 1x1 + residual            3.9e-08 .. 2.3e-07    4.3e-08 / 1.7e-07  (res5a_branch2c, 1x32x32)
    resnet50  f32  branch1 (shortcut 1x1, no ReLU) s2 2.2e-07 .. 7.4e-07    2.1e-07 / 8.9e-07  (res3a_branch1, 3x64x96)
    resnet50  f32  branch2a 1x1 s2                    2.5e-07 .. 5.1e-07    2.3e-07 / 1.0e-06  (res3a_branch2a, 3x64x96)
    resnet50  bf16 conv1 (7x7 s2)                     3.6e-07 .. 4.4e-07    9.3e-08 / 1.4e-06  (conv1, 1x32x32)            flips 4 / 16 allowed of 16384 (conv1, 1x32x32)
    resnet50  bf16 branch1 (shortcut 1x1, no ReLU)    1.0e-07 .. 1.3e-07    1.2e-08 / 5.2e-07  (res2a_branch1, 3x64x96)    flips 7 / 24 allowed of 264960 (res2a_branch1, 3x64x96)
    resnet50  bf16 branch2a 1x1                       1.0e-07 .. 4.4e-07    6.6e-08 / 9.9e-07  (res3c_branch2a, 3x64x96)   flips 4 / 8 allowed of 36864 (res3c_branch2a, 3x64x96)
    resnet50  bf16 branch2b 3x3                       7.7e-08 .. 3.5e-07    1.1e-07 / 9.7e-07  (res4c_branch2b, 3x64x96)   flips 2 / 8 allowed of 66240 (res2c_branch2b, 3x64x96)
    resnet50  bf16 branch2c 1x1 + residual            2.9e-08 .. 1.0e-07    1.4e-08 / 1.8e-07  (res2b_branch2c, 3x64x96)   flips 3 / 8 allowed of 264960 (res2b_branch2c, 3x64x96)
    resnet50  bf16 branch1 (shortcut 1x1, no ReLU) s2 1.4e-07 .. 2.9e-07    7.4e-08 / 1.1e-06  (res4a_branch1, 3x64x96)    flips 7 / 8 allowed of 36864 (res5a_branch1, 3x64x96)
    resnet50  bf16 branch2a 1x1 s2                    1.8e-07 .. 2.2e-07    1.1e-08 / 8.6e-07  (res3a_branch2a, 3x64x96)   flips 4 / 12 allowed of 36864 (res3a_branch2a, 3x64x96)
    probs     teacher-forced, vanilla: fp32 2.1e-07 .. 3.9e-07, bf16 1.2e-07 .. 3.9e-07 against the bar of 1e-5
    predict   fp32, free running against float64 fcn_ref: vanilla 3.6e-07, MobileNet 1.5e-07, ResNet50 1.2e-06 against 1e-5;
              bf16 vanilla: mean distance to the rounding oracle 2.5e-05 (float32- against float64-accumulating oracle
              1.3e-05: bar 4 x; to the fp32 oracle 5.8e-05), max 2.1e-03 against 4 x 2.1e-03

Every layer of every case passes on the unmodified kernels, and the e32 ranges are the synth weights' (tests/test_gpu_encoder_layers.py,
tests/test_gpu_fp32_layers.py): the regime moves no yardstick.  The largest share of an error allowance is 0.77 (fp32 vanilla f2 with
f32_two_level = 0: K = 576 in one chain, as under the synth weights), 0.45 among the default kernels (bf16 vanilla seg_feats at
20 x 64 x 64) and 0.38 among their BatchNorm layers (fp32 MobileNet conv1 at 1 x 32 x 32); the 2e-5 cap never binds (largest slack 6.6e-06).  The flip count comes closest at ResNet50's res5a_branch1 in bf16: 7 of 36864 elements against
the floor of 8.  f32_lean_tile = 0 gates with the default's figures on the vanilla model and changes no bit of any of the 27 / 54
act tensors; all 12 knob settings of (c) leave f1 .. f5 bit for bit at the three shapes; the zero class is exact in all 19
gated cases (5 / 27 / 37 layers each) and after the knobs of (c).  Nothing to fix in a kernel, the packer or the oracle.

(A negative "error" beyond the half step means every element lay inside it; it is printed as 0.)
"""
import json

import numpy as np
import pytest
import torch

import enc_chain_cases as cases
import trained_regime as T
from bf16_gate import check_layers

pytestmark = pytest.mark.gpu

MODELS = {"vanilla": "fcn_8", "mobilenet": "fcn_8_mobilenet", "resnet50": "fcn_8_resnet50"}
SMALL, LARGE = (1, 32, 32), (3, 64, 96)
INPUT_SEED = 11

_PARAMS = {}


@pytest.fixture(scope="module")
def flm():
    import flm_amd
    from flm_amd import _lib
    _lib.load()
    yield flm_amd
    _PARAMS.clear()


def _params(enc):
    """(params2, classes) of `enc`, built once per module."""
    if enc not in _PARAMS:
        if enc == "vanilla":
            from flm_amd.weights import synth_fcn8_weights
            base = synth_fcn8_weights(68, seed=2)
        else:
            base = cases.encoder_params(enc, keep=2)     # seeds 5 (MobileNet) and 6 (ResNet50)
        _PARAMS[enc] = T.trained_regime(base)
    return _PARAMS[enc]


def _crops(n, h, w):
    return np.random.default_rng(INPUT_SEED).integers(0, 256, (n, h, w, 3), dtype=np.uint8)


def _model(enc, dtype, h, w):
    from flm_amd.networks import LANDMARKS_MODELS
    model = LANDMARKS_MODELS[MODELS[enc]](68, input_height=h, input_width=w, dtype=dtype)
    model.load_weights(_params(enc)[0])
    return model


def _bn_layers(enc):
    """(device tensor name, conv, bn, relu, has a shortcut input) of every BatchNorm layer of `enc`, in network order."""
    from oracle import fcn_bf16_ref as B
    if enc == "vanilla":
        return [("f%d" % i, "enc%d" % i, "enc%d" % i, 1, False) for i in range(1, 6)]
    return [("act%d" % i, st.name, st.kw["bn"], st.relu, len(st.inputs) > 1)
            for i, st in enumerate(B.ENCODER_CHAINS[enc]) if st.op == "conv"]


def _check_zero_class(model, enc, n, label):
    """(d): exact equality on the zero-gamma channels of every layer without a shortcut input."""
    p2, classes = _params(enc)
    bad, checked = [], 0
    for name, conv, bn, relu, shortcut in _bn_layers(enc):
        if shortcut:
            continue
        z = classes[bn] == T.ZERO
        got = model.intermediate(name, n, "probs")[..., torch.from_numpy(z).cuda()].float().cpu().numpy().astype(np.float64)
        exp = T.zero_class_expected(p2[bn + "/beta"][z], relu, model.dtype == "bf16")
        assert got.shape[-1] == exp.size >= 2 and got.size >= exp.size
        checked += 1
        if not (got == exp).all():
            bad.append((name, conv, int((got != exp).sum()), got.size, float(np.abs(got - exp).max())))
    print("%s zero class: %d layers, %d differ from act(float32(beta))" % (label, checked, len(bad)))
    assert checked == {"vanilla": 5, "mobilenet": 27, "resnet50": 37}[enc]
    assert not bad, (label, bad)


def _record(label, reports):
    print("TRGATE " + json.dumps(dict(case=label, reports={k: {a: b for a, b in r.items() if a != "ok"} for k, r in reports.items()})))


# ---- (a) vanilla, whole network -----------------------------------------------------------------------------------------

VANILLA_CASES = [(dt, shape, None) for dt in ("f32", "bf16") for shape in ((1, 32, 32), (3, 96, 160), (20, 64, 64))]
VANILLA_CASES += [("f32", (3, 96, 160), "f32_lean_tile"), ("f32", (3, 96, 160), "f32_two_level")]


@pytest.mark.parametrize("dtype,shape,knob_off", VANILLA_CASES,
                         ids=["%s-%dx%dx%d%s" % (d, *s, "-%s=0" % k if k else "") for d, s, k in VANILLA_CASES])
def test_vanilla_layers_teacher_forced(flm, dtype, shape, knob_off):
    from flm_amd import _lib
    n, h, w = shape
    p2, _ = _params("vanilla")
    model = _model("vanilla", dtype, h, w)
    crops = _crops(n, h, w)
    xd = torch.from_numpy(crops).cuda()
    label = "fcn_8 %s %dx%dx%d%s" % (dtype, n, h, w, " %s=0" % knob_off if knob_off else "")
    with _lib.tuning(**({knob_off: 0} if knob_off else {})):
        probs = model.forward_device(xd, "probs").cpu().numpy()
        logits = model.forward_device(xd, "logits").cpu().numpy()
        torch.cuda.synchronize()
    for k in ("f5", "fc7", "seg_feats"):       # the two forwards wrote the same bits into their workspaces
        assert torch.equal(model.intermediate(k, n, "probs"), model.intermediate(k, n, "logits")), k
    reports = check_layers(model, p2, crops, n, "probs", logits=logits, probs=probs, label=label, dtype=dtype)
    assert list(reports) == ["f1", "f2", "f3", "f4", "f5", "fc6", "fc7", "score5", "fuse4", "seg_feats", "logits", "probs"]
    for k in ("f1", "f2", "f3", "f4", "f5"):
        assert reports[k]["nonzero"] >= 0.25, (k, reports[k]["nonzero"])
    _check_zero_class(model, "vanilla", n, label)
    _record(label, reports)


# ---- (b) MobileNet and ResNet50, encoder layers ----------------------------------------------------------------------------

ENC_CASES = [(enc, dt, shape, None) for enc in ("mobilenet", "resnet50") for dt in ("f32", "bf16") for shape in (SMALL, LARGE)]
ENC_CASES += [(enc, "f32", LARGE, "f32_lean_tile=0") for enc in ("mobilenet", "resnet50")]
ENC_CASES.sort(key=lambda c: c[0])


@pytest.mark.parametrize("enc,dtype,shape,variant", ENC_CASES,
                         ids=["%s-%s-%dx%dx%d%s" % (e, d, *s, "-" + v if v else "") for e, d, s, v in ENC_CASES])
def test_encoder_layers_teacher_forced(flm, enc, dtype, shape, variant):
    from flm_amd import _lib
    from oracle import fcn_bf16_ref as B
    n, h, w = shape
    p2, _ = _params(enc)
    model = _model(enc, dtype, h, w)
    crops = _crops(n, h, w)
    xd = torch.from_numpy(crops).cuda()
    label = "%s %s %dx%dx%d%s" % (MODELS[enc], dtype, n, h, w, " " + variant if variant else "")
    chain = B.ENCODER_CHAINS[enc]
    assert model.encoder_layer_names() == tuple(st.name for st in chain)
    if variant == "f32_lean_tile=0":             # "same bits" under negative, zero and large scales
        acts = lambda: [model.intermediate("act%d" % i, n, "probs").clone() for i in range(len(chain))]
        model.forward_device(xd, "probs")
        a0 = acts()
        with _lib.tuning(f32_lean_tile=0):
            model.forward_device(xd, "probs")
            a1 = acts()
        torch.cuda.synchronize()
        diff = [chain[i].name for i, (u, v) in enumerate(zip(a0, a1)) if not torch.equal(u, v)]
        print("%s: %d of %d act tensors differ from the default's" % (label, len(diff), len(a0)))
        assert not diff, diff
        assert all(bool(torch.isfinite(a).all()) and a.abs().max() > 0 for a in a0)
        return
    model.forward_device(xd, "probs")
    torch.cuda.synchronize()
    reports = check_layers(model, p2, crops, n, "probs", label=label, dtype=dtype, encoder=enc, head=False)
    assert list(reports) == [st.name for st in chain]      # no layer skipped
    for st in chain:
        if st.op == "conv":
            assert reports[st.name]["nonzero"] >= 0.25, (st.name, reports[st.name]["nonzero"])
        if st.relu == 2 and shape == LARGE:
            assert reports[st.name]["at6"] > 0, st.name
    _check_zero_class(model, enc, n, label)
    _record(label, reports)


# ---- (c) the "same bits" knobs of the bf16 BatchNorm layers ------------------------------------------------------------------

KNOBS = [dict(bf16_conv3_halo=0), dict(bf16_conv3_halo=2), dict(bf16_big_tiles=0), dict(bf16_big_tiles=2), dict(bf16_group_n=8),
         dict(bf16_lds_dma=0), dict(bf16_mfma16=0), dict(bf16_halo_mfma16=0),
         # ... and on the kernel each of the last four acts on, where the default does not select it
         dict(bf16_big_tiles=2, bf16_group_n=8), dict(bf16_big_tiles=2, bf16_lds_dma=0), dict(bf16_big_tiles=2, bf16_mfma16=0),
         dict(bf16_conv3_halo=2, bf16_halo_mfma16=0)]


@pytest.mark.parametrize("shape", [(3, 96, 160), (20, 64, 64), (48, 128, 128)], ids=lambda s: "%dx%dx%d" % s)
def test_bf16_same_bits_knobs(flm, shape):
    from flm_amd import _lib
    n, h, w = shape
    model = _model("vanilla", "bf16", h, w)
    xd = torch.from_numpy(_crops(n, h, w)).cuda()
    maps = lambda: [model.intermediate("f%d" % i, n, "probs").clone() for i in range(1, 6)]
    model.forward_device(xd, "probs")
    f0 = maps()
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(f.float()).all()) and float((f != 0).float().mean()) >= 0.25 for f in f0)
    bad = []
    for knobs in KNOBS:
        with _lib.tuning(**knobs):
            model.forward_device(xd, "probs")
            f1 = maps()
        torch.cuda.synchronize()
        diff = ["f%d" % (i + 1) for i, (u, v) in enumerate(zip(f0, f1)) if not torch.equal(u, v)]
        print("fcn_8 bf16 %dx%dx%d %s: %s" % (n, h, w, knobs, "same bits" if not diff else "DIFFERS in " + ", ".join(diff)))
        if diff:
            bad.append((knobs, diff))
    assert not bad, bad
    _check_zero_class(model, "vanilla", n, "fcn_8 bf16 %dx%dx%d after the knobs" % shape)


# ---- (e) free running through the public path ----------------------------------------------------------------------------------

@pytest.mark.parametrize("enc", list(MODELS))
def test_predict_fp32_against_the_unfused_float64_reference(flm, enc):
    from oracle import fcn_ref
    n, h, w = 2, 64, 96
    p2, _ = _params(enc)
    model = _model(enc, "f32", h, w)
    x = np.stack([fcn_ref.get_image_array_ref(c) for c in _crops(n, h, w)])
    got = model.predict(x)
    exp = fcn_ref.fcn8_predict_ref(x, p2, torch.float64, encoder=enc)
    assert got.shape == exp.shape == (n, (h + 8) * (w + 8), 68) and np.isfinite(got).all()
    err = float(np.abs(got - exp).max())
    print("%s f32 predict %dx%dx%d: probabilities max-abs error %.3g against float64 (bar 1e-5)" % (MODELS[enc], n, h, w, err))
    assert err <= 1e-5, (enc, err)


def test_predict_bf16_against_the_rounding_oracle(flm):
    from test_gpu_forward import _gate_against_the_rounding_oracle
    n, h, w = 2, 64, 96
    p2, _ = _params("vanilla")
    model = _model("vanilla", "bf16", h, w)
    img = _crops(n, h, w)
    got = model.predict(img)
    assert np.isfinite(got).all() and np.abs(got.sum(-1) - 1).max() < 1e-5
    _gate_against_the_rounding_oracle("fcn_8 trained regime %s" % ((n, h, w),), got, img, p2, "vanilla", False)
