"""The bf16 configuration, layer by layer, against oracle/fcn_bf16_ref.py -- the float64 restatement that rounds to
bfloat16 exactly where the kernels do.

(1) Teacher-forced checks (tests/bf16_gate.py): every layer of the vanilla fcn_8 gets the device's own input and must
    land on a bf16 value next to the exact result -- within half a bf16 step plus `slack` of the tensor's maximum -- and
    may disagree with round_bf16(exact) on no more than 4 x the share of elements the float32-accumulating CPU
    evaluation of the same inputs disagrees on.  slack = min(2e-5, 4 x e32), e32 = that evaluation's largest error.
    Shapes: the headline 2 x 256 x 256; 3 x 96 x 160 (ragged tiles in every layer, a 3 x 5 fc6 map); 1 x 32 x 32 (a
    1 x 1 f5: fc6 is all padding but its centre tap); 2 x 64 x 512.

(2) Exact arithmetic through flm_fcn8_run_layer: small-integer weights, biases and inputs keep every partial sum
    below 2^24, so products and sums are exact in any order and the output must equal the integer reference bit for
    bit (rounded once to bf16 where the layer stores bf16) -- any tap, padding, k-slice or pad-column indexing error
    shows at zero tolerance.  fc6, fc7 and the score convs; the encoder branch ("enc2" .. "enc5": BatchNorm that folds
    exactly, ReLU clamping 70 % of the sums, 2 x 2 max; maps of 2 x 2, 6 x 10 and 8 x 24 at 1, 3 and 17 faces) with enc1
    through a float32-input forward; and the decoder in isolation ("up5" / "up4" in place on their skip maps, "up3" as raw
    logits, with the score convs) at the 68-class layouts and at one class count per generic instantiation of
    launch_convt at its full and its ragged edge: 1, 16, 17, 36, 48, 52, 64, 65, 80, 84, 96 -- pad columns exact zeros.

Reference-side values and what the kernels measured on an MI355X over the four shapes (the 16 faces of the 512-face
launch of tests/test_gpu_baseline_configs.py beside them).  e32: the float32 CPU evaluation's largest error against
float64 on the same inputs, of the tensor's maximum (range over the shapes); "over": the kernels' largest
|got - exact64| beyond the half step, with the slack = 4 x e32 it was gated against, at the shape where the two came
closest; flips: elements that are not round_bf16(exact64), kernels | float32 reference, summed over the shapes.

    layer      e32 (reference)   over / slack (kernels)           flips kernels | reference   512 faces: over / slack, flips
    f1         0.9 .. 1.4e-07    1.9e-08 / 4.7e-07  (3x96x160)    38 | 50 of 3,899,392        1.8e-08 / 5.0e-07, 130 | 178
    f2         1.4 .. 1.7e-07    8.7e-08 / 6.7e-07  (2x256x256)   86 | 67 of 1,949,696        1.1e-07 / 8.9e-07, 368 | 350
    f3         1.6 .. 2.1e-07    9.0e-08 / 8.3e-07  (2x64x512)    56 | 49 of 974,848          8.4e-08 / 8.2e-07, 253 | 220
    f4         1.3 .. 1.9e-07    4.8e-08 / 7.6e-07  (2x256x256)   17 | 10 of 243,712          2.8e-07 / 9.1e-07, 75 | 44
    f5         1.8 .. 2.6e-07    4.3e-08 / 7.2e-07  (3x96x160)    3 | 4 of 60,928             7.4e-08 / 1.0e-06, 26 | 18
    fc6        1.4 .. 3.2e-07    9.9e-08 / 1.3e-06  (2x256x256)   101 | 83 of 974,848         7.5e-07 / 1.8e-06, 706 | 348
    fc7        1.7 .. 2.6e-07    4.4e-08 / 6.8e-07  (3x96x160)    68 | 52 of 974,848          2.5e-07 / 7.5e-07, 489 | 256
    score5     1.7 .. 2.4e-07    1.7e-07 / 7.4e-07  (3x96x160)                                8.3e-07 / 8.5e-07
    fuse4      1.5 .. 2.6e-07    1.7e-07 / 6.1e-07  (2x256x256)                               2.3e-07 / 6.1e-07
    seg_feats  1.0 .. 3.4e-07    2.0e-07 / 5.7e-07  (3x96x160)                                2.9e-07 / 7.0e-07
    logits     1.7 .. 3.7e-07    2.8e-07 / 8.8e-07  (3x96x160)
    probs      max-abs error 1.8e-07 .. 6.2e-07 against the bar of 1e-5

The 2e-5 cap never binds: every slack is 4 x e32.  At 512 faces fc6, fc7 and score5 run without split-K -- one chain of
K / 16 accumulator updates per output where the small batches add 8 to 32 partial sums -- and come closest to the
gate: score5 (K = 4096, 256 updates) uses 0.97 of its allowance, fc6's flips half of theirs.  Every integer case of (2)
matches bit for bit in both configurations (the twelve class counts included: 0 of up to 6,690,816 elements differ).

Fault injection (scratch build, not committed): with pack_conv_kernel<unsigned short> zeroing channels 64..95 of fc6's
centre tap, fc6 of 2 x 256 x 256 is over the half step by 4.0e-2 of its maximum against a slack of 1.3e-06 and flips
49.8 % of its elements (gate: 192 elements); the integer fc6 check fails at its first case (2,211 of 4,096 elements).
Against the fp32 oracle the same fc6 is 3.998e-2 of its maximum away, inside the 4e-2 it was held to before; fc7,
downstream, crossed its own 4e-2 by a fifth (4.9e-2), fuse4 and seg_feats stayed inside their 5e-2.
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


@pytest.fixture(scope="module")
def weights68():
    from flm_amd.weights import synth_fcn8_weights
    return synth_fcn8_weights(68, seed=2)


@pytest.mark.parametrize("n,h,w", [(2, 256, 256), (3, 96, 160), (1, 32, 32), (2, 64, 512)])
def test_bf16_layers_teacher_forced(flm, weights68, n, h, w):
    from flm_amd.networks import LANDMARKS_MODELS
    model = LANDMARKS_MODELS["fcn_8"](68, input_height=h, input_width=w, dtype="bf16")
    model.load_weights(weights68)
    crops = np.random.default_rng(100 + h + w).integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    xd = torch.from_numpy(crops).cuda()
    probs = model.forward_device(xd, "probs").cpu().numpy()
    logits = model.forward_device(xd, "logits").cpu().numpy()
    torch.cuda.synchronize()
    for k in ("f5", "fc7", "seg_feats"):   # the two forwards wrote the same bits into their workspaces
        assert torch.equal(model.intermediate(k, n, "probs"), model.intermediate(k, n, "logits")), k
    check_layers(model, weights68, crops, n, "probs", logits=logits, probs=probs, label="bf16 %dx%dx%d" % (n, h, w))


# ---- exact arithmetic through flm_fcn8_run_layer ---------------------------------------------------------------

ENC_BIAS = {"enc1": (-40, 10), "enc2": (-200, 50), "enc3": (-300, 75), "enc4": (-300, 75), "enc5": (-300, 75)}


def _int_params(seed=11):
    """fcn_8 tensors of small integers: conv kernels in [-2, 2], biases in [-8, 8].  The encoder's BatchNorm folds
    EXACTLY: moving_variance = float32(0.999) (with the float32 epsilon 1e-3 the scale is gamma * (1 - 6.5e-9), which
    rounds to gamma in float32), gamma in {0.5, 1, 2} per channel, moving_mean = beta = 0, integer biases shifted below
    zero so that the ReLU clamps a visible share of the outputs -- scale = gamma and shift = gamma * bias in float32."""
    from flm_amd.weights import fcn8_param_shapes
    rng = np.random.default_rng(seed)
    p = {}
    for name, shape in fcn8_param_shapes(68).items():
        if name.endswith("/kernel"):
            p[name] = rng.integers(-2, 3, shape).astype(np.float32)
        elif name.endswith("/bias"):
            p[name] = rng.integers(-8, 9, shape).astype(np.float32)
        elif name.endswith("/gamma") or name.endswith("/moving_variance"):
            p[name] = np.ones(shape, np.float32)
        else:
            p[name] = np.zeros(shape, np.float32)
    rng = np.random.default_rng(seed + 1)     # (a stream of its own: the head's tensors above stay what they were)
    for layer, (lo, hi) in ENC_BIAS.items():
        f = p[layer + "/bias"].shape
        p[layer + "/bias"] = rng.integers(lo, hi + 1, f).astype(np.float32)
        p[layer + "/gamma"] = rng.choice(np.array([0.5, 1.0, 2.0], np.float32), f)
        p[layer + "/moving_variance"] = np.full(f, 0.999, np.float32)
    return p


def _with_classes(base, c):
    """The integer tensors with the class-dependent ones (score convs, transposed convs) redrawn for c classes."""
    from flm_amd.weights import fcn8_param_shapes
    rng = np.random.default_rng(1000 + c)
    p = dict(base)
    for name, shape in fcn8_param_shapes(c).items():
        if name.split("/")[0] in ("score5", "score4", "score3", "up5", "up4", "up3"):
            p[name] = rng.integers(-2, 3, shape).astype(np.float32) if name.endswith("/kernel") else \
                rng.integers(-8, 9, shape).astype(np.float32)
    return p


@pytest.fixture(scope="module")
def int_models(flm):
    from flm_amd.networks import LANDMARKS_MODELS
    p = _int_params()
    models = {}
    for dt in ("f32", "bf16"):
        models[dt] = LANDMARKS_MODELS["fcn_8"](68, input_height=32, input_width=32, dtype=dt)
        models[dt].load_weights(p)
    return p, models


def _run_layer(model, layer, x_nhwc, cout, out_hw=None, skip=None):
    """flm_fcn8_run_layer on an integer-valued input; the output buffer carries guard rows that must stay untouched.
    out_hw: output grid when it is not the input's; skip: what the output buffer holds on entry ("up5" / "up4")."""
    from flm_amd import _lib
    lib = _lib.load()
    bf = model.dtype == "bf16"
    n, h, w, _ = x_nhwc.shape
    up = layer.startswith("up")   # the decoder reads float32 maps in both configurations
    xd = torch.from_numpy(x_nhwc).cuda().to(torch.bfloat16 if bf and not up else torch.float32).contiguous()
    out_bf = bf and (layer in ("fc6", "fc7") or layer.startswith("enc"))
    ho, wo = out_hw if out_hw else (h, w)
    rows, guard = n * ho * wo, 64
    y = torch.full((rows + guard, cout), -12345.0, dtype=torch.bfloat16 if out_bf else torch.float32, device="cuda")
    if skip is not None:
        y[:rows] = torch.from_numpy(np.ascontiguousarray(skip, np.float32).reshape(rows, cout)).cuda()
    _lib.check(lib.flm_fcn8_run_layer(_lib.stream_ptr(), _lib.ptr(model._packed), layer.encode(), _lib.ptr(xd), _lib.ptr(y),
                                      n, h, w, model.n_classes, model._dt), "flm_fcn8_run_layer")
    torch.cuda.synchronize()
    y = y.float().cpu().numpy()
    assert (y[rows:] == np.float32(y[rows, 0])).all() and y[rows, 0] != 0, "guard rows written"
    return y[:rows].reshape(n, ho, wo, cout).astype(np.float64)


_REF = {}   # both configurations run the same integer cases: one float64 reference each


def _int_reference(p, layer, x_nhwc, relu):
    key = (layer,) + x_nhwc.shape
    if key not in _REF or not np.array_equal(_REF[key][0], x_nhwc):
        _REF[key] = (x_nhwc, _int_reference_eval(p, layer, x_nhwc, relu))
    return _REF[key][1]


def _int_reference_eval(p, layer, x_nhwc, relu):
    import torch.nn.functional as F
    k = p[layer + "/kernel"].astype(np.float64)
    y = F.conv2d(torch.from_numpy(x_nhwc.astype(np.float64)).permute(0, 3, 1, 2), torch.from_numpy(k).permute(3, 2, 0, 1),
                 torch.from_numpy(p[layer + "/bias"].astype(np.float64)), padding=k.shape[0] // 2)
    y = y.permute(0, 2, 3, 1).numpy()
    # the premise: every partial sum, in any order, stays below 2^24
    bound = F.conv2d(torch.from_numpy(np.abs(x_nhwc).astype(np.float64)).permute(0, 3, 1, 2), torch.from_numpy(np.abs(k)).permute(3, 2, 0, 1),
                     None, padding=k.shape[0] // 2).max().item() + 8
    assert bound < 2 ** 24
    return np.maximum(y, 0) if relu else y


FC6_CASES = [(1, 1, 1), (64, 1, 1), (3, 3, 5), (17, 3, 5), (1, 7, 9), (17, 7, 9), (1, 8, 8), (3, 8, 8), (64, 8, 8)]


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_run_layer_fc6_is_exact_on_integers(int_models, dtype):
    """fc6 (7 x 7, K = 12,544, position-major): maps of 1 x 1 (all padding but the centre tap), 3 x 5, 7 x 9 and 8 x 8 at
    1, 3, 17 and 64 faces (ragged M in every tile shape).  Inputs in [-4, 4]: |sum| <= 8 * 12,544 + 8 < 2^24."""
    from oracle.fcn_bf16_ref import round_bf16
    p, models = int_models
    rng = np.random.default_rng(5)
    for n, h, w in FC6_CASES:
        x = rng.integers(-4, 5, (n, h, w, 256)).astype(np.float32)
        exp = _int_reference(p, "fc6", x, relu=True)
        if dtype == "bf16":
            exp = round_bf16(exp)
        got = _run_layer(models[dtype], "fc6", x, 4096)
        bad = got != exp
        print("fc6 %s %dx%dx%d: %d of %d elements differ, max |exp| %g" % (dtype, n, h, w, bad.sum(), bad.size, np.abs(exp).max()))
        assert not bad.any(), (dtype, n, h, w, int(bad.sum()), float(np.abs(got - exp).max()))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_run_layer_fc7_and_scores_are_exact_on_integers(int_models, dtype):
    """fc7 and score5 (K = 4096) on the fc6 grids; score4 / score3 (K = 256) on 256-channel maps of 180 and 720 pixels
    (3 faces of 6 x 10 and 12 x 20: the last 16-pixel slice of 180 holds 4).  The score layers store float32 in both
    configurations, 72 columns in bf16 (68..71 exact zeros) and 68 in fp32."""
    from oracle.fcn_bf16_ref import round_bf16
    p, models = int_models
    rng = np.random.default_rng(6)
    cp = 72 if dtype == "bf16" else 68
    cases = [("fc7", shp, 4096) for shp in ((1, 1, 1), (3, 3, 5), (17, 7, 9), (64, 8, 8))]
    cases += [("score5", shp, 4096) for shp in ((1, 1, 1), (3, 3, 5), (17, 7, 9), (64, 8, 8))]
    cases += [(layer, shp, 256) for layer in ("score4", "score3") for shp in ((3, 6, 10), (3, 12, 20), (1, 1, 1), (17, 7, 9))]
    for layer, (n, h, w), cin in cases:
        x = rng.integers(-4, 5, (n, h, w, cin)).astype(np.float32)
        exp = _int_reference(p, layer, x, relu=(layer == "fc7"))
        if layer == "fc7":
            if dtype == "bf16":
                exp = round_bf16(exp)
            got = _run_layer(models[dtype], layer, x, 4096)
        else:
            got = _run_layer(models[dtype], layer, x, cp)
            assert (got[..., 68:] == 0).all(), (layer, dtype, "pad columns")
            got = got[..., :68]
        bad = got != exp
        print("%s %s %dx%dx%d: %d of %d elements differ" % (layer, dtype, n, h, w, bad.sum(), bad.size))
        assert not bad.any(), (layer, dtype, n, h, w, int(bad.sum()), float(np.abs(got - exp).max()))


# ---- the encoder branch of flm_fcn8_run_layer, and enc1 through a float32-input forward ---------------------------

def _enc_reference(p, layer, x_nhwc):
    """conv + bias, times gamma, ReLU, 2 x 2 max in float64; asserts on the CPU that the packer's fold (_fold restates
    pack_affine_kernel) is exactly scale = gamma, shift = gamma * bias, and that every partial sum stays below 2^24."""
    import torch.nn.functional as F
    from oracle.fcn_bf16_ref import _fold
    k = p[layer + "/kernel"].astype(np.float64)
    g, b = p[layer + "/gamma"].astype(np.float64), p[layer + "/bias"].astype(np.float64)
    scale, shift = _fold(p, layer, layer)
    assert np.array_equal(scale, g) and np.array_equal(shift, g * b), (layer, "BatchNorm does not fold exactly")
    xt = torch.from_numpy(x_nhwc.astype(np.float64)).permute(0, 3, 1, 2)
    kt = torch.from_numpy(k).permute(3, 2, 0, 1)
    bound = (F.conv2d(xt.abs(), kt.abs(), None, padding=1).max().item() + np.abs(b).max()) * 2
    assert bound < 2 ** 24
    pre = F.conv2d(xt, kt, None, padding=1) * torch.from_numpy(g)[None, :, None, None] + torch.from_numpy(g * b)[None, :, None, None]
    y = F.max_pool2d(torch.relu(pre), 2, 2).permute(0, 2, 3, 1).numpy()
    return y, float((pre <= 0).float().mean()), float((y == 0).mean())


ENC_MAPS = [(n, h, w) for (h, w) in ((2, 2), (6, 10), (8, 24)) for n in (1, 3, 17)]


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_run_layer_encoder_is_exact_on_integers(int_models, dtype):
    """enc2 .. enc5 (3 x 3, BatchNorm + ReLU + 2 x 2 max fused; K = 576, 1152, 2304, 2304) on maps of 2 x 2 (every tap but
    the centre quad is padding), 6 x 10 and 8 x 24 at 1, 3 and 17 faces; inputs in [-4, 4].  bf16 stores round_bf16(exact)."""
    from oracle.fcn_bf16_ref import round_bf16
    p, models = int_models
    rng = np.random.default_rng(7)
    for i, cin in ((2, 64), (3, 128), (4, 256), (5, 256)):
        layer = "enc%d" % i
        cout = p[layer + "/bias"].shape[0]
        for n, h, w in ENC_MAPS:
            x = rng.integers(-4, 5, (n, h, w, cin)).astype(np.float32)
            exp, neg, zero = _enc_reference(p, layer, x)
            if dtype == "bf16":
                exp = round_bf16(exp)
            got = _run_layer(models[dtype], layer, x, cout, out_hw=(h // 2, w // 2))
            bad = got != exp
            print("%s %s %dx%dx%d: %d of %d elements differ; ReLU clamps %.0f %% before the pool, %.0f %% of the outputs are 0" % (
                layer, dtype, n, h, w, bad.sum(), bad.size, 100 * neg, 100 * zero))
            assert not bad.any(), (layer, dtype, n, h, w, int(bad.sum()), float(np.abs(got - exp).max()))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_enc1_is_exact_on_integers_through_a_float32_forward(int_models, dtype):
    """enc1 (3 input channels, K = 27; flm_enc1.hip) has no run_layer entry: integer pixels in [-4, 4] go in as the
    float32 preprocessed input (FLM_IN_F32_RGB) of a whole forward and f1 is read back."""
    from flm_amd.networks import LANDMARKS_MODELS
    from oracle.fcn_bf16_ref import round_bf16
    p, models = int_models
    rng = np.random.default_rng(8)
    for n, h, w in ((1, 32, 32), (3, 32, 32), (3, 64, 96)):
        model = LANDMARKS_MODELS["fcn_8"](68, input_height=h, input_width=w, dtype=dtype)
        model._packed = models[dtype]._packed          # the same packed integers at another input size
        x = rng.integers(-4, 5, (n, h, w, 3)).astype(np.float32)
        exp, neg, zero = _enc_reference(p, "enc1", x)
        if dtype == "bf16":
            exp = round_bf16(exp)
        model.forward_device(torch.from_numpy(x).cuda(), "probs")
        torch.cuda.synchronize()
        got = model.intermediate("f1", n, "probs").cpu().numpy().astype(np.float64)
        bad = got != exp
        print("enc1 %s %dx%dx%d: %d of %d elements differ; ReLU clamps %.0f %% before the pool, %.0f %% of the outputs are 0" % (
            dtype, n, h, w, bad.sum(), bad.size, 100 * neg, 100 * zero))
        assert not bad.any(), (dtype, n, h, w, int(bad.sum()), float(np.abs(got - exp).max()))


# ---- the decoder in isolation: up5 / up4 / up3 and the score convs at every class-tile count ----------------------

# 68: the special layouts (fp32 G = 17; bf16 Cp = 72, the fifth class tile shared at stride 8); then one count per generic
# instantiation of launch_convt (MT = ceil(C / 16) = 1 .. 6) at its full and its ragged edge
CLASS_COUNTS = [68, 1, 16, 17, 36, 48, 52, 64, 65, 80, 84, 96]
UP_GRIDS = {"up5": [(1, 1, 1), (3, 2, 3), (3, 3, 5), (17, 2, 2), (2, 8, 8)],
            "up4": [(1, 2, 2), (3, 4, 6), (3, 6, 10), (2, 16, 16)],
            "up3": [(1, 4, 4), (3, 8, 12), (2, 12, 20), (1, 32, 32)]}


def _cp(c, dtype):
    return (72 if dtype == "bf16" else 68) if c == 68 else 16 * ((c + 15) // 16)


def _convt_reference(p, layer, x_nhwc, skip_nhwc):
    """F.conv_transpose2d in float64, the top-left crop of fcn_ref.crop_ref and the skip add; every partial sum < 2^24."""
    import torch.nn.functional as F
    from oracle import fcn_ref
    s = 8 if layer == "up3" else 2
    k = torch.from_numpy(p[layer + "/kernel"].astype(np.float64)).permute(3, 2, 0, 1)   # (kh, kw, out, in) -> (in, out, kh, kw)
    xt = torch.from_numpy(x_nhwc.astype(np.float64)).permute(0, 3, 1, 2)
    assert F.conv_transpose2d(xt.abs(), k.abs(), None, stride=s).max().item() + 8 < 2 ** 24
    o = F.conv_transpose2d(xt, k, None, stride=s)
    if skip_nhwc is not None:
        sk = torch.from_numpy(skip_nhwc.astype(np.float64)).permute(0, 3, 1, 2)
        o, sk = fcn_ref.crop_ref(o, sk)
        o = o + sk
    return o.permute(0, 2, 3, 1).numpy()


@pytest.mark.parametrize("c", CLASS_COUNTS)
def test_run_layer_decoder_is_exact_on_integers(flm, int_models, c):
    """up5 / up4 (4 x 4, stride 2, crop + Add in place on the skip map), up3 (16 x 16, stride 8, raw logits; class counts
    that are multiples of 4) and score5 / score4 / score3 at one class count, in both types.  Grids: one partial
    64-position tile, tiles that span faces, and the far row and column of P = n (h + 1)(w + 1).  Integer kernels in
    [-2, 2], x in [-4, 4], skip maps in [-8, 8], pad columns zero on entry and exact zeros on exit."""
    from flm_amd.networks import LANDMARKS_MODELS
    base, models68 = int_models
    p = base if c == 68 else _with_classes(base, c)
    rng = np.random.default_rng(2000 + c)
    cases = []
    for layer in ("up5", "up4", "up3"):
        if layer == "up3" and c % 4:
            continue
        for n, h, w in UP_GRIDS[layer]:
            x = rng.integers(-4, 5, (n, h, w, c)).astype(np.float32)
            skip = None if layer == "up3" else rng.integers(-8, 9, (n, 2 * h, 2 * w, c)).astype(np.float32)
            cases.append((layer, x, skip, _convt_reference(p, layer, x, skip)))
    for layer, cin, shapes in (("score5", 4096, ((1, 1, 1), (3, 3, 5), (17, 7, 9))), ("score4", 256, ((3, 6, 10), (17, 7, 9))),
                               ("score3", 256, ((3, 12, 20), (1, 1, 1)))):
        for shp in shapes:
            x = rng.integers(-4, 5, shp + (cin,)).astype(np.float32)
            cases.append((layer, x, None, _int_reference_eval(p, layer, x, relu=False)))
    for dtype in ("f32", "bf16"):
        if c == 68:
            model = models68[dtype]
        else:
            model = LANDMARKS_MODELS["fcn_8"](c, input_height=32, input_width=32, dtype=dtype)
            model.load_weights(p)
        cp = _cp(c, dtype)
        padded = lambda a: np.concatenate([a, np.zeros(a.shape[:3] + (cp - c,), np.float32)], -1)
        for layer, x, skip, exp in cases:
            n, h, w, _ = x.shape
            if layer == "up3":
                got = _run_layer(model, layer, padded(x), c, out_hw=(8 * h + 8, 8 * w + 8))
            elif layer.startswith("up"):
                got = _run_layer(model, layer, padded(x), cp, out_hw=(2 * h, 2 * w), skip=padded(skip))
            else:
                got = _run_layer(model, layer, x, cp)
            assert (got[..., c:] == 0).all(), (layer, dtype, c, "pad columns", float(np.abs(got[..., c:]).max()))
            bad = got[..., :c] != exp
            print("%s %s C=%d %dx%dx%d: %d of %d elements differ" % (layer, dtype, c, n, h, w, bad.sum(), bad.size))
            assert not bad.any(), (layer, dtype, c, n, h, w, int(bad.sum()), float(np.abs(got[..., :c] - exp).max()))
        if c % 4:   # the raw-logits launch needs float4 rows: refused (FLM_ERR_UNSUPPORTED = -5), not mis-stored
            from flm_amd import _lib
            x, y = torch.zeros((1, 4, 4, cp), device="cuda"), torch.zeros((1, 40, 40, c), device="cuda")
            rc = _lib.load().flm_fcn8_run_layer(_lib.stream_ptr(), _lib.ptr(model._packed), b"up3", _lib.ptr(x), _lib.ptr(y),
                                                1, 4, 4, c, model._dt)
            assert rc == -5, rc
        del model
