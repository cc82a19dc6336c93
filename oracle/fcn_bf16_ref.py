"""float64 restatement of the bf16 configuration's forward (FLM_BF16).  TEST INFRASTRUCTURE ONLY.

The same graphs as oracle/fcn_ref.py, evaluated in float64 and rounded to bfloat16 (round to nearest, ties to
even) at exactly the points where the bf16 kernels round.  Every rounding point below was read off the kernel
that performs it and is cited next to the code that restates it (paths relative to
face-landmark-detector_amd/csrc/):

  weights   conv kernels of the implicit GEMMs and the transposed-conv kernels are rounded RAW, BatchNorm is not
            folded into them: flm_pack.hip pack_conv_kernel<unsigned short> / pack_convt_kernel<unsigned short> /
            pack_pw_pair_kernel, all through put(unsigned short*, ...) = (__bf16)v.
            The FIRST conv of an encoder keeps a float32 filter in the blob (pack_enc1_kernel, and the plain copies
            of MobileNet's / ResNet50's conv1).  The 3x3 first conv of the vanilla / VGG encoders rounds it when it
            builds its fragments (flm_enc1.hip enc1_bf16_kernel: `bw[ky][j][e] = (__bf16)wv`); MobileNet's conv1
            (flm_mobile.hip mb_conv1_kernel), ResNet50's conv1 (rn_conv1_kernel) and the depthwise filters
            (mb_depthwise_kernel) multiply in float32: NOT rounded.
  affine    BatchNorm and bias are one per-channel scale / shift, folded in float64 and stored as float32
            (flm_pack.hip pack_affine_kernel), applied to the float32 accumulator as fmaf(acc, scale, shift), then
            the residual add (ResNet50), ReLU / ReLU6 and the 2x2 max, then ONE rounding of the stored value
            (flm_igemm_bf16.hip epilogues, flm_igemm.hip igemm_kernel / splitk_reduce*_kernel, flm_conv3_halo.hip,
            flm_enc1.hip enc1_bf16_store_strip: f2bf / v_cvt_pk_bf16_f32).
  input     vanilla / VGG: the preprocessed RGB input (x - mean, float32) is staged as bf16 (enc1_bf16_kernel,
            px_u8 / stage_two_rows); MobileNet / ResNet50 conv1 read it as float32.
  maps      every encoder map, fc6 and fc7 are stored as bf16 (IgemmArgs::out_f32 = 0; store4<BF> in
            flm_mobile.hip, which also serves the 3x3 max-pool -- exact on bf16 values).  The ResNet50 shortcut is
            read back from its stored bf16 map and added in float32 before the ReLU (flm_igemm.hip igemm_kernel,
            `u += (float)bf16(a.res[o])`).
  fp32 maps score5, fuse4 and seg_feats are stored as float32 (out_f32 = 1) and re-read as bf16 OPERANDS by up5,
            up4 and up3 / up32 (flm_convt.hip: `t[0] = (__bf16)(ok ? v0.x : 0.f)` ...; flm_tail_bf16.hip the same
            for up4; flm_up3_wreg.hip up3_xpack_kernel).  score4 / score3 are added in float32.
  the rest  class columns are padded 68 -> 72 with zeros (flm_pack.hip convt_geom; exact); softmax and decode
            run in float32 on the float32 logits.

Stores to float32 maps are NOT restated as roundings (2^-24, a thousandth of the next operand rounding).

`accum=torch.float32` evaluates the SAME rounded operands with torch's float32 CPU convolutions and a float32
epilogue: a legitimate implementation in another summation order.  Its distance from the float64 evaluation is
the yardstick for what float32 accumulation can move (tests/test_oracle_fcn_bf16.py, tests/test_gpu_bf16_layers.py).

With rounding=False every function performs fcn_ref's float64 operations in fcn_ref's order: bit-identical.

The VGG, MobileNet and ResNet50 encoders are stated ONCE, as chains of Steps (ENCODER_CHAINS, written from the reference's
network files): run_chain evaluates a chain free running, encoder_layer_ref one step from given inputs -- what the
teacher-forced gate of tests/test_gpu_encoder_layers.py holds each device layer to.

A third arithmetic, the exact-fp32 configuration's (FLM_F32; layer_f32_ref, or fp32=True): the same packed form of every
conv -- raw float32 kernel (pack_conv_kernel<float> / pack_convt_kernel<float>), BatchNorm and bias as the float32-stored
scale / shift of pack_affine_kernel applied to the accumulator (flm_igemm.hip igemm_kernel, flm_enc1.hip) -- with no
bf16 rounding of weights, inputs or outputs, and transposed convs on the unrounded float32 maps.  accum=float64 is the
exact value of that arithmetic, accum=float32 the yardstick of the fp32 gate (tests/test_oracle_fcn_f32.py,
tests/test_gpu_fp32_layers.py).  It differs from fcn_ref's float64 only by the float32 storage of scale and shift.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from . import fcn_ref

BN_EPS = fcn_ref.BN_EPS
F64 = torch.float64


# ---- bfloat16 rounding and the gate built on it --------------------------------------------------------------

def round_bf16(a) -> np.ndarray:
    """Nearest bfloat16 (8 exponent bits, 7 fraction bits), ties to even, of float64 / float32 values, returned
    as float64.  Rounds the float64 value ONCE (no detour through float32).  Below 2^-126 the grid is the fixed
    subnormal step 2^-133; magnitudes that round past the largest finite value (0x7F7F = (2 - 2^-7) * 2^127)
    become infinities; NaN stays NaN; the sign of zero is kept."""
    if isinstance(a, np.ndarray) and a.dtype == np.float32 and a.size > (1 << 20):
        # large float32 tensors (the 100 M weights of fc6): the same rounding on the float32 bit pattern, a quarter of
        # the memory traffic; both forms are held to the bit-level restatement in tests/test_oracle_fcn_bf16.py
        u = np.ascontiguousarray(a).view(np.uint32)
        r = u + (np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1)))
        r &= np.uint32(0xFFFF0000)
        out = r.view(np.float32)
        nan = np.isnan(a)
        if nan.any():
            out[nan] = a[nan]
        return out.astype(np.float64)
    x = np.ascontiguousarray(np.asarray(a, dtype=np.float64))
    u = x.view(np.uint64)
    keep = np.uint64(52 - 7)
    lsb = (u >> keep) & np.uint64(1)
    r = (u + ((np.uint64(1) << (keep - np.uint64(1))) - np.uint64(1)) + lsb) & ~((np.uint64(1) << keep) - np.uint64(1))
    out = r.view(np.float64).copy()
    ax = np.abs(x)
    tiny = ax < 2.0 ** -126
    if tiny.any():
        out[tiny] = np.copysign(np.rint(ax[tiny] * 2.0 ** 133) * 2.0 ** -133, x[tiny])
    with np.errstate(invalid="ignore"):
        big = np.abs(out) >= 2.0 ** 128
    out[big] = np.copysign(np.inf, x[big])
    nan = np.isnan(x)
    out[nan] = x[nan]
    return out


def ulp_bf16(a) -> np.ndarray:
    """Spacing of the bfloat16 grid at |a| (2^-133 in the subnormal range)."""
    ax = np.abs(np.asarray(a, dtype=np.float64))
    e = np.floor(np.log2(np.maximum(ax, 2.0 ** -126)))
    return 2.0 ** (e - 7)


SLACK_CAP = 2e-5       # the fp32 suite's bar for the same layers (tests/test_gpu_forward.py)
SLACK_MARGIN = 4.0     # the MFMA sums 32-deep runs in an order of its own
SLACK_FLOOR = 2.0 ** -23  # one float32 step at the tensor's maximum: a float32 result cannot promise less
FLIP_MARGIN = 4.0
FLIP_FLOOR = 8         # elements: tiny tensors


def slack_from_reference(ref32, exact64) -> tuple:
    """(slack, e32): e32 = largest error of the float32-accumulating evaluation against the float64 one, relative
    to the tensor's maximum; slack = min(SLACK_CAP, max(SLACK_MARGIN * e32, SLACK_FLOOR))."""
    exact64 = np.asarray(exact64, dtype=np.float64)
    e32 = float(np.abs(np.asarray(ref32, dtype=np.float64) - exact64).max() / max(np.abs(exact64).max(), 1e-300))
    return min(SLACK_CAP, max(SLACK_MARGIN * e32, SLACK_FLOOR)), e32


def gate_excess(got, exact64, slack, stored_bf16) -> float:
    """Worst excess of |got - exact64| over the allowance, in units of slack * max|exact64| (<= 1 passes):
      bf16-stored: |got - exact64| <= ulp_bf16(exact64) / 2 + slack * max|exact64|
      fp32-stored: |got - exact64| <=                         slack * max|exact64|"""
    got = np.asarray(got, dtype=np.float64)
    exact64 = np.asarray(exact64, dtype=np.float64)
    assert got.shape == exact64.shape, (got.shape, exact64.shape)
    if not np.isfinite(got).all():
        return float("inf")
    unit = slack * max(np.abs(exact64).max(), 1e-300)
    err = np.abs(got - exact64)
    if stored_bf16:
        err = err - 0.5 * ulp_bf16(exact64)
    return float(err.max() / unit)


def flip_count(stored, exact64) -> int:
    """Elements whose stored bf16 value is not round_bf16(exact64)."""
    return int((np.asarray(stored, dtype=np.float64) != round_bf16(exact64)).sum())


def flips_allowed(ref_flips: int) -> int:
    return max(int(np.ceil(FLIP_MARGIN * ref_flips)), FLIP_FLOOR)


def layer_report(got, exact64, ref32_exact, ref32_stored, stored_bf16) -> dict:
    """The gate of one layer output `got` against the float64 evaluation `exact64` of the same input, with the
    float32-accumulating evaluation of that input (ref32_exact before, ref32_stored after the store's rounding)
    as the yardstick.  Keys: e32, slack, over (worst |got - exact64| beyond the half step, relative to the
    tensor's maximum: <= slack passes), and for bf16-stored layers flips / ref_flips / allowed / size; ok."""
    slack, e32 = slack_from_reference(ref32_exact, exact64)
    over = gate_excess(got, exact64, slack, stored_bf16) * slack
    rep = dict(e32=e32, slack=slack, over=over, ok=over <= slack)
    if stored_bf16:
        rep.update(flips=flip_count(got, exact64), ref_flips=flip_count(ref32_stored, exact64), size=int(np.size(exact64)))
        rep["allowed"] = flips_allowed(rep["ref_flips"])
        rep["ok"] = rep["ok"] and rep["flips"] <= rep["allowed"]
    return rep


def gate_layer(got, exact64, ref32_exact, ref32_stored, stored_bf16) -> dict:
    """layer_report of the first exact64.shape[-1] columns of `got`; the columns beyond them -- the class padding of
    score5 / fuse4 / seg_feats -- must be exact zeros (else ok = False and `pad` = their largest magnitude)."""
    got = np.asarray(got)
    c = np.shape(exact64)[-1]
    rep = layer_report(got[..., :c], exact64, ref32_exact, ref32_stored, stored_bf16)
    if got.shape[-1] > c and np.any(got[..., c:] != 0):
        rep["ok"] = False
        rep["pad"] = float(np.abs(got[..., c:]).max())
    return rep


PROBS_BAR = 1e-5       # the suite's bar on probabilities (tests/test_gpu_forward.py)


def probs_report(got, logits64) -> dict:
    """The probabilities `got` [N,H'*W',C] against the float64 softmax of `logits64` [N,H',W',C]: largest absolute
    error `err`, ok = err <= PROBS_BAR."""
    d = float(np.abs(np.asarray(got, np.float64) - softmax_ref(logits64)).max())
    return dict(err=d, ok=d <= PROBS_BAR)


def format_report(name, rep) -> str:
    s = "%-9s over-half-step %.3g (slack %.3g = min(2e-5, 4 x e32 %.3g))" % (name, rep["over"], rep["slack"], rep["e32"])
    if "flips" in rep:
        s += ", flips %d / %d = %.3g (float32 reference %d = %.3g, allowed %d)" % (
            rep["flips"], rep["size"], rep["flips"] / rep["size"], rep["ref_flips"], rep["ref_flips"] / rep["size"],
            rep["allowed"])
    return s + ("" if rep["ok"] else "   <-- FAILS")


# ---- arithmetic ----------------------------------------------------------------------------------------------

class Arith:
    """rounding: restate the bf16 rounding points (False: fcn_ref's float64 arithmetic, bit for bit).
    accum: torch.float64, or torch.float32 = the same rounded operands summed by torch's float32 CPU kernels.
    fp32: the exact-fp32 configuration (FLM_F32) -- the packed form of every conv (raw float32 kernel, BatchNorm and
    bias as _fold's float32-stored scale / shift applied to the accumulator) with NO bf16 rounding of weights, inputs
    or outputs; `accum` is honoured (float64: the exact value of that arithmetic; float32: the yardstick)."""

    def __init__(self, rounding=True, accum=F64, fp32=False, cache=None):
        assert accum in (torch.float64, torch.float32)
        self.cache = cache                           # see _weight: large operands kept between calls, or None
        self.fp32 = bool(fp32)
        self.rounding = bool(rounding) and not self.fp32
        self.folded = self.rounding or self.fp32     # the packer's scale / shift form instead of fcn_ref's BatchNorm
        self.accum = accum if self.folded else F64

    def q(self, t: torch.Tensor) -> torch.Tensor:
        """One bf16 rounding of a float64 tensor (identity with rounding off)."""
        if not self.rounding:
            return t
        return torch.from_numpy(round_bf16(t.numpy())).reshape(t.shape)


def _t64(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64)))


def _nchw(a):
    return _t64(a).permute(0, 3, 1, 2).contiguous()


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().numpy()


def _fold(p, conv, bn):
    """flm_pack.hip pack_affine_kernel: scale = gamma / sqrt(var + eps), shift = (bias - mean) * scale + beta in
    float64, both STORED AS float32; without BatchNorm scale = 1, shift = bias."""
    k = p[conv + ("/depthwise_kernel" if conv + "/depthwise_kernel" in p else "/kernel")]
    cout = k.shape[2] if conv + "/depthwise_kernel" in p else k.shape[3]
    b = np.asarray(p[conv + "/bias"], np.float64) if conv + "/bias" in p else np.zeros(cout)
    if bn is None:
        return np.ones(cout), b.astype(np.float32).astype(np.float64)
    s = np.asarray(p[bn + "/gamma"], np.float64) / np.sqrt(np.asarray(p[bn + "/moving_variance"], np.float64) + float(np.float32(BN_EPS)))
    sh = (b - np.asarray(p[bn + "/moving_mean"], np.float64)) * s + np.asarray(p[bn + "/beta"], np.float64)
    return s.astype(np.float32).astype(np.float64), sh.astype(np.float32).astype(np.float64)


WEIGHT_CACHE_MIN = 1 << 24


def _weight(kern, perm, rounded, cache=None):
    """A Keras kernel as the torch operand, rounded raw to bf16 where the packer rounds it (flm_pack.hip put()).
    `cache`: a dict the CALLER owns (Arith.cache); operands of kernels of at least WEIGHT_CACHE_MIN elements are then
    built once per (array, rounded) -- the float64 fc6 operand of a 2048-channel f5 is 3 GB."""
    k = np.asarray(kern)
    key = (id(kern), rounded, tuple(perm))
    if cache is not None and k.size >= WEIGHT_CACHE_MIN and key in cache and cache[key][0] is kern:
        return cache[key][1]
    w = round_bf16(k) if rounded else k.astype(np.float64)
    w = torch.from_numpy(w).permute(*perm).contiguous()
    if cache is not None and k.size >= WEIGHT_CACHE_MIN:
        cache[key] = (kern, w)
    return w


def _act(y, relu):
    if relu == 1:
        return torch.relu(y)
    if relu == 2:
        return torch.clamp(y, 0.0, 6.0)
    return y


def _conv_block(A: Arith, x, p, conv, bn=None, pad=0, stride=1, relu=0, pool=0, res=None, groups=1,
                round_w=True, round_x=False, round_y=True):
    """One conv layer as the bf16 configuration runs it: x (NCHW float64 values) -> (exact, stored).
    exact: float64 (accum=float32: the float32 result), before the rounding of the stored value."""
    dw = conv + "/depthwise_kernel" in p
    kern = p[conv + ("/depthwise_kernel" if dw else "/kernel")]
    if not A.folded:   # fcn_ref's operations, in its order
        if dw:
            w = fcn_ref._t(kern, F64).permute(2, 3, 0, 1).contiguous()
        else:
            w = fcn_ref._t(kern, F64).permute(3, 2, 0, 1).contiguous()
        b = fcn_ref._t(p[conv + "/bias"], F64) if conv + "/bias" in p else None
        y = F.conv2d(x, w, b, stride=stride, padding=pad, groups=groups)
        if bn is not None:
            y = fcn_ref._bn(y, p, bn, F64)
        if res is not None:
            y = y + res
        y = _act(y, relu)
        if pool:
            y = F.max_pool2d(y, 2, 2)
        return y, y
    w = _weight(kern, (2, 3, 0, 1) if dw else (3, 2, 0, 1), round_w and A.rounding, A.cache)
    xo = A.q(x) if round_x else x
    scale, shift = _fold(p, conv, bn)
    dt = A.accum
    acc = F.conv2d(xo.to(dt), w.to(dt), None, stride=stride, padding=pad, groups=groups)
    y = acc * _t64(scale).to(dt)[None, :, None, None] + _t64(shift).to(dt)[None, :, None, None]
    if res is not None:
        y = y + res.to(dt)
    y = _act(y, relu)
    if pool:
        y = F.max_pool2d(y, 2, 2)
    y = y.to(F64)
    return y, (A.q(y) if round_y else y)


def _convt_block(A: Arith, x, p, name, stride):
    """Transposed conv of the decoder: the float32 map x is re-read as a bf16 operand, the kernel is rounded raw
    (flm_convt.hip / flm_tail_bf16.hip / flm_up3_wreg.hip; flm_pack.hip pack_convt_kernel<unsigned short>)."""
    if not A.folded:
        return fcn_ref._convT(x, p[name + "/kernel"], stride, F64)
    w = _weight(p[name + "/kernel"], (3, 2, 0, 1), A.rounding, A.cache)   # (fp32 configuration: unrounded operands)
    return F.conv_transpose2d(A.q(x).to(A.accum), w.to(A.accum), None, stride=stride).to(F64)


# ---- encoders: lists of (exact, stored) per level --------------------------------------------------------------

def _vanilla_encoder(A, x, p):
    levels = []
    for i in range(1, 6):
        n = "enc%d" % i
        # enc1: flm_enc1.hip enc1_bf16_kernel rounds input and filter itself; enc2..5: packed bf16 filter
        e, x = _conv_block(A, x, p, n, bn=n, pad=1, relu=1, pool=1, round_x=(i == 1))
        levels.append((e, x))
    return levels


class Step:
    """One layer of an encoder chain: `name` (the Keras layer name; its parameters are p[name + "/..."]), `inputs` (names
    of the steps whose STORED outputs it reads, "x" = the preprocessed network input; a second input is the shortcut a
    ResNet `2c` conv adds before its ReLU), and the evaluation: step(A, p, *inputs_nchw) -> (exact, stored) in the
    arithmetic A.  op "conv": _conv_block with the keyword arguments `kw` (bn, pad, stride, relu, pool, round_w,
    round_x); op "maxpool3": MaxPooling2D(3x3, stride 2, 'valid'), no parameters, exact in every arithmetic."""

    def __init__(self, name, inputs, op="conv", depthwise=False, **kw):
        self.name, self.inputs, self.op, self.depthwise, self.kw = name, tuple(inputs), op, depthwise, kw
        self.stride = 2 if op == "maxpool3" else kw.get("stride", 1)
        self.relu = 0 if op == "maxpool3" else kw.get("relu", 0)
        self.pool = kw.get("pool", 0)

    def __call__(self, A, p, *xs):
        assert len(xs) == len(self.inputs), (self.name, len(xs))
        if self.op == "maxpool3":
            y = F.max_pool2d(xs[0], 3, 2)
            return y, y
        kw = dict(self.kw)
        if self.depthwise:
            kw["groups"] = p[self.name + "/depthwise_kernel"].shape[2]
        return _conv_block(A, xs[0], p, self.name, res=xs[1] if len(xs) > 1 else None, **kw)


def _vgg_chain():
    """networks/vgg16.py:27-72 (pretrained=None): five blocks of 2, 2, 3, 3, 3 x Conv2D(3x3, 'same', relu), each closed
    by MaxPooling2D(2x2, stride 2); the kernels fuse the pool into the block's last conv.  The first conv rounds its
    input and its float32 filter to bf16 itself (flm_enc1.hip enc1_bf16_kernel)."""
    steps, prev = [], "x"
    for b, k in ((1, 2), (2, 2), (3, 3), (4, 3), (5, 3)):
        for c in range(1, k + 1):
            name = "block%d_conv%d" % (b, c)
            steps.append(Step(name, (prev,), pad=1, relu=1, pool=int(c == k), round_x=(prev == "x")))
            prev = name
    return tuple(steps)


def _mobilenet_chain():
    """networks/mobilenet.py:59-114 (alpha 1): conv1 = ZeroPadding2D(1) + Conv2D(32, 3x3, stride 2, valid, no bias) + BN +
    ReLU6 (:16-28); blocks 1..13 = ZeroPadding2D(1) + DepthwiseConv2D(3x3, stride s, valid, no bias) + BN + ReLU6, then
    Conv2D(1x1, no bias) + BN + ReLU6 (:31-56); s = 2 at blocks 2, 4, 6, 12 (:82, 87, 92, 101).  conv1 and the
    depthwise convs multiply float32 filters, and conv1 reads the float32 input (flm_mobile.hip)."""
    steps = [Step("conv1", ("x",), bn="conv1_bn", pad=1, stride=2, relu=2, round_w=False)]
    prev = "conv1"
    for i in range(1, 14):
        dw, pw = "conv_dw_%d" % i, "conv_pw_%d" % i
        steps.append(Step(dw, (prev,), depthwise=True, bn=dw + "_bn", pad=1, stride=2 if i in (2, 4, 6, 12) else 1, relu=2,
                          round_w=False))
        steps.append(Step(pw, (dw,), bn=pw + "_bn", relu=2))
        prev = pw
    return tuple(steps)


def _resnet50_chain():
    """networks/resnet50.py:122-182 (pretrained=None): ZeroPadding2D(3) + Conv2D(64, 7x7, stride 2) + BN + ReLU (:142-148),
    MaxPooling2D(3x3, stride 2, valid) (:149), then stages 2..5 of 3, 4, 6, 3 bottleneck blocks (:151-172).  A stage's
    block `a` is a conv_block (:73-119): 1x1 (stride s) + BN + ReLU, 3x3 'same' + BN + ReLU, 1x1 + BN, and the shortcut
    1x1 (stride s) + BN of the block input, added before the last ReLU; s = 1 in stage 2 (:151), 2 from stage 3 on.  The
    other blocks are identity_blocks (:32-70): the same three convs at stride 1, the block input itself added.  The
    library evaluates a conv_block's shortcut before its main path.  conv1 multiplies a float32 filter by the float32
    input (rn_conv1_kernel); the shortcut is read back from its stored map."""
    def cbn(name, inputs, k, stride, relu, **kw):
        return Step(name, inputs, bn=name.replace("res", "bn", 1), pad=k // 2, stride=stride, relu=int(relu), **kw)

    steps = [Step("conv1", ("x",), bn="bn_conv1", pad=3, stride=2, relu=1, round_w=False),
             Step("max_pooling2d", ("conv1",), op="maxpool3")]
    prev = "max_pooling2d"
    for stage, blocks in ((2, "abc"), (3, "abcd"), (4, "abcdef"), (5, "abc")):
        for b in blocks:
            base = "res%d%s_branch" % (stage, b)
            s = 2 if (b == "a" and stage > 2) else 1
            shortcut = prev
            if b == "a":
                steps.append(cbn(base + "1", (prev,), 1, s, False))
                shortcut = base + "1"
            steps.append(cbn(base + "2a", (prev,), 1, s, True))
            steps.append(cbn(base + "2b", (base + "2a",), 3, 1, True))
            steps.append(cbn(base + "2c", (base + "2b", shortcut), 1, 1, True))
            prev = base + "2c"
    return tuple(steps)


# The three registry encoders as explicit chains (the vanilla one: tests/bf16_gate.py CHAIN), and the steps whose outputs
# are the levels f1..f5 the FCN head reads (ResNet50: f1 is its conv1; only f3..f5 are used).
ENCODER_CHAINS = {"vgg": _vgg_chain(), "mobilenet": _mobilenet_chain(), "resnet50": _resnet50_chain()}
ENCODER_LEVELS = {"vgg": ("block1_conv2", "block2_conv2", "block3_conv3", "block4_conv3", "block5_conv3"),
                  "mobilenet": ("conv_pw_1", "conv_pw_3", "conv_pw_5", "conv_pw_11", "conv_pw_13"),
                  "resnet50": ("conv1", "res2c_branch2c", "res3d_branch2c", "res4f_branch2c", "res5c_branch2c")}


def run_chain(chain, A, x, p) -> dict:
    """Free-running evaluation: every step reads the chain's own stored outputs.  {name: (exact, stored)}, NCHW."""
    out = {"x": (x, x)}
    for st in chain:
        out[st.name] = st(A, p, *[out[i][1] for i in st.inputs])
    return out


def _chain_encoder(encoder):
    def levels(A, x, p):
        out = run_chain(ENCODER_CHAINS[encoder], A, x, p)
        if encoder == "resnet50":   # (its levels have always been reported as stored)
            return [(out[n][1], out[n][1]) for n in ENCODER_LEVELS[encoder]]
        return [out[n] for n in ENCODER_LEVELS[encoder]]
    return levels


_vgg_encoder, _mobilenet_encoder, _resnet50_encoder = (_chain_encoder(e) for e in ("vgg", "mobilenet", "resnet50"))


def encoder_layer_ref(encoder: str, layer: str, inputs, p: dict, rounding=True, accum=F64, fp32=False):
    """One step of ENCODER_CHAINS[encoder], given its INPUT (NHWC; a tuple (main, shortcut) for ResNet50's `2c` convs):
    the sibling of layer_bf16_ref for the VGG, MobileNet and ResNet50 encoders, in the same three arithmetics (bf16
    rounding points; fp32=True: the exact-fp32 folded form; accum=float32: the yardstick).  Returns (exact, stored),
    NHWC float64.  The head and decoder on these encoders are layer_bf16_ref's (their widths come from `p`)."""
    st = next(s for s in ENCODER_CHAINS[encoder] if s.name == layer)
    xs = inputs if isinstance(inputs, tuple) else (inputs,)
    e, s = st(Arith(rounding, accum, fp32), p, *[_nchw(x) for x in xs])
    return _nhwc(e), _nhwc(s)


_ENCODERS = {"vanilla": _vanilla_encoder, "vgg": _vgg_encoder, "mobilenet": _mobilenet_encoder,
             "resnet50": _resnet50_encoder}


# ---- head and decoders, one function per checked layer ---------------------------------------------------------

def _fc6(A, f5, p):
    return _conv_block(A, f5, p, "fc6", pad=3, relu=1)


def _fc7(A, fc6, p):
    return _conv_block(A, fc6, p, "fc7", relu=1)


def _score(A, x, p, name):
    """1x1 classifier, float32 output (out_f32 = 1): no rounding of the result."""
    return _conv_block(A, x, p, name, round_y=False)[0]


def _fuse4(A, score5, f4, p):
    o = _convt_block(A, score5, p, "up5", 2)             # fcn.py:104-105
    o2 = _score(A, f4, p, "score4")                      # fcn.py:107-108
    o, o2 = fcn_ref.crop_ref(o, o2)                      # fcn.py:110
    return o + o2                                        # fcn.py:112


def _seg(A, fuse4, f3, p):
    o = _convt_block(A, fuse4, p, "up4", 2)              # fcn.py:114-115
    o2 = _score(A, f3, p, "score3")                      # fcn.py:116-117
    o2, o = fcn_ref.crop_ref(o2, o)                      # fcn.py:118
    return o2 + o                                        # fcn.py:119


def layer_bf16_ref(layer: str, inputs, p: dict, rounding=True, accum=F64, fp32=False, cache=None):
    """One layer of the vanilla fcn_8 in the bf16 configuration, given its INPUT (NHWC arrays; a tuple for the
    two-input layers).  Returns (exact, stored), NHWC float64: the unrounded output and the value the layer
    stores (rounded to bf16 for f1..f5 / fc6 / fc7; the float32-stored layers return exact twice).

      enc1: preprocessed float32 RGB input    enc2..enc5: f1..f4    fc6: f5    fc7: fc6    score5: fc7
      score4: f4    score3: f3    fuse4: (score5, f4)    seg_feats: (fuse4, f3)    logits: seg_feats
    Class columns beyond n_classes of score5 / fuse4 / seg_feats inputs are ignored (they hold zeros).
    fp32=True: the same layer in the fp32 configuration's arithmetic (Arith); exact and stored are then equal.
    cache: a dict of the caller's that keeps the float64 operands of large kernels between calls (_weight)."""
    A = Arith(rounding, accum, fp32, cache)
    c = p["score5/kernel"].shape[3]
    if layer in ("enc1", "enc2", "enc3", "enc4", "enc5"):
        e, s = _conv_block(A, _nchw(inputs), p, layer, bn=layer, pad=1, relu=1, pool=1, round_x=(layer == "enc1"))
    elif layer == "fc6":
        e, s = _fc6(A, _nchw(inputs), p)
    elif layer == "fc7":
        e, s = _fc7(A, _nchw(inputs), p)
    elif layer in ("score5", "score4", "score3"):
        e = s = _score(A, _nchw(inputs), p, layer)
    elif layer == "fuse4":
        e = s = _fuse4(A, _nchw(np.asarray(inputs[0])[..., :c]), _nchw(inputs[1]), p)
    elif layer == "seg_feats":
        e = s = _seg(A, _nchw(np.asarray(inputs[0])[..., :c]), _nchw(inputs[1]), p)
    elif layer == "logits":
        e = s = _convt_block(A, _nchw(np.asarray(inputs)[..., :c]), p, "up3", 8)
    else:
        raise KeyError(layer)
    return _nhwc(e), _nhwc(s)


def layer_f32_ref(layer: str, inputs, p: dict, accum=F64) -> np.ndarray:
    """One layer of the vanilla fcn_8 as the fp32 configuration (FLM_F32) evaluates it, given its input (the layers and
    inputs of layer_bf16_ref): folded float32 scale / shift, nothing rounded to bf16, sums in `accum`.  NHWC float64."""
    return layer_bf16_ref(layer, inputs, p, accum=accum, fp32=True)[0]


def fcn8_logits_bf16_ref(x_nhwc, p, return_intermediates=False, encoder="vanilla", rounding=True, accum=F64):
    """fcn_ref.fcn8_logits_ref in the bf16 configuration's arithmetic (free running: every layer reads the
    oracle's own rounded maps).  Returns float64 logits NHWC and, on request, the intermediates dict of
    fcn8_logits_ref plus `score5` (stored values)."""
    A = Arith(rounding, accum)
    lv = _ENCODERS[encoder](A, _nchw(x_nhwc), p)
    f = [s for _, s in lv]
    fc6 = _fc6(A, f[4], p)[1]
    fc7 = _fc7(A, fc6, p)[1]
    score5 = _score(A, fc7, p, "score5")                 # fcn.py:103
    fuse4 = _fuse4(A, score5, f[3], p)
    seg = _seg(A, fuse4, f[2], p)
    logits = _nhwc(_convt_block(A, seg, p, "up3", 8))    # fcn.py:121-122
    if return_intermediates:
        return logits, dict(f1=_nhwc(f[0]), f2=_nhwc(f[1]), f3=_nhwc(f[2]), f4=_nhwc(f[3]), f5=_nhwc(f[4]),
                            fc6=_nhwc(fc6), fc7=_nhwc(fc7), score5=_nhwc(score5), fuse4=_nhwc(fuse4),
                            seg_feats=_nhwc(seg))
    return logits


def fcn32_logits_bf16_ref(x_nhwc, p, encoder="vanilla", rounding=True, accum=F64):
    """fcn_ref.fcn32_logits_ref in the bf16 configuration's arithmetic."""
    A = Arith(rounding, accum)
    f5 = _ENCODERS[encoder](A, _nchw(x_nhwc), p)[4][1]
    fc7 = _fc7(A, _fc6(A, f5, p)[1], p)[1]
    score5 = _score(A, fc7, p, "score5")                 # fcn.py:143-144
    return _nhwc(_convt_block(A, score5, p, "up32", 32))  # fcn.py:145-146


def softmax_ref(logits_nhwc) -> np.ndarray:
    """networks/utils.py:28-30 in float64: [N,H,W,C] logits -> [N,H*W,C] probabilities."""
    t = _t64(logits_nhwc)
    n, h, w, c = t.shape
    return torch.softmax(t.reshape(n, h * w, c), dim=-1).numpy()


def predict_bf16_ref(x_nhwc, p, encoder="vanilla", fcn32=False, rounding=True, accum=F64) -> np.ndarray:
    """[N, H'*W', C] float64 probabilities of fcn_8 / fcn_32 on any encoder in the bf16 configuration."""
    fn = fcn32_logits_bf16_ref if fcn32 else fcn8_logits_bf16_ref
    return softmax_ref(fn(x_nhwc, p, encoder=encoder, rounding=rounding, accum=accum))
