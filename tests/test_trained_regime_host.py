"""CPU checks of tests/trained_regime.py: that the regime is what it claims, that the gate is not vacuous under it, and that
it discriminates -- all on the oracle (oracle/fcn_bf16_ref.py), no kernel runs here.

Why the regime exists.  Every kernel epilogue computes fmaf(acc, scale, shift), then the residual add, then ReLU / ReLU6,
then the 2x2 max.  Under the synth weights every folded scale is positive, and for a positive scale

    max over a 2x2 window of act(acc * s + sh)  ==  act(max(acc) * s + sh)        (rounding is monotone: the same bits)
    act(acc * |s| + sh)                         ==  act(acc * s + sh)

so an epilogue that pools before the affine (three of every four FMAs saved) or drops the sign of the scale passes every
test built on those weights BIT FOR BIT: test_synth_weights_cannot_see_pool_first_or_abs_scale asserts exactly that
equality -- it is the statement of the gap.  Under trained_regime() the same epilogues fail the teacher-forced gate
(oracle/fcn_bf16_ref.py gate_layer: slack = min(2e-5, max(4 x e32, 2^-23)) from the reference alone, in bf16 the half
step and the flip count) at every layer they apply to, by at least 1000 x the slack.

The wrong epilogues are restated HERE, on the oracle's own float64 accumulator of one layer (the conv of the layer's
rounded operands, before scale and shift; that the right epilogue on it gives the oracle's output bit for bit is asserted
for every layer), never in oracle/ and never in a kernel:

    (a) pool_first   2x2 max of the accumulators, then one affine and the activation      (pooled layers: vanilla enc1..5)
    (b) abs_scale    fmaf(acc, |scale|, shift)                                            (every BatchNorm layer)
    (c) act_first    ReLU / ReLU6 of the accumulator, then the affine                     (every layer with an activation)
    (d) res_after    the shortcut added after the ReLU                                    (ResNet50's 16 `2c` layers)

Shapes: the GPU cases' (tests/test_gpu_trained_regime.py) 1 x 32 x 32 and 3 x 64 x 96, vanilla also 3 x 96 x 160; free running
(every layer reads the oracle's own stored maps), in the fp32 arithmetic (Arith(fp32=True)) and the bf16 rounding one.

Printed by the tests below (inputs: default_rng(7) crops, regime seed 11).  Least non-zero share of a layer's exact output:
vanilla 0.567 (enc5, 3 x 96 x 160), MobileNet 0.476 (conv_dw_2, 1 x 32 x 32), ResNet50 0.444 (res2c_branch2b); tensor maxima 10 .. 40
(vanilla), 6 (MobileNet: 0.36 % .. 7.3 % of every ReLU6 layer at the clamp), 8.5 .. 106 (ResNet50).  Wrong epilogue over its slack,
smallest and largest factor over all layers, shapes and both arithmetics: pool_first 3.0e5 .. 2.6e6, abs_scale 1.7e5 .. 5.0e6,
act_first 3.6e5 .. 1.0e7, res_after 3.5e5 .. 1.0e7 -- the bar is 1000.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import enc_chain_cases as cases
import trained_regime as T
from oracle import fcn_bf16_ref as B
from oracle import fcn_ref

ENCODERS = ("vanilla", "mobilenet", "resnet50")
SHAPES = {"vanilla": ((1, 32, 32), (3, 64, 96), (3, 96, 160)), "mobilenet": ((1, 32, 32), (3, 64, 96)),
          "resnet50": ((1, 32, 32), (3, 64, 96))}
LARGE = (3, 64, 96)
ARITHS = {"f32": dict(fp32=True), "bf16": dict()}
VANILLA_CHAIN = tuple(B.Step("enc%d" % i, ("x" if i == 1 else "enc%d" % (i - 1),), bn="enc%d" % i, pad=1, relu=1, pool=1,
                             round_x=(i == 1)) for i in range(1, 6))
FAIL_FACTOR = 1000.0

_VANILLA, _REGIME, _RUNS = {}, {}, {}


def chain_of(enc):
    return VANILLA_CHAIN if enc == "vanilla" else B.ENCODER_CHAINS[enc]


def synth_params(enc):
    if enc == "vanilla":
        if not _VANILLA:
            from flm_amd.weights import synth_fcn8_weights
            _VANILLA["p"] = synth_fcn8_weights(68, seed=2)
        return _VANILLA["p"]
    return cases.encoder_params(enc, keep=2)             # MobileNet's and ResNet50's: drawn once for this module


def regime_params(enc):
    if enc not in _REGIME:
        _REGIME.clear()
        _REGIME[enc] = T.trained_regime(synth_params(enc))
    return _REGIME[enc]


def _input(shape):
    n, h, w = shape
    x = np.stack([fcn_ref.get_image_array_ref(c) for c in cases.crops(n, h, w)])
    return torch.from_numpy(x.astype(np.float64)).permute(0, 3, 1, 2).contiguous()


def _accumulator(A, st, p, xs):
    """The float64 accumulator of step `st` as oracle/fcn_bf16_ref.py _conv_block forms it: the conv of the operands,
    rounded where the arithmetic rounds them, before scale and shift."""
    kern = p[st.name + ("/depthwise_kernel" if st.depthwise else "/kernel")]
    w = B._weight(kern, (2, 3, 0, 1) if st.depthwise else (3, 2, 0, 1), st.kw.get("round_w", True) and A.rounding)
    x = A.q(xs[0]) if st.kw.get("round_x", False) else xs[0]
    return F.conv2d(x, w, None, stride=st.kw.get("stride", 1), padding=st.kw.get("pad", 0),
                    groups=kern.shape[2] if st.depthwise else 1)


def _col(v):
    return torch.from_numpy(np.asarray(v, np.float64))[None, :, None, None]


def _pool(y, pool):
    return F.max_pool2d(y, 2, 2) if pool else y


def right(acc, s, sh, res, relu, pool):
    y = acc * _col(s) + _col(sh)
    if res is not None:
        y = y + res
    return _pool(B._act(y, relu), pool)


def pool_first(acc, s, sh, res, relu, pool):      # (a)
    assert pool and res is None
    return B._act(F.max_pool2d(acc, 2, 2) * _col(s) + _col(sh), relu)


def abs_scale(acc, s, sh, res, relu, pool):       # (b)
    return right(acc, np.abs(s), sh, res, relu, pool)


def act_first(acc, s, sh, res, relu, pool):       # (c)
    y = B._act(acc, relu) * _col(s) + _col(sh)
    return _pool(y if res is None else y + res, pool)


def res_after(acc, s, sh, res, relu, pool):       # (d)
    return _pool(B._act(acc * _col(s) + _col(sh), relu) + res, pool)


WRONG = {"pool_first": pool_first, "abs_scale": abs_scale, "act_first": act_first, "res_after": res_after}


def applies(what, st):
    return {"pool_first": bool(st.pool), "abs_scale": True, "act_first": st.relu != 0, "res_after": len(st.inputs) > 1}[what]


def run(enc, regime, shape, arith):
    """One free-running pass of the oracle over `enc`'s chain; per conv layer a record of the exact output's statistics
    and of every applicable wrong epilogue's gate report.  Computed once per case and shared by the tests below."""
    key = (enc, regime, shape, arith)
    if key in _RUNS:
        return _RUNS[key]
    p, classes = regime_params(enc) if regime else (synth_params(enc), None)
    A, A32 = B.Arith(**ARITHS[arith]), B.Arith(accum=torch.float32, **ARITHS[arith])
    out, recs = {"x": _input(shape)}, []
    for st in chain_of(enc):
        xs = [out[i] for i in st.inputs]
        exact, stored = st(A, p, *xs)
        out[st.name] = stored
        if st.op != "conv":
            continue
        e32, s32 = st(A32, p, *xs)
        acc = _accumulator(A, st, p, xs)
        s, sh = B._fold(p, st.name, st.kw["bn"])
        res = xs[1] if len(xs) > 1 else None
        ex = exact.numpy()
        rec = dict(name=st.name, relu=st.relu, pool=st.pool, res=res is not None, scale=s, shift=sh,
                   restated=bool(torch.equal(right(acc, s, sh, res, st.relu, st.pool), exact)),
                   nonzero=float((ex != 0).mean()), max=float(np.abs(ex).max()), at6=float((ex == 6.0).mean()), wrong={})
        if classes is not None:
            cls = classes[st.kw["bn"]]
            rec["cls"] = cls
            rec["class_nonzero"] = {k: bool((ex[:, cls == k] != 0).any()) for k in range(7)}
        for what, fn in WRONG.items():
            if not applies(what, st):
                continue
            wrong = fn(acc, s, sh, res, st.relu, st.pool)
            rep = B.gate_layer(A.q(wrong).numpy(), ex, e32.numpy(), s32.numpy(), A.rounding)
            w = dict(equal=bool(torch.equal(wrong, exact)), over=rep["over"], slack=rep["slack"], ok=rep["ok"],
                     err=float((wrong - exact).abs().max() / exact.abs().max()))
            if classes is not None:
                neg = np.isin(cls, T.NEGATIVE)
                d = (wrong != exact).numpy()
                w["changed_on_negative"] = bool(d[:, neg].any())
                w["changed_elsewhere"] = bool(d[:, ~neg].any())
            rec["wrong"][what] = w
        recs.append(rec)
    _RUNS[key] = recs
    return recs


# ---- the regime ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("enc", ENCODERS)
def test_regime_is_what_it_claims(enc):
    p = synth_params(enc)
    before = {k: (id(v), v.copy()) for k, v in p.items() if v.size <= 4096}
    p2, classes = regime_params(enc)
    bns = T.bn_layers(p)
    assert len(bns) == {"vanilla": 5, "mobilenet": 27, "resnet50": 53}[enc] and list(classes) == bns
    chain_bn = {st.kw["bn"]: st for st in chain_of(enc) if st.op == "conv"}
    assert set(chain_bn) == set(bns)                     # every BatchNorm layer of the encoder, and nothing else
    touched = set()
    for bn in bns:
        conv = T.conv_of(bn)
        assert conv == chain_bn[bn].name, (bn, conv)     # the mapping is the oracle's chain's
        dw = conv + "/depthwise_kernel" in p
        kkey = conv + ("/depthwise_kernel" if dw else "/kernel")
        touched |= {kkey, conv + "/bias"} | {bn + "/" + t for t in ("gamma", "beta", "moving_mean", "moving_variance")}
        cls = classes[bn]
        n = cls.size
        assert n >= 32 and set(cls.tolist()) == set(range(7)), (bn, n)
        c = np.arange(n)
        assert np.array_equal(cls == T.ZERO, c % 16 == 6) and np.array_equal(np.isin(cls, (T.NEG,)), c % 4 == 1)
        assert np.array_equal(np.isin(cls, (T.SMALL, T.SMALL_NEG)), c % 8 == 3) and np.array_equal(np.isin(cls, (T.LARGE, T.LARGE_NEG)), c % 8 == 7)
        assert np.array_equal(np.isin(cls, (T.SMALL_NEG, T.LARGE_NEG)), (c % 4 == 3) & (c % 16 >= 8))
        scale, shift = B._fold(p2, conv, bn)
        scale0, _ = B._fold(p, conv, bn)
        neg = np.isin(cls, T.NEGATIVE)
        assert np.array_equal(scale < 0, neg), bn        # negative exactly on the negated channels
        assert np.array_equal(scale == 0, cls == T.ZERO) and (scale0 > 0).all(), bn
        z = np.flatnonzero(cls == T.ZERO)
        assert np.array_equal(shift[z], p2[bn + "/beta"][z].astype(np.float64)), bn
        assert np.array_equal(p2[bn + "/beta"][z], np.asarray(T.ZERO_BETAS, np.float32)[np.arange(z.size) % 3]), bn
        g0 = np.abs(p[bn + "/gamma"].astype(np.float64))
        assert np.array_equal(np.abs(p2[bn + "/gamma"])[cls != T.ZERO], np.abs(p[bn + "/gamma"])[cls != T.ZERO]), bn   # the synth magnitudes
        for k, (lo, hi) in T.SCALE_RATIO.items():
            ratio = np.abs(scale[cls == k]) / g0[cls == k]
            assert (ratio >= lo * (1 - 1e-6)).all() and (ratio <= hi * (1 + 1e-6)).all(), (bn, T.CLASS_NAMES[k], ratio.min(), ratio.max())
        # the pre-BatchNorm statistics follow the variance: the normalised mean and the normalised kernel stay the synth set's
        sd0, sd2 = (np.sqrt(q[bn + "/moving_variance"].astype(np.float64) + T.EPS) for q in (p, p2))
        np.testing.assert_allclose(p2[bn + "/moving_mean"] / sd2, p[bn + "/moving_mean"] / sd0, rtol=2e-7, atol=0)
        k0, k2 = (np.moveaxis(q[kkey].astype(np.float64), 2 if dw else 3, -1) for q in (p, p2))
        np.testing.assert_allclose(k2 / sd2, k0 / sd0, rtol=2e-7, atol=0)
        # channels whose variance stays keep every bit of kernel, bias, mean and variance; KEEP channels of everything
        same_var = ~np.isin(cls, (T.SMALL, T.SMALL_NEG, T.LARGE, T.LARGE_NEG))
        assert np.array_equal(k2[..., same_var], k0[..., same_var]), bn
        for t in ("moving_mean", "moving_variance") + (() if conv + "/bias" not in p else ("bias",)):
            key = (conv if t == "bias" else bn) + "/" + t
            assert np.array_equal(p2[key][same_var], p[key][same_var]), key
        for t in ("gamma", "beta"):
            assert np.array_equal(p2[bn + "/" + t][cls == T.KEEP], p[bn + "/" + t][cls == T.KEEP]), (bn, t)
    # nothing else is touched, and the input set is left as it was
    assert set(p2) == set(p)
    for k in p:
        assert (p2[k] is p[k]) == (k not in touched), k
    for k, (i, v) in before.items():
        assert id(p[k]) == i and np.array_equal(p[k], v), k
    # the same layer gets the same statistics whatever else the dict holds
    one = bns[len(bns) // 2]
    sub = {k: v for k, v in p.items() if k.split("/")[0] in (one, T.conv_of(one))}
    assert np.array_equal(T.trained_regime(sub)[0][one + "/moving_variance"], p2[one + "/moving_variance"])


def test_zero_class_constant():
    sh = np.array([0.5, -0.5, 6.5], np.float32)
    assert T.zero_class_expected(sh, 1, False).tolist() == [0.5, 0.0, 6.5]
    assert T.zero_class_expected(sh, 2, False).tolist() == [0.5, 0.0, 6.0]
    assert T.zero_class_expected(sh, 0, True).tolist() == [0.5, -0.5, 6.5]
    assert T.zero_class_expected(np.float32([0.1]), 1, True).tolist() == [float(B.round_bf16(np.float32([0.1]))[0])]


def test_vanilla_chain_is_the_oracles_vanilla_encoder():
    """The Steps this module walks the vanilla encoder with are layer_bf16_ref's enc1 .. enc5, bit for bit."""
    p, _ = regime_params("vanilla")
    for arith, kw in ARITHS.items():
        A = B.Arith(**kw)
        x = _input((1, 32, 32))
        for st in VANILLA_CHAIN:
            exact, stored = st(A, p, x)
            e, s = B.layer_bf16_ref(st.name, x.permute(0, 2, 3, 1).numpy(), p, **kw)
            assert np.array_equal(exact.permute(0, 2, 3, 1).numpy(), e) and np.array_equal(stored.permute(0, 2, 3, 1).numpy(), s)
            x = stored


# ---- non-vacuity and sensitivity, on the oracle alone -------------------------------------------------------------------

CASES = [(enc, shape, arith) for enc in ENCODERS for shape in SHAPES[enc] for arith in ARITHS]
IDS = ["%s-%dx%dx%d-%s" % (e, *s, a) for e, s, a in CASES]


@pytest.mark.parametrize("enc,shape,arith", CASES, ids=IDS)
def test_gate_is_not_vacuous_under_the_regime(enc, shape, arith):
    recs = run(enc, True, shape, arith)
    assert [r["name"] for r in recs] == [st.name for st in chain_of(enc) if st.op == "conv"]
    for r in recs:
        assert r["restated"], r["name"]                  # this module's accumulator and epilogue are the oracle's
        assert r["nonzero"] >= 0.25, (r["name"], r["nonzero"])
        for k in range(7):
            if k != T.ZERO:
                assert r["class_nonzero"][k], (r["name"], T.CLASS_NAMES[k])
        if r["relu"] == 2 and shape == LARGE:
            assert r["at6"] > 0, r["name"]
        for what, w in r["wrong"].items():
            assert w["changed_on_negative"], (r["name"], what)
    lo = min(recs, key=lambda r: r["nonzero"])
    print("%s %s %s: least non-zero share %.3f (%s), tensor maxima %.3g .. %.3g; ReLU6 clamp share %.4f .. %.4f"
          % (enc, shape, arith, lo["nonzero"], lo["name"], min(r["max"] for r in recs), max(r["max"] for r in recs),
             min((r["at6"] for r in recs if r["relu"] == 2), default=0), max((r["at6"] for r in recs if r["relu"] == 2), default=0)))


@pytest.mark.parametrize("enc,shape,arith", CASES, ids=IDS)
def test_wrong_epilogues_fail_the_gate_under_the_regime(enc, shape, arith):
    recs = run(enc, True, shape, arith)
    seen = {}
    for r in recs:
        for what, w in r["wrong"].items():
            seen.setdefault(what, []).append(w["over"] / w["slack"])
            assert not w["ok"] and w["over"] >= FAIL_FACTOR * w["slack"], (r["name"], what, w)
            if what in ("pool_first", "abs_scale"):      # exact wherever the scale is not negative
                assert not w["changed_elsewhere"], (r["name"], what)
    want = {"vanilla": {"pool_first": 5, "abs_scale": 5, "act_first": 5}, "mobilenet": {"abs_scale": 27, "act_first": 27},
            "resnet50": {"abs_scale": 53, "act_first": 49, "res_after": 16}}[enc]
    assert {k: len(v) for k, v in seen.items()} == want
    for what, v in seen.items():
        print("%s %s %s %-10s over / slack %.3g .. %.3g over %d layers" % (enc, shape, arith, what, min(v), max(v), len(v)))


@pytest.mark.parametrize("enc,arith", [(e, a) for e in ENCODERS for a in ARITHS])
def test_synth_weights_cannot_see_pool_first_or_abs_scale(enc, arith):
    """The gap: under the plain synth weights (a) and (b) give the right epilogue's bits at every layer."""
    recs = run(enc, False, LARGE, arith)
    n = 0
    for r in recs:
        assert r["restated"] and (r["scale"] > 0).all(), r["name"]
        for what in ("pool_first", "abs_scale"):
            if what in r["wrong"]:
                assert r["wrong"][what]["equal"] and r["wrong"][what]["ok"], (r["name"], what)
                n += 1
    assert n == {"vanilla": 10, "mobilenet": 27, "resnet50": 53}[enc]
