"""CPU checks of the fp32 arithmetic of oracle/fcn_bf16_ref.py (layer_f32_ref / fp32=True) and of the teacher-forced
fp32 gate tests/test_gpu_fp32_layers.py builds on it (tests/bf16_gate.py, dtype="f32").

  * the fp32 arithmetic in float64 is fcn_ref's float64 layer up to the float32 storage of the folded scale / shift:
    per element, before ReLU and the 2x2 max (both 1-Lipschitz),

        |folded - fcn_ref| <= |a s| (2^-24 + de) + |sh| 2^-24 + |(b - mean) s| de + 2^-40 (A |s| + (|b| + |mean|) |s| + |beta|)

    a = sum x w, A = sum |x||w|, s = gamma / sqrt(var + eps), sh = (b - mean) s + beta; 2^-24: one rounding to float32 of
    s and of sh; de = |float32(1e-3) - 1e-3| / (2 (var + 1e-3)), the packer's float32 epsilon against fcn_ref's double;
    the last term is the float64 rounding of either evaluation.  Layers without BatchNorm fold to scale 1 and a shift
    that IS the float32 bias: only the last term is left.  rounding=False itself stays fcn_ref bit for bit (pinned in
    tests/test_oracle_fcn_bf16.py);
  * the gate passes two float32 summation orders of the same layer (torch's float32 convolution; one float32 matmul per
    filter tap / kernel position, added in turn) and fails each wrong kernel: a dropped 32-channel k-run in fc6, a
    clamped instead of zero border tap in enc3, a skip crop shifted by one pixel in fuse4, the far tap (i0 - 1) of one
    phase row dropped in up3, a pad class admitted into the softmax sum, non-zero class pad columns.

One 128 x 128 face through the full-size vanilla fcn_8 (seed 2), every layer fed the float32-stored output of the one
before.  Printed by the tests below: e32 2.6e-7 .. 5.5e-7 per layer (slack 1.0e-6 .. 2.2e-6); the tap-serial float32
fc6 uses 0.23 of its slack, the position-serial up3 0.12; the wrong kernels are over their slack by factors of 5.6e4
(fc6 k-run: 7.0e-2 of the maximum), 1.4e5 (enc3 border tap: 0.20), 4.1e5 (fuse4 crop: 0.92), 6.3e5 (up3 far tap: 0.64);
the admitted pad class moves the probabilities by 3.4e-3 against the bar of 1e-5.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import fcn_bf16_ref as B
from oracle import fcn_ref
from test_oracle_fcn import tiny_params

LAYERS = ("enc1", "enc2", "enc3", "enc4", "enc5", "fc6", "fc7", "score5", "fuse4", "seg_feats", "logits")


def _chain(x, p):
    """Teacher-forced inputs of every layer: the fp32 arithmetic's own maps, stored as float32 like the device's."""
    it, src = {"x": x}, {}
    for name, layer, srcs in (("f1", "enc1", ("x",)), ("f2", "enc2", ("f1",)), ("f3", "enc3", ("f2",)), ("f4", "enc4", ("f3",)),
                              ("f5", "enc5", ("f4",)), ("fc6", "fc6", ("f5",)), ("fc7", "fc7", ("fc6",)),
                              ("score5", "score5", ("fc7",)), ("fuse4", "fuse4", ("score5", "f4")),
                              ("seg_feats", "seg_feats", ("fuse4", "f3")), ("logits", "logits", ("seg_feats",))):
        xin = it[srcs[0]] if len(srcs) == 1 else tuple(it[s] for s in srcs)
        src[layer] = xin
        it[name] = B.layer_f32_ref(layer, xin, p).astype(np.float32).astype(np.float64)
    return it, src


def _nchw(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64))).permute(0, 3, 1, 2)


def _conv64(x, k_hwio, pad):
    return F.conv2d(_nchw(x), torch.from_numpy(np.asarray(k_hwio, np.float64)).permute(3, 2, 0, 1), None, padding=pad)


def _convt64(x, k_hwoi, s):
    return F.conv_transpose2d(_nchw(x), torch.from_numpy(np.asarray(k_hwoi, np.float64)).permute(3, 2, 0, 1), None, stride=s)


def test_fp32_arithmetic_is_fcn_ref_up_to_the_float32_fold():
    p = tiny_params(5, seed=2)
    x = (np.random.default_rng(6).standard_normal((2, 64, 96, 3)) * 50).astype(np.float32)
    _, src = _chain(x, p)
    u24, u40 = 2.0 ** -24, 2.0 ** -40
    for layer in LAYERS:
        xin = src[layer]
        got = B.layer_f32_ref(layer, xin, p)
        ref, _ = B.layer_bf16_ref(layer, xin, p, rounding=False)
        assert got.dtype == np.float64 and got.shape == ref.shape, layer
        if layer.startswith("enc") or layer in ("fc6", "fc7", "score5"):
            k = p[layer + "/kernel"].astype(np.float64)
            a, A = _conv64(xin, k, k.shape[0] // 2), _conv64(np.abs(xin), np.abs(k), k.shape[0] // 2)
            col = lambda v: torch.from_numpy(np.asarray(v, np.float64))[None, :, None, None]
            b = p[layer + "/bias"].astype(np.float64)
            if layer.startswith("enc"):
                var, mean, beta = (p[layer + "/" + t].astype(np.float64) for t in ("moving_variance", "moving_mean", "beta"))
                s = p[layer + "/gamma"].astype(np.float64) / np.sqrt(var + 1e-3)
                sh = (b - mean) * s + beta
                de = abs(float(np.float32(1e-3)) - 1e-3) / (2 * (var + 1e-3))
                bound = a.abs() * col(np.abs(s) * (u24 + de)) + col(np.abs(sh) * u24 + np.abs((b - mean) * s) * de) \
                    + u40 * (A * col(np.abs(s)) + col((np.abs(b) + np.abs(mean)) * np.abs(s) + np.abs(beta)))
                bound = F.max_pool2d(bound, 2, 2)
                sc, sf = B._fold(p, layer, layer)          # what the fold stores IS float32, next to the float64 value
                assert np.array_equal(sc, sc.astype(np.float32)) and np.array_equal(sf, sf.astype(np.float32))
                assert (np.abs(sc - s) <= np.abs(s) * (u24 + de) * 1.001).all() and (np.abs(sf - sh) <= np.abs(sh) * u24 + np.abs((b - mean) * s) * de * 1.001 + 1e-300).all()
            else:
                bound = u40 * (A + col(np.abs(b)))
                sc, sf = B._fold(p, layer, None)
                assert np.array_equal(sc, np.ones_like(sc)) and np.array_equal(sf, b)
            bound = bound.permute(0, 2, 3, 1).numpy()
        else:
            up, score, s = dict(fuse4=("up5", "score4", 2), seg_feats=("up4", "score3", 2), logits=("up3", None, 8))[layer]
            bound = _convt64(np.abs(xin[0] if score else xin), np.abs(p[up + "/kernel"]), s) * u40
            if score:
                b2 = (_conv64(np.abs(xin[1]), np.abs(p[score + "/kernel"]), 0) + np.abs(p[score + "/bias"]).max()) * u40
                bound = bound[:, :, : b2.shape[2], : b2.shape[3]] + b2
            bound = bound.permute(0, 2, 3, 1).numpy()
        diff = np.abs(got - ref)
        print("%-9s max |fp32 arithmetic - fcn_ref| %.3g of the maximum, largest share of its bound %.3g" % (
            layer, diff.max() / np.abs(ref).max(), (diff / bound).max()))
        assert diff.shape == bound.shape and (diff <= bound).all(), (layer, float((diff - bound).max()))
        if layer.startswith("enc"):   # the float32 storage of scale / shift is restated: it moves the layer
            assert diff.max() >= 1e-3 * bound.max(), (layer, diff.max(), bound.max())
        # accum is honoured: float32 sums differ from float64 ones, by float32 rounding
        g32 = B.layer_f32_ref(layer, xin, p, accum=torch.float32)
        e = np.abs(g32 - got).max() / np.abs(got).max()
        assert 0 < e < 2e-6, (layer, e)
    # existing callers keep their results: the default is still the bf16 arithmetic, rounding off still fcn_ref
    assert not np.array_equal(B.layer_bf16_ref("fc6", src["fc6"], p)[0], B.layer_f32_ref("fc6", src["fc6"], p))
    assert B.Arith(False, torch.float32).accum == torch.float64 and not B.Arith(False).folded
    assert B.Arith(True, torch.float32, fp32=True).accum == torch.float32 and not B.Arith(fp32=True).rounding


# ---- the gate: float32 summation orders pass, wrong kernels fail ----------------------------------------------

@pytest.fixture(scope="module")
def face():
    from flm_amd.weights import synth_fcn8_weights
    p = synth_fcn8_weights(68, seed=2)
    img = np.random.default_rng(3).integers(0, 256, (1, 128, 128, 3), dtype=np.uint8)
    it, src = _chain(np.stack([fcn_ref.get_image_array_ref(im) for im in img]), p)
    return p, it, src


def _gate(got, layer, xin, p):
    exact = B.layer_f32_ref(layer, xin, p)
    r32 = B.layer_f32_ref(layer, xin, p, accum=torch.float32)
    rep = B.gate_layer(got, exact, r32, r32, False)
    return rep, exact


def test_float32_accumulation_passes_the_fp32_gate(face):
    p, it, src = face
    for layer in LAYERS:
        r32 = B.layer_f32_ref(layer, src[layer], p, accum=torch.float32)
        rep, exact = _gate(r32, layer, src[layer], p)
        print(B.format_report(layer, rep).replace("over-half-step", "error"))
        assert rep["ok"] and "flips" not in rep, (layer, rep)
        assert 0 < rep["e32"] < 1e-6 and rep["slack"] < B.SLACK_CAP, (layer, rep)


def test_fc6_fp32_gate_passes_another_order_and_fails_a_dropped_k_run(face):
    p, it, src = face
    f5, w, b = src["fc6"], p["fc6/kernel"], p["fc6/bias"]          # [1, 4, 4, 256]
    x = np.pad(f5.astype(np.float32), ((0, 0), (3, 3), (3, 3), (0, 0)))
    acc = np.zeros((1, 4, 4, 4096), np.float32)
    for ky in range(7):                                              # one float32 matmul per tap, taps added in turn
        for kx in range(7):
            acc += x[:, ky:ky + 4, kx:kx + 4, :] @ w[ky, kx]
    rep, exact = _gate(np.maximum(acc + b, np.float32(0)).astype(np.float64), "fc6", f5, p)
    print("fc6 tap-serial float32:", B.format_report("fc6", rep).replace("over-half-step", "error"))
    assert rep["ok"] and rep["over"] > 0, rep
    pre = _conv64(f5, w, 3).permute(0, 2, 3, 1).numpy() + b.astype(np.float64)
    assert np.abs(np.maximum(pre, 0) - exact).max() <= 1e-12 * np.abs(exact).max()     # the harness is the oracle's fc6
    bad = np.maximum(pre - f5[..., 64:96] @ w[3, 3, 64:96, :].astype(np.float64), 0)    # centre tap, channels 64..95
    rep, _ = _gate(bad, "fc6", f5, p)
    print("fc6 k-run dropped:", B.format_report("fc6", rep).replace("over-half-step", "error"))
    assert not rep["ok"] and rep["over"] > 100 * rep["slack"], rep


def test_encoder_fp32_gate_fails_a_clamped_border_tap(face):
    p, it, src = face
    f2, w = src["enc3"], p["enc3/kernel"].astype(np.float64)        # [1, 32, 32, 128]
    sc, sh = B._fold(p, "enc3", "enc3")

    def layer(pre):
        y = np.maximum(pre * sc + sh, 0)
        return y.reshape(1, 16, 2, 16, 2, -1).max(axis=(2, 4))

    pre = _conv64(f2, w, 1).permute(0, 2, 3, 1).numpy()
    rep, exact = _gate(layer(pre), "enc3", f2, p)
    assert rep["ok"] and rep["over"] < 1e-12, rep                    # the harness is the oracle's enc3
    bad = pre.copy()
    bad[:, 0] += f2[:, 0] @ w[0, 1]        # tap (ky, kx) = (0, 1) of output row 0 reads row -1: taken from row 0, not zero
    rep, _ = _gate(layer(bad), "enc3", f2, p)
    print("enc3 clamped border tap:", B.format_report("f3", rep).replace("over-half-step", "error"))
    assert not rep["ok"] and rep["over"] > 100 * rep["slack"], rep


def test_fuse4_fp32_gate_fails_a_shifted_skip_crop(face):
    p, it, src = face
    score5, f4 = src["fuse4"]                                        # [1, 4, 4, 68], [1, 8, 8, 256]
    up = _convt64(score5, p["up5/kernel"], 2).permute(0, 2, 3, 1).numpy()          # [1, 10, 10, 68]
    s4 = _conv64(f4, p["score4/kernel"], 0).permute(0, 2, 3, 1).numpy() + p["score4/bias"].astype(np.float64)
    rep, exact = _gate(up[:, :8, :8] + s4, "fuse4", (score5, f4), p)
    assert rep["ok"] and rep["over"] < 1e-12, rep                    # the harness is the oracle's fuse4
    rep, _ = _gate(up[:, 1:9, :8] + s4, "fuse4", (score5, f4), p)   # the crop window one row down
    print("fuse4 crop shifted by one row:", B.format_report("fuse4", rep).replace("over-half-step", "error"))
    assert not rep["ok"] and rep["over"] > 100 * rep["slack"], rep


def test_up3_fp32_gate_passes_another_order_and_fails_wrong_kernels(face):
    p, it, src = face
    seg, w = src["logits"], p["up3/kernel"]                          # [1, 16, 16, 68], (16, 16, out, in)
    n, hi, wi, c = seg.shape

    def scatter(x, wk, dtype):
        out = np.zeros((n, 8 * (hi - 1) + 16, 8 * (wi - 1) + 16, wk.shape[2]), dtype)
        xd = x.astype(dtype)
        for a in range(16):
            for b in range(16):
                out[:, a:a + 8 * hi:8, b:b + 8 * wi:8, :] += xd @ wk[a, b].astype(dtype).T
        return out

    rep, exact = _gate(scatter(seg, w, np.float32).astype(np.float64), "logits", seg, p)
    print("up3 position-serial float32:", B.format_report("logits", rep).replace("over-half-step", "error"))
    assert rep["ok"] and rep["over"] > 0, rep
    assert np.abs(scatter(seg, w, np.float64) - exact).max() <= 1e-12 * np.abs(exact).max()
    # the far tap of phase row a0 = 4 dropped: output rows 8 i0 + 4 lose kernel row 12 applied to input row i0 - 1
    w_far = w.copy()
    w_far[12] = 0
    rep, _ = _gate(scatter(seg, w_far, np.float64), "logits", seg, p)
    print("up3 far tap of one phase row dropped:", B.format_report("logits", rep).replace("over-half-step", "error"))
    assert not rep["ok"] and rep["over"] > 100 * rep["slack"], rep
    # non-zero class pad columns (a 72-column seg_feats whose columns 68..71 are not zeros)
    segp = np.concatenate([seg, np.zeros((n, hi, wi, 4))], -1)
    fuse4, f3 = src["seg_feats"]
    rep, _ = _gate(segp, "seg_feats", (fuse4, f3), p)
    assert rep["ok"] and "pad" not in rep, rep                       # zero pad columns: the layer itself passes
    segp[0, 3, 5, 70] = 1e-30
    rep, _ = _gate(segp, "seg_feats", (fuse4, f3), p)
    assert not rep["ok"] and rep["pad"] == 1e-30, rep
    # a pad class admitted into the softmax sum: the 16 m + 4 q + e < C mask off by one admits a logit of 0
    good = B.softmax_ref(exact)
    assert B.probs_report(good.astype(np.float32), exact)["ok"]
    lg = np.concatenate([exact, np.zeros(exact.shape[:3] + (1,))], -1)
    bad = B.softmax_ref(lg)[..., :c]
    rep = B.probs_report(bad.astype(np.float32), exact)
    print("softmax with one pad class admitted: max-abs error %.3g (bar %g), rows sum to 1 within %.3g" % (
        rep["err"], B.PROBS_BAR, np.abs(bad.sum(-1) - 1).max()))
    assert not rep["ok"] and rep["err"] > 100 * B.PROBS_BAR, rep
