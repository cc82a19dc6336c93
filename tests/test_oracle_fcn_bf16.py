"""CPU checks of oracle/fcn_bf16_ref.py, the float64 restatement of the bf16 configuration that rounds where the
kernels round, and of the gate tests/test_gpu_bf16_layers.py builds on it.

  * round_bf16 against a bit-level numpy restatement (ties to even, one float32 step on either side of a tie,
    negative values and +-0, the largest finite values, subnormal inputs) and against torch's bfloat16 cast;
  * rounding off: the float64 oracle bit for bit, all four encoders, fcn_8 and fcn_32; rounding on: each layer,
    given the same input, moves by no more than a half step per rounded operand predicts -- and does move;
  * the gate is neither too tight nor vacuous: float32 accumulation of the same rounded operands (torch's float32
    convolutions, and a tap-serial float32 sum in another order again) passes it at every layer; a dropped
    32-channel k-run of one tap, one border tap read from the clamped neighbour, and non-zero class pad columns
    68..71 each fail it (fc6 on an 8x8 map, up3) -- the dropped k-run of fc6 by a factor of 40,000, while it
    stayed inside the 4e-2 of the tensor's maximum the suite asked of fc6 before.

Reference-side values at one 256 x 256 face (seed 3; printed by test_float32_accumulation_passes_the_gate):
e32 = largest error of torch's float32 evaluation of the same rounded operands against float64, relative to the
tensor's maximum; the gate's slack is min(2e-5, max(4 * e32, 2^-23)).

    layer      e32       slack      flips of the float32 evaluation
    f1         1.1e-07   4.5e-07    9 / 1,048,576
    f2         1.6e-07   6.4e-07    22 / 524,288
    f3         2.2e-07   8.7e-07    16 / 262,144
    f4         2.0e-07   7.9e-07    4 / 65,536
    f5         1.8e-07   7.3e-07    1 / 16,384
    fc6        2.3e-07   9.2e-07    21 / 262,144   (tap-serial float32 sums: 4.4e-08 over the half step, 17 flips)
    fc7        1.9e-07   7.4e-07    16 / 262,144
    score5     1.7e-07   6.6e-07
    fuse4      1.1e-07   4.5e-07
    seg_feats  2.4e-07   9.4e-07
    logits     1.4e-07   5.5e-07

The wrong kernels against those: fc6 with a dropped k-run is 3.9e-2 of the maximum over the half step and flips 49.8 % of
the elements (clamped border tap: 1.3e-1, 20 %); up3 0.32 / 0.40 / 0.29 of the maximum (k-run, border tap, pad classes).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import fcn_bf16_ref as B
from oracle import fcn_ref
from test_oracle_fcn import tiny_params


# ---- the rounding helper -----------------------------------------------------------------------------------

def _bits_round(u32):
    """float32 bit patterns -> bf16 bit patterns << 16, round to nearest even on the integer image."""
    u = u32.astype(np.uint64)
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16).astype(np.uint32)


def _special_bits():
    rng = np.random.default_rng(0)
    hi = np.concatenate([rng.integers(0, 0x7F80, 4000), [0x0000, 0x0001, 0x007F, 0x0080, 0x3F80, 0x7F7E, 0x7F7F]]).astype(np.uint32)
    lows = np.array([0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF], np.uint32)  # exact, above, below a tie, tie, ...
    u = (hi[:, None] << 16 | lows[None, :]).ravel()
    u = np.concatenate([u, rng.integers(0, 0x7F800000, 200000).astype(np.uint32),
                        rng.integers(0, 0x00800000, 20000).astype(np.uint32)])      # subnormal float32 inputs
    return np.concatenate([u, u | np.uint32(0x80000000)])                            # and their negatives (-0 too)


def test_round_bf16_matches_the_bit_level_restatement():
    u = _special_bits()
    x = u.view(np.float32)
    assert np.isfinite(x).all()
    exp = _bits_round(u).view(np.float32).astype(np.float64)
    assert x.size < (1 << 20)
    big = np.tile(x, 4)                                              # above 2^20 elements: the float32 form of the helper
    assert big.size > (1 << 20) and np.array_equal(B.round_bf16(big), np.tile(exp, 4))
    assert np.array_equal(np.signbit(B.round_bf16(big)), np.signbit(np.tile(exp, 4)))
    got = B.round_bf16(x)                                            # the float64 form
    assert np.array_equal(got, exp)
    assert np.array_equal(B.round_bf16(x.astype(np.float64)), exp)
    assert np.array_equal(np.signbit(got), np.signbit(exp))          # -0 stays -0
    # a third witness: torch's cast
    tt = torch.from_numpy(x.copy()).to(torch.bfloat16).to(torch.float64).numpy()
    assert np.array_equal(got, tt)
    # the named cases, spelled out
    f = lambda b: np.array([b], np.uint32).view(np.float32)[0]
    assert B.round_bf16(f(0x3F808000)) == 1.0                        # tie, even below
    assert B.round_bf16(f(0x3F818000)) == 1.0 + 2.0 ** -6            # tie, even above
    assert B.round_bf16(f(0x3F807FFF)) == 1.0 and B.round_bf16(f(0x3F808001)) == 1.0 + 2.0 ** -7
    assert B.round_bf16(f(0x7F7F7FFF)) == (2 - 2.0 ** -7) * 2.0 ** 127   # largest finite bf16
    assert np.isposinf(B.round_bf16(f(0x7F7F8000))) and np.isneginf(B.round_bf16(f(0xFF7FFFFF)))
    assert B.round_bf16(f(0x00000001)) == 0.0 and B.round_bf16(f(0x00008001)) == 2.0 ** -133
    assert B.round_bf16(f(0x00008000)) == 0.0 and B.round_bf16(f(0x00018000)) == 2.0 ** -132   # subnormal ties
    assert np.isnan(B.round_bf16(np.nan))


def test_round_bf16_rounds_float64_once():
    """A float64 just above a tie must round up; a detour through float32 would land on the tie and round to even."""
    x = 1.0 + 2.0 ** -8 + 2.0 ** -40
    assert float(np.float32(x)) == 1.0 + 2.0 ** -8
    assert B.round_bf16(x) == 1.0 + 2.0 ** -7
    assert B.round_bf16(-x) == -(1.0 + 2.0 ** -7)
    assert B.round_bf16(1.0 + 2.0 ** -8 - 2.0 ** -40) == 1.0
    v = np.random.default_rng(1).standard_normal(10000) * 10.0 ** np.random.default_rng(2).integers(-30, 30, 10000)
    r = B.round_bf16(v)
    assert np.array_equal(B.round_bf16(r), r)                        # idempotent
    assert (np.abs(r - v) <= 0.5 * B.ulp_bf16(v)).all()
    assert np.array_equal(B.ulp_bf16(np.array([1.0, 1.99, 2.0, -0.75, 0.0])), 2.0 ** np.array([-7.0, -7, -6, -8, -133]))


# ---- rounding off: the float64 oracle, bit for bit ---------------------------------------------------------------

def _narrow_head(p, c5, n_classes, fc=16, seed=9):
    """The synthetic full-size encoders with a 16-wide head (the float64 fc6 of a 2048-channel f5 is 3 GB)."""
    rng = np.random.default_rng(seed)
    p = dict(p)
    p["fc6/kernel"] = (rng.standard_normal((7, 7, c5, fc)) * 0.02).astype(np.float32)
    p["fc6/bias"] = (rng.standard_normal(fc) * 0.1).astype(np.float32)
    p["fc7/kernel"] = (rng.standard_normal((1, 1, fc, fc)) * 0.3).astype(np.float32)
    p["fc7/bias"] = (rng.standard_normal(fc) * 0.1).astype(np.float32)
    p["score5/kernel"] = (rng.standard_normal((1, 1, fc, n_classes)) * 0.3).astype(np.float32)
    return p


def _encoder_cases():
    from flm_amd.weights import synth_mobilenet_weights, synth_resnet50_weights, synth_vgg_weights
    yield "vanilla", tiny_params(5, seed=1), None
    for enc, synth, c5 in (("vgg", synth_vgg_weights, 512), ("mobilenet", synth_mobilenet_weights, 1024),
                           ("resnet50", synth_resnet50_weights, 2048)):
        yield enc, _narrow_head(synth(5, seed=3), c5, 5), _narrow_head(synth(5, seed=3, fcn32=True), c5, 5)


@pytest.mark.parametrize("enc", ["vanilla", "vgg", "mobilenet", "resnet50"])
def test_rounding_off_is_the_float64_oracle_bit_for_bit(enc):
    name, p8, p32 = next(c for c in _encoder_cases() if c[0] == enc)
    x = (np.random.default_rng(4).standard_normal((2, 32, 64, 3)) * 50).astype(np.float32)
    lg, it = B.fcn8_logits_bf16_ref(x, p8, return_intermediates=True, encoder=enc, rounding=False)
    lg_ref, it_ref = fcn_ref.fcn8_logits_ref(x, p8, torch.float64, return_intermediates=True, encoder=enc)
    assert lg.dtype == np.float64 and np.array_equal(lg, lg_ref)
    for k in it_ref:
        assert np.array_equal(it[k], it_ref[k]), k
    assert set(it) == set(it_ref) | {"score5"}
    assert np.array_equal(B.predict_bf16_ref(x, p8, encoder=enc, rounding=False),
                          fcn_ref.fcn8_predict_ref(x, p8, torch.float64, encoder=enc))
    if p32 is None:
        p32 = dict(p8)
        p32["up32/kernel"] = (np.random.default_rng(5).standard_normal((64, 64, 5, 5)) * 0.05).astype(np.float32)
    assert np.array_equal(B.fcn32_logits_bf16_ref(x, p32, encoder=enc, rounding=False),
                          fcn_ref.fcn32_logits_ref(x, p32, torch.float64, encoder=enc))
    # rounding on: another network, still close (every operand carries 2^-9)
    on = B.fcn8_logits_bf16_ref(x, p8, encoder=enc)
    assert not np.array_equal(on, lg_ref) and np.abs(on - lg_ref).max() < 0.1 * np.abs(lg_ref).max()
    assert np.abs(B.predict_bf16_ref(x, p8, encoder=enc).sum(-1) - 1).max() < 1e-12


# ---- rounding on: what 2^-9 per operand predicts, layer by layer --------------------------------------------------

def _abs_conv(x, k_hwio, pad):
    return F.conv2d(torch.from_numpy(np.abs(x).astype(np.float64)).permute(0, 3, 1, 2), torch.from_numpy(np.abs(k_hwio).astype(np.float64)).permute(3, 2, 0, 1),
                    None, padding=pad)


def _abs_convt(x, k_hwoi, s):
    return F.conv_transpose2d(torch.from_numpy(np.abs(x).astype(np.float64)).permute(0, 3, 1, 2),
                              torch.from_numpy(np.abs(k_hwoi).astype(np.float64)).permute(3, 2, 0, 1), None, stride=s)


def test_rounding_moves_every_layer_by_what_the_operand_roundings_predict():
    """Teacher-forced at a small shape: the layer's input is the rounding oracle's own (bf16-valued) map, evaluated
    once with and once without rounding.  Per element |on - off| <= sum |x||w| * d * |scale| (+ the float32 rounding
    of scale / shift), d = 2^-8 for one rounded operand per product (the half step of an 8-bit significand: 2^-9 of the top
    of the value's binade, at most 2^-8 of the value itself) and 2 * 2^-8 + 2^-16 for two; ReLU and the 2x2 max are 1-Lipschitz.  The largest difference must also reach 2 % of the largest bound: the roundings happen."""
    p = tiny_params(5, seed=2)
    d1, d2 = 2.0 ** -8, 2.0 ** -7 + 2.0 ** -16
    x = (np.random.default_rng(6).standard_normal((2, 64, 96, 3)) * 50).astype(np.float32)
    _, it = B.fcn8_logits_bf16_ref(x, p, return_intermediates=True)
    src = dict(enc1=x, enc2=it["f1"], enc3=it["f2"], enc4=it["f3"], enc5=it["f4"], fc6=it["f5"], fc7=it["fc6"],
               score5=it["fc7"], fuse4=(it["score5"], it["f4"]), seg_feats=(it["fuse4"], it["f3"]), logits=it["seg_feats"])
    for layer, xin in src.items():
        on, stored = B.layer_bf16_ref(layer, xin, p)
        off, _ = B.layer_bf16_ref(layer, xin, p, rounding=False)
        if layer.startswith("enc") or layer in ("fc6", "fc7", "score5"):
            k = p[layer + "/kernel"]
            scale, shift = B._fold(p, layer, layer if layer.startswith("enc") else None)
            s64 = np.ones(k.shape[3]) if not layer.startswith("enc") else \
                p[layer + "/gamma"].astype(np.float64) / np.sqrt(p[layer + "/moving_variance"].astype(np.float64) + 1e-3)
            acc_abs = _abs_conv(xin, k, k.shape[0] // 2)
            bound = acc_abs * (d2 if layer == "enc1" else d1) * torch.from_numpy(np.abs(s64))[None, :, None, None]
            # scale / shift are float32 (2^-24 relative each; eps is a float32 too: 5e-11 relative to var + eps)
            bound = bound + (acc_abs * torch.from_numpy(np.abs(s64))[None, :, None, None] + torch.from_numpy(np.abs(shift))[None, :, None, None] + 1.0) * 2.0 ** -22
            if layer.startswith("enc"):
                bound = F.max_pool2d(bound, 2, 2)
            bound = bound.permute(0, 2, 3, 1).numpy()
        else:
            up, sc, s, skip = dict(fuse4=("up5", "score4", 2, 1), seg_feats=("up4", "score3", 2, 1), logits=("up3", None, 8, None))[layer]
            xt = xin[0] if sc else xin
            bound = _abs_convt(xt, p[up + "/kernel"], s) * d2
            if sc:
                b2 = _abs_conv(xin[1], p[sc + "/kernel"], 0) * d1
                bound = bound[:, :, : b2.shape[2], : b2.shape[3]] + b2
            bound = bound.permute(0, 2, 3, 1).numpy() + 1e-12
        diff = np.abs(on - off)
        assert diff.shape == bound.shape, layer
        assert (diff <= bound).all(), (layer, float((diff - bound).max()))
        assert diff.max() >= 0.02 * bound.max(), (layer, diff.max(), bound.max())
        if layer.startswith("enc") or layer in ("fc6", "fc7"):
            assert np.array_equal(stored, B.round_bf16(on)) and not np.array_equal(stored, on), layer
        else:
            assert np.array_equal(stored, on), layer
    # the free-running network is the chain of its layers
    lg, it2 = B.fcn8_logits_bf16_ref(x, p, return_intermediates=True)
    assert np.array_equal(B.layer_bf16_ref("logits", it2["seg_feats"], p)[0], lg)
    assert np.array_equal(B.layer_bf16_ref("fc6", it2["f5"], p)[1], it2["fc6"])


# ---- the gate: float32 accumulation passes, wrong kernels fail ---------------------------------------------------

@pytest.fixture(scope="module")
def face():
    """One 256 x 256 face through the full-size vanilla fcn_8 (K = 12,544 in fc6 on its 8 x 8 map)."""
    from flm_amd.weights import synth_fcn8_weights
    p = synth_fcn8_weights(68, seed=2)
    img = np.random.default_rng(3).integers(0, 256, (1, 256, 256, 3), dtype=np.uint8)
    x = np.stack([fcn_ref.get_image_array_ref(im) for im in img])
    _, it = B.fcn8_logits_bf16_ref(x, p, return_intermediates=True)
    src = dict(f1=("enc1", x), f2=("enc2", it["f1"]), f3=("enc3", it["f2"]), f4=("enc4", it["f3"]), f5=("enc5", it["f4"]),
               fc6=("fc6", it["f5"]), fc7=("fc7", it["fc6"]), score5=("score5", it["fc7"]),
               fuse4=("fuse4", (it["score5"], it["f4"])), seg_feats=("seg_feats", (it["fuse4"], it["f3"])),
               logits=("logits", it["seg_feats"]))
    return p, it, src


STORED_BF16 = ("f1", "f2", "f3", "f4", "f5", "fc6", "fc7")


def test_float32_accumulation_passes_the_gate(face):
    p, it, src = face
    for name, (layer, xin) in src.items():
        exact, _ = B.layer_bf16_ref(layer, xin, p)
        e32, s32 = B.layer_bf16_ref(layer, xin, p, accum=torch.float32)
        rep = B.layer_report(s32, exact, e32, s32, name in STORED_BF16)
        print(B.format_report(name, rep))
        assert rep["ok"], (name, rep)
        assert 0 < rep["e32"] < 1e-6, (name, rep["e32"])      # float32 sums of K <= 12,544: nowhere near the 2e-5 cap
        assert rep["slack"] < B.SLACK_CAP
        if name in STORED_BF16:
            assert rep["ref_flips"] <= 2e-3 * rep["size"], (name, rep)   # flips are rare: the share means something


def _tap_serial_f32(x_nhwc, wq_hwio, bias, pad):
    """conv + bias + ReLU with float32 sums in another order: one float32 matmul per filter tap, taps added in turn."""
    x = np.pad(x_nhwc.astype(np.float32), ((0, 0), (pad, pad), (pad, pad), (0, 0)))
    kh, kw = wq_hwio.shape[:2]
    n, h, w = x_nhwc.shape[:3]
    acc = np.zeros((n, h, w, wq_hwio.shape[3]), np.float32)
    for ky in range(kh):
        for kx in range(kw):
            acc += x[:, ky:ky + h, kx:kx + w, :] @ wq_hwio[ky, kx].astype(np.float32)
    return np.maximum(acc + bias.astype(np.float32), np.float32(0))


def _passes(got, exact, e32, s32, bf):
    rep = B.layer_report(got, exact, e32, s32, bf)
    return rep["ok"], rep


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def test_fc6_gate_passes_another_summation_order_and_fails_wrong_kernels(face):
    p, it, _ = face
    f5 = it["f5"]                                                    # [1, 8, 8, 256], bf16 values
    exact, stored = B.layer_bf16_ref("fc6", f5, p)
    e32, s32 = B.layer_bf16_ref("fc6", f5, p, accum=torch.float32)
    wq = B.round_bf16(p["fc6/kernel"])
    serial = _tap_serial_f32(f5, wq, p["fc6/bias"], 3).astype(np.float64)
    ok, rep = _passes(B.round_bf16(serial), exact, e32, s32, True)
    print("fc6 tap-serial float32:", B.format_report("fc6", rep))
    assert ok, rep

    def wrong(extra):                                                # exact pre-activation + extra, as a kernel stores it
        pre = F.conv2d(torch.from_numpy(f5).permute(0, 3, 1, 2), torch.from_numpy(wq).permute(3, 2, 0, 1), None, padding=3)
        pre = pre.permute(0, 2, 3, 1).numpy() + p["fc6/bias"].astype(np.float64) + extra
        return B.round_bf16(np.maximum(pre, 0.0))

    assert np.array_equal(wrong(0.0), stored)                        # the harness itself is the oracle's fc6
    # (a) one 32-channel k-run of one tap dropped: tap (3, 3) -- the only tap a 1 x 1 map would use -- channels 64..95
    drop = -(f5[..., 64:96] @ wq[3, 3, 64:96, :])
    # (b) one border tap reads the clamped neighbour instead of zero padding: tap (ky, kx) = (0, 3) reaches rows y - 3,
    #     which lie above the map for y = 0..2 and are then taken from row 0
    clamp = np.zeros_like(exact)
    clamp[:, 0:3] = (f5[:, 0:1] @ wq[0, 3])
    for what, extra in (("k-run dropped", drop), ("clamped border tap", clamp)):
        bad = wrong(extra)
        ok, rep = _passes(bad, exact, e32, s32, True)
        print("fc6 %s: %s; old bar: %.3g of the maximum (< 4e-2 passed)" % (what, B.format_report("fc6", rep), _rel(bad, stored)))
        assert not ok and rep["over"] > 10 * rep["slack"] and rep["flips"] > 10 * rep["allowed"], (what, rep)
        if what == "k-run dropped":
            assert _rel(bad, stored) < 4e-2                              # the bar this gate replaces let it through


def test_up3_gate_passes_another_summation_order_and_fails_wrong_kernels(face):
    p, it, _ = face
    seg = it["seg_feats"]                                            # [1, 32, 32, 68] float32-stored values
    exact, _ = B.layer_bf16_ref("logits", seg, p)
    e32, s32 = B.layer_bf16_ref("logits", seg, p, accum=torch.float32)
    xq, wq = B.round_bf16(seg), B.round_bf16(p["up3/kernel"])        # (16, 16, out, in)
    n, hi, wi, c = seg.shape

    def scatter(x, w, dtype):
        """out[8i + a, 8j + b, o] += x[i, j, c] * w[a, b, o, c], one matmul per kernel position, sums in `dtype`."""
        out = np.zeros((n, 8 * (hi - 1) + 16, 8 * (wi - 1) + 16, w.shape[2]), dtype)
        xd = x.astype(dtype)
        for a in range(16):
            for b in range(16):
                out[:, a:a + 8 * hi:8, b:b + 8 * wi:8, :] += xd @ w[a, b].astype(dtype).T
        return out

    assert np.abs(scatter(xq, wq, np.float64) - exact).max() <= 1e-12 * np.abs(exact).max()
    ok, rep = _passes(scatter(xq, wq, np.float32), exact, e32, s32, False)
    print("up3 position-serial float32:", B.format_report("logits", rep))
    assert ok, rep
    # (a) one 32-channel k-run of one tap dropped: kernel position (12, 5), input channels 32..63
    w_a = wq.copy()
    w_a[12, 5, :, 32:64] = 0.0
    # (b) a border tap reads the clamped neighbour: output row 4 (a0 = 4, input row i0 = 0) adds kernel row 12 applied to
    #     input row -1, taken from row 0 instead of zero
    bad_b = exact.copy()
    for b in range(16):
        bad_b[:, 4, b:b + 8 * wi:8, :] += xq[:, 0] @ wq[12, b].T
    # (c) classes 68..71 of the padded operands are not zero: the 72-column forms wrap around to classes 0..3
    x_c = np.concatenate([xq, xq[..., :4]], -1)
    w_c = np.concatenate([wq, wq[..., :4]], -1)
    for what, bad in (("k-run dropped", scatter(xq, w_a, np.float64)), ("clamped border tap", bad_b),
                      ("non-zero pad classes", scatter(x_c, w_c, np.float64))):
        ok, rep = _passes(bad, exact, e32, s32, False)
        print("up3 %s: %s; old bar: %.3g of the maximum" % (what, B.format_report("logits", rep), _rel(bad, exact)))
        assert not ok and rep["over"] > 10 * rep["slack"], (what, rep)
