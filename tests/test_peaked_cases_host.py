"""The cases of tests/peaked_cases.py reach the regimes they are named for -- on the float64 oracle alone, no GPU: what
keeps tests/test_gpu_peaked_maps.py from being vacuous.  Every case is evaluated once at 3 x 96 x 160 by
oracle/fcn_ref.fcn8_logits_ref in float64; the counts are taken on the float32-rounded float64 softmax.

Measured (the larger figure of the two random faces 0 and 2, of 1,188,096 probabilities per face; "range": the largest
per-pixel logit range; "tie4": the most pixels one class has at or above its 4th largest value; the last two columns are
the blank face 1, which has no zero, denormal, one or window argument at any gain):

    case             zeros      denormal   p == 1    in exp window   range    tie4     blank: range  tie4
    scaled4                0          0         0          0           42.6       4            3.1      4
    scaled16          12,210     42,252     1,572        886          170.5      79           12.3      4
    scaled64         951,309     62,178    10,079      2,841          682.0     330           49.3      4
    bilinear1              0          0         0          0            8.1       4            0.6      4
    bilinear8              0          0         0          0           64.9       7            4.6      5
    bilinear32       244,864    180,287     2,845      6,466          259.8   1,426           18.2      7
    bilinear128    1,012,299     27,038    11,308      1,122        1,039.1   4,902           72.8      5
    bilinear32dead   240,218    177,106     2,927      6,306          259.8   1,467           26.2      5
                     (its 67 live classes; class 5 is 0 at all 17,472 pixels of every face, about 2e5 below the rest)
"""
import numpy as np
import pytest
import torch

import peaked_cases as P

_CACHE = {}


def _logits(name):
    """float64 logits [3, 104, 168, 68] of a case: the base weights and the preprocessed crops are built once."""
    from flm_amd.weights import synth_fcn8_weights
    from oracle import fcn_ref
    if "base" not in _CACHE:
        _CACHE["base"] = synth_fcn8_weights(68, seed=2)
        _CACHE["x"] = np.stack([fcn_ref.get_image_array_ref(c) for c in P.case_crops()])
    return fcn_ref.fcn8_logits_ref(_CACHE["x"], P.case_weights(_CACHE["base"], name), dtype=torch.float64)


def test_bilinear_kernel_and_weight_edits():
    k = P.bilinear_up3(32.0)
    assert k.shape == (16, 16, 68, 68) and k.dtype == np.float32
    f = 1.0 - np.abs(np.arange(16) - 7.5) / 8.0
    assert np.array_equal(k[:, :, 3, 3], (32.0 * np.outer(f, f)).astype(np.float32))
    assert not k[:, :, 3, 4].any() and k[0, 0, 0, 0] == np.float32(32.0 / 256)   # same-class only; the corner tap
    # the four taps of every output phase sum to `gain`: a constant seg_feats map is reproduced times the gain
    assert np.allclose(k[:, :, 0, 0].reshape(2, 8, 2, 8).sum((0, 2)), 32.0)
    base = {"up3/kernel": np.ones((16, 16, 68, 68), np.float32), "score3/bias": np.zeros(68, np.float32)}
    w = P.peaked_weights(base, "scaled", 16.0)
    assert (w["up3/kernel"] == 16).all() and w["score3/bias"] is base["score3/bias"]
    w = P.peaked_weights(base, "bilinear", 32.0, dead=(5,), raised=(9,))
    assert w["score3/bias"][5] == np.float32(-2e5 / 32) and w["score3/bias"][9] == np.float32(12 / 32)
    assert not base["score3/bias"].any() and (base["up3/kernel"] == 1).all()      # the base is left alone
    with pytest.raises(AssertionError):
        P.peaked_weights(base, "scaled", 4.0, dead=(5,))
    img = P.crops(4, 8, 8, seed=1, blank=(0, 3))
    assert img.dtype == np.uint8 and (img[0] == 128).all() and (img[3] == 128).all() and img[1].std() > 50


def test_reference_helpers():
    lg = np.array([[0.0, -50.0, -250.0, -800.0], [1.0, 1.0, 1.0, 1.0]])
    p = P.softmax64(lg)
    assert p.dtype == np.float64 and np.allclose(p.sum(-1), 1) and p[0, 3] == 0 and 0 < p[0, 2] < 1e-100
    assert P.rel_err([1.0, 2.02, 5.0], [1.0, 2.0, 1e-40], 1e-30) == pytest.approx(0.01)
    assert P.rel_err([1.0], [1e-40], 1e-30) == 0.0
    assert 0 < P.e32(lg) < 1e-5
    r = P.regime(np.array([[0.0, -103.5, -200.0], [0.0, -80.0, -0.0]]))
    assert (r["window"], r["zeros"], r["denormal"]) == (1, 1, 1) and r["range"] == 200.0


@pytest.mark.parametrize("name", P.CASE_NAMES)
def test_case_reaches_its_regime(name):
    kind, gain, dead, raised = P.CASES[name]
    lg = _logits(name)
    live = [c for c in range(68) if c not in dead]
    for f in range(P.SHAPE[0]):
        r = P.regime(lg[f][..., live])
        print("%-15s face %d: %s" % (name, f, r))
        if f in P.BLANK:
            if gain <= 32:   # the blank crop of the same batch stays unsaturated
                assert (r["zeros"], r["denormal"], r["ones"], r["window"]) == (0, 0, 0, 0), (name, f, r)
                assert r["tie4"] <= 32, (name, f, r)
        elif name in P.SATURATED:
            assert r["zeros"] > 0 and r["denormal"] > 0 and r["ones"] > 0 and r["window"] > 0, (name, f, r)
            assert r["tie4"] > 32, (name, f, r)
        if name in P.UNSATURATED:
            assert r["min_nonzero"] >= 25 and r["zeros"] == 0, (name, f, r)
        if dead:
            p = P.softmax64(lg[f])
            assert not p[..., list(dead)].any(), "the dead class is not exactly 0 in float64"
