"""The BatchNorm statistics of a trained checkpoint, laid over any of the project's synthetic parameter sets.

The synth sets (flm_amd/weights.py) draw gamma ~ U(0.5, 1.5) (MobileNet 0.8 .. 1.6, ResNet50 0.8 .. 1.2, x 0.3 on the `2c`
layers) and moving_variance ~ U(0.5, 1.5): the folded scale gamma / sqrt(var + 1e-3) that pack_affine_kernel writes is a
positive number between 0.4 and 2.1 in every test built on them.  A trained checkpoint has negative gammas, gammas that
are exactly zero (dead or pruned channels) and running variances over four to six decades.  trained_regime() rewrites
every BatchNorm layer of a parameter dict so that each of these occurs in every layer, by channel index c:

    class        channels                gamma          moving_variance        folded scale
    KEEP         every other channel     synth          synth                  0.8 .. 1.4 x gamma
    NEG          c % 4 == 1              -gamma         synth                  negative
    ZERO         c % 16 == 6             0              synth                  0; beta = +0.5, -0.5, +6.5 in turn, so the
                                                                               constant is positive, clamped to 0, clamped to 6
    SMALL        c % 16 == 3             synth          10 ** U(-4, -2)        9.5 .. 30 x gamma
    LARGE        c % 16 == 7             synth          10 ** U(1.2, 2)        0.10 .. 0.25 x gamma
    SMALL_NEG    c % 16 == 11            -gamma         10 ** U(-4, -2)        -(9.5 .. 30) x gamma
    LARGE_NEG    c % 16 == 15            -gamma         10 ** U(1.2, 2)        -(0.10 .. 0.25) x gamma

The magnitudes of gamma stay the synth set's (ResNet50's 0.3 on the `2c` layers is what keeps its residual sums O(1)).
A channel whose variance changes keeps its post-BatchNorm distribution, as a trained layer does -- a channel with a small
running variance HAS small conv outputs: with r = sqrt((var2 + 1e-3) / (var + 1e-3)) in float64, the conv kernel's
output-channel slice, the conv bias and moving_mean are multiplied by r and cast to float32.  Nothing else is touched;
the input dict and its arrays are left as they were.
"""
import zlib

import numpy as np

EPS = 1e-3
KEEP, NEG, ZERO, SMALL, LARGE, SMALL_NEG, LARGE_NEG = range(7)
CLASS_NAMES = ("keep", "neg", "zero", "small", "large", "small_neg", "large_neg")
NEGATIVE = (NEG, SMALL_NEG, LARGE_NEG)
ZERO_BETAS = (0.5, -0.5, 6.5)
SMALL_VAR_LOG10, LARGE_VAR_LOG10 = (-4.0, -2.0), (1.2, 2.0)
# |scale| / |gamma| = 1 / sqrt(var + EPS) at the ends of each variance range (the synth sets: var in [0.5, 1.5])
SCALE_RATIO = {KEEP: (1 / np.sqrt(1.5 + EPS), 1 / np.sqrt(0.5 + EPS)),
               SMALL: (1 / np.sqrt(1e-2 + EPS), 1 / np.sqrt(1e-4 + EPS)),
               LARGE: (1 / np.sqrt(1e2 + EPS), 1 / np.sqrt(10 ** 1.2 + EPS))}
SCALE_RATIO.update({NEG: SCALE_RATIO[KEEP], SMALL_NEG: SCALE_RATIO[SMALL], LARGE_NEG: SCALE_RATIO[LARGE]})


def conv_of(bn: str) -> str:
    """The conv layer a BatchNorm layer normalises: enc<i> is its own conv, <layer>_bn -> <layer>, bn_conv1 -> conv1,
    bn<stage><block>_branch<x> -> res<stage><block>_branch<x>."""
    if bn.endswith("_bn"):
        return bn[:-3]
    if bn == "bn_conv1":
        return "conv1"
    if bn.startswith("bn") and "_branch" in bn:
        return "res" + bn[2:]
    return bn


def bn_layers(params) -> list:
    return [k[:-len("/gamma")] for k in params if k.endswith("/gamma")]


def channel_classes(n: int) -> np.ndarray:
    c = np.arange(n)
    cls = np.full(n, KEEP, np.int64)
    cls[c % 4 == 1] = NEG
    cls[c % 16 == 6] = ZERO
    cls[c % 16 == 3] = SMALL
    cls[c % 16 == 7] = LARGE
    cls[c % 16 == 11] = SMALL_NEG
    cls[c % 16 == 15] = LARGE_NEG
    return cls


def trained_regime(params: dict, seed: int = 11):
    """(params2, classes): `params` with every BatchNorm layer (every key ending in /gamma) rewritten as the module
    docstring says; classes[bn] is the integer class of every channel of BatchNorm layer `bn`.  The variances of a layer
    are drawn from default_rng([seed, crc32(bn)]): they do not depend on which other layers the dict holds."""
    p2, classes = dict(params), {}
    for bn in bn_layers(params):
        conv = conv_of(bn)
        dw = conv + "/depthwise_kernel" in params
        kkey = conv + ("/depthwise_kernel" if dw else "/kernel")
        gamma = np.asarray(params[bn + "/gamma"], np.float32).copy()
        beta = np.asarray(params[bn + "/beta"], np.float32).copy()
        var = np.asarray(params[bn + "/moving_variance"], np.float64)
        n = gamma.shape[0]
        cls = classes[bn] = channel_classes(n)
        rng = np.random.default_rng([seed, zlib.crc32(bn.encode())])
        small = 10.0 ** rng.uniform(*SMALL_VAR_LOG10, n)
        large = 10.0 ** rng.uniform(*LARGE_VAR_LOG10, n)
        var2 = var.copy()
        is_small, is_large = np.isin(cls, (SMALL, SMALL_NEG)), np.isin(cls, (LARGE, LARGE_NEG))
        var2[is_small] = small[is_small].astype(np.float32)
        var2[is_large] = large[is_large].astype(np.float32)
        gamma[np.isin(cls, NEGATIVE)] *= np.float32(-1)
        zero = np.flatnonzero(cls == ZERO)
        gamma[zero] = 0
        beta[zero] = np.asarray(ZERO_BETAS, np.float32)[np.arange(zero.size) % 3]
        r = np.sqrt((var2 + EPS) / (var + EPS))          # exactly 1 where the variance stays
        k = np.asarray(params[kkey], np.float64)
        p2[kkey] = (k * (r[None, None, :, None] if dw else r[None, None, None, :])).astype(np.float32)
        if conv + "/bias" in params:
            p2[conv + "/bias"] = (np.asarray(params[conv + "/bias"], np.float64) * r).astype(np.float32)
        p2[bn + "/moving_mean"] = (np.asarray(params[bn + "/moving_mean"], np.float64) * r).astype(np.float32)
        p2[bn + "/moving_variance"] = var2.astype(np.float32)
        p2[bn + "/gamma"], p2[bn + "/beta"] = gamma, beta
    return p2, classes


def zero_class_expected(shift, relu: int, bf16: bool) -> np.ndarray:
    """What a zero-gamma channel holds at every pixel: act(float32(shift)), in bf16 its rounding.  fmaf(acc, 0, shift) has
    no rounding and the 2x2 maximum of a constant is the constant."""
    from oracle.fcn_bf16_ref import round_bf16
    v = np.asarray(shift, np.float32).astype(np.float64)
    if relu:
        v = np.clip(v, 0.0, 6.0 if relu == 2 else np.inf)
    return round_bf16(v) if bf16 else v
