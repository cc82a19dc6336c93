"""Peaked, saturated and blank-crop probability maps for the 68-class fcn_8: case construction and float64 references.

synth_fcn8_weights keeps the logits' spread O(1) and its random up3 kernel makes each of the 64 output phases an
independent filter: diffuse, unsaturated maps.  A trained landmark network gives smooth, peaked maps with very large
logit ranges.  The cases here reach that regime from the same seeded weights by changing only `up3/kernel` (and, for the
dead / raised classes, `score3/bias`):

  kind="scaled"    the synthetic up3 kernel times `gain`: the same diffuse maps with `gain` times the logit range
  kind="bilinear"  up3 = bilinear_up3(gain), the customary FCN initialisation: class c of the output is the bilinear
                   x8 upsampling of class c of seg_feats times `gain` -- smooth maps, neighbouring pixels of a wave and
                   all 64 phases of a position alike

Every batch is 3 x 96 x 160 with face 1 a blank crop (constant 128): its seg_feats are still not constant -- the zero
padding of the encoder reaches every position of a 3 x 5 map -- but their spread is a fraction of a random crop's, so
the blank face stays unsaturated up to gain 32 while its neighbours saturate (tests/test_peaked_cases_host.py asserts
which regime every case and face reaches, on the float64 oracle alone).  No gain of the table had to be replaced to
reach a regime.

Nothing here imports the GPU library.
"""
import numpy as np
import torch

SHAPE = (3, 96, 160)          # faces, height, width of the case batches; face 1 is blank
BLANK = (1,)
SHAPE_256 = (2, 256, 256)     # the 256 x 256 geometry of the three bf16 candidate kernels
SEED = 7
DEAD, RAISED = 5, 9

#        name              kind        gain   dead      raised
CASES = {
    "scaled4":        ("scaled",     4.0,  (),       ()),
    "scaled16":       ("scaled",    16.0,  (),       ()),
    "scaled64":       ("scaled",    64.0,  (),       ()),
    "bilinear1":      ("bilinear",   1.0,  (),       ()),
    "bilinear8":      ("bilinear",   8.0,  (),       ()),
    "bilinear32":     ("bilinear",  32.0,  (),       ()),
    "bilinear128":    ("bilinear", 128.0,  (),       ()),
    "bilinear32dead": ("bilinear",  32.0,  (DEAD,),  (RAISED,)),
}
CASE_NAMES = tuple(CASES)
UNSATURATED = ("scaled4", "bilinear1", "bilinear8")
SATURATED = ("scaled16", "scaled64", "bilinear32", "bilinear128", "bilinear32dead")

EXP_WINDOW = (-103.97, -103.28)   # exp_nonpos (flm_convt_dev.h) returns the smallest denormal here, expf returns 0
FLOOR = 2.0 ** -100               # relative errors are gated where the float64 probability is at least this


def bilinear_up3(gain, n_classes=68):
    """(16, 16, C, C) float32: k[:, :, c, c] = gain * outer(f, f), f[i] = 1 - |i - 7.5| / 8; zero between classes."""
    f = 1.0 - np.abs(np.arange(16, dtype=np.float64) - 7.5) / 8.0
    k = np.zeros((16, 16, n_classes, n_classes), np.float32)
    tap = (float(gain) * np.outer(f, f)).astype(np.float32)
    for c in range(n_classes):
        k[:, :, c, c] = tap
    return k


def peaked_weights(base, kind, gain, dead=(), raised=()):
    """A copy of `base` (only the changed tensors are copied) with up3/kernel times `gain` (kind="scaled") or replaced by
    bilinear_up3(gain) (kind="bilinear").  kind="bilinear" only: score3/bias of every class in `dead` is lowered by
    2e5 / gain -- at a corner pixel the bilinear taps sum to 1/256, so the class sits 2e5 / 256 = 780 below the rest
    even there, and exp(-780) is 0 in float64 as in float32: the class is exactly 0 everywhere -- and that of every class
    in `raised` goes up by 12 / gain (12 in the logits of the interior)."""
    assert kind in ("scaled", "bilinear"), kind
    w = dict(base)
    if kind == "scaled":
        assert not dead and not raised, "dead / raised classes need the same-class bilinear kernel"
        w["up3/kernel"] = base["up3/kernel"] * np.float32(gain)
    else:
        c = base["up3/kernel"].shape[2]
        w["up3/kernel"] = bilinear_up3(gain, c)
        if dead or raised:
            b = np.array(base["score3/bias"], copy=True)
            for k in dead:
                b[k] -= np.float32(2e5 / gain)
            for k in raised:
                b[k] += np.float32(12.0 / gain)
            w["score3/bias"] = b
    return w


def case_weights(base, name):
    kind, gain, dead, raised = CASES[name]
    return peaked_weights(base, kind, gain, dead, raised)


def crops(n, h, w, seed, blank=()):
    """Random uint8 BGR crops [n, h, w, 3]; the faces listed in `blank` are the constant 128."""
    img = np.random.default_rng(seed).integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    for f in blank:
        img[f] = 128
    return img


def case_crops():
    return crops(*SHAPE, seed=SEED, blank=BLANK)


# ---- references ------------------------------------------------------------------------------------------------------

def softmax64(logits):
    """float64 softmax over the last axis."""
    x = np.asarray(logits, np.float64)
    e = np.exp(x - x.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def rel_err(got, ref, floor):
    """The largest |got / ref - 1| over ref >= floor (0.0 if nothing is)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    m = ref >= floor
    if not m.any():
        return 0.0
    return float(np.abs(got[m] / ref[m] - 1.0).max())


def softmax32(logits):
    """torch's float32 CPU softmax of the same logits."""
    return torch.softmax(torch.from_numpy(np.ascontiguousarray(logits, np.float32)), dim=-1).numpy()


def e32(logits, floor=FLOOR):
    """rel_err of torch's float32 CPU softmax of `logits` against softmax64: what a careful float32 evaluation gives."""
    return rel_err(softmax32(logits), softmax64(logits), floor)


def regime(logits):
    """What a [..., C] block of logits reaches, measured on its float32-rounded float64 softmax: counts of exact zeros,
    denormals and exact ones, of arguments x - max inside EXP_WINDOW, the largest per-pixel logit range, per class the
    number of pixels at or above its 4th largest value (the largest over classes: `tie4`) and the fewest non-zero pixels
    of a class (`min_nonzero`)."""
    x = np.asarray(logits, np.float64)
    c = x.shape[-1]
    x = x.reshape(-1, c)
    arg = x - x.max(-1, keepdims=True)
    p = softmax64(x).astype(np.float32)
    tiny = np.finfo(np.float32).tiny
    fourth = np.sort(p, axis=0)[-min(4, p.shape[0])]
    return dict(zeros=int((p == 0).sum()), denormal=int(((p > 0) & (p < tiny)).sum()), ones=int((p == 1).sum()),
                window=int(((arg > EXP_WINDOW[0]) & (arg < EXP_WINDOW[1])).sum()), range=float(-arg.min()),
                tie4=int((p >= fourth[None, :]).sum(0).max()), min_nonzero=int((p != 0).sum(0).min()),
                zero_classes=[int(k) for k in np.nonzero((p == 0).all(0))[0]], size=int(p.size))
