"""The softmax epilogue and the candidate path on peaked, saturated and blank-crop maps (tests/peaked_cases.py).

Every other forward test runs on synth_fcn8_weights' diffuse, unsaturated maps (per-pixel logit range at most 10.9, no
probability 0, denormal or 1, no ties at a class's n-th value) or on the exactly flat map.  The cases here scale the
synthetic up3 kernel by 4 / 16 / 64 or replace it by a bilinear one times 1 / 8 / 32 / 128 (one of them with a class
that is 0 everywhere and one raised); every batch is 3 x 96 x 160 with a blank crop between two random ones, and
tests/test_peaked_cases_host.py asserts on the float64 oracle which regime each case and face reaches.  Both types.

(a) softmax: "probs" (epilogue 1) against the float64 softmax of the device's own "logits" (epilogue 0 of the same
    accumulators; seg_feats of the two forwards bit-equal): max-abs <= 1e-5, rows sum to 1 within 1e-5, finite and >= 0,
    got <= 2^-99 where ref < 2^-100, and above that floor a relative error of at most 4 x e32 in fp32 (e32: torch's
    float32 CPU softmax of the same logits against float64, same floor) and 4 x e32 + 2e-6 in bf16 (v_exp_f32 and
    v_rcp_f32).  fp32 only, below the floor: |got - ref| <= 4 x e32 x ref + 2^-149 -- exp_nonpos rounds once into the
    denormals (v_ldexp_f32, half a step of 2^-149) and the product with 1 / sum <= 1 rounds once more (half a step on top
    of at most half a step), so an error above one step is not rounding.  (bf16: v_exp_f32 returns 0 below 2^-126.)
(b) "classmap" equals the reference's argmax except where its top two are within 2e-6.
(c) "landmarks" of the materialised path (landmark_candidates = 0), n_points 4 and 25, thresh 0 and 0.5, equal
    oracle.decode_ref.transfer_target_ref of the device's "probs" bit for bit (the bar of tests/test_gpu_decode.py for
    top-n), NaN and (-1, -1) in the same places; the dead class comes out as the reference says.
(d) the candidate path equals the materialised one bit for bit: n_points 4, 9, 25, 32 x thresh 0, 0.5 x
    candidate_sub_phases 0, 1; bf16 also with up3_cand8 = 0 / 3, up3_cand8_rows = 1 / 8 and up3_wreg = 1; one case at
    2 x 256 x 256 through each of the three bf16 kernels; one "landmark_stats" leg against decode_stats_device.
(e) the mixed batch the other way round -- four faces, only face 2 random -- with the lists' fills printed.
(f) from cand_cnt / cand_cap alone: over the case table each type takes every path -- flag clear; flag set with a list
    over its capacity; flag set with every list within it (a class short of n keys, or a lane's list that dropped one).
    No default-option run of the table overflows a list (the fullest is 46 % at n = 4), so the overflow legs are
    bilinear32 with candidate_cap_div = 64 and with candidate_sub_phases = 1 at n = 32.

Measured on an MI355X.  No kernel bug was found: every gate holds, the class maps equal the reference's argmax on all
52,416 pixels of every case and type (at most 2.7e-4 of the pixels have a top-2 gap below 2e-6; bilinear1: 2.2e-3, see
the test), the landmarks are the float64 decode's bit for bit (thresh 0.5 rejects 0 to 204 of the 204 landmarks; the dead
class is (-1, -1) in every face), and the candidate path is the materialised one bit for bit on every leg of (d), (e).

(a) relative error above 2^-100 / its bound (e32), then the largest |got - ref| - 4 e32 ref below 2^-100 in steps of
    2^-149 (bound: fp32 1, bf16 2^23 = 8,388,608), then non-zero where the float32-rounded reference is 0 / zero where
    it is not:

    case             fp32                                                    bf16
    scaled4          2.18e-06 / 8.66e-06 (2.17e-06)  -                       2.08e-06 / 1.07e-05 (2.18e-06)  -
    scaled16         4.09e-06 / 1.64e-05 (4.09e-06)  0.97    94 / 1          3.79e-06 / 1.83e-05 (4.07e-06)  8,383,967  0 / 83,490
    scaled64         4.05e-06 / 1.61e-05 (4.02e-06)  0.97   261 / 4          3.76e-06 / 1.82e-05 (4.05e-06)  8,388,254  0 / 124,205
    bilinear1        5.28e-07 / 2.00e-06 (5.00e-07)  -                       6.01e-07 / 3.70e-06 (4.24e-07)  -
    bilinear8        2.22e-06 / 8.76e-06 (2.19e-06)  -                       3.50e-06 / 1.05e-05 (2.12e-06)  -
    bilinear32       4.07e-06 / 1.63e-05 (4.07e-06)  0.99   923 / 28         3.71e-06 / 1.82e-05 (4.04e-06)  8,388,362  0 / 358,049
    bilinear128      4.02e-06 / 1.60e-05 (3.99e-06)  0.99    91 / 0          3.73e-06 / 1.55e-05 (3.37e-06)  8,385,398  0 / 53,621
    bilinear32dead   4.08e-06 / 1.63e-05 (4.07e-06)  0.98   893 / 25         3.71e-06 / 1.82e-05 (4.04e-06)  8,388,362  0 / 351,674

    Max-abs error at most 5.5e-7, rows sum to 1 within 5.6e-7.  The fp32 softmax is as good as torch's float32 one (error
    = e32: both round x - max once) and rounds into the denormals within the one step derived; the bf16 softmax returns
    0 for all but 0.5 % of the reference's denormals (v_exp_f32 has none) and is otherwise inside the fp32 bound -- no leg
    needed more room than these bounds.

(e), (f) keys per face (cand_cnt) and the path, default options; capacity 69,632 at n = 4 and 435,200 at n = 25.  First
    the 3-face batch (face 1 blank), then the 4-face one (only face 2 random).  "short": flag set, every list within
    capacity.

    case            type  n = 4               path    n = 25              path    n = 4                     path    n = 25                    path
    scaled4         f32   22402 31894 23191   clear   33639 44605 32516   clear   31894 31894 24019 31894   clear   44605 44605 32418 44605   clear
    scaled4         bf16  13800 20178 13909   clear   48433 77302 49064   clear   20178 20178 14034 20178   clear   77302 77302 48635 77302   clear
    scaled16        f32   21968 29398 22933   clear   31479 42888 31207   clear   29398 29398 23036 29398   clear   42888 42888 31204 42888   clear
    scaled16        bf16  12605 18341 13075   clear   44973 72172 46578   short   18341 18341 13799 18341   clear   72172 72172 45002 72172   clear
    scaled64        f32   23590 25936 24194   clear   31120 37527 30998   clear   25936 25936 24496 25936   clear   37527 37527 31143 37527   clear
    scaled64        bf16  15466 15655 15914   clear   44622 60587 46085   short   15655 15655 16281 15655   clear   60587 60587 44754 60587   clear
    bilinear1       f32   11845 11397 11620   clear   23274 24560 23576   clear   11397 11397 11279 11397   clear   24560 24560 23481 24560   clear
    bilinear1       bf16  5429 4650 5612      clear   30955 36292 32478   clear   4650 4650 4930 4650       clear   36292 36292 31461 36292   clear
    bilinear8       f32   9956 11389 10511    clear   23959 24196 24070   clear   11389 11389 9886 11389    clear   24196 24196 24329 24196   clear
    bilinear8       bf16  5669 5324 6591      clear   33892 34101 33770   short   5324 5324 5887 5324       clear   34101 34101 33680 34101   short
    bilinear32      f32   10402 11768 10909   clear   25853 24949 26412   clear   11768 11768 10655 11768   clear   24949 24949 26685 24949   clear
    bilinear32      bf16  7646 6294 8690      short   36406 33662 36369   short   6294 6294 8182 6294       short   33662 33662 36356 33662   short
    bilinear128     f32   16896 10129 17461   clear   33062 26171 33828   clear   10129 10129 17623 10129   clear   26171 26171 33682 26171   clear
    bilinear128     bf16  15353 6503 16229    short   43034 35812 42955   short   6503 6503 15956 6503      short   35812 35812 42756 35812   short
    bilinear32dead  f32   10393 11283 10947   short   25462 23322 26143   short   11283 11283 10672 11283   short   23322 23322 26410 23322   short
    bilinear32dead  bf16  7597 6252 8644      short   36078 30973 35840   short   6252 6252 8201 6252       short   30973 30973 36081 30973   short
    bilinear32      f32   candidate_cap_div = 64, n = 4: 10402 11768 10909 of 1,088: overflow;  candidate_sub_phases = 1, n = 32: 763950 1188096 766045 of 557,056: overflow
    bilinear32      bf16  candidate_cap_div = 64, n = 4:  7646  6294  8690 of 1,088: overflow;  candidate_sub_phases = 1, n = 32: 554664  589824 555669 of 557,056: overflow

    fp32 takes the fallback only for the dead class.  The bf16 "short" rows without a dead class are keys dropped by the
    16-entry lane lists of up3_cand8_kernel, not short classes: through the generic kernel (up3_cand8 = 0) and
    up3_wreg_kernel the same batches leave the flag clear with more keys -- bilinear32, n = 25: 38942 33959 38894 against
    36406 33662 36369; bilinear8, n = 25: 34713 34101 34617 against 33892 34101 33770; scaled16, n = 25: 44976 against
    44973 -- and at 2 x 256 x 256, n = 25, up3_cand8_kernel has 35696 25522 (short) against their 35715 25522 (clear).
    up3_cand8_rows = 8 drops up to two keys more than the default.  With one sampled phase per tile and n = 32 a face has
    fewer than 32 wave maxima per class: tau = 0 -> FLT_MIN and the blank face offers all of its 1,188,096 values.

Fault injection (a scratch build, not committed; wrong values only): exp_nonpos returning 0 for arguments below -87.
test_softmax_against_float64 fails in fp32 on the five saturated cases -- scaled16, scaled64, bilinear32, bilinear128,
bilinear32dead: 11.7 million steps of 2^-149 below the floor against the bound of 1; 54,788 to 366,081 probabilities are 0
where the reference is not -- and the other 122 tests pass: every other gate of (a) does too (the values lost are below
2^-125, far under the floor of the relative gate, which is why (a) has the one-step gate below the
floor), and (c), (d) compare two paths through the same exp.  The suite as it stood before these tests (364 GPU tests)
passes with the fault in the build.  Not injected: `>` for `>=` in the hit test and dropping the FLT_MIN clamp of tau --
by the code both end in the fewer-than-n-keys check or an overflow, so the fallback would still return exact values.
"""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import peaked_cases as P

pytestmark = pytest.mark.gpu

DTYPES = ("f32", "bf16")
N_POINTS = (4, 9, 25, 32)
THRESH = (0.0, 0.5)
MAT = dict(landmark_candidates=0)

_BASE, _RUNS, _FILLS = {}, {}, {}


@pytest.fixture(scope="module")
def flm():
    import flm_amd
    from flm_amd import _lib
    _lib.load()
    return flm_amd


def _base():
    if not _BASE:
        from flm_amd.weights import synth_fcn8_weights
        _BASE["w"] = synth_fcn8_weights(68, seed=2)
    return _BASE["w"]


def _model(name, dtype, h, w):
    from flm_amd.networks import LANDMARKS_MODELS
    model = LANDMARKS_MODELS["fcn_8"](68, input_height=h, input_width=w, dtype=dtype)
    model.load_weights(P.case_weights(_base(), name))
    return model


class Run:
    """One case in one type at 3 x 96 x 160: the model, the device's probabilities and logits, the float64 reference.
    Built once per module and left unchanged."""

    def __init__(self, name, dtype):
        n, h, w = P.SHAPE
        self.name, self.dtype, self.n = name, dtype, n
        self.model = _model(name, dtype, h, w)
        self.xd = torch.from_numpy(P.case_crops()).cuda()
        self.xd4 = torch.from_numpy(P.crops(4, h, w, seed=P.SEED + 1, blank=(0, 1, 3))).cuda()
        m = self.model
        self.probs = m.forward_device(self.xd, "probs").cpu().numpy()
        self.logits = m.forward_device(self.xd, "logits").cpu().numpy().reshape(n, -1, 68)
        torch.cuda.synchronize()
        assert torch.equal(m.intermediate("seg_feats", n, "probs"), m.intermediate("seg_feats", n, "logits"))
        self.ref = P.softmax64(self.logits)
        self.e32 = P.e32(self.logits)
        self.label = "%-14s %-4s" % (name, dtype)


def _run(name, dtype):
    if (name, dtype) not in _RUNS:
        _RUNS[(name, dtype)] = Run(name, dtype)
    return _RUNS[(name, dtype)]


def _lm(model, xd, n_points, thresh, opts):
    return model.forward_device(xd, "landmarks", n_points=n_points, thresh=thresh, opts=opts).cpu().numpy()


def _fills(model, xd, n_points, opts=None):
    """(cand_cnt[0 .. n - 1], the fallback flag, cand_cap) of one "landmarks" forward in a workspace of the caller's."""
    from flm_amd import _lib
    lib = _lib.load()
    n, h, w = int(xd.shape[0]), int(xd.shape[1]), int(xd.shape[2])
    ws = model.new_workspace(n, "landmarks", n_points, opts)
    model.forward_device(xd, "landmarks", n_points=n_points, workspace=ws, opts=opts)
    torch.cuda.synchronize()
    fo = model._opts(opts)

    def off(key):
        return lib.flm_fcn8_workspace_offset_opts(key, n, h, w, 68, model._dt, _lib.OUT_LANDMARKS, _lib.DECODE_TOPN,
                                                  n_points, C.byref(fo))
    cap, at = off(b"cand_cap"), off(b"cand_cnt")
    assert cap > 0 and at > 0, "this layout has no candidate lists"
    cnt = ws[at:at + 4 * (n + 1)].view(torch.int32).cpu().numpy().astype(np.int64)
    return cnt[:n], int(cnt[n]), int(cap)


def _path(cnt, flag, cap):
    return "clear" if not flag else ("overflow" if cnt.max() > cap else "short")


# ---- (a) the softmax ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", P.CASE_NAMES)
def test_softmax_against_float64(flm, name, dtype):
    r = _run(name, dtype)
    got, ref = r.probs, r.ref
    got64 = got.astype(np.float64)
    bound = 4 * r.e32 + (2e-6 if dtype == "bf16" else 0.0)
    rel = P.rel_err(got, ref, P.FLOOR)
    low = ref < P.FLOOR
    ref32 = ref.astype(np.float32)
    step = 2.0 ** -149
    low_err = float((np.abs(got64 - ref)[low] - 4 * r.e32 * ref[low]).max() / step) if low.any() else 0.0
    print("%s softmax: relative error %.3g (bound %.3g, e32 %.3g), max-abs %.3g, rows sum to 1 within %.3g, logit range %.1f; "
          "below 2^-100: largest value %.3g, error beyond 4 e32 ref %.2f steps of 2^-149; "
          "non-zero where the reference rounds to 0: %d, zero where it does not: %d (of %d zeros / %d denormals in the reference)"
          % (r.label, rel, bound, r.e32, np.abs(got64 - ref).max(), np.abs(got64.sum(-1) - 1).max(),
             float((r.logits.max(-1) - r.logits.min(-1)).max()), float(got[low].max()) if low.any() else 0.0, low_err,
             int(((got != 0) & (ref32 == 0)).sum()), int(((got == 0) & (ref32 != 0)).sum()), int((ref32 == 0).sum()),
             int(((ref32 != 0) & (ref32 < np.finfo(np.float32).tiny)).sum())))
    assert np.isfinite(got).all() and (got >= 0).all()
    assert np.abs(got64 - ref).max() <= 1e-5
    assert np.abs(got64.sum(-1) - 1).max() <= 1e-5
    assert not low.any() or got[low].max() <= 2.0 ** -99
    assert rel <= bound, (r.label, rel, bound)
    # below the floor: fp32 one step of 2^-149 (two roundings of half a step); bf16 2^-126 = 2^23 steps, since
    # v_exp_f32 returns 0 for every result below the normal range
    assert low_err <= (1.0 if dtype == "f32" else 2.0 ** 23), (r.label, low_err)
    for c in P.CASES[name][2]:
        assert not got[..., c].any(), "the dead class is not exactly 0"


# ---- (b) the class map -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", P.CASE_NAMES)
def test_classmap_is_the_reference_argmax(flm, name, dtype):
    r = _run(name, dtype)
    n, h, w = P.SHAPE
    cm = r.model.forward_device(r.xd, "classmap").cpu().numpy().reshape(n, -1)
    assert cm.min() >= 0 and cm.max() < 68
    diff = cm != r.ref.argmax(-1)
    srt = np.sort(r.ref, axis=-1)
    gap = srt[..., -1] - srt[..., -2]
    print("%s class map: %d of %d pixels differ from the reference's argmax; %.3g of the pixels have a top-2 gap below 2e-6"
          % (r.label, diff.sum(), diff.size, (gap < 2e-6).mean()))
    # bilinear1 keeps the rule but not test_fcn8_generic_class_counts' "fewer than 1e-3 of the pixels sit on ties": the
    # logits of its blank face span 0.6 over 68 classes, so 6e-3 of that face's pixels have their top two within 2e-6
    # on the float64 oracle whatever the seed (tests/test_peaked_cases_host.py's table: range 0.6)
    if name != "bilinear1":
        assert (gap < 2e-6).mean() < 1e-3, "the inputs sit on ties: pick another seed"
        assert diff.mean() < 1e-3
    if diff.any():
        assert gap[diff].max() < 2e-6, ("class map differs away from ties", float(gap[diff].max()))


# ---- (c) landmarks of the materialised path against the float64 decode -------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", P.CASE_NAMES)
def test_landmarks_against_the_reference_decode(flm, name, dtype):
    from oracle import decode_ref
    r = _run(name, dtype)
    n, h, w = P.SHAPE
    maps = r.probs.reshape(n, h + 8, w + 8, 68)
    for n_points, thresh in itertools.product((4, 25), THRESH):
        with np.errstate(all="ignore"):
            exp = decode_ref.transfer_target_ref(maps, thresh, n_points).reshape(n, 68, 2)
        got = _lm(r.model, r.xd, n_points, thresh, MAT)
        same = np.array_equal(got, exp, equal_nan=True)
        print("%s landmarks n=%d thresh=%g: %s; rejected %d of %d, NaN %d" % (r.label, n_points, thresh,
              "bit-equal" if same else "DIFFER at %d coordinates" % (~((got == exp) | (np.isnan(got) & np.isnan(exp)))).sum(),
              (exp[..., 0] == -1).sum(), exp[..., 0].size, np.isnan(exp).sum()))
        assert same, (r.label, n_points, thresh)
        for c in P.CASES[name][2]:   # the dead class: all zeros, so rejected at every thresh >= 0
            assert (got[:, c] == -1).all()


# ---- (d) the candidate path equals the materialised path ---------------------------------------------------------------

def _candidates_equal(r, xd, label, n_points_list=N_POINTS, subs=(0, 1)):
    for n_points, thresh in itertools.product(n_points_list, THRESH):
        ref = _lm(r.model, xd, n_points, thresh, MAT)
        for sub in subs:
            got = _lm(r.model, xd, n_points, thresh, dict(candidate_sub_phases=sub))
            assert np.array_equal(got, ref, equal_nan=True), (r.label, label, n_points, thresh, sub,
                                                              np.argwhere(~((got == ref) | (np.isnan(got) & np.isnan(ref))))[:8])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", P.CASE_NAMES)
def test_candidate_path_equals_materialised(flm, name, dtype):
    _candidates_equal(_run(name, dtype), _run(name, dtype).xd, "default")


BF16_KERNELS = {"generic": dict(up3_cand8=0), "cand8": dict(up3_cand8=3), "cand8 rows=1": dict(up3_cand8=3, up3_cand8_rows=1),
                "cand8 rows=8": dict(up3_cand8=3, up3_cand8_rows=8), "wreg": dict(up3_wreg=1)}


@pytest.mark.parametrize("kernel", list(BF16_KERNELS))
@pytest.mark.parametrize("name", P.CASE_NAMES)
def test_candidate_path_equals_materialised_bf16_kernels(flm, name, kernel):
    from flm_amd import _lib
    r = _run(name, "bf16")
    with _lib.tuning(**BF16_KERNELS[kernel]):
        _candidates_equal(r, r.xd, kernel)
        for n_points in (4, 25):
            cnt, flag, cap = _fills(r.model, r.xd, n_points)
            print("%s %-12s n=%-2d fills %s of %d, flag %d: %s" % (r.label, kernel, n_points, cnt, cap, flag, _path(cnt, flag, cap)))


@pytest.mark.parametrize("kernel", ["generic", "cand8", "wreg"])
def test_candidate_path_at_256_bf16_kernels(flm, kernel):
    """bilinear32 at 2 x 256 x 256 (face 1 blank): four bands of position rows per face in the weights-in-registers
    kernel, 1,104 positions per face in the other two."""
    from flm_amd import _lib
    if "m256" not in _RUNS:
        n, h, w = P.SHAPE_256
        _RUNS["m256"] = (_model("bilinear32", "bf16", h, w), torch.from_numpy(P.crops(n, h, w, seed=P.SEED + 2, blank=(1,))).cuda())
    model, xd = _RUNS["m256"]
    with _lib.tuning(**BF16_KERNELS[kernel]):
        for n_points in (4, 25):
            ref = _lm(model, xd, n_points, 0.0, MAT)
            got = _lm(model, xd, n_points, 0.0, None)
            assert np.array_equal(got, ref, equal_nan=True), (kernel, n_points)
            cnt, flag, cap = _fills(model, xd, n_points)
            print("bilinear32 bf16 2x256x256 %-7s n=%-2d fills %s of %d, flag %d: %s" % (kernel, n_points, cnt, cap, flag, _path(cnt, flag, cap)))


@pytest.mark.parametrize("dtype", DTYPES)
def test_landmark_stats_on_peaked_maps(flm, dtype):
    """The STATS instantiation of cand_merge_kernel: "landmark_stats" against decode_stats_device on the model's "probs"."""
    from flm_amd.utils.metrics import decode_stats_device
    r = _run("bilinear32", dtype)
    n, h, w = P.SHAPE
    probs = torch.from_numpy(r.probs).cuda().view(n, h + 8, w + 8, 68).contiguous()
    for n_points, sub in ((4, 0), (25, 0), (4, 1)):
        opts = dict(candidate_sub_phases=sub)
        rec = r.model.forward_device(r.xd, "landmark_stats", n_points=n_points, opts=opts).cpu().numpy()
        exp = decode_stats_device(probs, n_points, 0.0).cpu().numpy()
        assert np.array_equal(rec, exp, equal_nan=True), (r.label, n_points, sub)
        assert np.array_equal(rec[..., :2], _lm(r.model, r.xd, n_points, 0.0, opts), equal_nan=True)


# ---- (e) the mixed batches, (f) which path a run took ------------------------------------------------------------------

def _case_fills(name, dtype):
    """Fills and flag of the case's two batches at n_points 4 and 25, default options; printed once."""
    if (name, dtype) not in _FILLS:
        r = _run(name, dtype)
        out = {}
        for batch, xd in (("3 faces, 1 blank", r.xd), ("4 faces, 2 random", r.xd4)):
            for n_points in (4, 25):
                cnt, flag, cap = _fills(r.model, xd, n_points)
                out[(batch, n_points)] = (cnt, flag, cap)
                print("%s %-17s n=%-2d fills %s of %d, flag %d: %s" % (r.label, batch, n_points, cnt, cap, flag, _path(cnt, flag, cap)))
        _FILLS[(name, dtype)] = out
    return _FILLS[(name, dtype)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", P.CASE_NAMES)
def test_mixed_batch_one_random_face_among_blank_ones(flm, name, dtype):
    r = _run(name, dtype)
    _candidates_equal(r, r.xd4, "4 faces", n_points_list=(4, 25))
    _case_fills(name, dtype)


OVERFLOW_LEG = ("bilinear32", dict(candidate_cap_div=64))


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_path_is_taken(flm, dtype):
    taken = {}
    for name in P.CASE_NAMES:
        for key, (cnt, flag, cap) in _case_fills(name, dtype).items():
            taken.setdefault(_path(cnt, flag, cap), []).append((name,) + key)
    name, opts = OVERFLOW_LEG
    r = _run(name, dtype)
    cnt, flag, cap = _fills(r.model, r.xd, 4, opts)
    print("%s %s n=4 fills %s of %d, flag %d: %s" % (r.label, opts, cnt, cap, flag, _path(cnt, flag, cap)))
    taken.setdefault(_path(cnt, flag, cap), []).append((name, "cap_div", 4))
    assert np.array_equal(_lm(r.model, r.xd, 4, 0.0, opts), _lm(r.model, r.xd, 4, 0.0, MAT), equal_nan=True)
    # one sampled phase per tile gives a face fewer than 32 wave maxima per class at this shape: tau = 0 -> FLT_MIN
    one = dict(candidate_sub_phases=1)
    cnt, flag, cap = _fills(r.model, r.xd, 32, one)
    print("%s %s n=32 fills %s of %d, flag %d: %s" % (r.label, one, cnt, cap, flag, _path(cnt, flag, cap)))
    taken.setdefault(_path(cnt, flag, cap), []).append((name, "sub_phases=1", 32))
    for path in ("clear", "overflow", "short"):
        print("%s path %-8s: %s" % (dtype, path, taken.get(path, [])))
    assert taken.get("clear") and taken.get("overflow") and taken.get("short"), {k: len(v) for k, v in taken.items()}
