"""Forward, candidate path and standalone decodes on maps beyond 264 x 264 -- the sizes at which the code changes behaviour.

Every model class defaults to the reference's geometry, 416 x 608 (networks/fcn.py:167) -> a 424 x 616 map of 261,184
pixels; the other GPU tests stay at or below 256 x 256 (264 x 264 = 69,696).  Between the two lies the candidate path's
limit: a candidate key holds the pixel index in 17 bits, so landmark_candidates_enabled (flm_api_fcn.hip) and launch_convt
(flm_convt.hip) turn the path off from 2^17 output pixels on.  352 x 352 (360 x 360 = 129,600) is the last shape with
candidate lists, 352 x 384 (360 x 392 = 141,120) the first without.  tests/test_large_maps_host.py sweeps the layout rule
on the host; here:

(a) The default geometry, LANDMARKS_MODELS["fcn_8"](68) with no size arguments, one face, both types: the teacher-forced
    layer gate of tests/bf16_gate.py exactly as tests/test_gpu_fp32_layers.py and tests/test_gpu_bf16_layers.py apply it
    (pooled grids 208 x 304 .. 13 x 19, fc6 on 247 positions: two 128-row tiles, the second ragged); the class-map rule
    of test_fcn8_generic_class_counts; landmarks (n_points 4, 25, 0) and landmark records (n_points 4) bit-equal to
    decode_device / decode_stats_device of the same model's probabilities; no candidate buffers in the layout.  The
    free-running float64 oracle (oracle/fcn_ref.py) of the crop of seed 1024 has a top-2 gap below 2e-6 on 1.9e-5 of its
    pixels (checked on the CPU before the seed was fixed; 352 x 352 seed 704: 3.1e-5, 352 x 384 seed 736: 5.7e-5).
(b) The two sides of the limit, three faces, both types.  352 x 352: landmarks with candidates equal landmark_candidates
    = 0 bit for bit (n_points 4 and 25, thresh 0 and 0.5; bf16 also with up3_cand8 = 0 and 3), the fallback flag stays
    clear and every list below its capacity.  352 x 384: no cand_* buffers, the same workspace size and the same
    landmarks for both option values, equal to decode_device of the probabilities.  The bf16 layers of one of the three
    faces through the gate at both shapes.
(c) The standalone decodes on faces of more than 2^17 pixels -- decode_plan (flm_decode.hip) picks the chunks per face
    from the batch alone: one to three faces of 261,184 pixels are 32 chunks of 8,192 pixels, pixel indices need 18 bits.
    Random maps with two plateaux of exactly tied maxima: one in the last pixels of the map (indices above 2^17, the last
    chunk's tail), one across a chunk border computed as decode_plan computes it (the restatement is held to
    flm_decode_workspace_bytes).  1 x 424 x 616 x 68 (the LDS-DMA form; also with decode_lds_dma = 0), 3 x 424 x 616 x 68,
    2 x 300 x 450 x 5, 1 x 300 x 450 x 80 (24 channels per wave): flm_decode at n_points 1, 4, 25, 81, 128 and thresh 0,
    0.2 bit-equal to oracle/decode_ref.py transfer_target_ref; all-pixel mode within tests/test_gpu_decode.py's ALL_TOL;
    flm_decode_stats at the bars of tests/test_gpu_landmark_stats.py; flm_decode_sweep (0, 1, 4, 81) slice for slice as
    tests/test_gpu_eval.py.  The three-face case holds three channels per face to the oracle and every channel to the
    device's own single-face decode (another chunk plan input: faces = 1), bit for bit.
(d) predict(to_input_space=True), align_device on its output and graphs.CapturedPipeline(model, 1) at the default
    geometry: the capture holds the materialised landmark path and replays the eager sequence bit for bit.

What one run on an MI355X measured.  (a) 1 x 416 x 608, the kernels' largest |got - exact64| of the tensor's maximum (bf16:
beyond the half step) against the slack = 4 x e32 it was gated against; flips: elements that are not round_bf16(exact64),
kernels | float32 reference:

    layer      fp32: error / slack      bf16: over / slack       flips kernels | reference
    f1         2.3e-07 / 8.8e-07        1.9e-08 / 4.0e-07        42 | 43 of 4,046,848
    f2         1.7e-07 / 1.3e-06        8.1e-08 / 8.6e-07        91 | 93 of 2,023,424
    f3         2.3e-07 / 1.3e-06        1.1e-07 / 9.1e-07        77 | 48 of 1,011,712
    f4         1.8e-07 / 1.3e-06        4.0e-08 / 9.3e-07        14 | 8 of 252,928
    f5         1.5e-07 / 1.2e-06        1.5e-08 / 9.9e-07        1 | 4 of 63,232
    fc6        2.0e-07 / 2.5e-06        9.6e-08 / 1.5e-06        109 | 81 of 1,011,712
    fc7        2.1e-07 / 1.3e-06        6.8e-08 / 1.1e-06        74 | 61 of 1,011,712
    score5     2.4e-07 / 1.1e-06        2.3e-07 / 8.7e-07
    fuse4      2.1e-07 / 2.0e-06        2.2e-07 / 1.0e-06
    seg_feats  2.8e-07 / 2.1e-06        2.2e-07 / 1.2e-06
    logits     3.6e-07 / 2.4e-06        2.9e-07 / 9.4e-07
    probs      6.5e-07 (bar 1e-5)       5.7e-07 (bar 1e-5)

The kernels use at most 0.27 of their allowance (fp32 f1, bf16 score5), as on the small shapes; the 2e-5 cap never binds.  The class map equals the
teacher-forced oracle's argmax on all 261,184 pixels in both types (1.9e-5 / 3.1e-5 of its pixels have a top-2 gap below
2e-6).  Times of that case: the device work with its read-backs 0.10 s (fp32, the first launches of the process) and 0.02 s
(bf16), the float64 oracle on the CPU 2.0 s and 2.5 s, the test 2.5 s and 2.6 s; the bf16 gate of one face of 352 x 352 /
352 x 384 1.0 s / 1.1 s; no other test of the module above 0.4 s (building the 68-landmark single face and its sorts: 1.2 s,
once); the 25 tests together 14.6 s.
(b) 3 x 352 x 352, candidate keys per face against the capacity: n_points = 4 17,452 .. 17,859 of 69,632 in fp32 (fill
0.26; two sampled phases) and 11,337 .. 11,744 in bf16 (0.17; four phases); n_points = 25 31,358 .. 31,809 of 435,200 in fp32
(0.07) and 42,686 .. 43,256 in bf16 (0.10); fallback flag clear everywhere.  The bf16 layers of the middle face use at
most 0.35 of their allowance at both shapes (the logits).
(c) Every plan here is 32 chunks per face: 8,192 pixels at 424 x 616 (the last chunk holds 7,232; the middle border is
pixel 131,072 = 2^17 itself), 4,224 at 300 x 450 (the last holds 4,056; border 67,584).  Top-n coordinates and record
scores equal the oracle bit for bit; all-pixel coordinates differ from numpy's float32-hsum chain by at most 5.5e-5 px at
424 x 616 (one to two float32 steps of hsum at x near 300: the bar of 1e-4 px has a factor of two left at this size) and
2.6e-5 px at 300 x 450; all-pixel moments by at most 2.9e-11 px^2 (bound 6.5e-5), the score by one float32 step; sweep
slices equal the single decodes (all-pixel: 0 px).

Fault injection (scratch builds, not committed; wrong values or a refused call only; each run once).  (1) `1 << 17` as
`1 << 18` in landmark_candidates_enabled (flm_api_fcn.hip), launch_convt unchanged: the host sweep fails in all six
(n_points, type) cases and for the record layout (first at 128 x 960); on the GPU test_first_shape_without_candidate_lists
fails in both types, and so do test_default_geometry (both types: 261,184 < 2^18, the layout holds lists) and the captured
pipeline's test -- the forward there is refused by launch_convt ("a map below 2^17 pixels"); the 352 x 352 cases, the layer
gates and every decode case pass.  (2) decode_plan dropping the last, partial chunk of faces of 2^17 pixels and more
(`chunks = HW / px` there): all four shapes fail in test_decode_topn (the plan is not the library's), in
test_decode_all_pixel (4.6 .. 5.9 px from the oracle) and in test_decode_stats (coordinates not the oracle's bits);
tests/test_gpu_decode.py passes whole (its largest face has 69,696 pixels), and so do the forward tests of this module and
the sweep-against-decode cases, which compare the library with itself.
"""
import ctypes as C
import time

import numpy as np
import pytest
import torch

import stats_ref
from bf16_gate import check_layers
from oracle import decode_ref

pytestmark = pytest.mark.gpu

ALL_TOL = 1e-4                       # tests/test_gpu_decode.py: numpy's float32 pairwise hsum against the device's float64 sum
LIMIT = 1 << 17
LAST_CAND, FIRST_MAT = (352, 352), (352, 384)


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


@pytest.fixture(scope="module")
def M(flm):
    from flm_amd.utils import metrics
    return metrics


_ORACLE_CACHE = {}     # the oracle's large float64 operands (fc6, fc7), built once per (tensor, rounding) for the module


def _crops(n, h, w):
    """The seeds whose free-running float64 oracle was checked for ties on the CPU (module docstring): h + w."""
    return np.random.default_rng(h + w).integers(0, 256, (n, h, w, 3), dtype=np.uint8)


def _offset(model, name, n, n_points, opts=None, out_mode=None):
    from flm_amd import _lib
    fo = model._opts(opts)
    return _lib.load().flm_fcn_workspace_offset_opts(
        model._arch, name, n, model.input_height, model.input_width, model.n_classes, model._dt,
        _lib.OUT_LANDMARKS if out_mode is None else out_mode, _lib.DECODE_TOPN, n_points, C.byref(fo))


def _same(a, b):
    return torch.equal(a, b) or np.array_equal(a.cpu().numpy(), b.cpu().numpy(), equal_nan=True)


# ---- (a) the default geometry --------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_default_geometry(flm, weights68, M, dtype):
    from flm_amd import _lib
    from flm_amd.networks import LANDMARKS_MODELS
    from oracle import fcn_bf16_ref as B
    model = LANDMARKS_MODELS["fcn_8"](68) if dtype == "f32" else LANDMARKS_MODELS["fcn_8"](68, dtype=dtype)
    assert (model.input_height, model.input_width, model.output_height, model.output_width) == (416, 608, 424, 616)
    assert model.output_height * model.output_width >= LIMIT
    model.load_weights(weights68)
    n, h, w, oh, ow, c = 1, 416, 608, 424, 616, 68
    crops = _crops(n, h, w)
    label = "%s default 1x416x608" % dtype
    xd = torch.from_numpy(crops).cuda()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    probs_d = model.forward_device(xd, "probs")
    probs = probs_d.cpu().numpy()
    lg = model.forward_device(xd, "logits").cpu().numpy()
    torch.cuda.synchronize()
    t_gpu = time.perf_counter() - t0
    assert probs.shape == (n, oh * ow, c) and np.isfinite(probs).all()
    for k in ("f5", "fc7", "seg_feats"):   # the two forwards wrote the same bits into their workspaces
        assert torch.equal(model.intermediate(k, n, "probs"), model.intermediate(k, n, "logits")), k
    t0 = time.perf_counter()
    check_layers(model, weights68, crops, n, "probs", logits=lg, probs=probs, label=label, dtype=dtype, cache=_ORACLE_CACHE)
    t_cpu = time.perf_counter() - t0
    assert np.abs(probs.sum(-1) - 1).max() < 1e-5

    # class map: the rule of tests/test_gpu_fp32_layers.py test_fcn8_generic_class_counts
    t0 = time.perf_counter()
    cm = model.forward_device(xd, "classmap").cpu().numpy()
    torch.cuda.synchronize()
    seg = model.intermediate("seg_feats", n, "classmap").cpu().numpy().astype(np.float64)
    t_gpu += time.perf_counter() - t0
    assert cm.shape == (n, oh, ow) and cm.min() >= 0 and cm.max() < c, (cm.min(), cm.max())
    t0 = time.perf_counter()
    pr = B.softmax_ref(B.layer_bf16_ref("logits", seg, weights68, fp32=(dtype == "f32"), cache=_ORACLE_CACHE)[0]).reshape(n, oh, ow, c)
    diff = cm != pr.argmax(-1)
    srt = np.sort(pr, axis=-1)
    gap = srt[..., -1] - srt[..., -2]
    t_cpu += time.perf_counter() - t0
    print("%s class map: %d of %d pixels differ from the oracle's argmax; %.3g of the oracle's pixels have a top-2 gap below 2e-6"
          % (label, diff.sum(), diff.size, (gap < 2e-6).mean()))
    assert (gap < 2e-6).mean() < 1e-3, "the inputs sit on ties: pick another seed"
    if diff.any():
        assert gap[diff].max() < 2e-6, ("class map differs away from ties", float(gap[diff].max()))
    assert diff.mean() < 1e-3

    # landmarks and records: the layout has no candidate lists -- the decode of the probabilities, bit for bit
    t0 = time.perf_counter()
    pd = probs_d.view(n, oh, ow, c)
    for n_points in (4, 25, 0):
        if n_points:
            for name in (b"cand_sub", b"cand_tau", b"cand_keys", b"cand_cnt", b"cand_cap"):
                assert _offset(model, name, n, n_points) == -1, (name, n_points)
            assert _offset(model, b"probs", n, n_points) > 0
        lm = model.forward_device(xd, "landmarks", n_points=n_points)
        exp = M.decode_device(pd, n_points, 0.0)
        torch.cuda.synchronize()
        assert tuple(lm.shape) == (n, c, 2) and lm.dtype == torch.float64
        assert _same(lm, exp), (label, n_points)
        assert bool((lm[..., 0] >= 0).all()) and float(lm[..., 0].max()) < ow and float(lm[..., 1].max()) < oh
    assert _offset(model, b"cand_keys", n, 4, out_mode=_lib.OUT_LANDMARKS_STATS) == -1
    rec = model.forward_device(xd, "landmark_stats", n_points=4)
    exp = M.decode_stats_device(pd, 4, 0.0)
    torch.cuda.synchronize()
    assert _same(rec, exp), label
    assert torch.equal(rec[..., :2], model.forward_device(xd, "landmarks", n_points=4))
    t_gpu += time.perf_counter() - t0
    print("%s times: device work with its read-backs %.2f s, float64 oracle on the CPU %.2f s" % (label, t_gpu, t_cpu))


# ---- (b) the two sides of the 2^17 limit -----------------------------------------------------------------------------

_MODELS = {}


def _cliff_model(weights68, hw, dtype):
    """One model at a time (the packed weights are 285 MB in fp32), shared by the tests of one shape and type."""
    from flm_amd.networks import LANDMARKS_MODELS
    key = hw + (dtype,)
    if key not in _MODELS:
        _MODELS.clear()
        model = LANDMARKS_MODELS["fcn_8"](68, input_height=hw[0], input_width=hw[1], dtype=dtype)
        model.load_weights(weights68)
        _MODELS[key] = (model, torch.from_numpy(_crops(3, hw[0], hw[1])).cuda())
    return _MODELS[key]


def _lm(model, xd, n_points, thresh, candidates):
    return model.forward_device(xd, "landmarks", n_points=n_points, thresh=thresh,
                                opts=dict(landmark_candidates=1 if candidates else 0))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_last_shape_with_candidate_lists(flm, weights68, dtype):
    """352 x 352 -> 360 x 360 = 129,600 pixels, the largest square map below 2^17."""
    from flm_amd import _lib
    h, w = LAST_CAND
    n = 3
    assert (h + 8) * (w + 8) < LIMIT <= (h + 8) * (w + 32 + 8)
    model, xd = _cliff_model(weights68, LAST_CAND, dtype)
    on, off = dict(landmark_candidates=1), dict(landmark_candidates=0)
    rejected = kept = 0
    for n_points in (4, 25):
        assert _offset(model, b"cand_keys", n, n_points, on) > 0 and _offset(model, b"cand_keys", n, n_points, off) == -1
        assert model.workspace_bytes(n, "landmarks", n_points, on) > model.workspace_bytes(n, "landmarks", n_points, off)
        for thresh in (0.0, 0.5):
            ref = _lm(model, xd, n_points, thresh, candidates=False)
            assert tuple(ref.shape) == (n, 68, 2) and ref.dtype == torch.float64
            knobs = (None, 0, 3) if dtype == "bf16" else (None,)
            for knob in knobs:
                with _lib.tuning(**({} if knob is None else dict(up3_cand8=knob))):
                    got = _lm(model, xd, n_points, thresh, candidates=True)
                    torch.cuda.synchronize()
                assert torch.equal(got, ref), (dtype, n_points, thresh, knob, float((got - ref).abs().max()))
            rejected += int((ref[..., 0] == -1).sum())
            kept += int((ref[..., 0] != -1).sum())
        assert float(ref[..., 0].max()) < w + 8 and float(ref[..., 1].max()) < h + 8
    assert rejected and kept   # thresh 0.5 rejects part of the landmarks: both branches ran
    # the lists on these ordinary maps: no fallback, every face below the capacity
    for n_points in (4, 25):
        ws = model.new_workspace(n, "landmarks", n_points, on)
        model.forward_device(xd, "landmarks", n_points=n_points, workspace=ws, opts=on)
        torch.cuda.synchronize()
        cap, at = _offset(model, b"cand_cap", n, n_points, on), _offset(model, b"cand_cnt", n, n_points, on)
        cnt = ws[at:at + 4 * (n + 1)].view(torch.int32).cpu().numpy()
        print("%s 3x352x352 n_points %d: candidate keys per face %s of a capacity of %d (fill %.3f), fallback flag %d"
              % (dtype, n_points, cnt[:n].tolist(), cap, cnt[:n].max() / cap, cnt[n]))
        assert cnt[n] == 0, (dtype, n_points, "fallback flag raised")
        assert 68 * n_points <= cnt[:n].min() and cnt[:n].max() < cap, (dtype, n_points, cnt[:n], cap)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_first_shape_without_candidate_lists(flm, weights68, M, dtype):
    """352 x 384 -> 360 x 392 = 141,120 pixels, the smallest map from 2^17 on (with 384 x 352)."""
    h, w = FIRST_MAT
    n = 3
    assert (h + 8) * (w - 32 + 8) < LIMIT <= (h + 8) * (w + 8)
    model, xd = _cliff_model(weights68, FIRST_MAT, dtype)
    on, off = dict(landmark_candidates=1), dict(landmark_candidates=0)
    pd = model.forward_device(xd, "probs").view(n, h + 8, w + 8, 68)
    rejected = kept = 0
    for n_points in (4, 25):
        for opts in (on, off, None):
            for name in (b"cand_sub", b"cand_tau", b"cand_keys", b"cand_cnt", b"cand_cap"):
                assert _offset(model, name, n, n_points, opts) == -1, (name, n_points, opts)
        assert model.workspace_bytes(n, "landmarks", n_points, on) == model.workspace_bytes(n, "landmarks", n_points, off)
        for thresh in (0.0, 0.5):
            a = _lm(model, xd, n_points, thresh, candidates=True)
            b = _lm(model, xd, n_points, thresh, candidates=False)
            exp = M.decode_device(pd, n_points, thresh)
            torch.cuda.synchronize()
            assert torch.equal(a, b), (dtype, n_points, thresh)
            assert torch.equal(a, exp), (dtype, n_points, thresh, float((a - exp).abs().max()))
            rejected += int((a[..., 0] == -1).sum())
            kept += int((a[..., 0] != -1).sum())
    assert rejected and kept


@pytest.mark.parametrize("hw", [LAST_CAND, FIRST_MAT], ids=["352x352", "352x384"])
def test_bf16_layers_at_the_limit(flm, weights68, hw):
    """The teacher-forced bf16 gate on the middle face of the three (the oracle's cost of one face)."""
    n, f = 3, 1
    model, xd = _cliff_model(weights68, hw, "bf16")
    probs = model.forward_device(xd, "probs").cpu().numpy()
    logits = model.forward_device(xd[f:f + 1].contiguous(), "logits").cpu().numpy()
    torch.cuda.synchronize()
    check_layers(model, weights68, xd.cpu().numpy(), n, "probs", faces=[f], logits=logits, probs=probs[[f]],
                 label="bf16 3x%dx%d face %d" % (hw + (f,)), cache=_ORACLE_CACHE)


# ---- (c) standalone decodes beyond 2^17 pixels per face --------------------------------------------------------------

PT = 64                                       # flm_decode_dev.h: pixels per tile
N_POINTS = (1, 4, 25, 81, 128)
THRESH = (0.0, 0.2)
SWEEP_MODES = (0, 1, 4, 81)
DECODE_SHAPES = [(1, 424, 616, 68), (3, 424, 616, 68), (2, 300, 450, 5), (1, 300, 450, 80)]
PLATEAU = np.float32(0.984375)                # above every random value (at most 0.98)


def decode_plan(n, h, w):
    """flm_decode.hip decode_plan restated: (chunks per face, pixels per chunk)."""
    hw, faces = h * w, max(n, 1)
    best_s, best_u = 1, 0.0
    for s in range(1, 33):
        wgs = faces * s
        rounds = (wgs + 767) // 768
        u = wgs / (rounds * 768)
        if u > best_u * 1.05:
            best_u, best_s = u, s
    px = -(-hw // best_s)
    px = -(-px // PT) * PT                    # chunk_px = ceil(ceil(HW / s) / PT) * PT
    return -(-hw // px), px


class DecodeCase:
    """Maps of one shape with their planted ties, on the host and the device, and the oracle's results, computed once.
    Random float32 in [0.02, 0.98]; every third landmark at 1/8 (thresh 0.2 rejects those in both modes); landmark 1 of
    face 0 all zero (rejected at thresh 0 too); forty tied maxima in the last 60 pixels of the last face's last landmark
    (indices above 2^17, the tail of the last chunk); forty tied maxima across the middle chunk border of face 0,
    landmark 2 -- twenty on either side, so the top 25 take the upper twenty and five from the chunk below."""

    def __init__(self, shape):
        n, h, w, l = shape
        hw = h * w
        assert hw > LIMIT
        self.shape = shape
        self.chunks, self.chunk_px = decode_plan(n, h, w)
        assert self.chunks >= 4 and (self.chunks - 1) * self.chunk_px < hw <= self.chunks * self.chunk_px
        rng = np.random.default_rng(sum(shape))
        y = rng.random(shape, dtype=np.float32) * np.float32(0.96) + np.float32(0.02)
        y[..., ::3] *= np.float32(0.125)
        y[0, :, :, 1] = 0
        flat = y.reshape(n, hw, l)
        self.tail = (n - 1, l - 1)
        flat[n - 1, hw - 60:hw - 20, l - 1] = PLATEAU
        assert hw - 60 > LIMIT and hw - 60 >= (self.chunks - 1) * self.chunk_px
        self.border = (self.chunks // 2) * self.chunk_px
        self.straddle = (0, 2)
        flat[0, self.border - 20:self.border + 20, 2] = PLATEAU
        assert (l - 1) % 3 and y.max() == PLATEAU
        self.y = y
        self.hm = torch.from_numpy(y).cuda()
        # the channels held to the oracle: all of them, or -- three faces of 68 -- three per face, the planted ones among them
        if n * l <= 80:
            self.channels = [list(range(l))] * n
        else:
            self.channels = [[0, 1, 2], [5, 33, 66], [3, 20, l - 1]][:n]
        self.sub = [np.ascontiguousarray(y[f:f + 1][..., self.channels[f]]) for f in range(n)]
        self.orders = [stats_ref.stable_orders(s) for s in self.sub]
        self._topn, self._all = {}, {}

    def pick(self, got):
        """The oracle's channels of a device result [N,L,...]: a list per face."""
        return [got[f:f + 1][:, self.channels[f]] for f in range(self.shape[0])]

    def topn(self, n_points, thresh):
        """Per face: (transfer_target_ref [1,C',2], records_ref [1,C',6]) of the oracle's channels."""
        key = (n_points, thresh)
        if key not in self._topn:
            out = []
            for s, o in zip(self.sub, self.orders):
                with np.errstate(all="ignore"):
                    xy = decode_ref.transfer_target_ref(s, thresh, n_points, orders=o).reshape(1, s.shape[3], 2)
                out.append((xy, stats_ref.records_ref(s, n_points, thresh, o)))
            self._topn[key] = out
        return self._topn[key]

    def all_pixel(self, thresh):
        """Per face: (transfer_target_ref [1,C',2], records_ref, numpy-sum scores) of the all-pixel mode."""
        if thresh not in self._all:
            out = []
            for s in self.sub:
                with np.errstate(all="ignore"):
                    xy = decode_ref.transfer_target_ref(s, thresh, 0).reshape(1, s.shape[3], 2)
                out.append((xy,) + stats_ref.records_ref(s, 0, thresh))
            self._all[thresh] = out
        return self._all[thresh]


def _ids(shape):
    return "x".join(str(v) for v in shape)


@pytest.fixture(scope="module", params=DECODE_SHAPES, ids=_ids)
def case(request, flm):
    """One shape at a time (three faces are 213 MB): pytest runs the tests of a module-scoped parameter together."""
    return DecodeCase(request.param)


def test_decode_topn_on_large_faces(M, case):
    from flm_amd import _lib
    shape = case.shape
    n, h, w, l = shape
    print("%s: %d chunks of %d pixels per face (the last holds %d), plateau across pixel %d"
          % (_ids(shape), case.chunks, case.chunk_px, h * w - (case.chunks - 1) * case.chunk_px, case.border))
    lib = _lib.load()
    for n_max in (4, 128):   # the restated plan is the library's: its key lists are [n][chunks][l][n_max] 8-byte keys
        assert lib.flm_decode_workspace_bytes(n, h, w, l, _lib.DECODE_TOPN, n_max) == -(-(n * case.chunks * l * n_max * 8) // 256) * 256
    singles = {}
    rejected = kept = 0
    for n_points in N_POINTS:
        for thresh in THRESH:
            got = M.decode_device(case.hm, n_points, thresh)
            assert tuple(got.shape) == (n, l, 2) and got.dtype == torch.float64
            for g, (xy, _) in zip(case.pick(got.cpu().numpy()), case.topn(n_points, thresh)):
                assert np.array_equal(g, xy), (shape, n_points, thresh, np.abs(g - xy).max())
                rejected += int((xy[..., 0] == -1).sum())
                kept += int((xy[..., 0] != -1).sum())
            if l == 68:     # the register-prefetch stream gives the LDS-DMA ring's bits (n <= 64; beyond, both run the former)
                with _lib.tuning(decode_lds_dma=0):
                    other = M.decode_device(case.hm, n_points, thresh)
                assert torch.equal(other, got), (shape, n_points, thresh, "decode_lds_dma = 0")
            if n > 1:       # the decode is per face: a face alone (another plan input) gives the same bits, every channel
                for f in range(n):
                    alone = M.decode_device(case.hm[f:f + 1], n_points, thresh)
                    assert torch.equal(alone[0], got[f]), (shape, n_points, thresh, f)
    assert rejected and kept
    # the planted ties decide: the top 25 of the straddling plateau are its upper twenty and five from the chunk below
    f, ch = case.straddle
    top = np.arange(case.border - 5, case.border + 20)
    exp = np.array([np.mean(top % w), np.mean(top // w)])     # equal weights: the plain mean (float32 hsum aside)
    got = M.decode_device(case.hm, 25, 0.0)[f, ch].cpu().numpy()
    assert np.abs(got - exp).max() < 1e-3, (got, exp)


def test_decode_all_pixel_on_large_faces(M, case):
    from flm_amd import _lib
    shape = case.shape
    n, h, w, l = shape
    worst = 0.0
    rejected = 0
    same_plan = decode_plan(1, h, w) == (case.chunks, case.chunk_px)
    for thresh in THRESH:
        got = M.decode_device(case.hm, 0, thresh)
        for g, (xy, _, _) in zip(case.pick(got.cpu().numpy()), case.all_pixel(thresh)):
            assert np.array_equal(g[..., 0] == -1, xy[..., 0] == -1), (shape, thresh)
            worst = max(worst, float(np.abs(g - xy).max()))
            rejected += int((xy[..., 0] == -1).sum())
        if l == 68:
            with _lib.tuning(decode_lds_dma=0):
                assert torch.equal(M.decode_device(case.hm, 0, thresh), got), (shape, thresh, "decode_lds_dma = 0")
        for f in range(n if n > 1 else 0):
            # float64 partial sums per chunk, added in chunk order: the same bits where a face alone is cut into the same
            # chunks, within the sweep's 1e-9 px (tests/test_gpu_eval.py: another order of float64 additions) elsewhere
            alone = M.decode_device(case.hm[f:f + 1], 0, thresh)
            if same_plan:
                assert _same(alone[0], got[f]), (shape, thresh, f)
            else:
                a, b = alone[0].cpu().numpy(), got[f].cpu().numpy()
                assert np.array_equal(a == -1, b == -1) and np.abs(a - b).max() <= 1e-9, (shape, thresh, f)
    print("%s all-pixel: max |device - oracle| %.3g px (bar %g)" % (_ids(shape), worst, ALL_TOL))
    assert worst <= ALL_TOL and rejected


def _check_topn_records(got, xy, exp, n_points, where):
    """tests/test_gpu_landmark_stats.py test_standalone_topn, its bars."""
    assert np.array_equal(got[..., :2], xy, equal_nan=True), where
    assert np.array_equal(got[..., :2], exp[..., :2]), where
    assert np.array_equal(got[..., 2], exp[..., 2]), where
    rej = exp[..., 0] == -1
    assert np.array_equal(got[rej], exp[rej]), where                   # exactly (-1, -1, score, -1, -1, 0)
    assert np.all(exp[rej][:, 3:] == [-1.0, -1.0, 0.0])
    g, e = got[~rej], exp[~rej]
    if n_points == 1:
        assert np.all(g[:, 3:] == 0.0), where
    dv = np.abs(g[:, 3:5] - e[:, 3:5])
    assert np.all(dv <= 1e-12 * e[:, 3:5]), (where, dv.max())
    dc = np.abs(g[:, 5] - e[:, 5])
    assert np.all(dc <= 1e-12 * (e[:, 3] + e[:, 4])), (where, dc.max())
    assert np.all(g[:, 3:5] >= 0.0)
    return int(rej.sum()), int((~rej).sum())


def test_decode_stats_on_large_faces(M, case):
    shape = case.shape
    n, h, w, l = shape
    rejected = kept = 0
    for n_points in N_POINTS:
        for thresh in THRESH:
            got = M.decode_stats_device(case.hm, n_points, thresh)
            assert tuple(got.shape) == (n, l, 6) and got.dtype == torch.float64
            assert torch.equal(got[..., :2], M.decode_device(case.hm, n_points, thresh)), (shape, n_points, thresh)
            for f, (g, (xy, exp)) in enumerate(zip(case.pick(got.cpu().numpy()), case.topn(n_points, thresh))):
                r, k = _check_topn_records(g, xy, exp, n_points, (shape, n_points, thresh, f))
                rejected, kept = rejected + r, kept + k
            for f in range(n if n > 1 else 0):
                assert torch.equal(M.decode_stats_device(case.hm[f:f + 1], n_points, thresh)[0], got[f]), (shape, n_points, thresh, f)
    assert rejected and kept
    # all-pixel mode: tests/test_gpu_landmark_stats.py test_standalone_all_pixel, its bars
    bound = 4.0 * h * w * 2.0 ** -53 * (h * h + w * w)
    worst = worst_score = 0.0
    rejected = 0
    for thresh in THRESH:
        got = M.decode_stats_device(case.hm, 0, thresh)
        assert _same(got[..., :2], M.decode_device(case.hm, 0, thresh)), (shape, thresh)
        for g, (_, exp, score_np) in zip(case.pick(got.cpu().numpy()), case.all_pixel(thresh)):
            rel = np.abs(g[..., 2] - score_np) / np.where(score_np > 0, score_np, 1.0)
            worst_score = max(worst_score, float(rel.max()))
            assert rel.max() <= 2.0 ** -22, (shape, thresh, rel.max())
            rej = g[..., 0] == -1
            assert np.array_equal(rej, exp[..., 0] == -1), (shape, thresh)
            assert np.all(g[rej][:, [0, 1, 3, 4, 5]] == [-1.0, -1.0, -1.0, -1.0, 0.0])
            d = np.abs(g[~rej][:, 3:] - exp[~rej][:, 3:])
            worst = max(worst, float(d.max()))
            assert d.max() <= bound, (shape, thresh, d.max(), bound)
            assert np.all(g[~rej][:, 3:5] >= 0.0)
            rejected += int(rej.sum())
    print("%s all-pixel records: moments off by at most %.3g px^2 (bound %.3g), score by %.3g relative (bound %.3g)"
          % (_ids(shape), worst, bound, worst_score, 2.0 ** -22))
    assert rejected


def test_decode_sweep_on_large_faces(M, case):
    from test_gpu_eval import check_sweep_vs_decode
    shape = case.shape
    worst = 0.0
    for thresh in THRESH:
        worst = max(worst, check_sweep_vs_decode(M, case.hm, list(SWEEP_MODES), thresh))
    print("%s sweep %s: all-pixel max |sweep - decode| %.3g px (bar 1e-9)" % (_ids(shape), SWEEP_MODES, worst))


# ---- (d) the Python conveniences at the default geometry ---------------------------------------------------------------

def test_predict_align_and_captured_pipeline_at_the_default_geometry(flm, weights68):
    from flm_amd import alignment, graphs, prediction
    from flm_amd.networks import LANDMARKS_MODELS
    from oracle import warp_ref
    model = LANDMARKS_MODELS["fcn_8"](68)
    model.load_weights(weights68)
    h, w, oh, ow = 416, 608, 424, 616
    assert (model.input_height, model.input_width) == (h, w)
    rng = np.random.default_rng(71)
    crops = torch.from_numpy(rng.integers(0, 256, (1, h, w, 3), dtype=np.uint8)).cuda()
    lm = model.forward_device(crops, "landmarks", n_points=4)
    assert torch.equal(prediction.predict(crops, model), lm)
    # to_input_space: x * W / W', y * H / H' in float64 (prediction.predict's docstring); the ratios differ here
    lm_in = prediction.predict(crops, model, to_input_space=True)
    assert lm_in.is_cuda and np.array_equal(lm_in.cpu().numpy(), lm.cpu().numpy() * np.array([w / ow, h / oh]))
    assert bool((lm >= 0).all()) and float(lm_in[..., 0].max()) < w and float(lm_in[..., 1].max()) < h
    lm_np = prediction.predict(crops.cpu().numpy(), model, to_input_space=True)       # numpy in -> numpy out
    assert isinstance(lm_np, np.ndarray) and np.array_equal(lm_np, lm_in.cpu().numpy())
    # align_device on it: the fit bit-equal to the float64 restatement and to the in-kernel scale, the warp within 1 ULP
    tm = alignment.canonical_template(68, 112, 112)
    tmd = torch.from_numpy(tm).cuda()
    aligned, m = alignment.align_device(crops, lm_in, tmd, 112, 112)
    assert tuple(aligned.shape) == (1, 112, 112, 3) and aligned.dtype == torch.float32
    assert np.array_equal(m.cpu().numpy(), warp_ref.similarity_ref(lm_in.cpu().numpy(), tm))
    assert torch.equal(m, alignment.similarity_device(lm, tmd, (w / ow, h / oh)))
    exp = warp_ref.warp_affine_ref(crops.cpu().numpy(), m.cpu().numpy(), 112, 112)
    a, b = aligned.cpu().numpy().view(np.int32).astype(np.int64), exp.view(np.int32).astype(np.int64)
    a, b = np.where(a < 0, -(a & 0x7fffffff), a), np.where(b < 0, -(b & 0x7fffffff), b)   # monotone integer image of floats
    assert np.abs(a - b).max() <= 1
    # the captured graph holds the materialised landmark path (no candidate lists at this size) and replays it exactly
    pipe = graphs.CapturedPipeline(model, 1)
    assert pipe.n_points == 4 and _offset(model, b"cand_keys", 1, pipe.n_points) == -1
    assert pipe.workspace.numel() == model.workspace_bytes(1, "landmarks", 4, dict(landmark_candidates=0))
    assert pipe.scale == (w / ow, h / oh) and pipe.out_hw == (h, w)
    for rep in range(3):
        x = torch.from_numpy(rng.integers(0, 256, (1, h, w, 3), dtype=np.uint8)).cuda()
        lm_g, al_g, m_g = [t.clone() for t in pipe(x)]
        lm_e = model.forward_device(x, "landmarks", n_points=4)
        al_e, m_e = alignment.align_device(x, lm_e, pipe.template, h, w, pipe.scale)
        assert torch.equal(lm_g, lm_e) and torch.equal(m_g, m_e) and torch.equal(al_g, al_e), rep
        assert not torch.equal(lm_g, lm)                    # another input, another result: the replay read its input
