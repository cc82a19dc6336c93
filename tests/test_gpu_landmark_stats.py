"""GPU parity of the landmark records (flm_decode_stats, FLM_OUT_LANDMARKS_STATS) and of the confidence-weighted fit
(flm_similarity_from_landmarks_weighted) against the float64 restatements of tests/stats_ref.py, which stand on
oracle/decode_ref.py's chain for hsum, x and y.

Bars (include/flm.h states the arithmetic they follow from):
  top-n      x, y bit-equal to flm_decode; score bit-equal to the restatement; var_x, var_y within relative 1e-12 (at
             most 128 sequential float64 additions of non-negative terms, two roundings each: <= ~1.5e-14, 70x head
             room); cov_xy within 1e-12 * (var_x + var_y), since |dx*dy| <= (dx^2 + dy^2) / 2; n_points = 1 gives
             exact zeros; a rejected row is exactly (-1, -1, score, -1, -1, 0)
  all-pixel  x, y bit-equal to flm_decode(ALL); score within one float32 ulp (relative 2^-22) of numpy's float32 sum;
             moments within 4 * H*W * 2^-53 * (H^2 + W^2) px^2 of the float64 restatement (worst-case sequential-sum
             bound on a raw moment, x4 for the two sums, the division and the subtraction)
  forward    "landmark_stats" bit-equal to decode_stats_device on the same model's "probs", on every route
  fit        bit-equal to the sequential float64 restatement; unit weights bit-equal to oracle.warp_ref.similarity_ref
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import warp_ref  # noqa: E402

import stats_ref  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(3, 48, 56, 5), (2, 33, 17, 68), (1, 12, 11, 96), (5, 64, 64, 21), (2, 72, 72, 68)]   # the last: the LDS-DMA stream
N_POINTS = (1, 4, 33, 64, 100)                                                                # 100: two list registers
THRESH = (0.0, 0.3)


@pytest.fixture(scope="module")
def mods():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import flm_amd  # noqa: F401
    from flm_amd import _lib, alignment, prediction
    from flm_amd.utils import metrics
    _lib.load()
    return _lib, alignment, prediction, metrics


def _maps(shape):
    """Random positive float32 maps; every third landmark dimmed so that thresh 0.3 rejects part of them in both modes;
    a few planted peaks, a few exactly tied values (at and around the n-th place), one constant map, one all-zero
    landmark."""
    n, h, w, l = shape
    rng = np.random.default_rng(sum(shape))
    y = rng.random(shape, dtype=np.float32) * np.float32(0.96) + np.float32(0.02)
    y[..., ::3] *= np.float32(0.25)
    for _ in range(6):
        f, c = int(rng.integers(n)), int(rng.integers(l))
        r0, c0 = int(rng.integers(h - 2)), int(rng.integers(w - 2))
        y[f, r0:r0 + 2, c0:c0 + 2, c] = [[1.5, 1.25], [1.75, 2.0]]         # a planted peak
    f, c = 0, l - 1
    y[f, 1:4, 2:6, c] = np.float32(0.984375)                               # twelve exactly tied maxima
    y[n - 1, :, :, 0] = np.float32(0.5)                                    # a constant map: every pixel ties
    y[0, :, :, 1] = 0                                                      # an all-zero landmark: rejected
    return y


@pytest.fixture(scope="module")
def cases():
    """The maps of every shape with their stable argsorts, computed once and shared by the tests below."""
    out = {}
    for shape in SHAPES:
        y = _maps(shape)
        out[shape] = (y, stats_ref.stable_orders(y))
    return out


@pytest.mark.parametrize("shape", SHAPES)
def test_standalone_topn(mods, cases, shape):
    _lib, _, _, M = mods
    y, orders = cases[shape]
    hm = torch.from_numpy(y).cuda()
    worst_var = worst_cov = 0.0
    rejected = kept = 0
    for n in N_POINTS:
        for t in THRESH:
            got = M.decode_stats_device(hm, n, t).cpu().numpy()
            xy = M.decode_device(hm, n, t).cpu().numpy()
            exp = stats_ref.records_ref(y, n, t, orders)
            assert got.shape == shape[:1] + (shape[3], 6) and got.dtype == np.float64
            assert np.array_equal(got[..., :2], xy, equal_nan=True), (shape, n, t)
            assert np.array_equal(got[..., :2], exp[..., :2]), (shape, n, t)
            assert np.array_equal(got[..., 2], exp[..., 2]), (shape, n, t)
            rej = exp[..., 0] == -1
            assert np.array_equal(got[rej], exp[rej]), (shape, n, t)       # exactly (-1, -1, score, -1, -1, 0)
            assert np.all(exp[rej][:, 3:] == [-1.0, -1.0, 0.0])
            g, e = got[~rej], exp[~rej]
            if n == 1:
                assert np.all(g[:, 3:] == 0.0), (shape, t)
            dv = np.abs(g[:, 3:5] - e[:, 3:5])
            assert np.all(dv <= 1e-12 * e[:, 3:5]), (shape, n, t, dv.max())
            dc = np.abs(g[:, 5] - e[:, 5])
            assert np.all(dc <= 1e-12 * (e[:, 3] + e[:, 4])), (shape, n, t, dc.max())
            assert np.all(g[:, 3:5] >= 0.0)
            with np.errstate(invalid="ignore", divide="ignore"):
                worst_var = max(worst_var, float(np.nanmax(np.where(e[:, 3:5] > 0, dv / e[:, 3:5], 0.0), initial=0.0)))
                worst_cov = max(worst_cov, float(np.nanmax(np.where(e[:, 3] + e[:, 4] > 0, dc / (e[:, 3] + e[:, 4]), 0.0), initial=0.0)))
            rejected += int(rej.sum())
            kept += int((~rej).sum())
    print("top-n %s: worst relative error var %.3g, cov / (var_x + var_y) %.3g; %d rows kept, %d rejected"
          % (shape, worst_var, worst_cov, kept, rejected))
    assert rejected and kept                     # both branches ran
    # the numpy mirror: same records, numpy in -> numpy out
    assert np.array_equal(M.transfer_target_stats(y, 0.3, 4), M.decode_stats_device(hm, 4, 0.3).cpu().numpy())


@pytest.mark.parametrize("shape", SHAPES)
def test_standalone_all_pixel(mods, cases, shape):
    _lib, _, _, M = mods
    y, _ = cases[shape]
    n, h, w, l = shape
    hm = torch.from_numpy(y).cuda()
    bound = 4.0 * h * w * 2.0 ** -53 * (h * h + w * w)
    worst = worst_score = 0.0
    rejected = 0
    for t in THRESH:
        got = M.decode_stats_device(hm, 0, t).cpu().numpy()
        xy = M.decode_device(hm, 0, t).cpu().numpy()
        exp, score_np = stats_ref.records_ref(y, 0, t)
        assert np.array_equal(got[..., :2], xy, equal_nan=True), (shape, t)
        rel = np.abs(got[..., 2] - score_np) / np.where(score_np > 0, score_np, 1.0)
        worst_score = max(worst_score, float(rel.max()))
        assert rel.max() <= 2.0 ** -22, (shape, t, rel.max())
        rej = got[..., 0] == -1
        assert np.array_equal(rej, exp[..., 0] == -1), (shape, t)
        assert np.all(got[rej][:, [0, 1, 3, 4, 5]] == [-1.0, -1.0, -1.0, -1.0, 0.0])
        d = np.abs(got[~rej][:, 3:] - exp[~rej][:, 3:])
        worst = max(worst, float(d.max()))
        assert d.max() <= bound, (shape, t, d.max(), bound)
        assert np.all(got[~rej][:, 3:5] >= 0.0)
        rejected += int(rej.sum())
    print("all-pixel %s: moments off by at most %.3g px^2 (bound %.3g), score by %.3g relative (bound %.3g)"
          % (shape, worst, bound, worst_score, 2.0 ** -22))
    assert rejected
    # the register-prefetch stream gives the LDS-DMA stream's bits (68-landmark maps with 16-byte faces run the latter)
    if l == 68:
        with _lib.tuning(decode_lds_dma=0):
            other = M.decode_stats_device(hm, 0, 0.0).cpu().numpy()
        assert np.array_equal(other, M.decode_stats_device(hm, 0, 0.0).cpu().numpy(), equal_nan=True)


# ---- forward -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def weights68():
    from flm_amd.weights import synth_fcn8_weights
    return synth_fcn8_weights(68, seed=2)


def _forward_routes(mods, model, xd, routes):
    """"landmark_stats" on every (n_points, opts) route against decode_stats_device on the model's own "probs", and its
    first two columns against "landmarks"."""
    _lib, _, _, M = mods
    n = int(xd.shape[0])
    probs = model.forward_device(xd, "probs").reshape(n, model.output_height, model.output_width, model.n_classes).contiguous()
    for n_points, opts in routes:
        rec = model.forward_device(xd, "landmark_stats", n_points=n_points, opts=opts)
        assert tuple(rec.shape) == (n, model.n_classes, 6) and rec.dtype == torch.float64
        exp = M.decode_stats_device(probs, n_points, 0.0)
        assert torch.equal(rec, exp), (model.model_name, model.dtype, n_points, opts)
        lm = model.forward_device(xd, "landmarks", n_points=n_points, opts=opts)
        assert torch.equal(rec[..., :2], lm), (model.model_name, model.dtype, n_points, opts)
        assert bool((rec[..., 2] > 0).all()) and bool((rec[..., 3:5] >= 0).all())


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_forward_every_route(mods, weights68, dtype):
    _lib, _, _, M = mods
    from flm_amd.networks import LANDMARKS_MODELS
    n = 3
    model = LANDMARKS_MODELS["fcn_8"](68, input_height=64, input_width=64, dtype=dtype)
    model.load_weights(weights68)
    xd = torch.from_numpy(np.random.default_rng(51).integers(0, 256, (n, 64, 64, 3), dtype=np.uint8)).cuda()
    overflow = dict(candidate_cap_div=4096)
    _forward_routes(mods, model, xd, [(4, None), (4, overflow), (4, dict(landmark_candidates=0)), (64, None), (0, None)])
    # the routes are the ones named: the default call has candidate lists and leaves the overflow flag clear, the shrunk
    # lists raise it (so the gated materialising launches wrote the records), landmark_candidates = 0 has no lists
    lib = _lib.load()
    import ctypes as C
    for opts, flag in ((None, 0), (overflow, 1)):
        ws = model.new_workspace(n, "landmark_stats", 4, opts)
        model.forward_device(xd, "landmark_stats", n_points=4, workspace=ws, opts=opts)
        torch.cuda.synchronize()
        fo = model._opts(opts)
        off = lib.flm_fcn8_workspace_offset_opts(b"cand_cnt", n, 64, 64, 68, model._dt, _lib.OUT_LANDMARKS_STATS,
                                                 _lib.DECODE_TOPN, 4, C.byref(fo))
        assert off > 0
        cnt = ws[off:off + 4 * (n + 1)].view(torch.int32).cpu().numpy()
        assert int(cnt[n] != 0) == flag, (dtype, opts, cnt)
    fo = model._opts(dict(landmark_candidates=0))
    assert lib.flm_fcn8_workspace_offset_opts(b"cand_cnt", n, 64, 64, 68, model._dt, _lib.OUT_LANDMARKS_STATS,
                                              _lib.DECODE_TOPN, 4, C.byref(fo)) == -1
    # a thresh that rejects part of the landmarks, the empty batch, a caller's output tensor
    # (the median score -- a float32 value, so the call's float thresh is that number: it and everything below go)
    t = float(model.forward_device(xd, "landmark_stats", n_points=4)[..., 2].median())
    rec = model.forward_device(xd, "landmark_stats", n_points=4, thresh=t)
    lm = model.forward_device(xd, "landmarks", n_points=4, thresh=t)
    assert torch.equal(rec[..., :2], lm)
    rej = lm[..., 0] == -1
    assert bool(rej.any()) and bool((~rej).any())
    assert bool((rec[rej][:, 3:] == torch.tensor([-1.0, -1.0, 0.0], dtype=torch.float64, device="cuda")).all())
    assert bool((rec[rej][:, 2] <= t).all()) and bool((rec[~rej][:, 2] > t).all())
    assert tuple(model.forward_device(xd[:0], "landmark_stats", n_points=4).shape) == (0, 68, 6)
    out = torch.empty((n, 68, 6), dtype=torch.float64, device="cuda")
    assert model.forward_device(xd, "landmark_stats", n_points=4, out_tensor=out) is out
    assert torch.equal(out, model.forward_device(xd, "landmark_stats", n_points=4))
    with pytest.raises(ValueError):
        model.forward_device(xd, "landmark_stats", n_points=4, out_tensor=torch.empty((n, 68, 2), dtype=torch.float64, device="cuda"))
    model.max_batch = 2                                  # the batch slicing writes the same records
    assert torch.equal(out, model.forward_device(xd, "landmark_stats", n_points=4))


@pytest.mark.parametrize("case", ["fcn_8 5 classes", "fcn_32", "fcn_8 64x96"])
def test_forward_other_graphs(mods, weights68, case):
    from flm_amd.networks import LANDMARKS_MODELS
    from flm_amd.weights import synth_fcn8_weights, synth_fcn32_weights
    rng = np.random.default_rng(52)
    if case == "fcn_8 5 classes":
        model = LANDMARKS_MODELS["fcn_8"](5, input_height=64, input_width=64)
        model.load_weights(synth_fcn8_weights(5, seed=15))
        h, w = 64, 64
    elif case == "fcn_32":
        model = LANDMARKS_MODELS["fcn_32"](68, input_height=64, input_width=64, dtype="bf16")
        model.load_weights(synth_fcn32_weights(68, seed=2))
        h, w = 64, 64
    else:
        model = LANDMARKS_MODELS["fcn_8"](68, input_height=64, input_width=96, dtype="bf16")
        model.load_weights(weights68)
        h, w = 64, 96
    xd = torch.from_numpy(rng.integers(0, 256, (2, h, w, 3), dtype=np.uint8)).cuda()
    _forward_routes(mods, model, xd, [(4, None), (64, None), (0, None)])


# ---- weighted fit --------------------------------------------------------------------------------------------------
def _fit_inputs():
    rng = np.random.default_rng(13)
    lm = rng.uniform(0, 263, (7, 68, 2))
    lm[2, 5] = [-1, -1]
    lm[3, :] = -1            # every landmark rejected -> identity
    return rng, lm


def test_weighted_fit(mods):
    _lib, A, _, _ = mods
    rng, lm = _fit_inputs()
    tm = A.canonical_template(68, 256, 256)
    lmd, tmd = torch.from_numpy(lm).cuda(), torch.from_numpy(tm).cuda()
    ident = np.array([[1, 0, 0], [0, 1, 0]], np.float32)
    # unit weights: the unweighted kernel's arithmetic, bit for bit
    exp = warp_ref.similarity_ref(lm, tm)
    ones = torch.ones((7, 68), dtype=torch.float64, device="cuda")
    assert np.array_equal(A.similarity_device(lmd, tmd).cpu().numpy(), exp)
    assert np.array_equal(A.similarity_device(lmd, tmd, weights=ones).cpu().numpy(), exp)
    lib = _lib.load()
    m = torch.empty((7, 2, 3), dtype=torch.float32, device="cuda")
    _lib.check(lib.flm_similarity_from_landmarks_weighted(_lib.stream_ptr(), _lib.ptr(lmd), 2, None, 1, _lib.ptr(tmd), 7, 68,
                                                          1.0, 1.0, _lib.ptr(m)), "weighted, null weights")
    assert np.array_equal(m.cpu().numpy(), exp)
    # random positive weights with zeros, one negative and one NaN
    w = rng.uniform(0.01, 1.0, (7, 68))
    w[rng.random((7, 68)) < 0.15] = 0.0
    w[0, 3], w[1, 7] = -0.5, np.nan
    w[5, :] = 0.0
    w[5, 11] = 0.7           # a single positively weighted point -> identity
    wd = torch.from_numpy(w).cuda()
    rec = torch.full((7, 68, 6), 123.0, dtype=torch.float64, device="cuda")
    rec[..., :2] = lmd
    rec[..., 2] = wd
    for sc in ((1.0, 1.0), (256.0 / 264.0, 256.0 / 264.0)):
        e = stats_ref.weighted_similarity_ref(lm, tm, w, sc)
        got = A.similarity_device(lmd, tmd, sc, weights=wd).cpu().numpy()
        assert np.array_equal(got, e), sc
        # the columns of a record tensor read in place: the same bits as contiguous copies
        assert np.array_equal(A.similarity_device(rec[..., :2], tmd, sc, weights=rec[..., 2]).cpu().numpy(), got), sc
        assert np.array_equal(got[3], ident) and np.array_equal(got[5], ident)
        assert not np.array_equal(got[0], A.similarity_device(lmd, tmd, sc).cpu().numpy()[0])
    assert A._uniform_stride(rec[..., :2], 2) == 6 and A._uniform_stride(rec[..., 2], 1) == 6
    # the weights mean what they say: 10 of 68 landmarks 40 px off with weight 1e-6
    lm1, tm1, w1, m_true = stats_ref.similarity_case()
    args = (torch.from_numpy(lm1).cuda(), torch.from_numpy(tm1).cuda())
    mw = A.similarity_device(*args, weights=torch.from_numpy(w1).cuda()).cpu().numpy()[0].astype(np.float64)
    mu = A.similarity_device(*args).cpu().numpy()[0].astype(np.float64)
    err_w, err_u = np.abs(mw - m_true).max(), float(np.hypot(*(mu - m_true)[:, 2]))
    print("weighted fit off by %.3g (a, b, tx, ty), unweighted translation off by %.3g px" % (err_w, err_u))
    assert err_w < 1e-3
    assert err_u > 1.0
    # align_device passes the weights through
    crops = torch.from_numpy(rng.integers(0, 256, (7, 40, 48, 3), dtype=np.uint8)).cuda()
    al, m2 = A.align_device(crops, lmd, tmd, 32, 32, weights=wd)
    assert torch.equal(m2, A.similarity_device(lmd, tmd, weights=wd)) and torch.equal(al, A.warp_device(crops, m2, 32, 32))


# ---- end to end ----------------------------------------------------------------------------------------------------
def test_align_with_score_weights(mods, weights68):
    _lib, A, P, _ = mods
    from flm_amd.networks import LANDMARKS_MODELS
    rng = np.random.default_rng(53)
    model = LANDMARKS_MODELS["fcn_8"](68, input_height=64, input_width=64, dtype="bf16")
    model.load_weights(weights68)
    crops = torch.from_numpy(rng.integers(0, 256, (3, 64, 64, 3), dtype=np.uint8)).cuda()
    tm = torch.from_numpy(A.canonical_template(68, 64, 64)).cuda()
    sc = (64.0 / 72.0, 64.0 / 72.0)
    aligned, m, lm, score = P.align(crops, model, weights="score")
    rec = model.forward_device(crops, "landmark_stats", n_points=4)
    assert torch.equal(lm, rec[..., :2]) and torch.equal(score, rec[..., 2])
    assert torch.equal(m, A.similarity_device(rec[..., :2], tm, sc, weights=rec[..., 2]))
    assert torch.equal(aligned, A.warp_device(crops, m, 64, 64))
    # the default call is the unweighted code path, unchanged
    a0, m0, lm0 = P.align(crops, model)
    lm_plain = model.forward_device(crops, "landmarks", n_points=4)
    assert torch.equal(lm0, lm_plain) and torch.equal(lm0, lm)
    assert torch.equal(m0, A.similarity_device(lm_plain, tm, sc)) and torch.equal(a0, A.warp_device(crops, m0, 64, 64))
    # a tensor of weights; numpy in -> numpy out with the fourth value
    wt = torch.from_numpy(rng.uniform(0.1, 1.0, (3, 68))).cuda()
    a1, m1, lm1, w1 = P.align(crops, model, weights=wt)
    assert torch.equal(m1, A.similarity_device(lm_plain, tm, sc, weights=wt)) and torch.equal(w1, wt)
    res = P.align(crops.cpu().numpy(), model, weights="score")
    assert len(res) == 4 and all(isinstance(r, np.ndarray) for r in res)
    assert np.array_equal(res[1], m.cpu().numpy()) and np.array_equal(res[3], score.cpu().numpy())
    # predict(return_stats=True): three views of one record tensor
    lm_s, score_s, cov_s = P.predict(crops, model, return_stats=True)
    assert torch.equal(lm_s, rec[..., :2]) and torch.equal(score_s, rec[..., 2]) and torch.equal(cov_s, rec[..., 3:])
    assert lm_s.data_ptr() + 16 == score_s.data_ptr() and lm_s.data_ptr() + 24 == cov_s.data_ptr()
    assert torch.equal(P.predict(crops, model), lm_plain)
    lm_i, score_i, cov_i = P.predict(crops, model, to_input_space=True, return_stats=True)
    assert torch.equal(lm_i, P.predict(crops, model, to_input_space=True))       # the coordinates only
    assert torch.equal(score_i, score_s) and torch.equal(cov_i, cov_s)
    npres = P.predict(crops.cpu().numpy(), model, return_stats=True)
    assert all(np.array_equal(a, b.cpu().numpy()) for a, b in zip(npres, (lm_s, score_s, cov_s)))


def test_align_frames_with_score_weights(mods, weights68):
    _lib, A, P, _ = mods
    from flm_amd.networks import LANDMARKS_MODELS
    rng = np.random.default_rng(54)
    model = LANDMARKS_MODELS["fcn_8"](68, input_height=64, input_width=64, dtype="bf16")
    model.load_weights(weights68)
    ring = torch.from_numpy(rng.integers(0, 256, (2, 270, 480, 3), dtype=np.uint8)).cuda()
    faces = [[[30, 40, 130, 150], [300, 60, 420, 200]], [[200, 100, 290, 215]]]
    aligned, m, lm, boxes, score = P.align_frames(ring, faces, model, out_size=(56, 56), weights="score")
    crops, _, boxes_dev, idx_dev = P.crop_frames_device(ring, faces, 64, 64, frame_index=[0, 1], return_device=True)
    rec = model.forward_device(crops, "landmark_stats", n_points=4)
    tm = torch.from_numpy(A.canonical_template(68, 56, 56)).cuda()
    lmf = A.landmarks_to_frame_device(rec[..., :2].contiguous(), boxes_dev, (72, 72), (270, 480))
    assert torch.equal(boxes, boxes_dev) and torch.equal(lm, lmf) and torch.equal(score, rec[..., 2])
    assert torch.equal(m, A.similarity_device(lmf, tm, weights=rec[..., 2]))
    assert torch.equal(aligned, A.warp_frames_device(ring, m, 56, 56, frame_index_dev=idx_dev, boxes_dev=boxes_dev))
    # the default call is the unweighted code path, unchanged
    a0, m0, lm0, b0 = P.align_frames(ring, faces, model, out_size=(56, 56))
    assert torch.equal(lm0, lmf) and torch.equal(m0, A.similarity_device(lmf, tm))
    assert torch.equal(a0, A.warp_frames_device(ring, m0, 56, 56, frame_index_dev=idx_dev, boxes_dev=boxes_dev))
    assert not torch.equal(m0, m)
    e = P.align_frames(ring, [[], []], model, out_size=(56, 56), weights="score")
    assert len(e) == 5 and tuple(e[4].shape) == (0, 68)
