"""GPU: the evaluation path -- flm_decode_sweep against flm_decode and the golden vectors, flm_gaussian_heatmaps
against numpy, get_keypoints_metric against its CPU restatement, and evaluate() end to end.

Bars: a top-n slice of the sweep is BIT-equal to flm_decode(n) (same selection, same float32 hsum chain); an all-pixel
slice within 1e-9 px (float64 partial sums added in another order).  Against the reference's recorded outputs: top-n
exact where the selection is determined (its argsort breaks ties in no stated order), all-pixel 1e-4 px."""
import os

import numpy as np
import pytest
import torch

import eval_ref
from oracle import decode_ref, fcn_ref

pytestmark = pytest.mark.gpu
SWEEP = eval_ref.SWEEP


@pytest.fixture(scope="module")
def M():
    import flm_amd  # noqa: F401
    from flm_amd.utils import metrics
    from flm_amd import _lib
    _lib.load()
    return metrics


def check_sweep_vs_decode(M, hm, modes, thresh):
    got = M.decode_sweep_device(hm, modes, thresh).cpu().numpy()
    assert got.shape == (len(modes),) + tuple(hm.shape[:1]) + (hm.shape[3], 2)
    worst = 0.0
    for s, n in enumerate(modes):
        exp = M.decode_device(hm, n, thresh).cpu().numpy()
        if n >= 1:
            assert got[s].tobytes() == exp.tobytes(), (tuple(hm.shape), modes, n)
        else:
            e = float(np.nanmax(np.abs(got[s] - exp)))
            assert np.array_equal(np.isnan(got[s]), np.isnan(exp)) and e <= 1e-9, (tuple(hm.shape), e)
            worst = max(worst, e)
    return worst


def test_sweep_equals_decode_at_the_baseline_size(M):
    g = torch.Generator(device="cuda").manual_seed(21)
    hm = torch.rand((64, 264, 264, 68), device="cuda", generator=g)
    hm[0, :3, :40, 2] = 0.9375          # ties across the n-th place of several n
    hm[5, :, :, 7] = 0.0                # a rejected landmark
    e = check_sweep_vs_decode(M, hm, SWEEP, 0.0)
    e = max(e, check_sweep_vs_decode(M, hm, [25, 1, 0, 64, 9], 0.2))      # n_max <= 64: the LDS-DMA form
    print("baseline size: all-pixel max |sweep - decode| %.3g px" % e)


@pytest.mark.parametrize("shape,modes", [
    ((3, 37, 29, 5), [81, 4, 0, 4, 100]),        # h*w*l not a multiple of 4, duplicate and unordered modes, wide lists
    ((2, 40, 37, 68), [9, 0, 64, 1, 9]),          # 68 landmarks, n_max = 64
    ((2, 40, 37, 68), [65, 0, 1]),               # 68 landmarks, n_max just above 64
    ((2, 33, 17, 80), [128, 16, 0]),             # l > 68: 24 channels per wave
    ((1, 8, 9, 3), [128, 2, 72, 0]),             # a map smaller than n
    ((4, 24, 24, 68), [16, 4]),                  # no all-pixel mode
    ((2, 31, 33, 1), [0, 0]),                    # all-pixel only, one landmark
    ((3, 20, 21, 96), list(range(1, 17))),        # 16 modes, 96 landmarks
])
def test_sweep_equals_decode_odd_shapes(M, shape, modes):
    g = torch.Generator(device="cuda").manual_seed(sum(shape))
    hm = torch.rand(shape, device="cuda", generator=g)
    hm[0, :2, :5, 0] = 0.75
    for t in (0.0, 0.3):
        check_sweep_vs_decode(M, hm, modes, t)


def test_sweep_against_golden(M, golden_dir):
    gold = np.load(os.path.join(golden_dir, "eval_golden.npz"))
    modes = [int(n) for n in gold["modes"]]
    for name in ("gauss", "rand", "soft"):
        maps = gold[name]
        got = M.transfer_target_sweep(maps, modes).reshape(gold["xy_" + name].shape)
        for s, n in enumerate(modes):
            exp = gold["xy_" + name][s]
            if n >= 1:
                h, w, L = maps.shape[1:]
                gap = np.stack([decode_ref.topn_gap_rel(m.reshape(h * w, L), n) for m in maps]) if n < h * w else None
                det = np.ones(exp.shape[:2], bool) if gap is None else (gap > 0) | np.all(exp == -1, axis=-1)
                assert np.array_equal(got[s][det], exp[det]), (name, n)
                with np.errstate(all="ignore"):
                    stable = decode_ref.transfer_target_ref(maps, 0, n).reshape(exp.shape)
                assert np.array_equal(got[s], stable), (name, n)      # ties: the (value, index) rule
            else:
                assert np.abs(got[s] - exp).max() <= 1e-4, (name, n)


def _ulp_diff(a, b):
    a, b = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    a, b = np.where(a < 0, -(a & 0x7fffffff), a), np.where(b < 0, -(b & 0x7fffffff), b)
    return np.abs(a - b)


def test_gaussian_heatmaps_against_numpy(M):
    from flm_amd.data import generator
    rng = np.random.default_rng(4)
    total_ne, total = 0, 0
    for (h, w, l, sigma) in ((96, 96, 15, 3), (72, 72, 68, 3), (41, 67, 7, 2.5), (9, 5, 3, 1)):
        kp = np.concatenate([rng.uniform(-5, max(h, w) + 5, (l, 2)), np.array([[-1.0, -1.0], [3.0, 3.0]])])[:l]
        kp[0] = (w / 2.0, h / 2.0)
        kp[min(1, l - 1)] = (-1.0, -1.0)
        got = generator.generate_hm(h, w, kp, sigma)
        exp = eval_ref.generate_hm_ref(h, w, kp, sigma)
        assert got.dtype == np.float32 and got.shape == exp.shape == (h, w, l)
        d = _ulp_diff(got, exp)
        assert d.max() <= 1, ((h, w, l), int(d.max()))
        assert not got[:, :, min(1, l - 1)].any()
        total_ne += int((d != 0).sum())
        total += d.size
        if h == w:
            assert np.array_equal(exp, eval_ref.generate_hm_as_shipped(h, w, kp, sigma))
    # batch form, tensor in -> tensor out, and gaussian_k
    kpb = torch.from_numpy(rng.uniform(0, 40, (3, 5, 2))).cuda()
    hb = generator.generate_hm(40, 40, kpb)
    assert isinstance(hb, torch.Tensor) and hb.is_cuda and tuple(hb.shape) == (3, 40, 40, 5)
    for i in range(3):
        assert _ulp_diff(hb[i].cpu().numpy(), eval_ref.generate_hm_ref(40, 40, kpb[i].cpu().numpy())).max() <= 1
    gk = generator.gaussian_k(-1.0, -1.0, 3, 12, 10)
    assert gk.shape == (10, 12)
    assert _ulp_diff(gk, eval_ref.gaussian_k_ref(-1.0, -1.0, 3, 12, 10).astype(np.float32)).max() <= 1
    print("gaussian maps: %d of %d values differ from numpy (by 1 ulp at most)" % (total_ne, total))


def test_get_keypoints_metric_against_restatement(M):
    from flm_amd.data import generator
    rng = np.random.default_rng(8)
    n, h, w, l = 12, 48, 48, 68
    kp = rng.uniform(1, 46, (n, l, 2))
    kp[3, 5] = (-1, -1)
    kp[0, 7] = (20.0, 20.0)
    ytrue = generator.generate_hm(h, w, kp)
    ypred = (ytrue + rng.random(ytrue.shape, dtype=np.float32) * 0.05).astype(np.float32)
    actual = kp.reshape(n, 2 * l)
    got = M.get_keypoints_metric(ytrue, ypred, actual, nimage=10, plotting=False)
    assert got.shape == (10, 3)

    def decode(maps, n):
        """the oracle's decode for top-n (bit-equal to the device); the device's own all-pixel centroid, which agrees
        with numpy's float32 pairwise hsum only to ~1e-7 relative (test_gpu_decode.py: ALL_TOL)"""
        if n >= 1:
            with np.errstate(all="ignore"):
                return decode_ref.transfer_target_ref(maps, 0, n)
        return M.transfer_target_sweep(maps, [0])[0]
    exp = eval_ref.keypoints_metric_ref(ytrue[:10], ypred[:10], actual[:10], decode=decode)
    rel = np.abs(got / exp - 1)
    assert rel.max() <= 1e-12, rel.max()
    oracle_all = eval_ref.keypoints_metric_ref(ytrue[:10], ypred[:10], actual[:10], modes=[0])
    assert np.abs(got[-1] / oracle_all[0] - 1).max() <= 1e-5
    got2 = M.get_keypoints_metric(torch.from_numpy(ytrue).cuda(), torch.from_numpy(ypred).cuda(), actual,
                                  plotting=False, n_points_list=[4, 0, 100])
    exp2 = eval_ref.keypoints_metric_ref(ytrue, ypred, actual, modes=[4, 0, 100], decode=decode)
    assert np.abs(got2 / exp2 - 1).max() <= 1e-12
    import matplotlib
    matplotlib.use("Agg")
    M.get_keypoints_metric(ytrue, ypred, actual, nimage=4, plotting=True)


# ---- evaluate() end to end ---------------------------------------------------------------------------------------------
def _dataset(tmp_path, l):
    from PIL import Image
    rng = np.random.default_rng(12)
    sizes = [(64, 64), (80, 96), (50, 40), (64, 64), (120, 100), (33, 47), (64, 64), (90, 90), (72, 56)]
    images, kps = [], []
    for i, (h, w) in enumerate(sizes):
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        kp = np.stack([rng.uniform(0, w - 1, l), rng.uniform(0, h - 1, l)], axis=1)
        kp[i % l] = (-1, -1)
        Image.fromarray(np.ascontiguousarray(img[:, :, ::-1])).save(str(tmp_path / ("face%d.png" % i)))
        with open(str(tmp_path / ("face%d.pts" % i)), "w") as fp:
            fp.write("version: 1\n")
            fp.write("n_points: %d\n" % l)
            fp.write("{\n")
            for x, y in kp:
                fp.write(("-1 -1" if (x, y) == (-1, -1) else "%r %r" % (float(x), float(y))) + "\n")
            fp.write("}")
        images.append(img)
        kps.append(kp)
    return images, np.stack(kps)


def _composed(model, images, kps, M):
    """evaluate() from the package's public pieces: resize, forward, generate_hm, get_keypoints_metric."""
    from flm_amd.data import generator
    x = torch.stack([generator.resize_u8_device(torch.from_numpy(im).cuda(), model.input_height, model.input_width)
                     for im in images])
    probs = model.forward_device(x.contiguous(), "probs").view(len(images), model.output_height, model.output_width, -1)
    grid = []
    for im, kp in zip(images, kps):
        s = np.array([model.output_width / im.shape[1], model.output_height / im.shape[0]])
        grid.append(np.where(np.all(kp == -1, axis=1, keepdims=True), -1.0, kp * s))
    grid = np.stack(grid)
    true = generator.generate_hm(model.output_height, model.output_width, torch.from_numpy(grid).cuda())
    tab = M.get_keypoints_metric(true, probs.contiguous(), grid.reshape(len(images), -1), plotting=False)
    return tab, x, probs, grid


def test_evaluate_end_to_end(M, tmp_path):
    from flm_amd import evaluation
    from flm_amd.networks import LANDMARKS_MODELS
    from flm_amd.weights import synth_fcn8_weights
    l = 68
    images, kps = _dataset(tmp_path, l)
    params = synth_fcn8_weights(l, seed=2)
    tabs = {}
    for dt in ("f32", "bf16"):
        model = LANDMARKS_MODELS["fcn_8"](l, input_height=64, input_width=64, dtype=dt)
        model.load_weights(params)
        res = evaluation.evaluate(model, str(tmp_path), str(tmp_path))
        assert res.n_images == 9 and res.modes == tuple(SWEEP) and res.rmse.shape == (10, 3)
        assert res.best_n_points == SWEEP[int(np.argmin(res.rmse[:, 1]))]
        assert (res.n_counted > 0).all() and (res.n_counted <= 9 * 2 * (l - 1)).all()
        comp, x, probs, grid = _composed(model, images, kps, M)
        assert np.array_equal(res.rmse, comp), dt                    # one batch: the same sums in the same order
        arr = evaluation.evaluate(model, images=images, keypoints=kps, batch_size=4)
        # three batches: the forward's kernels are chosen per batch size (its probabilities differ in the last bits)
        # and the sums are taken in another order; the true-map column depends on neither
        assert np.abs(arr.rmse / res.rmse - 1).max() <= 1e-6
        assert np.abs(arr.rmse[:, 2] / res.rmse[:, 2] - 1).max() <= 1e-12
        assert np.array_equal(arr.n_counted, res.n_counted)
        tabs[dt] = res.rmse
        if dt == "f32":
            # the decoded points against those of the CPU oracle's probabilities, on the determined (face, class) pairs
            xr = np.stack([fcn_ref.get_image_array_ref(im) for im in x.cpu().numpy()])
            p64 = fcn_ref.fcn8_predict_ref(xr, params, torch.float64)
            oh, ow = model.output_height, model.output_width
            got = M.transfer_target_sweep(probs.contiguous(), SWEEP).cpu().numpy().reshape(10, 9, l, 2)
            worst, undet = 0.0, 0
            for s, n in enumerate(SWEEP):
                for i in range(9):
                    with np.errstate(all="ignore"):
                        ref = decode_ref.transfer_target_ref(p64[i].astype(np.float32).reshape(1, oh, ow, l), 0,
                                                             n).reshape(l, 2)
                    det = decode_ref.topn_gap_rel(p64[i], n) > 2e-5 if n >= 1 else np.ones(l, bool)
                    worst = max(worst, float(np.abs(got[s, i] - ref).max(-1)[det].max()))
                    undet += int((~det).sum())
            print("fp32 evaluate: decoded points vs oracle max %.3g px over determined pairs (%d undetermined of %d)"
                  % (worst, undet, 10 * 9 * l))
            assert worst <= 1e-4 and undet <= 0.1 * 10 * 9 * l
    rel = float(np.abs(tabs["bf16"] / tabs["f32"] - 1).max())
    print("bf16 vs fp32 RMSE table: max relative difference %.4g" % rel)
    assert rel <= 0.0035    # observed 0.0016; the bar is about twice it


def test_evaluate_rejects_wrong_keypoint_count(M, tmp_path):
    from flm_amd import evaluation
    from flm_amd.networks import LANDMARKS_MODELS
    from flm_amd.weights import synth_fcn8_weights
    model = LANDMARKS_MODELS["fcn_8"](68, input_height=64, input_width=64)
    model.load_weights(synth_fcn8_weights(68, seed=2))
    img = np.zeros((64, 64, 3), np.uint8)
    with pytest.raises(ValueError, match="Keypoint"):
        evaluation.evaluate(model, images=[img], keypoints=np.zeros((1, 67, 2)))
