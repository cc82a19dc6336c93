"""CPU restatements for the evaluation tests (TEST INFRASTRUCTURE ONLY): the reference's Gaussian target maps
(data/generator.py:274-296) and its n_points experiment (utils/metrics.py:112-154) composed as its docstring says,
on oracle/decode_ref.py's decode.  Pinned by tests/golden/eval_golden.npz (tests/golden/make_eval_golden.py)."""
import numpy as np

SWEEP = [nw * nw for nw in list(range(1, 10)) + [0]]   # :129-131 with Python 3's list(range(...))


def gaussian_k_ref(x0, y0, sigma, width, height):
    """data/generator.py:274-279 (float64 [height, width])."""
    x = np.arange(0, width, 1, float)
    y = np.arange(0, height, 1, float)[:, np.newaxis]
    return np.exp(-((x - x0) ** 2 + (y - y0) ** 2) / (2 * sigma ** 2))


def generate_hm_ref(height, width, keypoints, s=3):
    """data/generator.py:282-296 with x along the width.  The reference calls gaussian_k(x0, y0, s, height, width)
    -- (height, width) in the (width, height) slots, :293 -- which equals this on square maps only."""
    hm = np.zeros((height, width, len(keypoints)), dtype=np.float32)
    for i in range(len(keypoints)):
        if not np.array_equal(keypoints[i], [-1, -1]):
            hm[:, :, i] = gaussian_k_ref(keypoints[i][0], keypoints[i][1], s, width, height)
    return hm


def generate_hm_as_shipped(height, width, keypoints, s=3):
    """The reference's own call order (:293), for the square-map check."""
    hm = np.zeros((height, width, len(keypoints)), dtype=np.float32)
    for i in range(len(keypoints)):
        if not np.array_equal(keypoints[i], [-1, -1]):
            hm[:, :, i] = gaussian_k_ref(keypoints[i][0], keypoints[i][1], s, height, width)
    return hm


def get_rmse_ref(y_pred_xy, y_train_xy, pick_not_NA):
    """utils/metrics.py:112-115."""
    res = y_pred_xy[pick_not_NA] - y_train_xy[pick_not_NA]
    return np.sqrt(np.mean(res ** 2))


def keypoints_metric_ref(ytrain_dist, ypred_dist, ytrain_actual, modes=None, decode=None):
    """utils/metrics.py:118-142 as documented: [S,3] table.  `decode(maps, n)` -> [N, 2L]; default: the oracle's
    transfer_target_ref with thresh 0."""
    from oracle import decode_ref
    if decode is None:
        def decode(maps, n):
            with np.errstate(all="ignore"):
                return decode_ref.transfer_target_ref(maps, 0, n)
    res = []
    for n in (SWEEP if modes is None else modes):
        y_pred_xy = decode(ypred_dist, n)
        y_train_xy = decode(ytrain_dist, n)
        pick = y_train_xy != -1
        res.append([get_rmse_ref(y_pred_xy, y_train_xy, pick), get_rmse_ref(y_pred_xy, ytrain_actual, pick),
                    get_rmse_ref(y_train_xy, ytrain_actual, pick)])
    return np.array(res)


def golden_inputs():
    """The seeded inputs of eval_golden.npz: keypoints [3, 6, 2] on 24x24 grids (non-integer, half-integer and
    integer centres, one near a border, one missing), their Gaussian maps, random maps and softmax-like maps."""
    rng = np.random.default_rng(11)
    n, h, w, l = 3, 24, 24, 6
    kp = rng.uniform(2.0, 21.0, (n, l, 2))
    kp[0, 0] = (7.3, 11.8)       # non-integer
    kp[0, 1] = (10.5, 4.5)       # half-integer: ties in pairs
    kp[0, 2] = (12.0, 12.0)      # integer: rings of equal values
    kp[1, 3] = (0.4, 23.2)       # near a border
    kp[2, 4] = (-1.0, -1.0)      # missing
    kp[1, 5] = (6.0, 17.5)
    gauss = np.stack([generate_hm_ref(h, w, kp[i]) for i in range(n)])
    rand = rng.random((n, h, w, l), dtype=np.float32)
    logits = rng.standard_normal((n, h, w, l + 1)) * 3.0
    e = np.exp(logits - logits.max(axis=-1, keepdims=True))
    soft = (e / e.sum(axis=-1, keepdims=True))[..., :l].astype(np.float32)
    return kp, gauss, rand, soft
