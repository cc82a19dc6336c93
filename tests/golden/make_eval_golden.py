"""Generate tests/golden/eval_golden.npz by RUNNING the reference's own `get_average_xy` and `get_RMSE`.

Run where a checkout of the reference exists (it never travels with this repository):
    MPLBACKEND=Agg python tests/golden/make_eval_golden.py <reference checkout>

Inputs (tests/eval_ref.py: golden_inputs): Gaussian target maps of the restated generate_hm (centres at non-integer,
half-integer and integer positions, one near a border, one missing), random maps and softmax-like maps, 3 faces of
24x24x6.  Recorded: utils/metrics.py:46-80 at every n of the sweep (n = k*k, k = 1..9, then 0) for each map set, as
[S, N, L, 2]; and the [S, 3] RMSE tables of get_keypoints_metric (:118-142, composed with `list(range(1, 10)) + [0]`
and the documented n, not the argument slip at :98) for the random and for the softmax-like maps as predictions
against the Gaussian maps, with the keypoints as the true (x,y).  The fixture holds inputs and outputs only.
"""
import importlib.util
import os
import sys

import numpy as np

if len(sys.argv) != 2:
    raise SystemExit(__doc__)
REF = os.path.join(sys.argv[1], "keypoints_detector", "utils", "metrics.py")
spec = importlib.util.spec_from_file_location("ref_metrics", REF)
ref = importlib.util.module_from_spec(spec)
spec.loader.exec_module(ref)
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))
import eval_ref  # noqa: E402

kp, gauss, rand, soft = eval_ref.golden_inputs()
modes = np.array(eval_ref.SWEEP, np.int64)


def decode(maps, n):
    """transfer_target(maps, 0, n) as documented: get_average_xy per channel with n and thresh 0."""
    N, h, w, L = maps.shape
    out = np.zeros((N, 2 * L))
    for i in range(N):
        for c in range(L):
            with np.errstate(all="ignore"):
                xy = ref.get_average_xy(maps[i, :, :, c], h, w, int(n), 0)
            out[i, 2 * c:2 * c + 2] = float(xy[0]), float(xy[1])
    return out


out = dict(kp=kp, gauss=gauss, rand=rand, soft=soft, modes=modes)
for name, maps in (("gauss", gauss), ("rand", rand), ("soft", soft)):
    out["xy_" + name] = np.stack([decode(maps, n).reshape(maps.shape[0], maps.shape[3], 2) for n in modes])
actual = kp.reshape(kp.shape[0], -1)
for name, maps in (("rand", rand), ("soft", soft)):
    res = []
    for nw in list(range(1, 10)) + [0]:
        n_points = nw * nw
        y_pred_xy, y_train_xy = decode(maps, n_points), decode(gauss, n_points)
        pick = y_train_xy != -1
        res.append([ref.get_RMSE(y_pred_xy, y_train_xy, pick), ref.get_RMSE(y_pred_xy, actual, pick),
                    ref.get_RMSE(y_train_xy, actual, pick)])
    out["rmse_" + name] = np.array(res)
dst = os.path.join(HERE, "eval_golden.npz")
np.savez_compressed(dst, **out)
print("wrote", dst, os.path.getsize(dst), "bytes")
