"""Generate tests/golden/decode_sweep_golden.npz by RUNNING the reference's own `get_average_xy`.

Run where a checkout of the reference exists (it never travels with this repository):
    MPLBACKEND=Agg python tests/golden/make_decode_sweep_golden.py <reference checkout>

The seeded sweep of tests/test_oracle_decode.py::test_live_reference_property: 40 random heatmaps (4..69 rows and
columns, every fifth one float64), top-n in {0, 1, 2, 4, 7, 16} and threshold in {0, 0.3, 0.6}, each with what
utils/metrics.py:46-80 returns for it.  The fixture holds inputs and expected outputs only -- data, no reference source.
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

rng = np.random.default_rng(7)
out = {}
params = np.zeros((40, 2), np.float64)    # (n, thresh) per case
expected = np.zeros((40, 2), np.float64)  # (x, y) per case
for k in range(40):
    h, w = int(rng.integers(4, 70)), int(rng.integers(4, 70))
    hm = rng.random((h, w), dtype=np.float32)
    if k % 5 == 0:
        hm = hm.astype(np.float64)
    n = int(rng.choice([0, 1, 2, 4, 7, 16]))
    n = min(n, h * w)
    t = float(rng.choice([0.0, 0.3, 0.6]))
    with np.errstate(all="ignore"):
        xy = ref.get_average_xy(hm, h, w, n, t)
    out["hm_%02d" % k] = hm
    params[k] = n, t
    expected[k] = float(xy[0]), float(xy[1])
out.update(params=params, expected=expected)
dst = os.path.join(os.path.dirname(os.path.abspath(__file__)), "decode_sweep_golden.npz")
np.savez_compressed(dst, **out)
print("wrote", dst, os.path.getsize(dst), "bytes")
