"""Pin oracle/decode_ref.py against the reference's own utils/metrics.py.

Golden fixtures: tests/golden/decode_golden.npz, produced by
tests/golden/make_decode_golden.py which RUNS the reference implementation
(utils/metrics.py:46-109) in the build container, and
tests/golden/decode_sweep_golden.npz, produced the same way by
tests/golden/make_decode_sweep_golden.py.
"""
import os

import numpy as np
import pytest

from oracle import decode_ref


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "decode_golden.npz"))


def test_get_average_xy_matches_golden(gold):
    modes = gold["modes"]
    ths = gold["thresholds"]
    for name in gold["names"]:
        hm = gold["hm_" + str(name)]
        exp = gold["xy_" + str(name)]
        for i, n in enumerate(modes):
            for j, t in enumerate(ths):
                with np.errstate(all="ignore"):
                    got = decode_ref.get_average_xy_ref(hm, int(n), float(t) if t else 0)
                got = np.array([float(got[0]), float(got[1])])
                # same numpy ops in the same order -> bit-identical
                assert np.array_equal(got, exp[i, j]), (name, n, t, got, exp[i, j])


def test_transfer_target_as_shipped(gold):
    y = gold["tt_input"]
    with np.errstate(all="ignore"):
        a = decode_ref.transfer_target_ref(y, as_shipped=True)
        b = decode_ref.transfer_target_ref(y, 0.2, 25, as_shipped=True)
    assert np.array_equal(a, gold["tt_shipped_default"])
    # the positional slip makes the arguments irrelevant (utils/metrics.py:98)
    assert np.array_equal(b, gold["tt_shipped_args"])
    assert np.array_equal(gold["tt_shipped_default"], gold["tt_shipped_args"])
    # the all-zero landmark map is rejected as (-1,-1)
    assert a[1, 4] == -1 and a[1, 5] == -1
    # and the fixed-argument form equals as-shipped when asked for n=4, thresh=0
    with np.errstate(all="ignore"):
        c = decode_ref.transfer_target_ref(y, 0, 4)
    assert np.array_equal(a, c)


def test_live_reference_property(golden_dir):
    """Seeded sweep against what the reference's own get_average_xy returned for it (recorded in
    decode_sweep_golden.npz): 40 random heatmaps, float32 and float64, top-n 0..16, thresholds 0 / 0.3 / 0.6."""
    gold = np.load(os.path.join(golden_dir, "decode_sweep_golden.npz"))
    params, expected = gold["params"], gold["expected"]
    assert len(params) == len(expected) == 40
    for k in range(len(params)):
        hm = gold["hm_%02d" % k]
        h, w = hm.shape
        n, t = int(params[k, 0]), float(params[k, 1])
        with np.errstate(all="ignore"):
            got = decode_ref.get_average_xy_ref(hm, n, t)
        assert float(expected[k, 0]) == float(got[0]) and float(expected[k, 1]) == float(got[1]), (k, h, w, n, t)


def test_a_given_stable_order_changes_nothing(gold):
    """`order` / `orders` (the caller's stable argsort, so that one sort serves every n_points of a large map) against the
    default path: the golden maps, and random maps with a plateau of tied maxima, a zero map and rejections."""
    for name in gold["names"]:
        hm = gold["hm_" + str(name)]
        order = hm.argsort(axis=None, kind="stable")
        for n in (1, 4, 25):
            with np.errstate(all="ignore"):
                a, b = decode_ref.get_average_xy_ref(hm, n, 0, order), decode_ref.get_average_xy_ref(hm, n, 0)
            assert np.array_equal(np.array(a, np.float64), np.array(b, np.float64), equal_nan=True), (name, n)
    rng = np.random.default_rng(33)
    y = rng.random((2, 19, 23, 4), dtype=np.float32)
    y[0, 3:5, 2:12, 1] = 1.5
    y[1, :, :, 2] = 0
    y[..., 3] *= np.float32(0.125)
    orders = [[np.ascontiguousarray(y[f, :, :, c]).argsort(axis=None, kind="stable") for c in range(4)] for f in range(2)]
    for n in (1, 4, 25, 128, 0):
        for t in (0, 0.2):
            with np.errstate(all="ignore"):
                a, b = decode_ref.transfer_target_ref(y, t, n, orders=orders), decode_ref.transfer_target_ref(y, t, n)
            assert a.shape == (2, 8) and np.array_equal(a, b), (n, t)
    assert (b == -1).any() and (b != -1).any()


def test_topn_gap_rel_is_the_relative_gap_at_the_nth_place():
    """decode_ref.topn_gap_rel (the checker's "determined pair" criterion, used by bench.py and the config tests): against a
    full sort, with ties and with n + 1 = the whole map."""
    rng = np.random.default_rng(21)
    m = rng.random((500, 7)).astype(np.float64)
    m[10, 3] = m[20, 3] = m[:, 3].max() + 1.0            # a tie at the top
    for n in (1, 4, 25, 499):
        srt = np.sort(m, axis=0)[::-1]
        exp = (srt[n - 1] - srt[n]) / srt[n - 1]
        np.testing.assert_array_equal(decode_ref.topn_gap_rel(m, n), exp)
    assert decode_ref.topn_gap_rel(m, 1)[3] == 0.0        # the tie: gap zero -> undetermined for n = 1
