"""GPU parity of flm_flow_pyramid and flm_landmark_flow against tests/flow_ref.py, bit for bit: the pyramids byte for
byte, every landmark as its uint64 bits, every weight, err and flag -- over the cases of tests/flow_cases.py (K 1, 3, 9;
C 5, 68; 64x64 with three levels, 32x48 with two, 9x7 with one; luma and BGR crops; radius 7, 3 and 2; points on integer
positions, with fraction 31/32, within the radius of every border and in the corners; rejected inputs; a zero crop; a
crop that is flat at the coarse levels only; one iteration; matrices with a rotation; weights given and not).  Then the
accuracy of the reference's own properties on the device, the numpy convenience, and refused arguments."""
import numpy as np
import pytest
import torch

import flow_cases
import flow_ref

pytestmark = pytest.mark.gpu
SENT = 0x5a


@pytest.fixture(scope="module")
def mods():
    import flm_amd  # noqa: F401
    from flm_amd import _lib, alignment, prediction
    _lib.load()
    return _lib, alignment, prediction


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a).view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def run_case(alignment, c, with_w=True):
    o = c["opts"]
    flow = alignment.LandmarkFlow(**o)
    k = c["lm"].shape[0]
    both = dev(np.concatenate([c["prev"], c["cur"]]))
    pyr = alignment.flow_pyramid_device(both, o["levels"])
    w = dev(c["w"]) if (with_w and c["w"] is not None) else None
    lm, wt, err, flags = alignment.landmark_flow_device(pyr[:k], pyr[k:], dev(c["lm"]), dev(c["m"]), c["hw"], flow, weights=w)
    return pyr[:k], pyr[k:], lm, wt, err, flags


@pytest.mark.parametrize("i", range(len(flow_cases.cases())), ids=[c["name"] for c in flow_cases.cases()])
def test_device_equals_the_reference_bit_for_bit(mods, i):
    _, alignment, _ = mods
    c = flow_cases.cases()[i]
    got = run_case(alignment, c)
    exp = flow_cases.expected(i)
    for name, g, e in zip(("pyr_prev", "pyr_cur", "lm", "w", "err", "flags"), got, exp):
        g = g.cpu().numpy()
        assert g.dtype == e.dtype and g.shape == e.shape, (c["name"], name, g.dtype, g.shape, e.shape)
        bad = np.argwhere(bits(g) != bits(e))
        assert bad.size == 0, (c["name"], name, len(bad), bad[:4], g[tuple(bad[0][:2])], e[tuple(bad[0][:2])])
    flags = exp[5]
    print(c["name"], "accepted", int((flags == 0).sum()), "of", flags.size, "flags seen", sorted(set(flags.ravel().tolist())))


def test_cases_reach_every_path():
    """The cases together accept points and raise every flag but NOT_FINITE (which test_gates_on_the_device raises)."""
    seen, accepted = set(), 0
    for i in range(len(flow_cases.cases())):
        flags = flow_cases.expected(i)[5]
        accepted += int((flags == 0).sum())
        for bit in (1, 2, 4, 8, 16, 32):
            if (flags & bit).any():
                seen.add(bit)
    assert accepted > 500 and {1, 2, 4, 8, 16} <= seen, (accepted, seen)


def test_without_weights_and_into_given_buffers(mods):
    _, alignment, _ = mods
    i = 1
    c = flow_cases.cases()[i]
    assert c["w"] is not None
    _, _, lm, wt, err, flags = run_case(alignment, c, with_w=False)
    exp = flow_cases.expected(i)
    assert np.array_equal(bits(lm), bits(exp[2])) and np.array_equal(flags.cpu().numpy(), exp[5])
    assert np.array_equal(wt.cpu().numpy(), (exp[5] == 0).astype(np.float64))          # 1.0 for a tracked point, else 0
    # given buffers are written in place and nothing beside them
    k, n = c["lm"].shape[:2]
    flow = alignment.LandmarkFlow(**c["opts"])
    pyr = alignment.flow_pyramid_device(dev(np.concatenate([c["prev"], c["cur"]])), flow.levels)
    pad = torch.full((k * n * 2 + 16,), float(SENT), dtype=torch.float64, device="cuda")
    out = (pad[8:8 + k * n * 2].view(k, n, 2), None, None, torch.empty((k, n), dtype=torch.int32, device="cuda"))
    res = alignment.landmark_flow_device(pyr[:k], pyr[k:], dev(c["lm"]), dev(c["m"]), c["hw"], flow, weights=dev(c["w"]), out=out)
    assert res[0] is out[0] and res[3] is out[3]
    assert (pad[:8] == SENT).all() and (pad[-8:] == SENT).all()
    assert np.array_equal(bits(res[0]), bits(exp[2])) and np.array_equal(bits(res[1]), bits(exp[3]))


@pytest.mark.parametrize("shift", [(0.0, 0.0), (1.25, -0.75), (3.3, -2.6)])
def test_accuracy_on_the_device(mods, shift):
    """The properties tests/test_flow_host.py proves of the reference, here of the device, through the numpy convenience."""
    _, alignment, prediction = mods
    tex = flow_ref.texture(64, 64, 11)
    a, b = flow_ref.shifted(tex, 0.0, 0.0), flow_ref.shifted(tex, *shift)
    pts = np.random.default_rng(2).uniform(10.0, 53.0, (1, 68, 2))
    lm, err, flags = prediction.landmark_flow(a[None], b[None], pts, flow=alignment.LandmarkFlow(levels=3))
    assert (flags == 0).all()
    d = np.abs(lm - (pts + np.asarray(shift))).max()
    print("shift", shift, "worst", d)
    if shift == (0.0, 0.0):
        assert (err == 0).all() and np.array_equal(bits(lm), bits((pts + 0.5) - 0.5))
    else:
        assert d <= 0.1


def test_gates_on_the_device(mods):
    _, alignment, prediction = mods
    tex = flow_ref.texture(64, 64, 11)
    a, b = flow_ref.shifted(tex, 0.0, 0.0), flow_ref.shifted(tex, 3.3, -2.6)
    pts = np.random.default_rng(3).uniform(10.0, 53.0, (1, 68, 2))
    flat = np.full((1, 64, 64), 90, np.uint8)
    flow = alignment.LandmarkFlow(levels=3)
    lm, _, flags = prediction.landmark_flow(flat, flat, pts, flow=flow)
    assert (flags & flow_ref.LOW_TEXTURE).all() and (lm == -1.0).all()
    bad = np.array([[[-1.0, -1.0], [np.nan, 4.0], [5.0, np.inf]]])
    lm, err, flags = prediction.landmark_flow(a[None], b[None], bad, flow=flow)
    assert (flags == flow_ref.NO_HISTORY).all() and (err == -1).all() and (lm == -1.0).all()
    _, _, flags = prediction.landmark_flow(a[None], b[None], pts, flow=alignment.LandmarkFlow(levels=3, max_move=1.0))
    assert (flags == flow_ref.MOVED).all()
    _, _, flags = prediction.landmark_flow(a[None], b[None], np.array([[[62.0, 32.0], [30.0, 1.0]]]), flow=flow)
    assert (flags & flow_ref.OUTSIDE).all()
    # a matrix that throws the point out of reach: NOT_FINITE, before any sample is taken
    pyr = alignment.flow_pyramid_device(dev(np.stack([a, b])), 3)
    m = dev(np.array([[[1, 0, 3.0e6], [0, 1, 0]]], np.float32))
    lm, wt, err, flags = alignment.landmark_flow_device(pyr[:1], pyr[1:], dev(np.array([[[5.0, 5.0]]])), m, (64, 64), flow)
    assert flags.item() == flow_ref.NOT_FINITE and err.item() == -1 and wt.item() == 0.0 and (lm == -1.0).all()


def test_refused_arguments(mods):
    _lib, alignment, _ = mods
    flow = alignment.LandmarkFlow(levels=3)
    crops = torch.zeros((2, 64, 64, 3), dtype=torch.uint8, device="cuda")
    pyr = alignment.flow_pyramid_device(crops, 3)
    assert tuple(pyr.shape) == (2, 64 * 64 + 32 * 32 + 16 * 16) and not pyr.any()
    lm = torch.zeros((1, 5, 2), dtype=torch.float64, device="cuda")
    m = torch.zeros((1, 2, 3), dtype=torch.float32, device="cuda")
    with pytest.raises(ValueError, match="pyr_cur"):
        alignment.landmark_flow_device(pyr[:1], pyr[:1, :-1], lm, m, (64, 64), flow)
    with pytest.raises(ValueError, match="weights"):
        alignment.landmark_flow_device(pyr[:1], pyr[1:], lm, m, (64, 64), flow, weights=lm[..., 0].float())
    with pytest.raises(ValueError, match="must be"):
        alignment.landmark_flow_device(pyr[:1], pyr[1:], lm, m[:, :1], (64, 64), flow)
    with pytest.raises(ValueError, match="overlap"):
        alignment.landmark_flow_device(pyr[:1], pyr[1:], lm, m, (64, 64), flow, out=(lm, None, None, None))
    with pytest.raises(ValueError, match="out must be"):
        alignment.flow_pyramid_device(crops, 3, out=pyr[:, :-1])
