"""GPU parity of flm_landmark_flow_rows, flm_track_gather_flow and flm_track_flow_history_put against
tests/flow_rows_ref.py, bit for bit, over the cases of tests/flow_rows_cases.py (1 to 9 rows over 4 to 12 slots; C 5 and
68; 64x64 with three levels, 32x48 with two; a permuted slot map, inert rows, rejected history points, weights given and
NULL, radius 3 and 7, the check on and off, the occluded quadrant only the backward pass judges).  Then the pinned
equality that ties the rows kernel to flm_landmark_flow on the existing tests/flow_cases.py; the check on against off on
a pure shift; and the gather and the put with "a slot no row names keeps every bit" and "an off stream is not touched"."""
import numpy as np
import pytest
import torch

import flow_cases
import flow_rows_cases as rc
import flow_rows_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mods():
    import flm_amd  # noqa: F401
    from flm_amd import _lib, alignment, prediction
    _lib.load()
    return _lib, alignment, prediction


def dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a).view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def flow_of(alignment, c, max_fb):
    return alignment.LandmarkFlow(max_fb=max_fb if max_fb else None, **c["opts"])


def run_rows(alignment, c, max_fb, slot=None, lm=None, w="case"):
    n = len(c["prev"])
    pyr = alignment.flow_pyramid_device(dev(np.concatenate([c["prev"], c["cur"]])), c["opts"]["levels"])
    slot = np.arange(n, dtype=np.int32) if slot is None else slot
    return alignment.landmark_flow_rows_device(pyr[:n], pyr[n:], dev(slot), dev(c["lm"] if lm is None else lm), dev(c["m"]),
                                               c["hw"], flow_of(alignment, c, max_fb), weights=dev(c["w"] if w == "case" else w))


@pytest.mark.parametrize("i", range(len(rc.cases())), ids=[c["name"] for c in rc.cases()])
def test_rows_flow_equals_the_reference_bit_for_bit(mods, i):
    _, alignment, _ = mods
    c = rc.cases()[i]
    got = run_rows(alignment, c, c["max_fb"], slot=c["slot"])
    for name, g, e in zip(("lm", "w", "err", "fb", "flags"), got, rc.expected(i)):
        g = g.cpu().numpy()
        assert g.dtype == e.dtype and g.shape == e.shape, (c["name"], name, g.dtype, g.shape, e.shape)
        bad = np.argwhere(bits(g) != bits(e))
        assert bad.size == 0, (c["name"], name, len(bad), bad[:4], g[tuple(bad[0][:2])], e[tuple(bad[0][:2])])
    flags = rc.expected(i)[4]
    print(c["name"], "accepted", int((flags == 0).sum()), "of", flags.size, "flags seen", sorted(set(flags.ravel().tolist())))


def test_cases_reach_the_backward_pass_and_the_occlusion_condition_holds():
    seen, fb_ran = set(), 0
    for i in range(len(rc.cases())):
        _, _, _, fb, flags = rc.expected(i)
        seen |= set(flags.ravel().tolist())
        fb_ran += int((fb >= 0).sum())
    assert fb_ran > 500 and {0, 1, 2, 8, 64} <= seen, (fb_ran, seen)
    only_fb, passed = rc.occlusion_holds()
    assert only_fb >= 5 and passed >= 5, (only_fb, passed)


@pytest.mark.parametrize("i", range(len(flow_cases.cases())), ids=[c["name"] for c in flow_cases.cases()])
def test_identity_rows_with_the_check_off_equal_landmark_flow(mods, i):
    """The equality contract: slot[r] = r, n = n_slots, max_fb = 0 -> the bits of flm_landmark_flow, on ITS cases.  One
    kernel serves both calls, so this compares its launch without a slot with its launch on slot[r] = r."""
    _, alignment, _ = mods
    c = flow_cases.cases()[i]
    k = c["lm"].shape[0]
    pyr = alignment.flow_pyramid_device(dev(np.concatenate([c["prev"], c["cur"]])), c["opts"]["levels"])
    flow = alignment.LandmarkFlow(**c["opts"])
    args = (dev(c["lm"]), dev(c["m"]), c["hw"], flow)
    old = alignment.landmark_flow_device(pyr[:k], pyr[k:], *args, weights=dev(c["w"]))
    new = alignment.landmark_flow_rows_device(pyr[:k], pyr[k:], torch.arange(k, dtype=torch.int32, device="cuda"), *args,
                                              weights=dev(c["w"]))
    for name, a, b in zip(("lm", "w", "err", "flags"), old, (new[0], new[1], new[2], new[4])):
        assert a.dtype == b.dtype and np.array_equal(bits(a), bits(b)), (c["name"], name)
    assert (new[3] == -1.0).all()
    exp = flow_cases.expected(i)                              # and so the bits of the reference of that call
    assert np.array_equal(bits(new[0]), bits(exp[2])) and np.array_equal(new[4].cpu().numpy(), exp[5])


def test_the_check_changes_nothing_but_its_own_flag_on_a_pure_shift(mods):
    _, alignment, _ = mods
    c = rc.cases()[1]                                         # three BGR rows, a shift of (1.25, -0.75), one zero crop
    off, on = run_rows(alignment, c, 0.0, slot=c["slot"]), run_rows(alignment, c, 1.0, slot=c["slot"])
    f0, f1 = off[4].cpu().numpy(), on[4].cpu().numpy()
    assert np.array_equal(f0, f1 & ~flow_rows_ref.FB)        # the flags other than FB
    keep = (f1 & flow_rows_ref.FB) == 0
    assert np.array_equal(bits(off[0])[keep], bits(on[0])[keep]) and np.array_equal(bits(off[1])[keep], bits(on[1])[keep])
    assert (on[0].cpu().numpy()[~keep] == -1.0).all() and (on[1].cpu().numpy()[~keep] == 0.0).all()
    assert np.array_equal(off[2].cpu().numpy(), on[2].cpu().numpy())          # err is the forward pass's
    assert (off[3] == -1.0).all() and ((on[3] >= 0).cpu().numpy() == (f0 == 0)).all()
    ok = (f1 == 0)
    print("accepted without", int((f0 == 0).sum()), "with", int(ok.sum()), "largest fb", float(np.sqrt(on[3].cpu().numpy()[ok].max())))
    assert ok.sum() >= 0.9 * (f0 == 0).sum()                  # a pure shift comes back to where it started


def gather_on_device(alignment, a, pad=3):
    """The call on copies of the case on the device.  Returns every tensor it may write, by the reference's names."""
    d = {k: dev(a[k]) for k in ("stream_on", "frame_idx_stream", "dt_stream", "best_q", "reset", "age", "cursor", "m_crop",
                                "boxes", "flow_frame", "flow_ready")}
    dt = None if d["age"] is None else (d["dt_stream"] if d["dt_stream"] is not None else a["dt"])
    out = alignment.track_gather_flow_device(d["m_crop"], d["boxes"], d["flow_frame"], d["flow_ready"], a["k"],
                                             (a["fh"], a["fw"]), a["n"], stream_on=d["stream_on"],
                                             frame_index=d["frame_idx_stream"], dt=dt, best_q=d["best_q"], reset=d["reset"],
                                             age=d["age"], cursor=d["cursor"])
    names = dict(slot="slot_c", m="m_c", boxes="boxes_c", frame_index="frame_idx_c", prev_frame_index="prev_frame_idx_c",
                 dt="dt_c", best_q="best_q_c", reset="reset_c", counts="counts")
    got = {names[k]: v for k, v in out.items()}
    got.update({k: d[k] for k in ("reset", "age", "cursor", "flow_ready") if d[k] is not None})
    return got, d


@pytest.mark.parametrize("i", range(len(rc.gather_cases())), ids=[c["name"] for c in rc.gather_cases()])
def test_gather_equals_the_reference(mods, i):
    _, alignment, _ = mods
    a, want = rc.gather_cases()[i], rc.gather_expected(i)
    got, d = gather_on_device(alignment, a)
    assert set(got) == set(want)
    for name, v in want.items():
        g = got[name].cpu().numpy()
        assert g.dtype == v.dtype and np.array_equal(bits(g), bits(v)), (a["name"], name, g, v)
    for name in ("m_crop", "boxes", "best_q", "flow_frame", "stream_on", "frame_idx_stream", "dt_stream"):   # only read
        if a[name] is not None:
            assert np.array_equal(bits(d[name]), bits(a[name])), name
    if a["stream_on"] is not None:                            # an off stream is not touched
        off = np.repeat(a["stream_on"] == 0, a["k"])
        assert off.any()
        for name in ("reset", "age", "flow_ready"):
            if a[name] is not None:
                assert np.array_equal(bits(got[name])[off], bits(a[name])[off]), name
        assert not np.isin(got["slot_c"].cpu().numpy(), np.flatnonzero(off)).any()


@pytest.mark.parametrize("i", range(len(rc.put_cases())), ids=[c["name"] for c in rc.put_cases()])
def test_put_equals_the_reference(mods, i):
    _, alignment, _ = mods
    a = rc.put_cases()[i]
    d = {k: dev(a[k]) for k in ("slot", "status_rows", "frame_idx_c", "lm_rows", "w_rows", "hist_lm", "hist_w", "flow_frame",
                                "flow_ready")}
    res = alignment.track_flow_history_device(d["slot"], d["status_rows"], d["frame_idx_c"], d["flow_frame"], d["flow_ready"],
                                              lm_rows=d["lm_rows"], hist_lm=d["hist_lm"], w_rows=d["w_rows"], hist_w=d["hist_w"])
    assert res is d["flow_ready"]
    for name, want in zip(("hist_lm", "hist_w", "flow_frame", "flow_ready"), rc.put_expected(i)):
        if want is not None:
            assert np.array_equal(bits(d[name]), bits(want)), (a["name"], name)
    named = set(int(v) for v in a["slot"] if 0 <= v < len(a["flow_ready"]))
    rest = [g for g in range(len(a["flow_ready"])) if g not in named]
    assert rest                                               # a slot no row names keeps every bit
    for name in ("hist_lm", "hist_w", "flow_frame", "flow_ready"):
        if a[name] is not None:
            assert np.array_equal(bits(d[name])[rest], bits(a[name])[rest]), name
