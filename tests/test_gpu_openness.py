"""flm_face_openness on the GPU against tests/parts_ref.py, bit for bit: the records by row and by slot (N = 7 and 130 --
one workgroup and three; G = 3 default measures plus a V = 1 and a V = 4 one; missing points, a width just below and just
above min_width, NaN coordinates, zero and NaN weights, a zero width), and the blink state over scripted sequences of
12 ticks on 6 slots -- a closure that counts, one too short, one too long, a not-ok tick and a reset in mid-closure --
through the all-slots form, a rows form with inert rows that names half the slots, and per-row dt on the device."""
import numpy as np
import pytest
import torch

import parts_ref as ref

pytestmark = pytest.mark.gpu
MEASURES = ref.DEFAULT_MEASURES + ref.EXTRA_MEASURES
SENT = -1234.5


@pytest.fixture(scope="module")
def mods():
    import flm_amd  # noqa: F401
    from flm_amd import _lib, alignment, prediction
    _lib.load()
    return _lib, alignment, prediction


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def u64(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.mark.parametrize("n", [7, 130])
def test_records_by_row_and_by_slot(mods, n):
    _, A, _ = mods
    opts = A.Openness(MEASURES, min_width=4.0)
    lm, w = ref.openness_landmarks(n, 4)
    g = len(MEASURES)
    for weights in (None, w):
        want = ref.openness(lm, weights, MEASURES, 4.0)
        assert {0.0, 1.0} == set(want[..., 2].ravel().tolist())
        buf = torch.full((n + 2, g, 4), SENT, dtype=torch.float64, device="cuda")
        got = A.face_openness_device(dev(lm), opts, weights=None if weights is None else dev(weights), out=buf[1:-1])
        assert np.array_equal(u64(got.cpu().numpy()), u64(want)), weights is None
        assert bool((buf[0] == SENT).all()) and bool((buf[-1] == SENT).all())
    # the stated rows: a missing point, widths around min_width, NaN coordinates, a zero width
    assert (want[1, 0] == [-1, -1, 0, -1]).all() and want[2, 0, 2] == 0.0 and want[2, 0, 1] < 4.0 and want[2, 1, 2] == 1.0
    assert want[3, 0, 2] == 0.0 and want[3, 2, 2] == 0.0 and want[5, 2, 2] == 0.0 and want[5, 2, 1] == 0.0
    # by slot: rows scattered over n + 9 slots, inert rows among them; unnamed slots keep their bits
    rng = np.random.default_rng(n)
    n_slots = n + 9
    slot = rng.permutation(n_slots)[:n].astype(np.int32)
    slot[::5] = -1
    slot[3] = n_slots
    want = ref.openness(lm, w, MEASURES, 4.0, slot=slot, rec=np.full((n_slots, g, 4), SENT))
    out = torch.full((n_slots, g, 4), SENT, dtype=torch.float64, device="cuda")
    rec = torch.full((n, 68, 6), 5.0, dtype=torch.float64, device="cuda")      # read in place from a record tensor
    rec[..., :2] = dev(lm)
    rec[..., 2] = dev(w)
    got = A.face_openness_device(rec[..., :2], opts, weights=rec[..., 2], slot=dev(slot), out=out)
    assert got.data_ptr() == out.data_ptr() and np.array_equal(u64(got.cpu().numpy()), u64(want))
    assert (want == SENT).all(axis=(1, 2)).sum() == n_slots - (slot[(slot >= 0) & (slot < n_slots)]).size


def test_prediction_face_openness(mods):
    _, A, P = mods
    lm, w = ref.openness_landmarks(7, 4)
    want = ref.openness(lm, w, ref.DEFAULT_MEASURES, 4.0)
    res = P.face_openness(lm, weights=w)
    assert isinstance(res["record"], np.ndarray) and np.array_equal(u64(res["record"]), u64(want))
    assert np.array_equal(res["openness"], want[..., 0]) and np.array_equal(res["ok"], want[..., 2])
    res = P.face_openness(dev(lm), weights=dev(w), openness=A.Openness(MEASURES))
    assert res["record"].is_cuda and tuple(res["width"].shape) == (7, 5)
    with pytest.raises(ValueError):
        P.face_openness(lm[:, :5])


def script():
    o, not_ok, resets, events = ref.eye_script()
    th = dict(ref.DEFAULT_TH, min_closed=0.05, max_closed=0.2)
    return o, not_ok, resets, events, th


def run_script(A, form):
    """The scripted ticks on the device and in the reference, compared after every tick.  Returns the final state."""
    o, not_ok, resets, events, th = script()
    ticks, n_slots = o.shape
    g = 3
    opts = A.Openness(ref.DEFAULT_MEASURES, min_closed=th["min_closed"], max_closed=th["max_closed"], min_width=4.0)
    rng = np.random.default_rng(17)
    total = n_slots + 4 if form != "all" else n_slots                   # rows forms: four slots no row ever names
    state_h = np.tile(np.array(ref.STATE_EMPTY), (total, g, 1))
    state_h[n_slots:] = SENT
    rec_h = np.full((total, g, 4), SENT)
    reset_h = np.zeros(total, np.int32)
    reset_h[n_slots:] = 9
    state_d, rec_d, reset_d = dev(state_h), dev(rec_h), dev(reset_h)
    for t in range(ticks):
        lm_slots = ref.eye_landmarks(o[t], {s for tt, s in not_ok if tt == t})
        for tt, s in resets:
            if tt == t:
                reset_h[s] = 1
                reset_d[s] = 1
        if form == "all":
            rows = np.arange(n_slots)
            slot, lm, dt, status = None, lm_slots, 0.04, None
        else:
            # every slot is served on every tick -- the script's closures count served ticks -- by TWO calls that name
            # half the slots each, in a shuffled order, with inert rows between them
            rows = None
        calls = [(slot, lm, dt, status)] if form == "all" else []
        if form != "all":
            perm = rng.permutation(n_slots)
            for half in (perm[:3], perm[3:]):
                sl = np.full(5, -1, np.int32)
                pos = rng.permutation(5)[:3]
                sl[pos] = half
                sl[[i for i in range(5) if i not in pos][0]] = total + 3           # inert: past the slots
                lm = rng.uniform(5.0, 300.0, (5, 68, 2))                            # inert rows hold open, valid faces
                lm[pos] = lm_slots[half]
                if form == "rows_dt":       # per-row dt on the device; a status row that is not 0 would freeze the state
                    dt = np.full(5, 0.5)
                    dt[pos] = 0.04
                else:
                    dt = 0.04
                calls.append((sl, lm, dt, np.zeros(5, np.int32)))
        for sl, lm, dt, status in calls:
            before = reset_h.copy()
            ref.openness(lm, None, ref.DEFAULT_MEASURES, 4.0, th, slot=sl, rec=rec_h, state=state_h, reset=reset_h, dt=dt,
                         status=status, frame_id=100 + t)
            A.face_openness_device(dev(lm), opts, slot=None if sl is None else dev(sl), out=rec_d, state=state_d,
                                   reset=reset_d, dt=dev(dt) if np.ndim(dt) else dt,
                                   status_rows=None if status is None else dev(status), frame_id=100 + t)
            assert np.array_equal(u64(state_d.cpu().numpy()), u64(state_h)), (form, t)
            assert np.array_equal(u64(rec_d.cpu().numpy()), u64(rec_h)), (form, t)
            got_reset = reset_d.cpu().numpy()
            assert np.array_equal(got_reset, reset_h), (form, t)
            served = np.arange(total) if sl is None else sl[(sl >= 0) & (sl < total)]
            unserved = np.setdiff1d(np.arange(total), served)
            assert (got_reset[served] == 0).all() and np.array_equal(got_reset[unserved], before[unserved]), (form, t)
    if form != "all":    # the slots no row named keep the sentinel pattern and their flag
        assert (u64(state_d.cpu().numpy()[n_slots:]) == u64(np.array([SENT]))).all()
        assert (u64(rec_d.cpu().numpy()[n_slots:]) == u64(np.array([SENT]))).all()
        assert (reset_d.cpu().numpy()[n_slots:] == 9).all()
    final = state_d.cpu().numpy()[:n_slots]
    for m in range(g):
        assert final[:, m, 2].tolist() == [float(v) for v in events], (form, m)      # the hand count
    return final


def test_state_all_slots_rows_and_row_dt(mods):
    _, A, _ = mods
    a = run_script(A, "all")
    b = run_script(A, "rows")
    c = run_script(A, "rows_dt")
    assert np.array_equal(u64(a), u64(b)) and np.array_equal(u64(a), u64(c))
    assert a[0, 0, 6] == 106.0 and a[4, 0, 6] == -1.0


def test_state_keeps_its_bits_where_the_contract_says(mods):
    """A status that is not 0, a dt on the device that is not finite and > 0, and a measure that is not ok leave the state
    alone (a pending reset is still served); a slot that sits a tick out keeps state and flag."""
    _, A, _ = mods
    opts = A.Openness(ref.DEFAULT_MEASURES)
    lm = ref.eye_landmarks(np.array([0.1, 0.1, 0.1, 0.1, 0.1]), {4})
    state_h = np.tile(np.array([1.0, 0.07, 2.0, 0.1, 0.5, 3.0, 42.0, 0.0]), (5, 3, 1))
    reset_h = np.array([0, 0, 0, 1, 1], np.int32)
    status = np.array([0, 8, 0, 8, 0], np.int32)
    dt = np.array([0.04, 0.04, np.nan, 0.04, 0.04])
    slot = np.array([0, 1, 2, 3, 4], np.int32)
    state_d, reset_d = dev(state_h), dev(reset_h)
    rec_h = np.zeros((5, 3, 4))
    ref.openness(lm, None, ref.DEFAULT_MEASURES, 4.0, ref.DEFAULT_TH, slot=slot, rec=rec_h, state=state_h, reset=reset_h, dt=dt,
                 status=status, frame_id=3)
    out = torch.zeros((5, 3, 4), dtype=torch.float64, device="cuda")
    A.face_openness_device(dev(lm), opts, slot=dev(slot), out=out, state=state_d, reset=reset_d, dt=dev(dt),
                           status_rows=dev(status), frame_id=3)
    got = state_d.cpu().numpy()
    assert np.array_equal(u64(got), u64(state_h)) and np.array_equal(u64(out.cpu().numpy()), u64(rec_h))
    assert not reset_d.cpu().numpy().any()
    start = np.array([1.0, 0.07, 2.0, 0.1, 0.5, 3.0, 42.0, 0.0])
    assert (got[1] == start).all() and (got[2] == start).all()                  # status, NaN dt
    assert (got[3] == ref.STATE_EMPTY).all() and (got[4] == ref.STATE_EMPTY).all()   # reset served, nothing added
    assert got[0, 0, 1] == 0.07 + 0.04 and got[0, 0, 4] == 0.5 + 0.04
