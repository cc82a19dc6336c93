"""GPU parity of flm_head_pose against tests/head_pose_ref.py: the first 15 doubles of every record and factor_out bit
for bit, the three angles against numpy's atan2 / asin on the kernel's own R; landmarks and weights read in place from a
record tensor, records scattered to slots past inert rows; refused arguments.  Then FaceTracker(pose=) on a synthetic
ring: `tracker.pose` against the restatement on the landmarks the step methods return, the slots a partial step leaves
alone, the best shot driven by the pose's factor, and a tracker without pose against one with."""
import ctypes as C

import numpy as np
import pytest
import torch

import face_quality_ref as qref
import head_pose_ref as href

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
ANGLE_TOL = 1e-12     # both libms are within a few ULP (2.2e-16 each at values below pi) of the true atan2 / asin
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


def same_bits(a, b):
    a, b = bits(a), bits(b)
    return a.shape == b.shape and np.array_equal(a, b)


def assert_records(got, exp, what):
    """got: the kernel's records; exp: the restatement's.  15 doubles bit for bit, the angles by numpy on got's own R."""
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.shape == exp.shape and got.dtype == np.float64, (what, got.shape, exp.shape)
    bad = np.nonzero((bits(got[:, :15]) != bits(exp[:, :15])).any(axis=1))[0]
    assert bad.size == 0, (what, bad[:5], got[bad[:2]], exp[bad[:2]])
    ang = href.angles_of(got)
    ok = got[:, 14] == 1.0
    err = np.abs(got[:, 15:] - ang)[ok]
    assert err.size == 0 or err.max() <= ANGLE_TOL, (what, err.max())
    assert same_bits(got[~ok][:, 15:], np.zeros((int((~ok).sum()), 3))), what     # +0.0, bit for bit
    return int(ok.sum())


# ---- the inputs ---------------------------------------------------------------------------------------------------------------
MODEL68 = (href.DEFAULT_INDICES, href.DEFAULT_POINTS)
# five points for C = 7: landmark 9 does not exist, and the points of landmarks 2 and 5 coincide -- at most four take part,
# three of them distinct: always coplanar, never ok, whatever cnt says
MODEL7 = ([0, 2, 3, 5, 9], [[0.0, 0.0, 0.0], [-40.0, -30.0, 25.0], [40.0, -30.0, 25.0], [-40.0, -30.0, 25.0], [0.0, 50.0, 10.0]])


def draw(rng, n, c, model, special_from=0):
    """n faces of c landmarks: the model under a drawn pose plus noise where it names a landmark, anything elsewhere; 30 %
    of all landmarks rejected; faces with no point, with three, with the coplanar four and with (-1, y) points; weights
    with 0, a negative value and NaN among them."""
    idx, xyz = np.asarray(model[0]), np.asarray(model[1], f64)
    lm = rng.uniform(0.0, 400.0, (n, c, 2))
    inside = idx < c
    for r in range(n):
        rot = href.rotation(*rng.uniform(-1.0, 1.0, 2), rng.uniform(-3.0, 3.0))
        lm[r, idx[inside]] = (href.project(xyz, rot, rng.uniform(0.2, 1.5), 600.0, 600.0) + rng.normal(0.0, 1.5, (len(idx), 2)))[inside]
    assert lm.min() >= 0.0
    posed = lm.copy()
    lm[rng.random((n, c)) < 0.3] = -1.0
    w = rng.uniform(0.05, 1.0, (n, c))
    w[rng.random((n, c)) < 0.1] = 0.0
    w[rng.random((n, c)) < 0.05] = -0.5
    w[rng.random((n, c)) < 0.05] = np.nan
    for r in range(n):
        kind = (r + special_from) % 7
        named = idx[inside]
        if kind == 0:                                   # no landmark at all
            lm[r] = -1.0
        elif kind == 1:                                 # exactly three take part
            lm[r, named] = rng.uniform(1.0, 300.0, (len(named), 2))
            w[r, named] = 0.5
            lm[r, named[3:]] = -1.0
        elif kind == 2 and c == 68:                     # the four coplanar corners alone
            lm[r, named] = rng.uniform(1.0, 300.0, (len(named), 2))
            w[r, named] = 0.75
            lm[r, [30, 8]] = -1.0
        elif kind == 3:                                 # (-1, y) and (x, -1): one negative coordinate rejects the point
            lm[r, named[0], 0] = -1.0
            lm[r, named[1], 1] = -1.0
        elif kind == 4:                                 # every named landmark present, unit-like weights: a fit that can be ok
            w[r, named] = rng.uniform(0.3, 1.0, len(named))
            lm[r, named] = posed[r, named]
    return lm, w


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("c,model", [(68, MODEL68), (7, MODEL7)], ids=["c68", "c7"])
@pytest.mark.parametrize("n", [1, 3, 70])
def test_records_match_the_restatement(mods, n, c, model, seed):
    L, A, P = mods
    rng = np.random.default_rng(1000 * seed + 10 * n + c)
    lm, w = draw(rng, n, c, model, special_from=seed if n > 1 else 4 - 2 * seed)    # n = 1: an ok face, the coplanar four, none
    with_w = seed != 1
    min_frontal = [0.0, 0.3, 0.9][seed]
    hm = A.HeadModel(*model)
    exp = href.fit(lm, w if with_w else None, *model)
    out = torch.empty((n, A.POSE_REC), dtype=torch.float64, device="cuda")
    out.view(torch.uint8).fill_(SENT)
    fac = torch.full((n,), 7.0, dtype=torch.float64, device="cuda")
    lm_d, w_d = dev(lm), dev(w) if with_w else None
    hm.tensors(lm_d.device)                               # the model's one upload
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")               # the call synchronises nothing
    try:
        got = A.head_pose_device(lm_d, hm, weights=w_d, opts=A.HeadPose(min_frontal=min_frontal), out=out, factor_out=fac)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert got is out
    n_ok = assert_records(out, exp, (n, c, seed))
    assert same_bits(fac, href.factor(exp, min_frontal)), (fac.cpu().numpy(), href.factor(exp, min_frontal))
    counts = sorted(set(exp[:, 13].astype(int).tolist()))
    print("n", n, "c", c, "seed", seed, "ok", n_ok, "of", n, "counts", counts)
    if c == 7:
        assert n_ok == 0
    elif n == 70:
        assert n_ok >= 10 and n - n_ok >= 10 and {0, 3}.issubset(counts)        # both branches, and the special faces
        assert (href.factor(exp, min_frontal) == 0.0).any() and (href.factor(exp, min_frontal) > 0.0).any()


def test_strides_and_scatter(mods):
    L, A, P = mods
    n, c, n_slots = 70, 68, 90
    rng = np.random.default_rng(77)
    lm, w = draw(rng, n, c, MODEL68)
    rec6 = rng.uniform(0.0, 1.0, (n, c, L.LANDMARK_REC))
    rec6[..., :2], rec6[..., 2] = lm, w
    rec_d = dev(rec6)
    hm = A.HeadModel.default(c)
    exp = href.fit(lm, w, *MODEL68)
    # in place from the record tensor
    dense = A.head_pose_device(rec_d[..., :2], hm, weights=rec_d[..., 2])
    assert rec_d[..., :2].data_ptr() == rec_d.data_ptr() and not rec_d[..., :2].is_contiguous()
    n_ok = assert_records(dense, exp, "in place")
    assert 10 <= n_ok <= n - 10
    # a permutation of the slots with inert rows: -1 and n_slots
    slot = rng.permutation(n_slots)[:n].astype(np.int32)
    inert = np.array([0, 5, 33, 69])
    slot[inert[::2]], slot[inert[1::2]] = -1, n_slots
    valid = np.setdiff1d(np.arange(n), inert)
    out = torch.empty((n_slots, A.POSE_REC), dtype=torch.float64, device="cuda")
    out.view(torch.uint8).fill_(SENT)
    fac = torch.full((n,), 7.0, dtype=torch.float64, device="cuda")
    A.head_pose_device(rec_d[..., :2], hm, weights=rec_d[..., 2], opts=A.HeadPose(min_frontal=0.3), slot=dev(slot), out=out,
                       factor_out=fac)
    got = out.cpu().numpy()
    assert same_bits(got[slot[valid]], dense.cpu().numpy()[valid]), "a named slot holds its row's record"
    unnamed = np.setdiff1d(np.arange(n_slots), slot[valid])
    assert len(unnamed) == n_slots - len(valid) and (bits(got[unnamed]).view(np.uint8) == SENT).all()
    exp_fac = href.factor(exp, 0.3)
    exp_fac[inert] = 0.0
    assert same_bits(fac, exp_fac)
    # the same inputs one row at a time: the result does not depend on the launch shape
    single = torch.empty_like(dense)
    for r in range(n):
        A.head_pose_device(rec_d[r:r + 1, :, :2], hm, weights=rec_d[r:r + 1, :, 2], out=single[r:r + 1])
    assert same_bits(single, dense)


def test_refused_arguments(mods):
    L, A, P = mods
    n, c = 4, 68
    hm = A.HeadModel.default(c)
    rec = torch.zeros((n, c, 6), dtype=torch.float64, device="cuda")
    lm, w = rec[..., :2], rec[..., 2]
    flat = rec.view(-1)
    with pytest.raises(ValueError, match="overlap"):
        A.head_pose_device(lm, hm, out=flat[:n * 18].view(n, 18))                      # over the landmarks
    with pytest.raises(ValueError, match="overlap"):
        A.head_pose_device(lm, hm, factor_out=flat[10:10 + n])                         # inside the records' gaps
    with pytest.raises(ValueError, match="overlap"):
        A.head_pose_device(torch.zeros((n, c, 2), dtype=torch.float64, device="cuda"), hm, weights=w, out=flat[:n * 18].view(n, 18))
    both = torch.zeros((n * 19,), dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError, match="overlap"):
        A.head_pose_device(lm, hm, out=both[:n * 18].view(n, 18), factor_out=both[n * 18 - 1:n * 19 - 1])
    slot = torch.arange(n, dtype=torch.int32, device="cuda")
    for kw in (dict(out=torch.zeros((n, 18), dtype=torch.float32, device="cuda")),                      # dtype
               dict(out=torch.zeros((n, 36), dtype=torch.float64, device="cuda")[:, ::2]),              # not contiguous
               dict(out=torch.zeros((n + 1, 18), dtype=torch.float64, device="cuda")),                  # rows without slot
               dict(factor_out=torch.zeros((n + 1,), dtype=torch.float64, device="cuda")),
               dict(slot=slot),                                                                         # slot without out
               dict(slot=slot.to(torch.int64), out=torch.zeros((9, 18), dtype=torch.float64, device="cuda")),
               dict(weights=torch.zeros((n, c - 1), dtype=torch.float64, device="cuda")),
               dict(weights=w.to(torch.float32))):
        with pytest.raises(ValueError):
            A.head_pose_device(lm, hm, **kw)
    with pytest.raises(ValueError):
        A.head_pose_device(lm.to(torch.float32), hm)
    # the C call itself
    lib = L.load()
    idx, xyz = hm.tensors(rec.device)
    out = torch.zeros((n, 18), dtype=torch.float64, device="cuda")
    call = lambda pose, factor: lib.flm_head_pose(L.stream_ptr(), L.ptr(rec), 6, C.c_void_p(rec.data_ptr() + 16), 6, n, c,
                                                  L.ptr(idx), L.ptr(xyz), 6, None, None, 0, pose, factor)
    assert call(L.ptr(flat[100:]), None) == -1 and b"overlaps lm_dev" in lib.flm_last_error()
    assert call(L.ptr(out), L.ptr(out[1:])) == -1 and b"overlap" in lib.flm_last_error()
    assert call(L.ptr(out), L.ptr(both)) == 0
    torch.cuda.synchronize()
    assert same_bits(out, href.fit(np.zeros((n, c, 2)), np.zeros((n, c)), *MODEL68))     # zero weights: nothing takes part


# ---- FaceTracker(pose=) --------------------------------------------------------------------------------------------------------
RH, RW, CAP, S = 64, 96, 9, 3
FACES = [(20, 8, 60, 50), (40, 2, 90, 60), (-6, 20, 30, 58), (30, 10, 80, 60)]
SEEDS = {0: ([0, 2], FACES[:2]), 1: ([1], FACES[2:3]), 2: ([0], FACES[3:])}       # stream -> (its local slots, the boxes)
SEEDED = [0, 2, 4, 6]
NOT_OK = href.not_ok(0)


@pytest.fixture(scope="module")
def ring():
    rng = np.random.default_rng(31)
    return dev(rng.integers(0, 256, (8, RH, RW, 3), dtype=np.uint8))


@pytest.fixture(scope="module")
def model():
    from flm_amd.networks import LANDMARKS_MODELS
    from flm_amd.weights import synth_fcn8_weights
    m = LANDMARKS_MODELS["fcn_8"](68, input_height=64, input_width=64, dtype="bf16")
    m.load_weights(synth_fcn8_weights(68, seed=2))
    return m


def seed_four(tr):
    for i, (slots, faces) in SEEDS.items():
        tr.seed(slots, faces, stream=i)


def restate(lm, pose=None):
    return href.fit(lm.cpu().numpy(), None, *MODEL68, min_volume=1e-6 if pose is None else pose.min_volume)


@pytest.mark.parametrize("smooth", [None, True])
def test_step_writes_every_slot(mods, ring, model, smooth):
    L, A, P = mods
    tr = P.FaceTracker(model, (RH, RW), 3, smooth=smooth, pose=True)
    tr.seed([0, 1], FACES[:2])                                   # slot 2 holds no face
    assert same_bits(tr.pose, np.stack([NOT_OK] * 3))
    n_ok = 0
    for t in range(4):
        aligned, m_align, lm, status = tr.step(ring, t)
        n_ok += assert_records(tr.pose, restate(lm), ("step", t))
        assert same_bits(tr.pose[2], NOT_OK) and (lm[2] == -1).all()
    print("smooth", smooth, "ok records over 4 steps:", n_ok, "status", tr.status.tolist())


def test_partial_steps_scatter_and_keep(mods, ring, model):
    L, A, P = mods
    tr = P.FaceTracker(model, (RH, RW), CAP, streams=S, pose=A.HeadPose(min_volume=1e-5))
    seed_four(tr)
    tr.step(ring, [1, 3, 5])
    sentinel = torch.empty_like(tr.pose)
    sentinel.view(torch.uint8).fill_(SENT)
    # step_active: streams 2 and 0
    seed_four(tr)
    tr.pose.copy_(sentinel)
    aligned, m_align, lm, status, slots = tr.step_active(ring, [2, None, 4], [2, 0])
    assert slots.tolist() == [6, 7, 8, 0, 1, 2]
    assert_records(tr.pose[slots.to(torch.int64)], restate(lm, tr.head_pose), "step_active")
    assert same_bits(tr.pose[3:6], sentinel[3:6])
    # step_live: four live slots, a budget of two
    seed_four(tr)
    tr.pose.copy_(sentinel)
    aligned, m_align, lm, status, slots = tr.step_live(ring, [6, 7, 0], 2)
    served = slots.tolist()
    assert served == SEEDED[:2] and tr.live_counts.tolist()[:3] == [4, 2, 2]
    assert_records(tr.pose[slots.to(torch.int64)], restate(lm, tr.head_pose), "step_live")
    rest = [g for g in range(CAP) if g not in served]
    assert same_bits(tr.pose[rest], sentinel[rest])
    # the next call serves the two that waited, and an inert row writes nothing
    tr.pose.copy_(sentinel)
    aligned, m_align, lm, status, slots = tr.step_live(ring, [1, 2, 3], 3)
    served = [g for g in slots.tolist() if g >= 0]
    assert served[:2] == SEEDED[2:] and (len(served) == 3 or -1 in slots.tolist())     # slots 0 and 2 follow if they live
    k = len(served)
    assert_records(tr.pose[slots[:k].to(torch.int64)], restate(lm[:k], tr.head_pose), "step_live, second call")
    rest = [g for g in range(CAP) if g not in served]
    assert same_bits(tr.pose[rest], sentinel[rest])


# The landmarks of a network with synthetic weights are no face: under the six-point model nearly every fit comes out turned
# away.  A model of 17 arbitrary points on every fourth landmark spreads R[2][2] over [-1, 1], so that min_frontal = 0.5
# divides the faces; it is also the tracker's custom-model path.
MIN_FRONTAL = 0.5
MODEL17 = (list(range(0, 68, 4)), np.random.default_rng(5).uniform(-100.0, 100.0, (17, 3)).tolist())


def test_best_shot_takes_the_pose_factor(mods, ring, model):
    L, A, P = mods
    shot = A.BestShot(sharp_ref=1e6, min_exposed=0.25)
    pose = A.HeadPose(model=A.HeadModel(*MODEL17), min_frontal=MIN_FRONTAL)
    tr = P.FaceTracker(model, (RH, RW), 3, best_shot=shot, pose=pose)
    st, passed, failed = None, 0, 0
    for t in range(5):
        if t in (0, 3):
            tr.seed([0, 1, 2], FACES[:3])
        aligned, m_align, lm, status = [x.cpu().numpy() for x in tr.step(ring, t)]
        if st is None:
            st = qref.new_state(aligned, 3, 68)
        exp = href.fit(lm, None, *MODEL17)
        assert_records(tr.pose, exp, ("best", t))
        factor = href.factor(exp, MIN_FRONTAL)
        passed, failed = passed + int((factor > 0).sum()), failed + int((factor == 0).sum())
        rec = qref.record(aligned, A.AlignedFormat(), shot.dark, shot.bright)
        reset = np.full(3, 1 if t in (0, 3) else 0, np.int32)
        taken = qref.best_update(st, aligned, rec, lm, t, factor=factor, status=status, reset=reset, m=m_align,
                                 sharp_ref=shot.sharp_ref, min_exposed=shot.min_exposed)
        print("frame", t, "status", status.tolist(), "factor", factor.tolist(), "taken", taken.tolist(), "best_q", st["best_q"].tolist())
        assert same_bits(tr.best_q, st["best_q"]), (t, tr.best_q.cpu().numpy(), st["best_q"])
        assert same_bits(tr.best_frame, st["best_frame"]) and same_bits(tr.gallery, st["gallery"]), t
    print("faces at or above min_frontal:", passed, "below it or not ok:", failed)
    assert passed > 0 and failed > 0
    assert (st["best_q"] == 0.0).any() and (st["best_q"] > 0.0).any()   # a best held at factor 0, and one that counted


def test_a_tracker_without_pose_is_unchanged(mods, ring, model):
    L, A, P = mods
    plain = P.FaceTracker(model, (RH, RW), CAP, streams=S, smooth=True)
    posed = P.FaceTracker(model, (RH, RW), CAP, streams=S, smooth=True, pose=True)
    assert plain.pose is None and plain.head_pose is None
    for tr in (plain, posed):
        seed_four(tr)
    for t in range(3):
        fi = [(3 * t + 2 * i + 1) % 8 for i in range(S)]
        a, b = plain.step(ring, fi, dt=0.04), posed.step(ring, fi, dt=0.04)
        for x, y in zip(a, b):
            assert x.dtype == y.dtype and same_bits(x, y), t
        for name in ("m_crop", "boxes", "status", "misses", "filter_state", "frame_slots"):
            assert same_bits(getattr(plain, name), getattr(posed, name)), (name, t)
