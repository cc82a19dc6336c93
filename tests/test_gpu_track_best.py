"""GPU parity of flm_track_best_update against tests/face_quality_ref.py, bit for bit: random sequences of updates with
drawn status words, reset masks, weights over partly rejected landmarks and factors (NaN among them), on outputs
pre-filled with a sentinel so that an untaken slot and the bytes beyond the K faces are shown untouched.  Then
FaceTracker(best_shot=True) on a synthetic ring with synthetic weights: `step` returns the bits of a tracker without
best_shot, and `best()` equals the reference driven by what `step` itself returned."""
import numpy as np
import pytest
import torch

import aligned_format_ref as fref
import face_quality_ref as ref

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
K, C_PTS, UPDATES = 5, 7, 6
RH, RW = 96, 128


@pytest.fixture(scope="module")
def mods():
    import flm_amd  # noqa: F401
    from flm_amd import _lib, alignment, prediction
    _lib.load()
    return _lib, alignment, prediction


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def bits_equal(got, exp):
    got = got.cpu().numpy()
    assert got.dtype == exp.dtype and got.shape == exp.shape, (got.dtype, exp.dtype, got.shape, exp.shape)
    u = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    return np.array_equal(np.ascontiguousarray(got).view(u), np.ascontiguousarray(exp).view(u))


def draw_update(rng, fmt, h, w, blur):
    """One frame's inputs for K slots: faces in the format (some blurred, one black), and everything that decides."""
    img = rng.uniform(0, 255, (K, h, w, 3)).astype(f32)
    for i in range(K):
        for _ in range(int(blur[i])):
            img[i] = ref.box_blur(img[i])
    if rng.random() < 0.5:
        img[rng.integers(K)] = 0.0                                        # all dark: e = 0, never eligible
    faces = fref.convert(img, fmt)
    lm = rng.uniform(0, 100, (K, C_PTS, 2))
    lm[rng.random((K, C_PTS)) < 0.3] = -1.0                               # rejected landmarks
    lm[rng.integers(K), :, :] = -1.0                                      # a slot without any
    lm[rng.integers(K), 0, 0] = -1.0                                      # (-1, y) is not rejected
    wts = rng.uniform(0, 1, (K, C_PTS))
    factor = rng.choice([1.0, 0.5, 2.0, 0.0, -1.0, np.nan, np.inf], K, p=[.4, .15, .15, .1, .05, .1, .05])
    status = rng.choice([0, 0, 0, 1, 4, 64], K).astype(np.int32)
    reset = rng.choice([0, 0, 0, 1, 5], K).astype(np.int32)
    m = rng.normal(0, 2, (K, 2, 3)).astype(f32)
    return faces, lm, wts, factor, status, reset, m


CASES = [("nhwc", "uint8", "bgr", (1.0,) * 3, (0.0,) * 3, 8, 8), ("nchw", "float16", "rgb", (1.0 / 127.5,) * 3, (-1.0,) * 3, 112, 112)]


@pytest.mark.parametrize("case", CASES, ids=["u8_nhwc_8x8", "f16_nchw_112x112"])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_sequences_match_the_reference(mods, case, seed):
    L, A, P = mods
    fmt, (h, w) = case[:5], case[5:]
    rng = np.random.default_rng(100 + seed)
    sharp_ref = [100.0, 3e4, 1e6][seed]                 # (noise saturates the customary 100: the larger ones tell faces apart)
    opts = A.BestShot(sharp_ref=sharp_ref, min_exposed=0.5)
    with_w, with_factor, with_status, with_reset, with_m = [(seed >> b) & 1 == 0 for b in range(3)] + [seed != 1, seed != 2]
    shape = fref.convert(np.zeros((K, h, w, 3), f32), fmt)
    # the device state, every output pre-filled with a sentinel; the gallery has one more face than K: the bytes beyond
    SENT = 0x5a
    gal_all = torch.full((K + 1,) + shape.shape[1:], 0, dtype=dev(shape).dtype, device="cuda")
    gal_all.view(torch.uint8).fill_(SENT)
    gallery = gal_all[:K]
    q = [dev(np.full(K, -1.0)), dev(np.full(K, 777.0))]
    bframe = dev(np.full(K, -99, np.int64))
    bm, blm, brec = dev(np.full((K, 2, 3), 9.5, f32)), dev(np.full((K, C_PTS, 2), 9.5)), dev(np.full((K, 8), -99, np.int64))
    st = dict(gallery=gal_all[:K].cpu().numpy().copy(), best_q=np.full(K, -1.0), best_frame=np.full(K, -99, np.int64),
              best_m=np.full((K, 2, 3), 9.5, f32), best_lm=np.full((K, C_PTS, 2), 9.5), best_rec=np.full((K, 8), -99, np.int64))
    n_taken = n_kept = 0
    for t in range(UPDATES):
        faces, lm, wts, factor, status, reset, m = draw_update(rng, fmt, h, w, rng.integers(0, 3, K))
        rec = ref.record(faces, fmt)
        kw = dict(w=wts if with_w else None, factor=factor if with_factor else None, status=status if with_status else None,
                  reset=reset if with_reset else None, m=m if with_m else None)
        taken = ref.best_update(st, faces, rec, lm, 1000 + t, sharp_ref=sharp_ref, **kw)
        n_taken += int(taken.sum())
        n_kept += int((~taken).sum())
        faces_d, lm_d = dev(faces), dev(lm)
        dkw = dict(status=dev(status) if with_status else None, reset=dev(reset) if with_reset else None,
                   weights=dev(wts) if with_w else None, factor=dev(factor) if with_factor else None,
                   m=dev(m) if with_m else None)
        rec_d = torch.empty((K, 8), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")                           # the two calls synchronise nothing
        try:
            A.face_quality_device(faces_d, A.AlignedFormat(*fmt), out=rec_d)
            out = A.track_best_update_device(faces_d, rec_d, lm_d, q[0], q[1], gallery, bframe, 1000 + t, opts=opts,
                                             best_m=bm if with_m else None, best_lm=blm, best_rec=brec, **dkw)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert out is q[1]
        assert np.array_equal(rec_d.cpu().numpy(), rec)
        q.reverse()
        assert bits_equal(q[0], st["best_q"]), (t, q[0].cpu().numpy(), st["best_q"])
        assert bits_equal(gallery, st["gallery"]), t
        assert bits_equal(bframe, st["best_frame"]) and bits_equal(blm, st["best_lm"]) and bits_equal(brec, st["best_rec"]), t
        assert bits_equal(bm, st["best_m"]), t
        assert (gal_all[K].view(torch.uint8) == SENT).all(), t            # the bytes beyond the K faces
    print(case[:2], "seed", seed, "taken", n_taken, "kept", n_kept)
    assert n_taken >= K and n_kept >= K                                    # both branches were exercised


def test_strided_views_and_unaligned_gallery(mods):
    """lm and w as views of a landmark record tensor (stride 6), and a gallery that is not congruent with the faces
    modulo 16: the copy falls back to bytes and writes nothing beyond."""
    L, A, P = mods
    rng = np.random.default_rng(9)
    fmt = CASES[0][:5]
    faces, lm, wts, factor, status, reset, m = draw_update(rng, fmt, 8, 8, np.zeros(K, int))
    status[:] = 0
    factor[:] = 1.0
    rec = ref.record(faces, fmt)
    rec6 = np.zeros((K, C_PTS, 6))
    rec6[..., :2], rec6[..., 2] = lm, wts
    rec6_d = dev(rec6)
    buf = torch.full((K * 192 + 40,), 0x5a, dtype=torch.uint8, device="cuda")
    gallery = buf[3:3 + K * 192].view(K, 8, 8, 3)
    st = dict(ref.new_state(faces, K, C_PTS), gallery=np.full_like(faces, 0x5a))
    taken = ref.best_update(st, faces, rec, lm, 5, w=wts)
    assert taken.any()
    q_out, bframe = dev(np.zeros(K)), dev(np.full(K, -1, np.int64))
    blm = dev(np.full((K, C_PTS, 2), -1.0))
    A.track_best_update_device(dev(faces), dev(rec), rec6_d[..., :2], dev(np.full(K, -1.0)), q_out, gallery, bframe, 5,
                               weights=rec6_d[..., 2], best_lm=blm)
    assert bits_equal(q_out, st["best_q"]) and bits_equal(gallery, st["gallery"]) and bits_equal(bframe, st["best_frame"])
    assert bits_equal(blm, st["best_lm"])
    assert (buf[:3] == 0x5a).all() and (buf[3 + K * 192:] == 0x5a).all()


def test_overlap_is_refused(mods):
    L, A, P = mods
    faces = torch.zeros((K, 8, 8, 3), dtype=torch.uint8, device="cuda")
    rec = torch.zeros((K, 8), dtype=torch.int64, device="cuda")
    lm = torch.zeros((K, C_PTS, 2), dtype=torch.float64, device="cuda")
    qq = torch.full((2 * K,), -1.0, dtype=torch.float64, device="cuda")
    gallery, bframe = torch.zeros_like(faces), torch.zeros((K,), dtype=torch.int64, device="cuda")
    with pytest.raises(ValueError, match="overlap"):
        A.track_best_update_device(faces, rec, lm, qq[:K], qq[:K], gallery, bframe, 0)
    with pytest.raises(ValueError, match="overlap"):
        A.track_best_update_device(faces, rec, lm, qq[:K], qq[1:K + 1], gallery, bframe, 0)
    lib = L.load()
    args = lambda q_in, q_out: (L.stream_ptr(), L.ptr(faces), 192, K, L.ptr(rec), None, None, L.ptr(lm), 2, None, 1, C_PTS, None,
                                None, 0, None, q_in, q_out, L.ptr(gallery), L.ptr(bframe), None, None, None)
    assert lib.flm_track_best_update(*args(L.ptr(qq), L.ptr(qq))) == -1 and b"overlap" in lib.flm_last_error()
    assert lib.flm_track_best_update(*args(L.ptr(qq[2:]), L.ptr(qq))) == -1 and b"overlap" in lib.flm_last_error()
    assert lib.flm_track_best_update(*args(L.ptr(qq), L.ptr(qq[K:]))) == 0          # adjacent halves are two buffers
    torch.cuda.synchronize()
    assert (qq[K:] == -1.0).all() and (gallery == 0).all()                           # (n_lap = 0 in a zero record: nothing taken)


# ---- FaceTracker(best_shot=True) -------------------------------------------------------------------------------------------
FACES = [(20, 8, 60, 50), (40, 2, 90, 60), (60, 30, 120, 90)]
SHARP, RESEED_BEFORE, RESEED_SLOT = 2, 3, 1


@pytest.fixture(scope="module")
def ring():
    """Five frames of one scene: frame 2 is the sharp original, the others are box-blurred copies (twice)."""
    rng = np.random.default_rng(31)
    base = rng.integers(0, 256, (RH // 4, RW // 4, 3)).astype(f32)
    base = np.kron(base, np.ones((4, 4, 1), f32))                        # 4 px blocks: edges the blur can soften
    soft = ref.box_blur(ref.box_blur(base))
    frames = [np.clip(np.rint(base if f == SHARP else soft), 0, 255).astype(np.uint8) for f in range(5)]
    return dev(np.stack(frames))


@pytest.fixture(scope="module")
def model():
    from flm_amd.networks import LANDMARKS_MODELS
    from flm_amd.weights import synth_fcn8_weights
    m = LANDMARKS_MODELS["fcn_8"](68, input_height=64, input_width=64, dtype="f32")
    m.load_weights(synth_fcn8_weights(68, seed=2))
    return m


@pytest.mark.parametrize("weights,matcher", [(None, True), ("score", False)])
def test_face_tracker_keeps_the_best_shot(mods, ring, model, weights, matcher):
    L, A, P = mods
    fmt = A.AlignedFormat.matcher() if matcher else None
    shot = A.BestShot(sharp_ref=1e6, min_exposed=0.25)
    plain = P.FaceTracker(model, (RH, RW), 3, weights=weights, aligned_format=fmt)
    tr = P.FaceTracker(model, (RH, RW), 3, weights=weights, aligned_format=fmt, best_shot=shot)
    with pytest.raises(ValueError):
        plain.best()
    with pytest.raises(ValueError):
        plain.step(ring, 0, frame_id=3)
    st = None
    for t in range(5):
        if t == 0:
            plain.seed([0, 1, 2], FACES)
            tr.seed([0, 1, 2], FACES)
        if t == RESEED_BEFORE:
            plain.seed([RESEED_SLOT], [FACES[RESEED_SLOT]])
            tr.seed([RESEED_SLOT], [FACES[RESEED_SLOT]])
        exp = plain.step(ring, t)
        m_prev, b_prev = tr.m_crop.clone(), tr.boxes.clone()             # what this step cuts its crops with
        got = tr.step(ring, t)
        best = tr.best()
        for a, b in zip(got, exp):                                        # the four returns: the bits of a plain tracker
            assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), t
        aligned, m_align, lm, status = [x.cpu().numpy() if x.dtype != torch.bfloat16 else x for x in got]
        afmt = fmt if fmt is not None else A.AlignedFormat()
        if st is None:
            st = ref.new_state(aligned, 3, 68)
        rec = ref.record(aligned, afmt, shot.dark, shot.bright)
        w = None
        if weights == "score":                                            # the scores of this step's forward: recomputed here
            crops = A.warp_frames_device(ring, m_prev, 64, 64, frame_index_dev=torch.full((3,), t, dtype=torch.int32, device="cuda"),
                                         boxes_dev=b_prev, fmt=A.AlignedFormat("nhwc", "uint8"))
            w = model.forward_device(crops, "landmark_stats", n_points=4, thresh=0.0)[..., 2].cpu().numpy()
        reset = np.zeros(3, np.int32)
        if t == 0:
            reset[:] = 1
        if t == RESEED_BEFORE:
            reset[RESEED_SLOT] = 1
        taken = ref.best_update(st, aligned, rec, lm, t, w=w, status=status, reset=reset, m=m_align, sharp_ref=shot.sharp_ref,
                                min_exposed=shot.min_exposed)
        print("frame", t, "status", status.tolist(), "taken", taken.tolist(), "best_q", st["best_q"].tolist())
        gallery, best_q, best_frame, best_m, best_lm = best
        assert all(x.is_cuda for x in best)
        assert bits_equal(best_q, st["best_q"]), (t, best_q.cpu().numpy(), st["best_q"])
        assert bits_equal(gallery, st["gallery"]) and bits_equal(best_frame, st["best_frame"]), t
        assert bits_equal(best_m, st["best_m"]) and bits_equal(best_lm, st["best_lm"]) and bits_equal(tr.best_rec, st["best_rec"]), t
        if t == SHARP:
            q_sharp = st["best_q"].copy()
    # the re-seeded slot's best comes from after the re-seed (or it holds none)
    assert st["best_q"][RESEED_SLOT] == -1.0 or st["best_frame"][RESEED_SLOT] >= RESEED_BEFORE
    # a slot that was tracked on the sharp frame and not re-seeded kept that frame: the blurred ones never beat it
    for s in range(3):
        if s != RESEED_SLOT and q_sharp[s] > 0.0 and st["best_frame"][s] != -1:
            assert st["best_q"][s] >= q_sharp[s]


def test_update_resets_births_and_keeps_matches(mods, ring, model):
    """`update`: a slot born from a detection forgets its best with the next step; a slot whose track a detection
    confirms keeps it.  No synchronisation in `update`."""
    L, A, P = mods
    tr = P.FaceTracker(model, (RH, RW), 3, best_shot=A.BestShot(sharp_ref=1e6, min_exposed=0.25),
                       associate=A.TrackAssociation(square=False))
    tr.seed([0], [FACES[0]])
    tr.step(ring, SHARP)
    assert tr._best_reset.tolist() == [0, 0, 0] and tr.best_frame.tolist()[0] in (-1, 0)
    # slot 0's own box (IoU 1: a match, unless the step lost the track) and a box far from it (a birth into slot 1)
    own = tr.boxes[0].tolist()
    alive = own[2] > own[0] and own[3] > own[1]
    det = dev(np.asarray([own if alive else FACES[0], [70, 40, 120, 90]], np.int32))
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        _, slot_det, _ = tr.update(det)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    sd = slot_det.tolist()
    print("slot_det", sd, "alive", alive)
    assert sd[2] == -1 and (sd[:2] == [0, 1] if alive else sd[0] == 0 and sd[1] == 1)
    assert tr._best_reset.tolist() == [0 if alive else 1, 1, 0]          # births alone
    q0 = tr.best_q.clone()
    tr.step(ring, 0, frame_id=77)
    assert tr._best_reset.tolist() == [0, 0, 0]                           # the step has used the mask
    bq, bf = tr.best_q.tolist(), tr.best_frame.tolist()
    assert bq[2] == -1.0 and (bq[1] == -1.0 or bf[1] == 77)
    if alive:
        assert bq[0] >= float(q0[0])                                      # a confirmed track keeps its best
