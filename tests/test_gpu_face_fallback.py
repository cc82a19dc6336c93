"""fallback_faces: the candidate path redoes only the faces whose lists fail (flm_fallback_opts).

fcn_8, 68 classes, weights and crops of tests/peaked_cases.py, 96 x 160 crops (104 x 168 maps), 3 to 7 faces per batch
(leg 8: 9 faces of 256 x 256).  Every leg runs `_check`, which compares with the materialised path
(landmark_candidates = 0) bit for bit -- NaN and (-1, -1) in the same places -- and holds the bookkeeping against what
the test computes itself from cand_redo:

    R = the number of flags set;  fallback_counts = {R, R if R <= B else 0, R > B, B}  (B = min(budget, n))
    fallback_rows = the flagged faces ascending (the first B of them when R > B), then -1
    cand_redo is all zero exactly when cand_cnt[n] is 0
    the "probs" region, NaN before the call: untouched when R = 0; when 0 < R <= B row r < R holds the "probs" forward of
    face fallback_rows[r] bit for bit and every row from R on is still NaN; when R > B all n rows are written
    (not looked at under up3_wreg = 1, which uses the region as scratch)

Legs: 1 clear batch; 2 an overflow in a proper subset (candidate_cap_div between the fills); 3 budgets; 4 every raising
kernel, with cand_redo containing {cnt > cap} and every face that has a class with fewer than n_points non-zero pixels;
5 the merge site (a class dead in every face, and a class dead in two faces of five); 6 records; 7 workspace reuse; 8 faces ending inside workgroups; 9 the tracker.
Without the feature every leg fails at the missing entry point (flm_fcn_forward_fb / the fallback_faces argument).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import peaked_cases as P

pytestmark = pytest.mark.gpu

MAT = dict(landmark_candidates=0)
_BASE, _MODELS, _REF = {}, {}, {}
KERNELS = {"cand8": dict(up3_cand8=3), "generic": dict(up3_cand8=0), "cand8 rows=8": dict(up3_cand8=3, up3_cand8_rows=8),
           "wreg": dict(up3_wreg=1)}


@pytest.fixture(scope="module")
def lib():
    import flm_amd  # noqa: F401
    from flm_amd import _lib
    _lib.load()
    return _lib


def _model(name, dtype, h=96, w=160):
    if (name, dtype, h, w) not in _MODELS:
        from flm_amd.networks import LANDMARKS_MODELS
        from flm_amd.weights import synth_fcn8_weights
        if not _BASE:
            _BASE["w"] = synth_fcn8_weights(68, seed=2)
        m = LANDMARKS_MODELS["fcn_8"](68, input_height=h, input_width=w, dtype=dtype)
        m.load_weights(P.case_weights(_BASE["w"], name))
        _MODELS[(name, dtype, h, w)] = m
    return _MODELS[(name, dtype, h, w)]


def _crops(key):
    """The batches of the legs, built once: "3" the case batch (face 1 blank), "4" four faces with 0, 1, 3 blank, "7" seven
    faces with 2 and 5 blank, "9x256" nine 256 x 256 faces with 1, 4 and 8 blank."""
    if key not in _REF:
        n, h, w = P.SHAPE
        _REF[key] = torch.from_numpy({"3": lambda: P.case_crops(),
                                      "4": lambda: P.crops(4, h, w, seed=P.SEED + 1, blank=(0, 1, 3)),
                                      "7": lambda: P.crops(7, h, w, seed=P.SEED + 3, blank=(2, 5)),
                                      "9x256": lambda: P.crops(9, 256, 256, seed=P.SEED + 4, blank=(1, 4, 8))}[key]()).cuda()
    return _REF[key]


def _reference(model, name, dtype, key, n_points, thresh, out):
    """The materialised path's result and the "probs" forward of a batch, computed once and left unchanged (CUDA)."""
    k = (name, dtype, key, n_points, thresh, out)
    if k not in _REF:
        _REF[k] = model.forward_device(_crops(key), out, n_points=n_points, thresh=thresh, opts=MAT).clone()
    pk = (name, dtype, key, "probs")
    if pk not in _REF:
        _REF[pk] = model.forward_device(_crops(key), "probs").clone()
    return _REF[k], _REF[pk]


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _check(lib, name, dtype, key, n_points, budget, opts=None, thresh=0.0, out="landmarks", look_at_probs=True, ws=None,
           hw=(96, 160)):
    """One forward with fallback_faces = budget into a workspace whose "probs" region is NaN; returns what it read."""
    L = lib.load()
    model = _model(name, dtype, *hw)
    xd = _crops(key)
    n = int(xd.shape[0])
    ref, probs_ref = _reference(model, name, dtype, key, n_points, thresh, out)
    if ws is None:
        ws = model.new_workspace(n, out, n_points, opts, fallback_faces=budget)
    fo, fb = model._opts(opts), lib.FallbackOpts.make(budget)
    om = lib.OUT_LANDMARKS_STATS if out == "landmark_stats" else lib.OUT_LANDMARKS

    def off(nm):
        return L.flm_fcn_workspace_offset_fb(model._arch, nm, n, hw[0], hw[1], 68, model._dt, om, lib.DECODE_TOPN, n_points,
                                             C.byref(fo), C.byref(fb))
    px = (hw[0] + 8) * (hw[1] + 8)
    region = ws[off(b"probs"):off(b"probs") + 4 * n * px * 68].view(torch.float32).view(n, px, 68)
    region.fill_(float("nan"))
    got = model.forward_device(xd, out, n_points=n_points, thresh=thresh, opts=opts, workspace=ws, fallback_faces=budget)
    counts = model.fallback_counts(ws).cpu().numpy().astype(np.int64)
    rows_t, redo_t = model.fallback_rows(ws)
    rows, redo = rows_t.cpu().numpy(), redo_t.cpu().numpy()
    cap = int(off(b"cand_cap"))
    cnt = ws[off(b"cand_cnt"):off(b"cand_cnt") + 4 * (n + 1)].view(torch.int32).cpu().numpy().astype(np.int64)
    B = min(budget, n)
    label = "%s %s batch %s n_points=%d B=%d %s" % (name, dtype, key, n_points, budget, opts or "")
    assert _bits_equal(got, ref), (label, "landmarks differ from the materialised path")
    assert set(np.unique(redo)) <= {0, 1}
    faces = np.nonzero(redo)[0]
    R = len(faces)
    print("%s: R = %d of %d %s, fills %s of %d, flag %d, counts %s" % (label, R, n, faces.tolist(), cnt[:n].tolist(), cap,
                                                                      cnt[n], counts.tolist()))
    assert (R == 0) == (cnt[n] == 0), (label, "cand_redo and cand_cnt[n] disagree")
    assert counts.tolist() == [R, R if R <= B else 0, int(R > B), B], (label, counts.tolist())
    assert rows.tolist() == (faces[:B].tolist() + [-1] * B)[:B], (label, rows.tolist())
    assert set(np.nonzero(cnt[:n] > cap)[0]) <= set(faces), (label, "an overflowing face is not flagged")
    if look_at_probs:
        nan_rows = torch.isnan(region).all(dim=2).all(dim=1).cpu().numpy()
        if R == 0:
            assert nan_rows.all(), (label, "the probability region was written")
        elif R <= B:
            assert _bits_equal(region[:R], probs_ref[torch.from_numpy(faces).cuda()]), (label, "compact rows differ from probs")
            assert nan_rows[R:].all() and not nan_rows[:R].any(), (label, nan_rows.tolist())
        else:
            assert _bits_equal(region, probs_ref), (label, "whole-batch redo differs from probs")
    return dict(R=R, faces=faces, cnt=cnt[:n], flag=int(cnt[n]), cap=cap, counts=counts, rows=rows, ws=ws, got=got,
                probs_ref=probs_ref, label=label)


# ---- 1 -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ("f32", "bf16"))
def test_clear_batch_touches_nothing(lib, dtype):
    r = _check(lib, "scaled4", dtype, "3", 4, 2)
    assert r["R"] == 0 and r["counts"].tolist() == [0, 0, 0, 2]


# ---- 2, 3 ----------------------------------------------------------------------------------------------------------------

DIV5 = dict(candidate_cap_div=5)   # fills 16896 / 10129 / 17461 of 69,632: a fifth of the capacity separates them


@pytest.mark.parametrize("key", ("3", "4"))
def test_overflow_in_a_proper_subset(lib, key):
    n = int(_crops(key).shape[0])
    r = _check(lib, "bilinear128", "f32", key, 4, n, DIV5)
    expected = np.nonzero(r["cnt"] > r["cap"])[0]
    assert 0 < len(expected) < n, "choose another divisor: fills %s, capacity %d" % (r["cnt"].tolist(), r["cap"])
    # no other site can raise here: fp32, no dead class
    assert r["faces"].tolist() == expected.tolist()
    assert r["rows"].tolist() == expected.tolist() + [-1] * (n - len(expected))


@pytest.mark.parametrize("budget", (1, 2, 3, 10 ** 6))
def test_budgets(lib, budget):
    r = _check(lib, "bilinear128", "f32", "3", 4, budget, DIV5)
    assert r["R"] == 2, "choose another divisor"
    want = {1: [2, 0, 1, 1], 2: [2, 2, 0, 2], 3: [2, 2, 0, 3], 10 ** 6: [2, 2, 0, 3]}[budget]
    assert r["counts"].tolist() == want


# ---- 4 -------------------------------------------------------------------------------------------------------------------

def _short_faces(probs_ref, n_points):
    """Faces in which some class has fewer than n_points pixels with p > 0 in the materialised probabilities."""
    nz = (probs_ref > 0).sum(dim=1)                      # [n, 68]
    return set(np.nonzero((nz < n_points).any(dim=1).cpu().numpy())[0].tolist())


@pytest.mark.parametrize("kernel", list(KERNELS))
@pytest.mark.parametrize("n_points", (4, 25))
@pytest.mark.parametrize("name", ("bilinear32", "bilinear128"))
def test_every_raising_kernel(lib, name, n_points, kernel):
    with lib.tuning(**KERNELS[kernel]):
        r = _check(lib, name, "bf16", "7", n_points, 4, look_at_probs=kernel != "wreg")
    short = _short_faces(r["probs_ref"], n_points)
    print("%s %s: faces with a class short of %d non-zero pixels: %s" % (r["label"], kernel, n_points, sorted(short)))
    assert short <= set(r["faces"].tolist())
    if kernel.startswith("cand8"):   # the lane lists drop keys on these maps (tests/test_gpu_peaked_maps.py: "short")
        assert r["R"] > 0, "nothing raised: the leg checks nothing"


@pytest.mark.parametrize("kernel", list(KERNELS))
def test_overflow_through_every_kernel(lib, kernel):
    with lib.tuning(**KERNELS[kernel]):
        r = _check(lib, "bilinear32", "bf16", "3", 4, 3, dict(candidate_cap_div=64), look_at_probs=kernel != "wreg")
    assert r["R"] == 3 and (r["cnt"] > r["cap"]).all()


# ---- 5 -------------------------------------------------------------------------------------------------------------------

def test_merge_site_dead_class(lib):
    """Every face raises at cand_merge_kernel's "fewer than n keys" check.  A dead class is dead in EVERY face, so this leg
    cannot show a wrong face index at the merge site on its own; the containment check of test_every_raising_kernel is
    empty on these weights (no class is short there).  test_merge_site_flags_the_right_faces is the cover."""
    r = _check(lib, "bilinear32dead", "f32", "3", 4, 3)
    assert r["R"] == 3 and r["counts"].tolist() == [3, 3, 0, 3]
    assert not (r["cnt"] > r["cap"]).any()
    r = _check(lib, "bilinear32dead", "f32", "3", 4, 2)
    assert r["counts"].tolist() == [3, 0, 1, 2]


def _brightness_weights():
    """bilinear32 weights in which class P.DEAD is dead in BRIGHT faces only.  Output channel 0 of enc1..enc3 is turned
    into a brightness detector -- centre tap only (enc1: the mean of the three colours; enc2, enc3: channel 0), identity
    BatchNorm -- so f3[0] = the max-pooled ReLU of (pixel - mean): at least 70 at every position of a crop whose pixels
    are all >= 200, exactly 0 at every position of a crop whose pixels are all <= 50 (no padding effect: one tap).
    score3 takes -1000 x f3[0] into class P.DEAD: at least 7e4 below the rest in a bright face, even at a corner pixel,
    where the bilinear taps sum to 32 / 256 (a gap of 8,750: exp() is 0) -- and nothing at all in a dark face."""
    w = dict(P.case_weights(_BASE["w"], "bilinear32"))
    for i in (1, 2, 3):
        k = np.array(w["enc%d/kernel" % i], copy=True)
        k[:, :, :, 0] = 0.0
        if i == 1:
            k[1, 1, :, 0] = 1.0 / 3.0
        else:
            k[1, 1, 0, 0] = 1.0
        w["enc%d/kernel" % i] = k
        for t, v in (("bias", 0.0), ("gamma", 1.0), ("beta", 0.0), ("moving_mean", 0.0), ("moving_variance", 1.0)):
            a = np.array(w["enc%d/%s" % (i, t)], copy=True)
            a[0] = v
            w["enc%d/%s" % (i, t)] = a
    k = np.array(w["score3/kernel"], copy=True)
    k[0, 0, 0, P.DEAD] -= 1000.0
    w["score3/kernel"] = k
    return w


def test_merge_site_flags_the_right_faces(lib):
    """A class that is short of n keys in SOME faces only: P.DEAD is exactly 0 in the bright faces 1 and 3 of a batch of
    five and alive in the dark faces 0, 2, 4 (_brightness_weights).  fp32 through the generic kernel has no lane lists and
    the lists stay far inside their capacity, so cand_merge_kernel's "fewer than n keys" check is the only site that
    raises: cand_redo must be exactly {1, 3} -- a wrong face index there would flag another face or miss one."""
    from flm_amd.networks import LANDMARKS_MODELS
    _model("bilinear32", "f32")   # (fills _BASE)
    if ("brightness", "f32", 96, 160) not in _MODELS:
        m = LANDMARKS_MODELS["fcn_8"](68, input_height=96, input_width=160, dtype="f32")
        m.load_weights(_brightness_weights())
        _MODELS[("brightness", "f32", 96, 160)] = m
    if "5bright" not in _REF:
        rng = np.random.default_rng(P.SEED + 5)
        img = rng.integers(0, 51, (5, 96, 160, 3), dtype=np.uint8)
        for f in (1, 3):
            img[f] = rng.integers(200, 256, (96, 160, 3), dtype=np.uint8)
        _REF["5bright"] = torch.from_numpy(img).cuda()
    for budget in (5, 2, 1):
        r = _check(lib, "brightness", "f32", "5bright", 4, budget)
        short = _short_faces(r["probs_ref"], 4)
        dead = (r["probs_ref"][:, :, P.DEAD] > 0).sum(dim=1).cpu().tolist()
        print("%s: non-zero pixels of class %d per face %s, short faces %s" % (r["label"], P.DEAD, dead, sorted(short)))
        assert short == {1, 3}, "the construction no longer gives a class that is short in faces 1 and 3 only"
        assert not (r["cnt"] > r["cap"]).any()
        assert r["faces"].tolist() == [1, 3]
        assert (r["got"][[1, 3], P.DEAD] == -1).all().item() and not (r["got"][[0, 2, 4], P.DEAD] == -1).any().item()


# ---- 6 -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("leg", ("overflow f32", "short bf16"))
def test_records(lib, leg):
    from flm_amd.utils.metrics import decode_stats_device
    if leg == "overflow f32":
        r = _check(lib, "bilinear128", "f32", "3", 4, 3, DIV5, out="landmark_stats")
    else:
        r = _check(lib, "bilinear32", "bf16", "7", 4, 4, out="landmark_stats")
    assert 0 < r["R"]
    n = r["probs_ref"].shape[0]
    exp = decode_stats_device(r["probs_ref"].view(n, 104, 168, 68).contiguous(), 4, 0.0)
    assert _bits_equal(r["got"], exp), leg


# ---- 7 -------------------------------------------------------------------------------------------------------------------

def test_workspace_reuse(lib):
    # one workspace, sized for the default options (the larger layout; a forward only asks for room enough): first the
    # batch of leg 2 with its divisor, then the clear batch with the default capacity -- other weights, another layout
    ws = _model("scaled4", "f32").new_workspace(3, "landmarks", 4, None, fallback_faces=2)
    first = _check(lib, "bilinear128", "f32", "3", 4, 2, DIV5, ws=ws)
    assert first["R"] == 2
    r = _check(lib, "scaled4", "f32", "3", 4, 2, ws=ws)
    assert r["counts"].tolist() == [0, 0, 0, 2] and r["rows"].tolist() == [-1, -1]


def test_the_model_does_not_keep_a_workspace_alive(lib):
    """fallback_counts finds a caller-owned workspace through a weak reference: dropping the workspace frees its memory."""
    import gc
    model = _model("bilinear128", "f32")
    xd = _crops("3")
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    ws = model.new_workspace(3, "landmarks", 4, DIV5, fallback_faces=2)
    size = ws.numel()
    model.forward_device(xd, "landmarks", n_points=4, opts=DIV5, workspace=ws, fallback_faces=2)
    assert model.fallback_counts(ws).cpu().tolist() == [2, 2, 0, 2]
    key = id(ws)
    assert key in model._fb_last
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() >= before + size
    del ws
    gc.collect()
    assert key not in model._fb_last
    assert torch.cuda.memory_allocated() < before + size, "the dropped workspace is still allocated"
    other = torch.empty(16, dtype=torch.uint8, device="cuda")
    with pytest.raises(KeyError):
        model.fallback_counts(other)


# ---- 8 -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("budget", (4, 9))
def test_faces_end_inside_workgroups(lib, budget):
    """256 x 256: 33 x 33 = 1089 positions per face against workgroups of 128, so rows of the compact launch begin and end
    inside workgroups, the last live row's as well."""
    r = _check(lib, "bilinear32", "bf16", "9x256", 4, budget, hw=(256, 256))
    assert r["R"] > 0


# ---- 9 -------------------------------------------------------------------------------------------------------------------

def test_tracker_returns_the_same_bits(lib):
    import scenario as sc
    from flm_amd import prediction
    S = sc.Script()
    ring = torch.from_numpy(S.frames()).cuda()
    model = _model("bilinear32", "bf16", sc.IN, sc.IN)
    runs = []
    for fb in (0, 4, 8):   # (4: the issue's budget; 8 = the capacity, so the per-face path serves every step as well)
        tr = prediction.FaceTracker(model, (sc.FH, sc.FW), sc.CAP, out_size=(sc.OUT, sc.OUT), streams=sc.STREAMS, samples=1,
                                    fallback_faces=fb)
        steps = []
        for t in range(3):
            if t == 0:
                tr.update(S.detections(t)[0])
            res = tr.step(ring, [S.ring_slot(s, t) for s in range(sc.STREAMS)])
            steps.append([x.clone() for x in res[:4]] + [tr.m_crop.clone()])
            if fb:
                print("tracker step %d: fallback_counts %s" % (t, model.fallback_counts(tr._ws_active).cpu().tolist()))
        runs.append(steps)
    for other in runs[1:]:
        for t, (a, b) in enumerate(zip(runs[0], other)):
            for x, y in zip(a, b):
                assert x.dtype == y.dtype and torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8)), t
