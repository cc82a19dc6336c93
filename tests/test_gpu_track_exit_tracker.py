"""FaceTracker(exits=...) on the GPU: a scenario of eight ticks -- a seed, steps, an `update` that ends a duplicate and
starts a track, a track that is lost, a rebirth by the next `update`, a `step_active` / `step_live` tick (or, with one
stream, a `step_live` tick and a `retire()` on demand) in which the reborn slot is not served, a `seed` over that slot and
over a live one, and `retire(flush=True)` at the end -- on a synthetic ring with synthetic weights, once with one stream and
once with three.  After every tick the ring, the head and the ids equal tests/track_exit_ref.py applied to the state
downloaded before the tick; every exit's face is the gallery row as it was when its track ended; every started track
appears exactly once among exits, discards and overruns; ids are distinct and ascending in birth order; and a second
tracker without `exits` returns bit-identical step outputs and best() tensors on every tick.

Synthetic weights lose tracks at will, so the scenario pins what it needs between the ticks, on both trackers alike: the
slots it keeps alive get their box, matrix and status back, and a best shot of a known quality with random pixels."""
import numpy as np
import pytest
import torch

import track_exit_ref as xref

pytestmark = pytest.mark.gpu
RH, RW, CAP, Q = 270, 480, 9, 4
BOX = {0: (40, 30, 140, 130), 3: (200, 20, 290, 110), 4: (300, 120, 400, 220), 6: (60, 150, 150, 240)}
FAR1, FAR2, OVER0 = (330, 10, 400, 80), (170, 150, 250, 230), (20, 20, 120, 120)
OUTSIDE = 16


@pytest.fixture(scope="module")
def mods():
    import flm_amd  # noqa: F401
    from flm_amd import _lib, alignment, prediction
    _lib.load()
    return _lib, alignment, prediction


@pytest.fixture(scope="module")
def ring():
    rng = np.random.default_rng(31)
    return torch.from_numpy(rng.integers(0, 256, (8, RH, RW, 3), dtype=np.uint8)).cuda()


@pytest.fixture(scope="module")
def model():
    from flm_amd.networks import LANDMARKS_MODELS
    from flm_amd.weights import synth_fcn8_weights
    m = LANDMARKS_MODELS["fcn_8"](68, input_height=64, input_width=64, dtype="bf16")
    m.load_weights(synth_fcn8_weights(68, seed=2))
    return m


def view_bits(x):
    return x.view(torch.int64) if x.dtype == torch.float64 else x.view(torch.int32) if x.dtype == torch.float32 else x


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(view_bits(a), view_bits(b))


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[x.dtype.itemsize])


def as_bytes(t):
    return t.contiguous().view(torch.uint8).reshape(int(t.shape[0]), -1).cpu().numpy()


def download(tr):
    """The state of a tracker with exits as flm_track_retire will read it, in the names of tests/track_exit_ref.py."""
    g = lambda n: getattr(tr, n).cpu().numpy().copy()
    best_q = g("best_q")
    best_q[g("_exit_stale")] = -1.0          # a slot no step has served since its track was named holds no best of its own
    return dict(boxes=g("boxes"), status=g("status"), best_q=best_q, gallery=as_bytes(tr.gallery), best_frame=g("best_frame"),
                best_m=g("best_M"), best_lm=g("best_landmarks"), best_rec=g("best_rec"), born=g("_born"), track_id=g("track_id"),
                born_frame=g("born_frame"), head=g("exit_head"), x_gallery=as_bytes(tr.exit_faces), x_meta=g("exit_meta"),
                x_q=g("exit_q"), x_m=g("exit_M"), x_lm=g("exit_landmarks"), x_rec=g("exit_rec"), exit_row=g("exit_row"))


IN_OUT = ("born", "track_id", "born_frame", "head", "x_gallery", "x_meta", "x_q", "x_m", "x_lm", "x_rec", "exit_row")


@pytest.mark.parametrize("streams", [1, 3])
def test_the_exit_queue_over_a_scenario(mods, ring, model, streams):
    L, A, P = mods
    k = CAP // streams
    mk = lambda **kw: P.FaceTracker(model, (RH, RW), CAP, best_shot=A.BestShot(sharp_ref=1e6, min_exposed=0.25), weights="score",
                                    associate=A.TrackAssociation(square=False), streams=streams, **kw)
    ex, plain = mk(exits=Q), mk()
    both = (ex, plain)
    rng = np.random.default_rng(7 + streams)
    keep = {}                                # slot -> the box the scenario keeps it alive with
    started, exits, discards, overruns = [], [], [], []
    face_shape = None

    def pin(t):
        """Between two ticks, on both trackers alike: the kept slots live on, with a best shot of a known quality."""
        for slot, box in keep.items():
            b = torch.tensor([box], dtype=torch.int32, device="cuda")
            m, st = A.track_seed_device(b, (64, 64), (RH, RW))
            face = torch.from_numpy(rng.standard_normal(face_shape).astype(np.float32)).cuda()
            for tr in both:
                tr.boxes[slot], tr.m_crop[slot], tr.status[slot] = b[0], m[0], st[0]
                tr.best_q[slot] = 0.3 + 0.01 * slot + 0.001 * t
                tr.best_frame[slot] = 100 + t
                tr.gallery[slot] = face

    def update(stream, dets):
        out = None
        for tr in both:
            out = tr.update(dets if streams == 1 else [dets if i == stream else None for i in range(streams)])
        return out

    def tick(t, how, flush=False, **kw):
        """One tick on both trackers; the exits against the restatement on the state downloaded before it."""
        fid = 100 + t
        s = download(ex)
        pre = {n: v.copy() for n, v in s.items()}
        out = xref.retire(s, RH, RW, frame_id=fid, flush=flush, min_q=0.0)
        fi = [(3 * t + 2 * i + 1) % 8 for i in range(streams)]
        fi = fi[0] if streams == 1 and how == "step" else fi
        res = []
        for tr in both:
            if how == "step":
                res.append(tr.step(ring, fi, frame_id=fid))
            elif how == "active":
                res.append(tr.step_active(ring, fi, frame_id=fid, **kw))
            elif how == "live":
                res.append(tr.step_live(ring, fi, frame_id=fid, **kw))
            elif tr is ex:
                head = tr.retire(flush=flush, frame_id=fid)
                assert head is tr.exit_head
        if res:
            assert len(res[0]) == len(res[1])
            for a, b in zip(*res):                                     # the step's returns: the bits of a tracker without exits
                assert same(a, b), (t, how)
            for a, b in zip(ex.best(), plain.best()):
                assert same(a, b), (t, how)
            for n in ("m_crop", "boxes", "status", "_best_reset", "best_rec"):
                assert same(getattr(ex, n), getattr(plain, n)), (n, t, how)
        post = download(ex)
        for n in IN_OUT:
            assert np.array_equal(bits(post[n]), bits(s[n])), (n, t, how)
        faces, meta, xq, xm, xlm, head = ex.exits()
        assert faces is ex.exit_faces and meta is ex.exit_meta and head is ex.exit_head and same(ex.track_id, torch.from_numpy(s["track_id"]).cuda())
        for slot in np.flatnonzero(out["written"]):                    # the face is the gallery row as it was when the track ended
            row = int(post["exit_row"][slot])
            assert np.array_equal(post["x_gallery"][row], pre["gallery"][slot]) and post["x_q"][row] == pre["best_q"][slot]
            assert post["x_meta"][row, 0] == pre["track_id"][slot] and post["x_meta"][row, 1] == slot and post["x_meta"][row, 3] == fid
            exits.append((int(pre["track_id"][slot]), int(post["x_meta"][row, 5])))
        discards.extend(int(v) for v in pre["track_id"][post["exit_row"] == -2])
        overruns.extend(int(v) for v in pre["track_id"][post["exit_row"] == -3])
        started.extend(int(v) for v in post["track_id"][out["births"]])
        print("tick", t, how, "exit_row", post["exit_row"].tolist(), "ids", post["track_id"].tolist(), "head", post["head"].tolist())
        return out, post

    with pytest.raises(ValueError, match="exits"):
        plain.exits()
    # ---- tick 0: four tracks begin
    for tr in both:
        tr.seed(list(BOX), list(BOX.values()))
    face_shape = tuple(ex.gallery.shape[1:])
    assert ex.track_id.tolist() == [-1] * CAP and ex.exit_head.tolist() == [0, 0, 0, 0]
    out, post = tick(0, "step")
    assert post["track_id"].tolist() == [0, -1, -1, 1, 2, -1, 3, -1, -1] and out["E"] == 0     # ascending slot, from 0
    keep.update(BOX)
    pin(0)
    # ---- tick 1: a second track on the face of slot 0 begins in slot 2
    for tr in both:
        tr.seed([2], [BOX[0]])
    out, post = tick(1, "step")
    assert post["track_id"][2] == 4 and out["E"] == 0
    keep[2] = BOX[0]
    pin(1)
    # ---- tick 2: the update ends the duplicate in slot 2 and starts a track from the other detection in slot 1, the one
    # slot of stream 0 that held no face (a slot killed in a call is not reused in it)
    det_slot, slot_det, _ = update(0, [BOX[0], FAR1])
    assert det_slot.reshape(-1)[:2].tolist() == [0, 1] and int(ex.status[2]) == L.TRACK_DUPLICATE
    new1 = 1
    del keep[2]
    out, post = tick(2, "step")
    assert out["E"] == 1 and post["exit_row"][2] >= 0                  # the duplicate's track: queued with its best shot
    row = post["exit_row"][2]
    assert post["x_meta"][row].tolist()[:2] == [4, 2] and post["x_meta"][row, 5] == L.TRACK_DUPLICATE
    assert post["track_id"][new1] == 5 and post["track_id"][2] == -1
    keep[new1] = FAR1
    pin(2)
    # ---- tick 3: the track of slot 3 leaves the frame and is lost
    for tr in both:
        tr.boxes[3], tr.status[3] = 0, OUTSIDE
    del keep[3]
    out, post = tick(3, "step")
    assert out["E"] == 1 and post["exit_row"][3] >= 0 and post["x_meta"][post["exit_row"][3]].tolist()[:2] == [1, 3]
    assert post["x_meta"][post["exit_row"][3], 5] == OUTSIDE            # why it was lost, as the retire call found it
    assert post["track_id"][3] == -1
    pin(3)
    # ---- tick 4: the next update starts a track in the lowest free slot (of stream 1: the lost track's own slot); the
    # tick does not serve it
    det_slot, _, _ = update(1 if streams > 1 else 0, [FAR2])
    reborn = int(det_slot.reshape(-1)[0]) if streams == 1 else int(det_slot[1][0])
    assert reborn == (2 if streams == 1 else 3) and reborn not in keep
    if streams == 1:
        out, post = tick(4, "live", budget=1)                          # the one row goes to slot 0
    else:
        out, post = tick(4, "active", active=[0])
    first_id = int(post["track_id"][reborn])
    assert first_id == 6 and int(ex._best_reset[reborn]) == 1 and bool(ex._exit_stale[reborn])
    keep[reborn] = FAR2
    pin(4)
    # ---- tick 5: another tick that does not serve it
    if streams == 1:
        out, post = tick(5, "retire")
    else:
        out, post = tick(5, "live", budget=CAP, active=[0, 2])
    assert out["E"] == 0 and post["track_id"][reborn] == first_id and int(ex._best_reset[reborn]) == 1
    pin(5)
    # ---- tick 6: a seed over the slot no step has served, and over the live slot 0
    for tr in both:
        tr.seed([0, reborn], [OVER0, FAR2])
    out, post = tick(6, "step")
    assert post["exit_row"][reborn] == -2 and first_id in discards      # it never had a best shot of its own
    assert post["exit_row"][0] >= 0 and post["x_meta"][post["exit_row"][0]].tolist()[:2] == [0, 0]
    assert post["x_meta"][post["exit_row"][0], 5] == -1                 # restarted before its end was seen
    assert sorted(post["track_id"][[0, reborn]].tolist()) == [7, 8] and not ex._exit_stale.any()
    keep[0] = OVER0
    pin(6)
    # ---- tick 7: the end of the video
    out, post = tick(7, "retire", flush=True)
    assert (post["track_id"] == -1).all() and out["E"] == len(keep) and post["head"][3] == max(len(keep) - Q, 0)
    assert all(end == -2 for _, end in exits[-min(len(keep), Q):])
    # ---- every started track exactly once; ids distinct and ascending in birth order
    assert started == list(range(len(started))) == list(range(int(post["head"][1]))) and len(started) == 9
    ended = [i for i, _ in exits] + discards + overruns
    assert sorted(ended) == started, (exits, discards, overruns)
    assert post["head"].tolist() == [len(exits) + len(overruns), len(started), len(discards), len(overruns)]
    rows, lost = A.exit_rows(int(post["head"][0]), 0, Q)               # a consumer that looks only now
    assert lost == post["head"][0] - Q and [int(post["x_meta"][r, 6]) for r in rows] == list(range(lost, int(post["head"][0])))
