"""GPU parity of the filtered track step: flm_track_step_filtered against tests/track_filter_ref.py (the header's
arithmetic in numpy float64) over sequences of frames, bit for bit on all seven outputs at every step; its two identities
against flm_track_step on the device; prediction.FaceTracker(smooth=True) against the same sequence made by hand.
Every comparison is exact: each operation is one IEEE float64 operation on both sides.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import track_filter_cases as cases
import track_filter_ref

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
IN, GRID, FH, FW, SC, DT = cases.IN, cases.GRID, cases.FH, cases.FW, cases.SC, cases.DT
KS, CS = (1, 3, 70), (1, 5, 68, 130)      # C = 130: the thread loop takes three rounds (two full ones and a tail of 2)
SEVEN = ("lm_frame", "m_align", "m_next", "boxes_next", "status", "state", "lm_raw")
FIVE = SEVEN[:5]


@pytest.fixture(scope="module")
def mods():
    import flm_amd  # noqa: F401
    from flm_amd import _lib, alignment, prediction
    _lib.load()
    return _lib, alignment, prediction


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def bits_equal(got, exp):
    """Bit equality of a CUDA tensor and a numpy array of the same type (NaNs and signed zeros compare by their bits)."""
    got = got.cpu().numpy()
    assert got.dtype == exp.dtype and got.shape == exp.shape, (got.dtype, exp.dtype, got.shape, exp.shape)
    u = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    return np.array_equal(np.ascontiguousarray(got).view(u), np.ascontiguousarray(exp).view(u))


_SEQ = {}


def sequence(k, c, weighted, **kw):
    """The reference's closed loop, computed once per case and left unchanged."""
    key = (k, c, weighted, tuple(sorted(kw.items())))
    if key not in _SEQ:
        _SEQ[key] = cases.sequence(k, c, weighted, **kw)
    return _SEQ[key]


class Chain:
    """The device side of one sequence: the tracker's buffers (m_next / boxes_next aliased onto m_crop / boxes, the state
    in place), stepped through ctypes.  Before each step the host puts into the buffers what the sequence changed by hand
    (the poisoned entry, the re-seeded faces); everything else is what the previous launch left there."""

    def __init__(self, L, seq, stride, align, raw, filt=None):
        s0 = seq["steps"][0]
        self.L, self.seq, self.stride, self.align, self.filt = L, seq, stride, align, filt
        self.k, self.c = seq["k"], seq["c"]
        self.m, self.boxes, self.state = dev(s0["m_crop"]), dev(s0["boxes"]), dev(s0["state"])
        self.tc, self.ta = dev(seq["tc"]), dev(seq["ta"])
        k, c = self.k, self.c
        self.out = dict(lm_frame=torch.full((k, c, 2), 777.0, dtype=torch.float64, device="cuda"),
                        m_align=torch.full((k, 2, 3), 777.0, dtype=torch.float32, device="cuda") if align else None,
                        m_next=self.m, boxes_next=self.boxes,
                        status=torch.full((k,), 777, dtype=torch.int32, device="cuda"), state=self.state,
                        lm_raw=torch.full((k, c, 2), 777.0, dtype=torch.float64, device="cuda") if raw else None)

    def step(self, t, filtered=True):
        L, k, c, stride, o = self.L, self.k, self.c, self.stride, self.out
        s = self.seq["steps"][t]
        if t:                                                       # what the host changed between two steps
            prev = self.seq["steps"][t - 1]["exp"]
            for name, buf in (("state", self.state), ("m_crop", self.m), ("boxes", self.boxes)):
                was = prev[{"m_crop": "m_next", "boxes": "boxes_next"}.get(name, name)]
                rows = [f for f in range(k) if not np.array_equal(s[name][f], was[f], equal_nan=name == "state")]
                for f in rows:
                    buf[f] = dev(s[name][f])
        rng = np.random.default_rng(5 + t)
        rec = rng.uniform(-3, 99, (k, c, stride))                   # junk in the columns nobody may read
        rec[..., :2] = s["lm"]
        w_d, ws = None, 1
        if s["w"] is not None:
            if stride > 2:
                rec[..., 2] = s["w"]
            rec_d = dev(rec)
            w_d, ws = (rec_d.view(-1)[2:], stride) if stride > 2 else (dev(s["w"]), 1)
        else:
            rec_d = dev(rec)
        opts = L.TrackOpts.make()
        args = (L.stream_ptr(), L.ptr(rec_d), stride, None if w_d is None else L.ptr(w_d), ws, L.ptr(self.m), L.ptr(self.boxes),
                k, c, SC, SC, IN, IN, FH, FW, L.ptr(self.tc), L.ptr(self.ta) if self.align else None, C.byref(opts),
                L.ptr(o["lm_frame"]), None if o["m_align"] is None else L.ptr(o["m_align"]), L.ptr(self.m), L.ptr(self.boxes),
                L.ptr(o["status"]))
        if filtered:
            fo = L.TrackFilter.make(**(self.filt or track_filter_ref.DEFAULTS))
            L.check(L.load().flm_track_step_filtered(*args, C.byref(fo), DT, L.ptr(self.state),
                                                     None if o["lm_raw"] is None else L.ptr(o["lm_raw"])),
                    "flm_track_step_filtered")
        else:
            L.check(L.load().flm_track_step(*args), "flm_track_step")
        return o


@pytest.mark.parametrize("c", CS)
@pytest.mark.parametrize("k", KS)
def test_filtered_step_matches_the_reference_over_a_sequence(mods, k, c):
    L, A, P = mods
    for weighted in (False, True):
        seq = sequence(k, c, weighted)
        for stride in (2, 6):
            for align in (True, False):
                for raw in (True, False):
                    ch = Chain(L, seq, stride, align, raw)
                    for t, s in enumerate(seq["steps"]):
                        got = ch.step(t)
                        for name in SEVEN:
                            if got[name] is not None:
                                assert bits_equal(got[name], s["exp"][name]), (name, t + 1, weighted, stride, align, raw)
    # the filter did something: from step 2 on most points of a living face are not where the raw ones are
    if c >= 5:
        e = seq["steps"][1]["exp"]
        assert (e["lm_frame"][0] != e["lm_raw"][0]).any()


@pytest.mark.parametrize("c", CS)
@pytest.mark.parametrize("k", KS)
def test_without_history_and_with_an_infinite_cutoff_it_is_the_plain_step(mods, k, c):
    L, A, P = mods
    for weighted in (False, True):
        # an empty state at every step of the default sequence: the five outputs of flm_track_step
        seq = sequence(k, c, weighted)
        for t in range(len(seq["steps"])):
            got = {}
            for filtered in (True, False):
                ch = Chain(L, seq, 6, True, True)
                ch.seq = dict(seq, steps=seq["steps"][t:])
                ch.m, ch.boxes = dev(seq["steps"][t]["m_crop"]), dev(seq["steps"][t]["boxes"])
                ch.out.update(m_next=ch.m, boxes_next=ch.boxes)
                ch.state.fill_(-1.0)
                got[filtered] = {n: v.clone() for n, v in ch.step(0, filtered).items() if v is not None}
            for name in FIVE:
                assert torch.equal(got[True][name].view(torch.uint8), got[False][name].view(torch.uint8)), (name, t + 1)
            assert torch.equal(got[True]["lm_raw"].view(torch.uint8), got[False]["lm_frame"].view(torch.uint8))
        # min_cutoff = +inf over 4 chained steps: the chain of flm_track_step
        inf = dict(min_cutoff=float("inf"), beta=15.0, d_cutoff=1.0)
        seq = sequence(k, c, weighted, steps=4, filt=tuple(sorted(inf.items())))
        a, b = Chain(L, seq, 2, True, False, filt=inf), Chain(L, seq, 2, True, False)
        histories = 0
        for t in range(4):
            histories += int((a.state[..., 0] >= 0).sum())
            ga, gb = a.step(t, True), b.step(t, False)
            for name in FIVE:
                assert torch.equal(ga[name].view(torch.uint8), gb[name].view(torch.uint8)), (name, t + 1)
                assert bits_equal(ga[name], seq["steps"][t]["exp"][name])
        if c >= 5:
            assert histories > 0                        # (the filter ran with a history, and changed nothing)


# ---- FaceTracker(smooth=True) against the sequence made by hand -------------------------------------------------------
RH, RW, CAP = 64, 96, 3
FACES = [(20, 8, 60, 50), (40, 2, 90, 60), (-6, 20, 30, 58)]
RESEED = (1, (36, 4, 84, 56))                              # after step 2: slot 1 from a new detector box


@pytest.fixture(scope="module")
def ring():
    """Four frames of one textured scene that drifts by a pixel a frame, with fresh noise on each."""
    rng = np.random.default_rng(31)
    big = rng.integers(0, 256, (RH + 8, RW + 8, 3)).astype(f64)
    frames = [np.clip(big[t:t + RH, t:t + RW] + rng.integers(-2, 3, (RH, RW, 3)), 0, 255).astype(np.uint8) for t in range(4)]
    return dev(np.stack(frames))


@pytest.fixture(scope="module")
def model():
    from flm_amd.networks import LANDMARKS_MODELS
    from flm_amd.weights import synth_fcn8_weights
    m = LANDMARKS_MODELS["fcn_8"](68, input_height=64, input_width=64, dtype="bf16")
    m.load_weights(synth_fcn8_weights(68, seed=2))
    return m


def test_face_tracker_smooth_is_the_sequence_made_by_hand(mods, ring, model):
    L, A, P = mods
    tr = P.FaceTracker(model, (RH, RW), CAP, smooth=True)
    assert tr.filter_state is None
    tr.seed(range(CAP), FACES)
    assert tuple(tr.filter_state.shape) == (CAP, 68, 6) and tr.filter_state.dtype == torch.float64
    assert (tr.filter_state == -1).all()
    # by hand: the public pieces, nothing aliased
    filt = A.LandmarkFilter()
    sq = dev(np.asarray(P.face_boxes([list(b) for b in FACES]), np.int32))
    m, _ = A.track_seed_device(sq, (64, 64), (RH, RW))
    boxes = sq.clone()
    state = torch.full((CAP, 68, 6), -1.0, dtype=torch.float64, device="cuda")
    tc, ta = dev(A.canonical_template(68, 64, 64)), dev(A.canonical_template(68, 112, 112))
    u8 = A.AlignedFormat("nhwc", "uint8")
    smoothed = 0
    for t in range(4):
        if t == 2:
            slot, box = RESEED
            tr.seed([slot], [box])
            assert (tr.filter_state[slot] == -1).all() and (tr.filter_state[0, :, 0] >= 0).any()
            one = dev(np.asarray(P.face_boxes([list(box)]), np.int32))
            sm, _ = A.track_seed_device(one, (64, 64), (RH, RW))
            m, boxes = m.clone(), boxes.clone()
            m[slot], boxes[slot], state[slot] = sm[0], one[0], -1.0
        idx = torch.full((CAP,), t, dtype=torch.int32, device="cuda")
        crops = A.warp_frames_device(ring, m, 64, 64, frame_index_dev=idx, boxes_dev=boxes, fmt=u8)
        lm = model.forward_device(crops, "landmarks", n_points=4, thresh=0.0)
        raw = torch.empty((CAP, 68, 2), dtype=torch.float64, device="cuda")
        before = state.clone()
        lmf, ma, mn, bn, st = A.track_step_device(lm, m, boxes, (72, 72), (64, 64), (RH, RW), tc, ta, filter=filt, dt=DT,
                                                  state=state, lm_raw=raw)
        aligned = A.warp_frames_device(ring, ma, 112, 112, frame_index_dev=idx, boxes_dev=boxes)
        got = tr.step(ring, t, dt=DT) if t % 2 else tr.step(ring, t)          # (1/fps of the defaults is DT)
        for a, b in zip(got, (aligned, ma, lmf, st)):
            assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), t
        assert torch.equal(tr.filter_state, state) and torch.equal(tr.m_crop, mn) and torch.equal(tr.boxes, bn)
        plain = A.track_step_device(lm, m, boxes, (72, 72), (64, 64), (RH, RW), tc, ta)
        assert torch.equal(raw, plain[0])
        fresh = [s for s in range(CAP) if t == 0 or (t == 2 and s == RESEED[0])]
        for s in fresh:                                   # a slot's first step after a seed is the unfiltered step
            assert (before[s] == -1).all()
            for a, b in zip((lmf, ma, mn, bn, st), plain):
                assert torch.equal(a[s], b[s]), (t, s)
        smoothed += int((lmf != raw).sum())
        print("step %d status %s, %d coordinates moved by the filter" % (t + 1, st.tolist(), int((lmf != raw).sum())))
        m, boxes = mn, bn
    assert smoothed > 0                                   # (some track lived long enough to have a history)
    plain = P.FaceTracker(model, (RH, RW), CAP)
    plain.seed(range(CAP), FACES)
    plain.step(ring, 0)
    assert plain.smooth is None and plain.filter_state is None
