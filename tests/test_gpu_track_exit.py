"""GPU parity of flm_track_retire against tests/track_exit_ref.py through ctypes, bit for bit on every output and every
in/out tensor, with the ring pre-filled with a sentinel pattern (rows no track was written to must keep it): slot counts
on both sides of a wave, of the workgroup's chunk of 1024 slots and of several chunks; rings smaller and larger than the
number of exits; face sizes from one byte to a 112x112x3 bf16 face, aligned and offset by 2 bytes inside a larger buffer
(the element-access path, with guard bytes around the ring); the optional triples given and absent; three chained calls per
case, so that the sequence wraps the ring, ids continue from head[1] and born is seen cleared; and a flush.  Then the
wrapper inside sync-debug "error"."""
import ctypes as C

import numpy as np
import pytest
import torch

import track_exit_ref as xref

pytestmark = pytest.mark.gpu
FH, FW = 270, 480
NC = 5
# boxes without pixels -- plainly empty, and empty only after the clip to fh x fw -- and boxes with some
EMPTY = [(0, 0, 0, 0), (-40, 10, 0, 60), (FW, 10, FW + 30, 60), (10, FH, 60, FH + 9), (50, 50, 50, 90), (90, 40, 60, 80)]
FULL = [(10, 10, 60, 60), (-5, -5, 1, 1), (FW - 1, FH - 1, FW + 90, FH + 90), (-2 ** 31, -2 ** 31, 2 ** 31 - 1, 2 ** 31 - 1)]


@pytest.fixture(scope="module")
def mods():
    import flm_amd  # noqa: F401
    from flm_amd import _lib, alignment
    _lib.load()
    return _lib, alignment


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[x.dtype.itemsize])


def set_boxes(s, rng, live):
    k = len(live)
    pick = rng.integers(0, 1000, k)
    for t in range(k):
        s["boxes"][t] = FULL[pick[t] % len(FULL)] if live[t] else EMPTY[pick[t] % len(EMPTY)]


def fresh_bests(s, rng):
    """What the steps between two retire calls may have changed: the best shots, their records, the status words."""
    k = len(s["best_q"])
    q = rng.uniform(0.0, 1.0, k)
    kind = rng.integers(0, 10, k)
    q[kind == 0] = -1.0
    q[kind == 1] = np.nan
    q[kind == 2] = 0.0
    s["best_q"][:] = q
    s["status"][:] = rng.integers(0, 128, k)
    s["best_frame"][:] = rng.integers(-1, 2 ** 40, k)
    s["gallery"][:] = rng.integers(0, 256, s["gallery"].shape, dtype=np.uint8)
    if "best_m" in s:
        s["best_m"][:] = rng.standard_normal(s["best_m"].shape).astype(np.float32)
        s["best_lm"][:] = rng.uniform(-1, 500, s["best_lm"].shape)
        s["best_rec"][:] = rng.integers(0, 2 ** 50, s["best_rec"].shape)


GUARD = 64     # bytes kept around the ring and the gallery of an offset case


class Device:
    """The tensors of one case on the device, kept over the chained calls; the gallery and the ring of faces are views at
    `offset` bytes into larger buffers whose other bytes must not change."""

    def __init__(self, s, offset):
        self.offset = offset
        self.t = {n: dev(v) for n, v in s.items() if n not in ("gallery", "x_gallery")}
        for n in ("gallery", "x_gallery"):
            v = s[n]
            buf = torch.full((v.size + 2 * GUARD + offset,), 0x5C, dtype=torch.uint8, device="cuda")
            view = buf[GUARD + offset:GUARD + offset + v.size].view(v.shape)
            view.copy_(dev(v))
            assert view.data_ptr() % 16 == (buf.data_ptr() + GUARD + offset) % 16
            self.t[n], self.t[n + "_buf"] = view, buf

    def upload(self, s, names):
        for n in names:
            self.t[n].copy_(dev(s[n]))

    def call(self, L, frame_id, flush, opts):
        t = self.t
        p = lambda n: L.ptr(t[n]) if n in t else None
        k, q = int(t["track_id"].shape[0]), int(t["x_q"].shape[0])
        return L.load().flm_track_retire(
            L.stream_ptr(), p("boxes"), p("status"), k, FH, FW, p("best_q"), p("gallery"), int(t["gallery"].shape[1]),
            p("best_frame"), p("best_m"), p("best_lm"), NC, p("best_rec"), frame_id, flush, opts, p("born"), p("track_id"),
            p("born_frame"), p("head"), q, p("x_gallery"), p("x_meta"), p("x_q"), p("x_m"), p("x_lm"), p("x_rec"), p("exit_row"))

    def assert_equals(self, s, what):
        for n, exp in s.items():
            got = self.t[n].cpu().numpy()
            assert got.dtype == exp.dtype and got.shape == exp.shape, (n, what)
            assert np.array_equal(bits(got), bits(exp)), (n,) + tuple(what)
        for n in ("gallery", "x_gallery"):
            buf, size = self.t[n + "_buf"].cpu().numpy(), s[n].size
            lead = GUARD + self.offset
            assert (buf[:lead] == 0x5C).all() and (buf[lead + size:] == 0x5C).all(), (n, "guard bytes") + tuple(what)


# (K, Q, face_bytes, optional triples, offset of the faces, more exits than rows expected in the first call)
CASES = [
    (1, 1, 1, True, 0, False), (1, 7, 37, False, 2, False),
    (63, 2, 6, True, 0, True), (63, 64, 37, True, 2, False),
    (64, 7, 37, False, 2, True), (64, 1, 75264, True, 0, True),
    (65, 64, 4104, True, 0, False), (65, 2, 75264, False, 2, True),
    (1024, 7, 37, True, 2, True), (1024, 64, 6, False, 0, True),
    (1025, 2, 6, False, 0, True), (1025, 64, 4104, True, 2, True),
    (2500, 64, 4104, True, 0, True), (2500, 1, 1, True, 0, True), (2500, 7, 6, False, 2, True),
]


# ... and a flush in the first call: one slot, fewer exits than rows, more exits than rows
PARAMS = [c + (False,) for c in CASES] + [c + (True,) for c in CASES if c[:2] in ((1, 1), (65, 64), (1025, 2))]


@pytest.mark.parametrize("k,q,fb,optional,offset,overrun,flush_first", PARAMS)
def test_retire_matches_the_restatement_over_three_calls(mods, k, q, fb, optional, offset, overrun, flush_first):
    L, A = mods
    rng = np.random.default_rng(1000 * k + 10 * q + fb % 7 + (5 if flush_first else 0))
    s = xref.new_state(k, q, fb, NC, optional=optional)
    # ---- call 0: every combination of (held, born, live), a head that is not at zero
    held, born, live = rng.random(k) < 0.7, rng.random(k) < 0.35, rng.random(k) < 0.55
    if k >= 8:
        for i in range(8):                                             # ... guaranteed, whatever the draw
            held[i], born[i], live[i] = bool(i & 1), bool(i & 2), bool(i & 4)
    s["track_id"][:] = np.where(held, rng.permutation(k) + 1000, rng.choice([-1, -7], k))
    s["born"][:] = np.where(born, rng.integers(1, 4, k) * rng.choice([-1, 1], k), 0)
    s["born_frame"][:] = rng.integers(0, 99, k)
    set_boxes(s, rng, live)
    fresh_bests(s, rng)
    if k >= 8:
        s["best_q"][[1, 3]] = (-1.0, 0.9)                              # of the tracks that end, one is discarded, one emitted
    s["head"][:] = (rng.integers(0, 50), 5000, 3, 1)
    d = Device(s, offset)
    min_q = 0.0 if q % 2 else 0.125
    opts = C.byref(L.ExitOpts.make(min_q)) if min_q else None          # NULL means the defaults
    seen, rows_written = [], set()
    for call in range(3):
        if call == 1:        # nothing changes but the boxes: every slot is live.  born must be seen cleared: it is not uploaded
            set_boxes(s, rng, np.ones(k, bool))
            d.upload(s, ["boxes"])
        if call == 2:        # up to Q held slots end with a best shot, some more without one; births elsewhere
            fresh_bests(s, rng)
            held = s["track_id"] >= 0
            hs = rng.permutation(np.flatnonzero(held))
            n_good = min(q, len(hs), max(1, k // 4))
            good, bad = hs[:n_good], hs[n_good:n_good + 3]
            live = np.ones(k, bool)
            live[good] = live[bad] = False
            s["best_q"][good] = rng.uniform(0.5, 1.0, len(good))
            s["best_q"][bad] = rng.choice([-1.0, np.nan], len(bad))
            free = np.flatnonzero(~held)
            live[free] = rng.random(len(free)) < 0.6
            s["born"][free] = (rng.random(len(free)) < 0.5).astype(np.int32)
            set_boxes(s, rng, live)
            d.upload(s, ["boxes", "status", "best_q", "best_frame", "gallery", "born"] + (["best_m", "best_lm", "best_rec"] if optional else []))
        flush = 1 if flush_first and call == 0 else 0
        before = {n: v.copy() for n, v in s.items()}
        out = xref.retire(s, FH, FW, frame_id=700 + call, flush=flush, min_q=min_q)
        rc = d.call(L, 700 + call, flush, opts)
        assert rc == 0, L.load().flm_last_error()
        d.assert_equals(s, (k, q, fb, call))
        seen.append(out)
        rows_written |= set(s["exit_row"][s["exit_row"] >= 0].tolist())
        e = out["E"]
        if call == 0:
            if k >= 8:
                combos = {(bool(h), bool(b), bool(l)) for h, b, l in zip(out["held"], out["born"], out["live"])}
                assert len(combos) == 8
            if overrun and not flush_first:
                assert e > q and s["head"][3] > before["head"][3] and (s["exit_row"] == -3).sum() == e - q
            assert (s["exit_row"] == -2).sum() == out["discarded"].sum() and (out["discarded"].any() or k < 8)
        if call == 1:
            assert e == 0 and out["B"] == 0 and (s["exit_row"] == -1).all() and not s["born"].any()
            for n in ("x_gallery", "x_meta", "x_q", "head", "track_id", "born_frame"):
                assert np.array_equal(bits(s[n]), bits(before[n])), n
        if call == 2 and (before["track_id"] >= 0).any():
            assert 0 < e <= q and s["head"][3] == before["head"][3]
            assert sorted(s["x_meta"][s["exit_row"][out["written"]], 6].tolist()) == list(range(before["head"][0], s["head"][0]))
        assert s["head"][0] == before["head"][0] + e and s["head"][1] == before["head"][1] + out["B"]
        ids = s["track_id"][out["births"]]
        assert ids.tolist() == list(range(before["head"][1], s["head"][1]))                # ascending slot, from head[1]
    untouched = sorted(set(range(q)) - rows_written)                   # a row no call wrote to keeps the sentinel
    assert untouched or not (q == 64 and k <= 65)
    assert (s["x_meta"][untouched] == -77).all() and (s["x_gallery"][untouched] == 0xA5).all() and (s["x_q"][untouched] == -7.5).all()
    print(k, q, fb, "E per call:", [o["E"] for o in seen], "B:", [o["B"] for o in seen], "head:", s["head"].tolist())


def test_the_wrapper_writes_what_the_raw_call_writes_without_a_synchronisation(mods):
    L, A = mods
    k, q, fb = 70, 4, 37
    rng = np.random.default_rng(5)
    s = xref.new_state(k, q, fb, NC)
    s["track_id"][:] = np.where(rng.random(k) < 0.6, np.arange(k), -1)
    s["born"][:] = rng.random(k) < 0.3
    set_boxes(s, rng, rng.random(k) < 0.5)
    fresh_bests(s, rng)
    t = {n: dev(v) for n, v in s.items()}
    xref.retire(s, FH, FW, frame_id=3, flush=True, min_q=0.25)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):                              # (the mode is live in this build: a download raises)
            t["head"][0].item()
        rows = A.track_retire_device(t["boxes"], t["status"], (FH, FW), t["best_q"], t["gallery"], t["best_frame"], t["born"],
                                     t["track_id"], t["born_frame"], t["head"], t["x_gallery"], t["x_meta"], t["x_q"],
                                     t["exit_row"], 3, flush=True, opts=A.TrackExits(q, 0.25), best_m=t["best_m"],
                                     best_lm=t["best_lm"], best_rec=t["best_rec"], x_m=t["x_m"], x_lm=t["x_lm"], x_rec=t["x_rec"])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert rows is t["exit_row"]
    for n, exp in s.items():
        assert np.array_equal(bits(t[n].cpu().numpy()), bits(exp)), n
    with pytest.raises(ValueError, match="overlap"):
        A.track_retire_device(t["boxes"], t["status"], (FH, FW), t["best_q"], t["gallery"], t["best_frame"], t["born"],
                              t["track_id"], t["track_id"], t["head"], t["x_gallery"], t["x_meta"], t["x_q"], t["exit_row"], 3)
    with pytest.raises(ValueError, match="both or neither"):
        A.track_retire_device(t["boxes"], t["status"], (FH, FW), t["best_q"], t["gallery"], t["best_frame"], t["born"],
                              t["track_id"], t["born_frame"], t["head"], t["x_gallery"], t["x_meta"], t["x_q"], t["exit_row"], 3,
                              best_m=t["best_m"])
    with pytest.raises(ValueError, match="rows of opts"):
        A.track_retire_device(t["boxes"], t["status"], (FH, FW), t["best_q"], t["gallery"], t["best_frame"], t["born"],
                              t["track_id"], t["born_frame"], t["head"], t["x_gallery"], t["x_meta"], t["x_q"], t["exit_row"], 3,
                              opts=A.TrackExits(q + 1))
    with pytest.raises(ValueError, match="x_faces"):
        A.track_retire_device(t["boxes"], t["status"], (FH, FW), t["best_q"], t["gallery"], t["best_frame"], t["born"],
                              t["track_id"], t["born_frame"], t["head"], t["x_gallery"].view(q, fb, 1), t["x_meta"], t["x_q"],
                              t["exit_row"], 3)
