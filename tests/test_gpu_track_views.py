"""flm_track_views_update and flm_track_exit_views on the GPU, alone: synthetic faces (bytes), quality records, landmarks,
weights and pose records -- no model.  Every parametrisation chains six updates (a reset of every row, fresh faces, an
exact repeat that must tie everywhere, resets and status != 0 rows, better faces, fresh faces) and compares every output
array bit for bit with tests/track_views_ref.py applied to the state downloaded before the update; then moves the views
of some slots into exit rings of one and of four rows.  All state starts as the byte 0x4B and is carved, with guards,
from one tests/arena.py allocation: untaken bins, unnamed slots, the guards and every input must keep every byte.

N in {1, 5, 70} (70: more than one wave of decision threads); B in {1, 3, 6}; face_bytes in {105, 112, 4112, 16405}: 105
and 16405 with the faces and the gallery one byte off a 16-byte line (the element path, a ragged tail), 112 on the 16-byte
path, 4112 a second trip of a thread through the copy loop, 16405 more than the 16384 bytes one copy workgroup is dealt: a
grid of two chunks, and in the exit kernel the split of blockIdx.x into chunk and bin.  Both forms: direct (row == slot) and
rows (permuted slots, n_slots > N, inert rows).  Last, every rejection of the two wrappers that needs tensors on the
device."""
import numpy as np
import pytest
import torch

import track_views_ref as vref
from arena import Arena

pytestmark = pytest.mark.gpu
FILL, GUARD, C = 0x4B, 256 << 10, 5
EDGES = {1: ((), ()), 3: ((-0.3, 0.3), ()), 6: ((-0.3, 0.3), (0.0,))}
SHARP_REF, MIN_EXPOSED = 100.0, 0.5


@pytest.fixture(scope="module")
def mods():
    import flm_amd  # noqa: F401
    from flm_amd import _lib, alignment
    _lib.load()
    return _lib, alignment


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[x.dtype.itemsize])


def bin_centre(b, u_edges, v_edges):
    """(u, v) well inside bin b."""
    nu = len(u_edges) + 1
    iu, iv = b % nu, b // nu
    mid = lambda e, i: 0.0 if not e else (e[0] - 0.4 if i == 0 else e[-1] + 0.4 if i == len(e) else 0.5 * (e[i - 1] + e[i]))
    return mid(u_edges, iu), mid(v_edges, iv)


def make_inputs(rng, i, n, n_slots, b, fb, rows, prev):
    """The inputs of update i (a dict of numpy arrays); update 2 repeats update 1 but for the faces."""
    u_edges, v_edges = EDGES[b]
    faces = rng.integers(0, 256, (n, fb), dtype=np.uint8)
    if i == 2:
        return dict(prev, faces=faces, reset=np.zeros(n, np.int32))   # (a reset would let the repeat in again)
    rec = np.zeros((n, 8), np.int64)
    rec[:, 0], rec[:, 3] = 100, 64
    rec[:, 4] = rng.integers(-50, 50, n)
    sharp = rng.uniform(10.0, 60.0, n) + (50.0 if i == 4 else 0.0) + (200.0 if i == 5 else 0.0) * (rng.random(n) < 0.3)
    rec[:, 5] = (64 * 256 * sharp).astype(np.int64)
    rec[:, 6] = rng.choice([0, 10, 25, 50, 60], n, p=[0.4, 0.2, 0.2, 0.1, 0.1])     # 60 dark of 100: e = 0.4 < min_exposed
    rec[:, 7] = rng.choice([0, 5], n)
    stats = rng.uniform(0.0, 1.0, (n, C, 6))                          # a landmark record tensor: x, y, score, ...
    stats[..., :2] *= 100.0
    stats[rng.random((n, C)) < 0.2, :2] = -1.0                        # points that take no part in wbar
    if n > 2:
        stats[2, :, :2] = -1.0                                        # no landmark at all: wbar = 0, q = 0
    status = np.where(rng.random(n) < (0.3 if i == 3 else 0.1), 2, 0).astype(np.int32)
    reset = np.ones(n, np.int32) if i == 0 else (rng.random(n) < 0.4).astype(np.int32) if i == 3 else np.zeros(n, np.int32)
    m = rng.standard_normal((n, 2, 3)).astype(np.float32)
    pose = rng.standard_normal((n_slots, 18))
    pose[:, 14] = 1.0
    for g in range(n_slots):                                           # slot g aims at bin (i + g) of its own cycle
        cyc = b - 1 if (b > 1 and g % 3 == 0) else b                   # every third slot never sees its last bin
        pose[g, 6], pose[g, 7] = bin_centre((i + g) % cyc, u_edges, v_edges)
        pose[g, 6] = -pose[g, 6]                                       # u = -pose[6]
    pose[rng.random(n_slots) < 0.1, 14] = 0.0                          # a fit that is not ok
    if n_slots > 4:
        pose[4, 6], pose[4, 14] = np.nan, 1.0                          # a NaN u
    if rows:
        if n >= 5:                                                     # permuted, another way in every update; the last slot is never named
            perm = prev["perm"] if prev else rng.permutation(n_slots - 1)[:n].astype(np.int32)
            slot = np.roll(perm, -i)
            slot[1], slot[3] = -1, n_slots                             # inert rows
        else:
            slot = np.full(n, n_slots - 2, np.int32)
            if i in (3, 5):
                slot[0] = -1 if i == 3 else n_slots
    else:
        slot = None
    if i == 3:
        reset[0] = 1
    if i in (0, 1, 3) and (not rows or 0 <= slot[0] < n_slots):        # row 0 counts in these updates, whatever was drawn
        g0 = int(slot[0]) if rows else 0
        status[0], rec[0, 6], pose[g0, 14] = 0, 0, 1.0
        if not np.isfinite(pose[g0, 6]):
            pose[g0, 6] = 0.0
        stats[0, 0, :2] = (5.0, 6.0)
        stats[0, 0, 2] = 0.5 + 0.1 * i
    return dict(faces=faces, rec=rec, stats=stats, status=status, reset=reset, m=m, pose=pose, slot=slot,
                perm=perm if rows and n >= 5 else None)


@pytest.mark.parametrize("rows", [False, True], ids=["direct", "rows"])
@pytest.mark.parametrize("fb", [105, 112, 4112, 16405])
@pytest.mark.parametrize("b", [1, 3, 6])
@pytest.mark.parametrize("n", [1, 5, 70])
def test_update_chain_and_exit_views(mods, n, b, fb, rows):
    L, A = mods
    u_edges, v_edges = EDGES[b]
    opts = A.PoseViews.from_edges(u_edges, v_edges, sharp_ref=SHARP_REF, min_exposed=MIN_EXPOSED)
    assert opts.bins == b
    n_slots = n + 3 if rows else n
    off = fb % 2                                                       # the faces and the gallery one byte off a 16-byte line
    rng = np.random.default_rng(1000 * n + 10 * b + fb + (7 if rows else 0))
    sb = n_slots * b
    ar = Arena(FILL, [("faces", n * fb + off, 16, True), ("rec", n * 64, 8, True), ("stats", n * C * 48, 8, True),
                      ("status", n * 4, 4, True), ("reset", n * 4, 4, True), ("m", n * 24, 4, True), ("slot", n * 4, 4, True),
                      ("pose", n_slots * 144, 8, True), ("view_q", sb * 8, 8), ("view_frame", sb * 8, 8),
                      ("view_gallery", sb * fb + off, 16), ("view_m", sb * 24, 4), ("view_lm", sb * C * 16, 8),
                      ("view_pose", sb * 144, 8), ("take", n * 4, 4)], device="cuda", guard=GUARD)
    out_views = dict(view_q=ar.view("view_q", torch.float64, (n_slots, b)), view_frame=ar.view("view_frame", torch.int64, (n_slots, b)),
                     view_gallery=ar.region("view_gallery")[off:off + sb * fb].view(n_slots, b, fb),
                     view_m=ar.view("view_m", torch.float32, (n_slots, b, 2, 3)),
                     view_lm=ar.view("view_lm", torch.float64, (n_slots, b, C, 2)),
                     view_pose=ar.view("view_pose", torch.float64, (n_slots, b, 18)))
    take_dev = ar.view("take", torch.int32, (n,))
    state = vref.new_state(n_slots, b, (fb,), np.uint8, C, fill=FILL)
    download = lambda: {k: v.cpu().numpy() for k, v in out_views.items()}
    taken_bins, kept_decisions, prev = set(), 0, None
    for i in range(6):
        inp = make_inputs(rng, i, n, n_slots, b, fb, rows, prev)
        prev = inp
        pad = np.full(off, FILL, np.uint8)
        faces = ar.put("faces", np.concatenate([pad, inp["faces"].reshape(-1)]))[off:].view(n, fb)
        rec, stats = ar.put("rec", inp["rec"]), ar.put("stats", inp["stats"])
        status, reset, m = ar.put("status", inp["status"]), ar.put("reset", inp["reset"]), ar.put("m", inp["m"])
        pose = ar.put("pose", inp["pose"])
        slot = ar.put("slot", inp["slot"]) if rows else None
        before = download()
        for k in state:                                                # the restatement runs on the state the device holds
            assert np.array_equal(bits(before[k]), bits(state[k])), (k, i)
        lm, w = inp["stats"][..., :2], inp["stats"][..., 2]
        want = vref.update(state, inp["faces"], inp["rec"], lm, inp["pose"], 40 + i, u_edges, v_edges, w=w, status=inp["status"],
                           reset=inp["reset"], m=inp["m"], slot=inp["slot"], sharp_ref=SHARP_REF, min_exposed=MIN_EXPOSED)
        got = A.track_views_update_device(faces, rec, stats[..., :2], pose, out_views["view_q"], out_views["view_frame"],
                                          out_views["view_gallery"], take_dev, 40 + i, status=status, reset=reset,
                                          weights=stats[..., 2], m=m, opts=opts, slot=slot, view_m=out_views["view_m"],
                                          view_lm=out_views["view_lm"], view_pose=out_views["view_pose"])
        assert got is take_dev
        torch.cuda.synchronize()
        take = take_dev.cpu().numpy()
        print("update", i, "take", take.tolist()[:16], "want", want.tolist()[:16])
        assert np.array_equal(take, want), i
        after = download()
        for k in state:
            assert np.array_equal(bits(after[k]), bits(state[k])), (k, i)
        ar.check_guards()                                              # the guards, and every input unchanged
        assert bytes(ar.region("faces")[:off].cpu().numpy()) == bytes([FILL] * off)
        assert bytes(ar.region("view_gallery")[:off].cpu().numpy()) == bytes([FILL] * off)
        valid = np.ones(n, bool) if not rows else (inp["slot"] >= 0) & (inp["slot"] < n_slots)
        taken_bins |= set(int(v) for v in want[want >= 0])
        kept_decisions += int(((want < 0) & valid).sum())
        if i == 2:
            assert (want == -1).all()                                  # the repeat ties everywhere: the earlier frame stays
    assert kept_decisions >= 1 and len(taken_bins) >= (2 if b > 1 else 1), (taken_bins, kept_decisions)
    untouched = bits(state["view_q"]) == bits(np.frombuffer(bytes([FILL] * 8), np.float64))[0]
    if rows:
        assert untouched[n_slots - 1].all()                            # a slot no row ever named still holds the fill

    # ---- the exits: rings of one and of four rows
    filled = state["view_q"] >= 0.0
    mixed = filled.any(axis=1) & ~filled.all(axis=1)
    order = sorted(range(n_slots), key=lambda g: (not mixed[g], g))    # slots with both filled and empty bins first
    if b > 1:
        assert mixed[order[0]], "no slot holds both a filled and an empty bin"
    for q in (1, 4):
        n_out = min(q, (n_slots + 1) // 2)
        exit_row = np.array([[-1, -2, -3][g % 3] for g in range(n_slots)], np.int32)
        for j, g in enumerate(order[:n_out]):
            exit_row[g] = (j + 1) % q                                  # distinct rows, not in slot order
        if n_slots > 2 * q:
            exit_row[order[-1]] = q                                    # a row outside the ring writes nothing either
        qb = q * b
        xr = Arena(FILL, [("x_view_q", qb * 8, 8), ("x_view_frame", qb * 8, 8), ("x_view_gallery", qb * fb + off, 16),
                          ("x_view_m", qb * 24, 4), ("x_view_lm", qb * C * 16, 8), ("x_view_pose", qb * 144, 8)],
                   device="cuda", guard=GUARD)
        ring_dev = dict(x_view_q=xr.view("x_view_q", torch.float64, (q, b)), x_view_frame=xr.view("x_view_frame", torch.int64, (q, b)),
                        x_view_gallery=xr.region("x_view_gallery")[off:off + qb * fb].view(q, b, fb),
                        x_view_m=xr.view("x_view_m", torch.float32, (q, b, 2, 3)),
                        x_view_lm=xr.view("x_view_lm", torch.float64, (q, b, C, 2)),
                        x_view_pose=xr.view("x_view_pose", torch.float64, (q, b, 18)))
        ring = {k: v.cpu().numpy().copy() for k, v in ring_dev.items()}
        vref.exit_views(state, ring, exit_row)
        ret = A.track_exit_views_device(torch.from_numpy(exit_row).cuda(), out_views["view_q"], out_views["view_frame"],
                                        out_views["view_gallery"], ring_dev["x_view_q"], ring_dev["x_view_frame"],
                                        ring_dev["x_view_gallery"], view_m=out_views["view_m"], view_lm=out_views["view_lm"],
                                        view_pose=out_views["view_pose"], x_view_m=ring_dev["x_view_m"],
                                        x_view_lm=ring_dev["x_view_lm"], x_view_pose=ring_dev["x_view_pose"])
        assert ret is ring_dev["x_view_q"]
        torch.cuda.synchronize()
        for k, v in ring_dev.items():
            assert np.array_equal(bits(v.cpu().numpy()), bits(ring[k])), (k, q)
        xr.check_guards()
        ar.check_guards()
        after = download()
        for k in state:                                                # the sources are inputs here
            assert np.array_equal(bits(after[k]), bits(state[k])), (k, q)
        if b > 1:                                                      # an empty bin of an exiting slot: the ring's bytes survive
            g = order[0]
            row, empty = int(exit_row[g]), int(np.flatnonzero(~filled[g])[0])
            assert (ring["x_view_gallery"][row, empty] == FILL).all() and not ring["x_view_q"][row, empty] >= 0.0
        written = sorted(int(r) for r in exit_row if 0 <= r < q)
        assert len(set(written)) == len(written) == n_out
        for row in set(range(q)) - set(written):                       # a ring row nobody was written to
            assert all((bits(v[row]).reshape(-1).view(np.uint8) == FILL).all() for v in ring.values())


# ---- the rejections of the two wrappers that need tensors on the device ------------------------------------------------------
class Pool:
    """Tensors carved from one zeroed allocation at byte offsets the test chooses, so that two of them can share bytes."""

    def __init__(self, nbytes):
        self.buf = torch.zeros((nbytes,), dtype=torch.uint8, device="cuda")
        self.cur = 0
        self.at = {}                                                   # name -> (offset, bytes)

    def carve(self, off, dtype, shape):
        nb = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        return self.buf[off:off + nb].view(dtype).view(tuple(shape))

    def new(self, name, dtype, shape):
        """The next tensor, with a gap after it that is larger than any tensor of the test (so a tensor carved over its end,
        or directly after it, touches no third one)."""
        t = self.carve(self.cur, dtype, shape)
        self.at[name] = (self.cur, t.numel() * t.element_size())
        self.cur += (t.numel() * t.element_size() + 255) // 256 * 256 + 2048
        return t

    def over_the_end_of(self, name, dtype, shape):
        """A tensor that begins in the last 8 bytes of `name` and runs on past it."""
        off, nb = self.at[name]
        return self.carve(off + nb - 8, dtype, shape)

    def after(self, name, dtype, shape):
        """A tensor that begins at the first byte after `name`: adjacent, no overlap."""
        off, nb = self.at[name]
        return self.carve(off + nb, dtype, shape)


def test_wrappers_reject_bad_tensors_before_any_launch(mods):
    L, A = mods
    n, b, c, q = 4, 3, 5, 2
    f64, i64, i32, f32, f16 = torch.float64, torch.int64, torch.int32, torch.float32, torch.float16
    z = lambda shape, dtype: torch.zeros(shape, dtype=dtype, device="cuda")
    P = Pool(1 << 18)
    stats = P.new("stats", f64, (n, c, 6))
    spec = dict(faces=(f16, (n, 2, 2, 3)), rec=(i64, (n, 8)), pose=(f64, (n, 18)), status=(i32, (n,)), reset=(i32, (n,)),
                m=(f32, (n, 2, 3)), slot=(i32, (n,)), view_q=(f64, (n, b)), view_frame=(i64, (n, b)),
                view_gallery=(f16, (n, b, 2, 2, 3)), take=(i32, (n,)), view_m=(f32, (n, b, 2, 3)), view_lm=(f64, (n, b, c, 2)),
                view_pose=(f64, (n, b, 18)))
    good = {k: P.new(k, *v) for k, v in spec.items()}
    good["slot"].copy_(torch.tensor([2, 0, 3, 1], dtype=i32))
    good["pose"][:, 14] = 1.0
    good.update(lm=stats[..., :2], weights=stats[..., 2], frame_id=3, opts=A.PoseViews.from_edges((-0.3, 0.3)))
    order = ("faces", "rec", "lm", "pose", "view_q", "view_frame", "view_gallery", "take", "frame_id")
    inputs = ("faces", "rec", "pose", "status", "reset", "m", "slot")
    outputs = ("view_q", "view_frame", "view_gallery", "take", "view_m", "view_lm", "view_pose")

    def update(**kw):
        a = dict(good, **kw)
        return A.track_views_update_device(*[a[k] for k in order], **{k: v for k, v in a.items() if k not in order})

    def refused(match, **kw):
        with pytest.raises(ValueError, match=match):
            update(**kw)

    assert update() is good["take"]                                    # what is refused below differs from this in one argument
    assert update(slot=None) is good["take"]
    # no output may overlap an input or another output: the end of every other tensor, and the byte after it
    for out in outputs:
        for other in inputs + tuple(o for o in outputs if o != out):
            refused("%s and %s|%s and %s" % (other, out, out, other), **{out: P.over_the_end_of(other, *spec[out])})
            assert update(**{out: P.after(other, *spec[out])}) is not None, (out, other)
        # the landmarks and the weights are strided views of one record tensor: their spans count, gaps included
        off = P.at["stats"][0]
        refused("lm and %s" % out, **{out: P.carve(off + 16, *spec[out])})                     # over the first score
        refused("lm and %s|weights and %s" % (out, out), **{out: P.carve(off + P.at["stats"][1] - 40, *spec[out])})
    assert update(view_q=P.after("stats", f64, (n, b))) is good["take"]
    same = P.new("same", f64, (n, b))
    refused("view_q and view_frame|view_frame and view_q", view_q=same, view_frame=same.view(i64))   # one inside the other
    refused("status and take|take and status", take=good["status"])
    # what goes together, and the sizes
    refused("view_m needs m", m=None)
    refused("one record per face", slot=None, pose=z((n + 1, 18), f64))
    refused("rows", faces=z((65536, 1), torch.uint8))
    refused("rows", faces=z((0, 2, 2, 3), f16))
    refused("1 <= C <= 1024", lm=z((n, 1025, 2), f64), weights=None)
    refused("lm must be", lm=z((n + 1, c, 2), f64), weights=None)
    refused("opts", opts=A.BestShot())
    refused("frame_id", frame_id=0.5)
    # the rows form takes its number of slots from the pose: every view tensor must have as many
    wide = dict(pose=z((n + 2, 18), f64), view_q=z((n + 2, b), f64), view_frame=z((n + 2, b), i64), view_gallery=z((n + 2, b, 2, 2, 3), f16),
                view_m=z((n + 2, b, 2, 3), f32), view_lm=z((n + 2, b, c, 2), f64), view_pose=z((n + 2, b, 18), f64))
    assert update(**wide) is good["take"]
    for name in ("view_q", "view_frame", "view_gallery", "view_m", "view_lm", "view_pose"):
        refused(name, **{k: v for k, v in wide.items() if k != name})
    # the type, shape and layout of every tensor
    for name, bad in (("faces", good["faces"].cpu()), ("faces", z((n, 2, 3, 2), f16).transpose(2, 3)), ("rec", z((n, 8), i32)),
                      ("rec", z((n, 7), i64)), ("rec", z((n + 1, 8), i64)), ("lm", z((n, c, 2), f32)), ("lm", z((n, c, 3), f64)),
                      ("pose", z((n, 18), f32)), ("pose", z((n, 17), f64)), ("pose", z((n, 36), f64)[:, ::2]), ("pose", good["pose"].cpu()),
                      ("status", z((n,), i64)), ("status", z((n + 1,), i32)), ("reset", z((n,), f32)), ("reset", z((n + 1,), i32)),
                      ("weights", z((n, c + 1), f64)), ("weights", z((n, c), f32)), ("m", z((n, 3, 2), f32)), ("m", z((n, 2, 3), f64)),
                      ("slot", z((n,), i64)), ("slot", z((n + 1,), i32)), ("slot", good["slot"].cpu()),
                      ("take", z((n,), i64)), ("take", z((n + 1,), i32)), ("take", good["take"].cpu()),
                      ("view_q", z((n, b), f32)), ("view_q", z((n, b + 1), f64)), ("view_q", z((n + 1, b), f64)),
                      ("view_q", z((n, 2 * b), f64)[:, ::2]), ("view_frame", z((n, b), i32)), ("view_frame", z((n, b - 1), i64)),
                      ("view_gallery", z((n, b, 2, 2, 3), f32)), ("view_gallery", z((n, b, 2, 3, 3), f16)),
                      ("view_gallery", z((n, b + 1, 2, 2, 3), f16)), ("view_gallery", z((n + 1, b, 2, 2, 3), f16)),
                      ("view_gallery", z((n * b, 2, 2, 3), f16)), ("view_gallery", good["view_gallery"].cpu()),
                      ("view_m", z((n, b, 3, 2), f32)), ("view_m", z((n, b, 2, 3), f64)), ("view_lm", z((n, b, c + 1, 2), f64)),
                      ("view_lm", z((n, b, c, 2), f32)), ("view_pose", z((n, b, 17), f64)), ("view_pose", z((n, b, 18), f32))):
        refused("m must be|K,2,3|%d,2,3" % n if name == "m" else name, **{name: bad})

    # ---- track_exit_views_device
    xspec = dict(exit_row=(i32, (n,)), x_view_q=(f64, (q, b)), x_view_frame=(i64, (q, b)), x_view_gallery=(f16, (q, b, 2, 2, 3)),
                 x_view_m=(f32, (q, b, 2, 3)), x_view_lm=(f64, (q, b, c, 2)), x_view_pose=(f64, (q, b, 18)))
    xgood = {k: P.new(k, *v) for k, v in xspec.items()}
    xgood["exit_row"].copy_(torch.tensor([1, -1, -2, 0], dtype=i32))
    xgood.update({k: good[k] for k in ("view_q", "view_frame", "view_gallery", "view_m", "view_lm", "view_pose")})
    xspec.update({k: spec[k] for k in ("view_q", "view_frame", "view_gallery", "view_m", "view_lm", "view_pose")})
    xorder = ("exit_row", "view_q", "view_frame", "view_gallery", "x_view_q", "x_view_frame", "x_view_gallery")

    def exit_views(**kw):
        a = dict(xgood, **kw)
        return A.track_exit_views_device(*[a[k] for k in xorder], **{k: v for k, v in a.items() if k not in xorder})

    def xrefused(match, **kw):
        with pytest.raises(ValueError, match=match):
            exit_views(**kw)

    assert exit_views() is xgood["x_view_q"]
    none3 = dict(view_m=None, view_lm=None, view_pose=None, x_view_m=None, x_view_lm=None, x_view_pose=None)
    assert exit_views(**none3) is xgood["x_view_q"]
    for name in ("view_m", "x_view_m", "view_lm", "x_view_lm", "view_pose", "x_view_pose"):   # a source without its ring buffer, or the reverse
        xrefused("both or neither", **{name: None})
    names = tuple(xspec)
    for a_name in names:                                               # no two tensors may overlap
        for b_name in names:
            if a_name != b_name:
                xrefused("%s and %s|%s and %s" % (a_name, b_name, b_name, a_name), **{b_name: P.over_the_end_of(a_name, *xspec[b_name])})
                beside = P.after(a_name, *xspec[b_name])
                if b_name == "exit_row":
                    beside.fill_(-1)                                   # (no slot exits: rows written in one call must be distinct)
                assert exit_views(**{b_name: beside}) is not None, (a_name, b_name)
    xrefused("x_view_q", x_view_q=z((65536, b), f64))
    xrefused("view_q", view_q=z((n, 65), f64))
    for name, bad in (("exit_row", z((n,), i64)), ("exit_row", z((n + 1,), i32)), ("exit_row", xgood["exit_row"].cpu()),
                      ("view_q", z((n, b), f32)), ("view_q", z((n, 2 * b), f64)[:, ::2]), ("view_q", z((n * b,), f64)),
                      ("view_frame", z((n, b), i32)), ("view_frame", z((n, b + 1), i64)), ("view_gallery", z((n, b + 1, 2, 2, 3), f16)),
                      ("view_gallery", z((n + 1, b, 2, 2, 3), f16)), ("view_gallery", good["view_gallery"].cpu()),
                      ("x_view_q", z((q, b + 1), f64)), ("x_view_q", z((q, b), f32)), ("x_view_q", z((q * b,), f64)),
                      ("x_view_frame", z((q, b), i32)), ("x_view_frame", z((q + 1, b), i64)), ("x_view_gallery", z((q, b, 2, 2, 3), f32)),
                      ("x_view_gallery", z((q, b, 2, 3, 3), f16)), ("x_view_gallery", z((q + 1, b, 2, 2, 3), f16)),
                      ("x_view_gallery", z((q, b + 1, 2, 2, 3), f16)), ("view_m", z((n, b, 3, 2), f32)), ("x_view_m", z((q, b, 2, 3), f64)),
                      ("x_view_m", z((q + 1, b, 2, 3), f32)), ("view_lm", z((n, b, c, 3), f64)), ("view_lm", z((n, b, 1025, 2), f64)),
                      ("x_view_lm", z((q, b, c + 1, 2), f64)), ("view_pose", z((n, b, 17), f64)), ("x_view_pose", z((q, b, 18), f32)),
                      ("x_view_pose", z((q, b + 1, 18), f64))):
        xrefused(name, **{name: bad})

    # ---- the gallery check itself
    A._check_view_faces(good["view_gallery"], (n, b), good["faces"], "view_gallery")
    A._check_view_faces(xgood["x_view_gallery"], (q, b), good["view_gallery"][:, 0], "x_view_gallery")
    g = z((n, b, 2, 2, 3), f16)
    for bad in (g.cpu(), g.float(), g[:, :, :1], g[:, :2], g.view(n * b, 2, 2, 3), g.transpose(0, 1), z((b, n, 2, 2, 3), f16), None, [1]):
        with pytest.raises(ValueError, match="view_gallery must be"):
            A._check_view_faces(bad, (n, b), good["faces"], "view_gallery")
    torch.cuda.synchronize()
    assert (good["take"].cpu().numpy() == -1).all()                    # (records of zeros: n_lap = 0, nothing is ever eligible)
