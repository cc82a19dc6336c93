"""GPU parity of the three calls that step a subset of the slots -- flm_track_gather_streams, flm_track_step_rows,
flm_track_best_update_rows -- against tests/track_rows_ref.py through ctypes, on buffers pre-filled with junk (NaNs
included), bit for bit on every tensor, the tracker's own included: a slot no row names must keep its junk.  Then the
rows calls at slot[r] = r against the calls they extend on the device, the three wrappers, and FaceTracker.step_active
against `step` (all streams), against a sequence made by hand at the same batch (a schedule of streams that sit ticks
out), with device arguments, and at streams=1.  Every comparison is exact.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import face_quality_ref as qref
import nv12_ref
import track_filter_cases as cases
import track_filter_ref as fref
import track_rows_ref as rref

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
IN, GRID, FH, FW, SC = cases.IN, cases.GRID, cases.FH, cases.FW, cases.SC
NAN, INF = float("nan"), float("inf")


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
    u = {1: np.uint8, 4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    return np.array_equal(np.ascontiguousarray(got).view(u), np.ascontiguousarray(exp).view(u))


def view_bits(x):
    return x.view(torch.int64) if x.dtype == torch.float64 else x.view(torch.int32) if x.dtype == torch.float32 else x


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(view_bits(a), view_bits(b))


class sync_error:
    """Inside: a transfer or a synchronisation raises (checked on entry when `probe` is given)."""

    def __init__(self, probe=None):
        self.probe = probe

    def __enter__(self):
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        if self.probe is not None:
            try:
                with pytest.raises(RuntimeError):      # (the mode is live in this build: a download raises)
                    self.probe.item()
            except BaseException:
                torch.cuda.set_sync_debug_mode("default")
                raise

    def __exit__(self, *exc):
        torch.cuda.set_sync_debug_mode("default")


def junk64(rng, shape, lo=-50.0, hi=300.0, p_nan=0.08):
    x = rng.uniform(lo, hi, shape)
    x[rng.random(shape) < p_nan] = np.nan
    return x


# ---- flm_track_gather_streams ------------------------------------------------------------------------------------------
def _active_of(s, a, seed):
    return np.random.default_rng(seed).permutation(s)[:a].tolist()


GATHER = [(1, 1, [0]), (3, 3, [2, 0]), (5, 16, _active_of(5, 5, 1)), (70, 4, _active_of(70, 33, 2)), (5, 3, [4, -1, 1, 5])]


def gather_state(s, k, seed):
    rng = np.random.default_rng(seed)
    n = s * k
    m = junk64(rng, (n, 2, 3), -3, 3).astype(f32)
    boxes = rng.integers(-20, 400, (n, 4)).astype(np.int32)
    bq = junk64(rng, (n,), -1, 1)
    reset = rng.choice([0, 0, 1, 7, -3], n).astype(np.int32)
    fi = rng.integers(0, 8, s).astype(np.int32)
    dt = junk64(rng, (s,), -0.1, 0.2)
    dt[::3] = np.inf
    return m, boxes, bq, reset, fi, dt


def gpu_gather(L, active, s, k, m, boxes, fi, dt, bq, reset):
    a = len(active)
    n = a * k
    t = dict(m=dev(m), boxes=dev(boxes), fi=None if fi is None else dev(fi), dt=None if dt is None else dev(dt),
             bq=None if bq is None else dev(bq), reset=None if reset is None else dev(reset))
    o = dict(slot=torch.full((n,), 777, dtype=torch.int32, device="cuda"),
             m=torch.full((n, 2, 3), NAN, dtype=torch.float32, device="cuda"),
             boxes=torch.full((n, 4), 777, dtype=torch.int32, device="cuda"),
             frame_index=torch.full((n,), 777, dtype=torch.int32, device="cuda"),
             dt=None if dt is None else torch.full((n,), NAN, dtype=torch.float64, device="cuda"),
             best_q=None if bq is None else torch.full((n,), NAN, dtype=torch.float64, device="cuda"),
             reset=None if reset is None else torch.full((n,), 777, dtype=torch.int32, device="cuda"))
    p = lambda x: None if x is None else L.ptr(x)
    act = dev(np.asarray(active, np.int32))
    L.check(L.load().flm_track_gather_streams(L.stream_ptr(), L.ptr(act), a, s, k, p(t["fi"]), p(t["dt"]), L.ptr(t["m"]),
                                              L.ptr(t["boxes"]), p(t["bq"]), p(t["reset"]), L.ptr(o["slot"]), L.ptr(o["m"]),
                                              L.ptr(o["boxes"]), L.ptr(o["frame_index"]), p(o["dt"]), p(o["best_q"]),
                                              p(o["reset"])), "flm_track_gather_streams")
    return t, o


@pytest.mark.parametrize("s,k,active", GATHER)
def test_gather_matches_the_reference(mods, s, k, active):
    L = mods[0]
    m, boxes, bq, reset, fi, dt = gather_state(s, k, 10 * s + k)
    for combo in range(8):                                   # with and without each of the three optional groups
        w_dt, w_bq, w_rs = combo & 1, combo & 2, combo & 4
        args = (fi if combo not in (0, 5) else None, dt if w_dt else None, bq if w_bq else None, reset if w_rs else None)
        exp = rref.gather_streams(active, s, k, m, boxes, *args)
        t, o = gpu_gather(L, active, s, k, m, boxes, *args)
        for name in ("slot", "m", "boxes", "frame_index", "dt", "best_q", "reset"):
            if exp[name] is None:
                assert o[name] is None
            else:
                assert bits_equal(o[name], exp[name]), (name, combo)
        # what is only read keeps its bits; reset is cleared for the named streams alone
        assert bits_equal(t["m"], m) and bits_equal(t["boxes"], boxes)
        if w_bq:
            assert bits_equal(t["bq"], bq)
        if w_rs:
            assert bits_equal(t["reset"], exp["reset_global"])
            named = sorted(v for v in active if 0 <= v < s)
            rows = np.concatenate([np.arange(v * k, (v + 1) * k) for v in named])
            others = np.setdiff1d(np.arange(s * k), rows)
            assert not exp["reset_global"][rows].any() and np.array_equal(exp["reset_global"][others], reset[others])
    inert = [a for a, v in enumerate(active) if not 0 <= v < s]
    for a in inert:
        assert (exp["slot"][a * k:(a + 1) * k] == -1).all()
    assert (exp["slot"] >= 0).sum() == (len(active) - len(inert)) * k


# ---- flm_track_step_rows -----------------------------------------------------------------------------------------------
NS, CS = (1, 6, 70), (1, 68, 130)      # C = 130: the thread loop takes three rounds (two full ones and a tail of 2)
GLOBAL = ("m_next", "boxes_next", "status", "state")
COMPACT = ("lm_frame", "m_align", "lm_raw", "status_rows")
_SEQ = {}


def sequence(n, c, weighted):
    key = (n, c, weighted)
    if key not in _SEQ:
        _SEQ[key] = cases.sequence(n, c, weighted, steps=2)
    return _SEQ[key]


def slot_map(n, n_slots, seed):
    """A non-monotone permutation of a subset of the slots; from six rows on, two inert rows (-1 and n_slots)."""
    while True:
        slot = np.random.default_rng(seed).permutation(n_slots)[:n].astype(np.int32)
        if n < 6:
            return slot
        slot[1], slot[n - 1] = -1, n_slots
        if (np.diff(slot[slot >= 0]) < 0).any() and (np.diff(slot[slot >= 0]) > 0).any():
            return slot
        seed += 1000                                         # (a draw that happens to be sorted: the next one)


def row_dt(n, t):
    """One time step per row: ordinary values, and the four that are not > 0 and finite."""
    dt = 1.0 / np.random.default_rng(n + t).uniform(10, 60, n)
    if n >= 6:
        dt[[0, 3] if t == 0 else [3, 4]] = [0.0, NAN] if t == 0 else [-1.0 / 30, INF]
    elif t == 1:
        dt[0] = NAN
    return dt


def global_junk(n_slots, c, seed):
    rng = np.random.default_rng(seed)
    return dict(m_next=junk64(rng, (n_slots, 2, 3), -3, 3).astype(f32), boxes_next=rng.integers(-9, 500, (n_slots, 4)).astype(np.int32),
                status=rng.integers(0, 2 ** 20, n_slots).astype(np.int32), state=junk64(rng, (n_slots, c, 6), 0.0, 300.0, 0.03))


def gpu_step_rows(L, s, slot, glob, tc, ta, stride, align, filt, raw, dt):
    """flm_track_step_rows on the device buffers `glob` (written in place); -> the compact outputs, pre-filled with junk."""
    n, c = s["lm"].shape[:2]
    rng = np.random.default_rng(5)
    rec = rng.uniform(-3, 99, (n, c, stride))                   # junk in the columns nobody may read
    rec[..., :2] = s["lm"]
    w_d, ws = None, 1
    if s["w"] is not None and stride > 2:
        rec[..., 2] = s["w"]
    rec_d = dev(rec)
    if s["w"] is not None:
        w_d, ws = (rec_d.view(-1)[2:], stride) if stride > 2 else (dev(s["w"]), 1)
    o = dict(lm_frame=torch.full((n, c, 2), 777.0, dtype=torch.float64, device="cuda"),
             m_align=torch.full((n, 2, 3), NAN, dtype=torch.float32, device="cuda") if align else None,
             lm_raw=torch.full((n, c, 2), NAN, dtype=torch.float64, device="cuda") if filt and raw else None,
             status_rows=torch.full((n,), 777, dtype=torch.int32, device="cuda"))
    p = lambda x: None if x is None else L.ptr(x)
    m_c, b_c, slot_d = dev(s["m_crop"]), dev(s["boxes"]), dev(slot)
    dt_d = dev(np.asarray(dt, f64)) if filt and np.ndim(dt) else None
    opts = L.TrackOpts.make()
    fo = L.TrackFilter.make(**fref.DEFAULTS) if filt else None
    L.check(L.load().flm_track_step_rows(
        L.stream_ptr(), L.ptr(rec_d), stride, p(w_d), ws, L.ptr(m_c), L.ptr(b_c), n, c, SC, SC, IN, IN, FH, FW, L.ptr(tc),
        L.ptr(ta) if align else None, C.byref(opts), L.ptr(o["lm_frame"]), p(o["m_align"]), L.ptr(glob["m_next"]),
        L.ptr(glob["boxes_next"]), L.ptr(glob["status"]), None if fo is None else C.byref(fo),
        float(dt) if filt and not np.ndim(dt) else 0.0, L.ptr(glob["state"]) if filt else None, p(o["lm_raw"]), L.ptr(slot_d),
        int(glob["status"].shape[0]), p(dt_d), L.ptr(o["status_rows"])), "flm_track_step_rows")
    assert bits_equal(m_c, s["m_crop"]) and bits_equal(b_c, s["boxes"]) and bits_equal(slot_d, slot)
    return o


@pytest.mark.parametrize("c", CS)
@pytest.mark.parametrize("n", NS)
def test_step_rows_matches_the_reference_over_two_steps(mods, n, c):
    L = mods[0]
    n_slots = 2 * n + 3
    slot = slot_map(n, n_slots, 7 * n + c)
    junk = global_junk(n_slots, c, n + c)
    seen = set()
    for weighted in (False, True):
        seq = sequence(n, c, weighted)
        tc, ta = dev(seq["tc"]), dev(seq["ta"])
        for filt in (False, True):
            # the reference, once per (weights, filter): two steps on the carried state
            exp, g = [], {k: v for k, v in junk.items()}
            for t, s in enumerate(seq["steps"]):
                r = rref.step_rows(s["lm"], s["w"], s["m_crop"], s["boxes"], slot, SC, SC, IN, IN, FH, FW, seq["tc"], seq["ta"],
                                   g["m_next"], g["boxes_next"], g["status"], state=g["state"] if filt else None,
                                   dt=row_dt(n, t) if filt else None, filt=dict(fref.DEFAULTS) if filt else None)
                if not filt:
                    r["state"] = g["state"]
                exp.append(r)
                g = {k: r[k] for k in GLOBAL}
            for stride in (2, 6):
                for align in (True, False):
                    for raw in ((True, False) if filt else (False,)):
                        glob = {k: dev(v) for k, v in junk.items()}
                        for t, s in enumerate(seq["steps"]):
                            o = gpu_step_rows(L, s, slot, glob, tc, ta, stride, align, filt, raw, row_dt(n, t))
                            what = (t, weighted, filt, stride, align, raw)
                            for name in COMPACT:
                                if o[name] is not None:
                                    assert bits_equal(o[name], exp[t][name]), (name,) + what
                            for name in GLOBAL:
                                assert bits_equal(glob[name], exp[t][name]), (name,) + what
            # conditions on the inputs: what the cases are there for is in the data
            e0, e1 = exp
            named = np.zeros(n_slots, bool)
            named[slot[(slot >= 0) & (slot < n_slots)]] = True
            for name in GLOBAL:                              # the slots no row names keep their junk (NaNs among it)
                u = {4: np.uint32, 8: np.uint64}[junk[name].dtype.itemsize]
                assert np.array_equal(e1[name][~named].view(u), junk[name][~named].view(u)), name
                if filt or name != "state":
                    assert not np.array_equal(e1[name][named].view(u), junk[name][named].view(u)), name
            if n >= 6:
                seen.add("inert")
                for r in (1, n - 1):
                    assert e0["status_rows"][r] == rref.DEAD and (e0["lm_frame"][r] == -1).all()
                    assert np.array_equal(e0["m_align"][r], np.array([[1, 0, 0], [0, 1, 0]], f32))
                assert e0["status_rows"][2] & 1 and slot[2] >= 0                                            # a dead row
                assert c < 2 or (e0["status_rows"] == 0).any()                 # (one point is too few for a fit)
                if filt:                                     # a row with a bad dt lost its history and nothing else
                    for r in (0, 3):
                        gs = slot[r]
                        assert not e0["status_rows"][r] & 1 and 0 <= gs < n_slots
                        ok = e0["lm_raw"][r, :, 0] >= 0
                        assert ok.any() and np.array_equal(e0["lm_frame"][r][ok], e0["lm_raw"][r][ok])
                        assert (e0["state"][gs][ok][:, 2:4] == 0).all()
                        seen.add("bad dt")
                    good = [r for r in range(4, n - 1) if not e0["status_rows"][r] & 1]
                    assert c < 5 or any((e0["lm_frame"][r] != e0["lm_raw"][r]).any() for r in good)                  # the filter ran
                    for r in (3, 4):                         # and the second step's bad rows restart from the raw points
                        ok = e1["lm_raw"][r, :, 0] >= 0
                        assert np.array_equal(e1["lm_frame"][r][ok], e1["lm_raw"][r][ok])
    assert n < 6 or seen == {"inert", "bad dt"}


@pytest.mark.parametrize("n,c", [(6, 68), (70, 130), (3, 1)])
def test_identity_rows_are_the_calls_they_extend_on_the_device(mods, n, c):
    L = mods[0]
    slot = dev(np.arange(n, dtype=np.int32))
    for weighted in (False, True):
        seq = sequence(n, c, weighted)
        s = seq["steps"][1]
        tc, ta = dev(seq["tc"]), dev(seq["ta"])
        w_d = None if s["w"] is None else dev(s["w"])
        lm_d = dev(s["lm"])
        for filt in (True, False):
            got = []
            for rows in (False, True):
                m_c, b_c = dev(s["m_crop"]), dev(s["boxes"])
                o = dict(lm_frame=torch.full((n, c, 2), 777.0, dtype=torch.float64, device="cuda"),
                         m_align=torch.full((n, 2, 3), 777.0, dtype=torch.float32, device="cuda"),
                         m_next=torch.full((n, 2, 3), 777.0, dtype=torch.float32, device="cuda"),
                         boxes_next=torch.full((n, 4), 777, dtype=torch.int32, device="cuda"),
                         status=torch.full((n,), 777, dtype=torch.int32, device="cuda"), state=dev(s["state"]),
                         lm_raw=torch.full((n, c, 2), 777.0, dtype=torch.float64, device="cuda"))
                opts, fo = L.TrackOpts.make(), L.TrackFilter.make(**fref.DEFAULTS)
                args = (L.stream_ptr(), L.ptr(lm_d), 2, None if w_d is None else L.ptr(w_d), 1, L.ptr(m_c), L.ptr(b_c), n, c, SC,
                        SC, IN, IN, FH, FW, L.ptr(tc), L.ptr(ta), C.byref(opts), L.ptr(o["lm_frame"]), L.ptr(o["m_align"]),
                        L.ptr(o["m_next"]), L.ptr(o["boxes_next"]), L.ptr(o["status"]))
                fargs = (C.byref(fo), cases.DT, L.ptr(o["state"]), L.ptr(o["lm_raw"]))
                if rows:
                    o["status_rows"] = torch.full((n,), 777, dtype=torch.int32, device="cuda")
                    tail = (L.ptr(slot), n, None, L.ptr(o["status_rows"]))
                    L.check(L.load().flm_track_step_rows(*args, *(fargs if filt else (None, 0.0, None, None)), *tail),
                            "flm_track_step_rows")
                elif filt:
                    L.check(L.load().flm_track_step_filtered(*args, *fargs), "flm_track_step_filtered")
                else:
                    L.check(L.load().flm_track_step(*args), "flm_track_step")
                got.append(o)
            for name in ("lm_frame", "m_align", "m_next", "boxes_next", "status") + (("state", "lm_raw") if filt else ()):
                assert same(got[0][name], got[1][name]), (name, weighted, filt)
            assert torch.equal(got[1]["status_rows"], got[1]["status"])
            if filt:
                assert bits_equal(got[1]["state"], s["exp"]["state"])


# ---- flm_track_best_update_rows ----------------------------------------------------------------------------------------
BEST_N, BEST_C = 7, 5
BEST_STATE = ("gallery", "best_q", "best_frame", "best_m", "best_lm", "best_rec")
_BEST = {}


def best_case(kind):
    """Seven rows onto 17 slots: taken, a tie (not taken), reset and taken, reset and not eligible, two inert rows, a row
    that loses to what its slot holds.  Computed once per face format."""
    if kind in _BEST:
        return _BEST[kind]
    rng = np.random.default_rng(3)
    n, c, n_slots = BEST_N, BEST_C, 2 * BEST_N + 3
    if kind == "u8":
        faces = rng.integers(0, 256, (n, 5, 7, 3)).astype(np.uint8)                    # 105 bytes: no 16-byte path
        fmt = ("nhwc", "uint8", "bgr", (1, 1, 1), (0, 0, 0))
    else:
        faces = rng.integers(0, 256, (n, 112, 112, 3)).astype(f32)
        fmt = ("nhwc", "float32", "bgr", (1, 1, 1), (0, 0, 0))
    rec = qref.record(faces, fmt)
    lm = rng.uniform(0, 200, (n, c, 2))
    lm[1, 2] = -1.0
    w = rng.uniform(0.1, 1.0, (n, c))
    factor = rng.uniform(0.5, 1.0, n)
    m = rng.normal(0, 1, (n, 2, 3)).astype(f32)
    status = np.array([0, 0, 0, 8, 0, 0, 0], np.int32)
    reset = np.array([0, 0, 1, 5, 1, 0, 0], np.int32)
    slot = np.array([11, 4, 16, 0, -1, n_slots, 7], np.int32)
    _BEST[kind] = dict(faces=faces, rec=rec, lm=lm, w=w, factor=factor, m=m, status=status, reset=reset, slot=slot, n_slots=n_slots)
    return _BEST[kind]


def best_snapshot(cs, full):
    """best_q_c for the case: row 1 ties with its own quality, rows 2 and 6 hold more than any face can reach."""
    kw = dict(w=cs["w"], factor=cs["factor"], status=cs["status"]) if full else {}
    q, ok = qref.quality(cs["rec"], cs["lm"], **kw)
    assert ok[[0, 1, 2, 6]].all() and (q[[0, 1, 2, 6]] > 0).all() and (not full or not ok[3])
    bq = np.array([-1.0, q[1], 5.0, 0.25, 0.5, 0.5, 5.0])
    return bq


def best_junk(cs, seed):
    rng = np.random.default_rng(seed)
    n_slots, c = cs["n_slots"], BEST_C
    f = cs["faces"]
    gal = rng.integers(0, 256, (n_slots,) + f.shape[1:]).astype(f.dtype)
    if f.dtype == f32:
        gal.reshape(-1)[::97] = np.nan
    return dict(gallery=gal, best_q=junk64(rng, (n_slots,), -1, 1), best_frame=rng.integers(-5, 99, n_slots).astype(np.int64),
                best_m=junk64(rng, (n_slots, 2, 3), -3, 3).astype(f32), best_lm=junk64(rng, (n_slots, c, 2)),
                best_rec=rng.integers(0, 2 ** 40, (n_slots, 8)).astype(np.int64))


def offset_bytes(x, lead):
    """x on the device at `lead` bytes past an allocation's start, so that its base is not congruent with another
    tensor's modulo 16."""
    nbytes = x.size * x.itemsize
    buf = torch.zeros(nbytes + 64, dtype=torch.uint8, device="cuda")
    view = buf[lead:lead + nbytes].view({np.dtype(np.uint8): torch.uint8, np.dtype(f32): torch.float32}[x.dtype]).view(x.shape)
    view.copy_(dev(x))
    return view


@pytest.mark.parametrize("kind", ["u8", "f32"])
def test_best_update_rows_matches_the_reference(mods, kind):
    L = mods[0]
    cs = best_case(kind)
    n, c, n_slots = BEST_N, BEST_C, cs["n_slots"]
    face_bytes = cs["faces"][0].size * cs["faces"].itemsize
    for full in (True, False):                               # every optional pointer present, then absent
        bq_c = best_snapshot(cs, full)
        junk = best_junk(cs, 11)
        st = {k: v.copy() for k, v in junk.items()}
        kw = dict(w=cs["w"], factor=cs["factor"], status_rows=cs["status"], reset_c=cs["reset"], m=cs["m"]) if full else \
            dict(with_m=False, with_lm=False, with_rec=False)
        taken = rref.best_update_rows(st, cs["faces"], cs["rec"], cs["lm"], cs["slot"], bq_c, 42, **kw)
        assert taken.tolist() == ([True, False, True, False, False, False, False] if full else
                                  [True, False, False, True, False, False, False])
        if full:
            assert st["best_q"][0] == -1.0                   # reset and not eligible: the slot holds no best
        g = {k: dev(v) for k, v in junk.items()}
        faces = dev(cs["faces"])
        g["gallery"] = offset_bytes(junk["gallery"], 4)
        assert (faces.data_ptr() - g["gallery"].data_ptr()) % 16 != 0
        t = {k: dev(cs[k]) for k in ("rec", "lm", "w", "factor", "m", "status", "reset", "slot")}
        bq_d = dev(bq_c)
        p = lambda x: L.ptr(x) if full else None
        L.check(L.load().flm_track_best_update_rows(
            L.stream_ptr(), L.ptr(faces), face_bytes, n, L.ptr(t["rec"]), p(t["status"]), p(t["reset"]), L.ptr(t["lm"]), 2,
            p(t["w"]), 1, c, p(t["factor"]), p(t["m"]), 42, None, L.ptr(t["slot"]), n_slots, L.ptr(bq_d), L.ptr(g["best_q"]),
            L.ptr(g["gallery"]), L.ptr(g["best_frame"]), p(g["best_m"]), p(g["best_lm"]), p(g["best_rec"])),
            "flm_track_best_update_rows")
        for name in BEST_STATE:
            assert bits_equal(g[name], st[name]), (name, full)
        assert bits_equal(bq_d, bq_c) and bits_equal(faces, cs["faces"])
        named = np.zeros(n_slots, bool)
        named[cs["slot"][(cs["slot"] >= 0) & (cs["slot"] < n_slots)]] = True
        for name in BEST_STATE:                              # untouched slots keep their junk bit for bit
            assert np.array_equal(st[name][~named].view(np.uint8), junk[name][~named].view(np.uint8)), name
        assert np.array_equal(st["gallery"][cs["slot"][1]].view(np.uint8), junk["gallery"][cs["slot"][1]].view(np.uint8))
        assert np.array_equal(st["gallery"][cs["slot"][0]].view(np.uint8), cs["faces"][0].view(np.uint8))


@pytest.mark.parametrize("kind", ["u8", "f32"])
def test_identity_best_rows_are_the_best_update_on_the_device(mods, kind):
    L = mods[0]
    cs = best_case(kind)
    n, c = BEST_N, BEST_C
    face_bytes = cs["faces"][0].size * cs["faces"].itemsize
    bq_c = best_snapshot(cs, True)
    junk = best_junk(dict(cs, n_slots=n), 13)
    faces = dev(cs["faces"])
    t = {k: dev(cs[k]) for k in ("rec", "lm", "w", "factor", "m", "status", "reset")}
    slot, bq_in = dev(np.arange(n, dtype=np.int32)), dev(bq_c)
    got = []
    for rows in (False, True):
        g = {k: dev(v) for k, v in junk.items()}
        head = (L.stream_ptr(), L.ptr(faces), face_bytes, n, L.ptr(t["rec"]), L.ptr(t["status"]), L.ptr(t["reset"]),
                L.ptr(t["lm"]), 2, L.ptr(t["w"]), 1, c, L.ptr(t["factor"]), L.ptr(t["m"]), 9, None)
        tail = (L.ptr(bq_in), L.ptr(g["best_q"]), L.ptr(g["gallery"]), L.ptr(g["best_frame"]), L.ptr(g["best_m"]),
                L.ptr(g["best_lm"]), L.ptr(g["best_rec"]))
        if rows:
            L.check(L.load().flm_track_best_update_rows(*head, L.ptr(slot), n, *tail), "flm_track_best_update_rows")
        else:
            L.check(L.load().flm_track_best_update(*head, *tail), "flm_track_best_update")
        got.append(g)
    for name in BEST_STATE:
        a, b = got[0][name], got[1][name]
        assert torch.equal(a.view(torch.uint8).reshape(-1) if a.dtype != torch.uint8 else a.reshape(-1),
                           b.view(torch.uint8).reshape(-1) if b.dtype != torch.uint8 else b.reshape(-1)), name
    assert not bits_equal(got[1]["best_q"], junk["best_q"])


# ---- the three wrappers ------------------------------------------------------------------------------------------------
def test_wrappers_return_what_the_raw_calls_write_without_a_synchronisation(mods):
    L, A, P = mods
    # gather
    s, k, active = 5, 3, [4, -1, 1, 5]
    m, boxes, bq, reset, fi, dt = gather_state(s, k, 99)
    exp = rref.gather_streams(active, s, k, m, boxes, fi, dt, bq, reset)
    t = [dev(x) for x in (m, boxes, fi, dt, bq, reset)]
    act = dev(np.asarray(active, np.int32))
    mine = torch.full((len(active) * k,), 777, dtype=torch.int32, device="cuda")
    with sync_error(probe=act):
        snap = A.track_gather_streams_device(act, t[0], t[1], k, frame_index=t[2], dt=t[3], best_q=t[4], reset=t[5],
                                             out=dict(slot=mine))
    assert snap["slot"] is mine and sorted(snap) == ["best_q", "boxes", "dt", "frame_index", "m", "reset", "slot"]
    for name in snap:
        assert bits_equal(snap[name], exp[name]), name
    assert bits_equal(t[5], exp["reset_global"])
    with sync_error():
        bare = A.track_gather_streams_device(act, t[0], t[1], k)
    assert sorted(bare) == ["boxes", "frame_index", "m", "slot"] and not bare["frame_index"].any()
    with pytest.raises(ValueError, match="needs its input"):
        A.track_gather_streams_device(act, t[0], t[1], k, out=dict(dt=snap["dt"]))
    with pytest.raises(ValueError, match="overlap"):
        A.track_gather_streams_device(act, t[0], t[1], k, out=dict(m=t[0][:len(active) * k]))
    with pytest.raises(ValueError, match="slots_per_stream"):
        A.track_gather_streams_device(act, t[0], t[1], 4)
    with pytest.raises(ValueError, match="frame_index"):
        A.track_gather_streams_device(act, t[0], t[1], k, frame_index=t[2][:-1])
    # step rows
    n, c = 6, 68
    n_slots = 2 * n + 3
    seq = sequence(n, c, True)
    s0 = seq["steps"][0]
    slot = slot_map(n, n_slots, 1)
    junk = global_junk(n_slots, c, 2)
    dts = row_dt(n, 0)
    r = rref.step_rows(s0["lm"], s0["w"], s0["m_crop"], s0["boxes"], slot, SC, SC, IN, IN, FH, FW, seq["tc"], seq["ta"],
                       junk["m_next"], junk["boxes_next"], junk["status"], state=junk["state"], dt=dts, filt=dict(fref.DEFAULTS))
    glob = {name: dev(v) for name, v in junk.items()}
    rec = np.zeros((n, c, 6))
    rec[..., :2], rec[..., 2] = s0["lm"], s0["w"]
    rec_d, m_c, b_c, slot_d, dt_d = dev(rec), dev(s0["m_crop"]), dev(s0["boxes"]), dev(slot), dev(dts)
    tc, ta = dev(seq["tc"]), dev(seq["ta"])
    raw = torch.full((n, c, 2), NAN, dtype=torch.float64, device="cuda")
    with sync_error():
        lmf, ma, st_rows = A.track_step_rows_device(
            rec_d[..., :2], m_c, b_c, slot_d, (GRID, GRID), (IN, IN), (FH, FW), tc, glob["m_next"], glob["boxes_next"],
            glob["status"], tmpl_align=ta, weights=rec_d[..., 2], filter=A.LandmarkFilter(), dt=dt_d, state=glob["state"],
            lm_raw=raw)
    for got, name in ((lmf, "lm_frame"), (ma, "m_align"), (st_rows, "status_rows"), (raw, "lm_raw")):
        assert bits_equal(got, r[name]), name
    for name in GLOBAL:
        assert bits_equal(glob[name], r[name]), name
    with pytest.raises(ValueError, match="overlap"):
        A.track_step_rows_device(rec_d[..., :2], glob["m_next"][:n], b_c, slot_d, (GRID, GRID), (IN, IN), (FH, FW), tc,
                                 glob["m_next"], glob["boxes_next"], glob["status"])
    with pytest.raises(ValueError, match="overlap"):
        A.track_step_rows_device(rec_d[..., :2], m_c, glob["boxes_next"][3:3 + n], slot_d, (GRID, GRID), (IN, IN), (FH, FW), tc,
                                 glob["m_next"], glob["boxes_next"], glob["status"])
    with pytest.raises(ValueError, match="slot"):
        A.track_step_rows_device(rec_d[..., :2], m_c, b_c, slot_d[:-1], (GRID, GRID), (IN, IN), (FH, FW), tc, glob["m_next"],
                                 glob["boxes_next"], glob["status"])
    with pytest.raises(ValueError, match="dt"):
        A.track_step_rows_device(rec_d[..., :2], m_c, b_c, slot_d, (GRID, GRID), (IN, IN), (FH, FW), tc, glob["m_next"],
                                 glob["boxes_next"], glob["status"], filter=A.LandmarkFilter(), dt=dt_d[:-1], state=glob["state"])
    # best rows
    cs = best_case("u8")
    bq_c = best_snapshot(cs, True)
    junk = best_junk(cs, 11)
    st = {name: v.copy() for name, v in junk.items()}
    rref.best_update_rows(st, cs["faces"], cs["rec"], cs["lm"], cs["slot"], bq_c, 42, w=cs["w"], factor=cs["factor"],
                          status_rows=cs["status"], reset_c=cs["reset"], m=cs["m"])
    g = {name: dev(v) for name, v in junk.items()}
    t = {name: dev(cs[name]) for name in ("faces", "rec", "lm", "w", "factor", "m", "status", "reset", "slot")}
    bq_d = dev(bq_c)
    with sync_error():
        out = A.track_best_update_rows_device(t["faces"], t["rec"], t["lm"], t["slot"], bq_d, g["best_q"], g["gallery"],
                                              g["best_frame"], 42, status_rows=t["status"], reset_c=t["reset"], weights=t["w"],
                                              factor=t["factor"], m=t["m"], best_m=g["best_m"], best_lm=g["best_lm"],
                                              best_rec=g["best_rec"])
    assert out is g["best_q"]
    for name in BEST_STATE:
        assert bits_equal(g[name], st[name]), name
    with pytest.raises(ValueError, match="overlap"):
        A.track_best_update_rows_device(t["faces"], t["rec"], t["lm"], t["slot"], g["best_q"][:BEST_N], g["best_q"], g["gallery"],
                                        g["best_frame"], 42)
    with pytest.raises(ValueError, match="gallery"):
        A.track_best_update_rows_device(t["faces"], t["rec"], t["lm"], t["slot"], bq_d, g["best_q"], g["gallery"][:, :4],
                                        g["best_frame"], 42)
    with pytest.raises(ValueError, match="best_m needs m"):
        A.track_best_update_rows_device(t["faces"], t["rec"], t["lm"], t["slot"], bq_d, g["best_q"], g["gallery"],
                                        g["best_frame"], 42, best_m=g["best_m"])


# ---- FaceTracker.step_active -------------------------------------------------------------------------------------------
RH, RW, CAP, S, K = 64, 96, 9, 3, 3
FACES = [(20, 8, 60, 50), (40, 2, 90, 60), (-6, 20, 30, 58), (30, 10, 80, 60)]
SEEDS = {0: ([0, 2], FACES[:2]), 1: ([1, 2], FACES[2:]), 2: ([0], FACES[:1])}     # stream -> (its local slots, the boxes)
STATE = ("m_crop", "boxes", "status", "misses", "filter_state")
BEST = ("gallery", "best_q", "best_frame", "best_M", "best_landmarks", "best_rec", "_best_reset")


@pytest.fixture(scope="module")
def rings(mods):
    L, A, P = mods
    rng = np.random.default_rng(31)
    bgr = rng.integers(0, 256, (8, RH, RW, 3), dtype=np.uint8)
    nv = np.stack([nv12_ref.pack_slot(*nv12_ref.bgr_to_nv12(bgr[f], "bt709"), RW, RH, RH * 3 // 2) for f in range(8)])
    return {"bgr": (dev(bgr), None), "nv12": (dev(nv), A.FrameFormat.nv12(RH, RW, matrix="bt709"))}


@pytest.fixture(scope="module")
def model():
    from flm_amd.networks import LANDMARKS_MODELS
    from flm_amd.weights import synth_fcn8_weights
    m = LANDMARKS_MODELS["fcn_8"](68, input_height=64, input_width=64, dtype="bf16")
    m.load_weights(synth_fcn8_weights(68, seed=2))
    return m


def make_tracker(mods, model, ff, smooth, best_shot, streams=S, capacity=CAP):
    L, A, P = mods
    return P.FaceTracker(model, (RH, RW), capacity, frame_format=ff, smooth=smooth, best_shot=best_shot,
                         weights="score" if best_shot else None, associate=A.TrackAssociation(match_iou=2.0), streams=streams)


def state_of(tr):
    names = STATE[:4] + (("filter_state",) if tr.smooth is not None else ()) + (BEST if tr.best_shot is not None else ())
    return {n: getattr(tr, n).clone() for n in names}


def assert_state(a, b, what):
    assert sorted(a) == sorted(b)
    for name in a:
        assert same(a[name], b[name]), (name,) + tuple(what)


@pytest.mark.parametrize("best_shot", [None, True])
@pytest.mark.parametrize("smooth", [None, True])
def test_all_streams_active_is_step(mods, rings, model, smooth, best_shot):
    """(a): the batch is the same, so every returned tensor and every state tensor has the bits of `step`."""
    L, A, P = mods
    for source in ("bgr", "nv12"):
        ring, ff = rings[source]
        one, two = [make_tracker(mods, model, ff, smooth, best_shot) for _ in range(2)]
        for tr in (one, two):
            for i, (slots, faces) in SEEDS.items():
                tr.seed(slots, faces, stream=i)
        dt = dict(dt=0.04) if smooth else {}
        for t, fi in enumerate(([0, 3, 6], [1, 4, 7], [2, 5, 0])):
            fid = dict(frame_id=100 + t) if best_shot and t == 1 else {}
            exp = [x.clone() for x in one.step(ring, fi, **dt, **fid)]
            got = two.step_active(ring, fi, [0, 1, 2], **dt, **fid)
            assert len(got) == 5 and torch.equal(got[4].cpu(), torch.arange(CAP, dtype=torch.int32))
            for a, b in zip(got[:4], exp):
                assert same(a, b), (source, t)
            assert_state(state_of(one), state_of(two), (source, t))
            if t == 0:
                assert (exp[3] == 0).any() and exp[0].any()
        assert one._steps == two._steps == 3
        assert two._ws_active is not None and two._ws_active.numel() == model.workspace_bytes(
            CAP, "landmark_stats" if best_shot else "landmarks", 4)


SCHEDULE = ([0, 1, 2], [0], [2, 0], [1], [0, 2], [1, 2])
RING_SLOT = lambda t, i: (3 * t + 2 * i + 1) % 8            # the ring slot stream i reads at tick t
BORN = 1 * K + 0                                            # stream 1's free slot: where the update's detection is born


def hand_tick(mods, tr, model, ring, ff, fi, active, dt_of, frame_id):
    """One tick made by hand on the tensors of `tr` at the SAME batch: hand-gathered matrices and boxes, the warps, the
    forward, track_step_device per stream on gathered copies of the state with the stream's own dt, the best update on
    gathered copies, and everything scattered back."""
    L, A, P = mods
    g = torch.tensor([a * K + j for a in active for j in range(K)], dtype=torch.int64, device="cuda")
    idx = dev(np.repeat(np.asarray([fi[a] for a in active], np.int32), K))
    m_c, b_c = tr.m_crop.index_select(0, g).contiguous(), tr.boxes.index_select(0, g).contiguous()
    crops = A.warp_frames_device(ring, m_c, 64, 64, frame_index_dev=idx, boxes_dev=b_c, samples=tr.crop_samples,
                                 fmt=A.AlignedFormat("nhwc", "uint8"), src=ff)
    if tr.weights is None:
        lm, wd = model.forward_device(crops, "landmarks", n_points=tr.n_points, thresh=tr.thresh), None
    else:
        rec = model.forward_device(crops, "landmark_stats", n_points=tr.n_points, thresh=tr.thresh)
        lm, wd = rec[..., :2], rec[..., 2]
    n = int(g.shape[0])
    lmf = torch.empty((n, 68, 2), dtype=torch.float64, device="cuda")
    ma, mn = [torch.empty((n, 2, 3), dtype=torch.float32, device="cuda") for _ in range(2)]
    bn = torch.empty((n, 4), dtype=torch.int32, device="cuda")
    st = torch.empty((n,), dtype=torch.int32, device="cuda")
    for i, a in enumerate(active):
        sl = slice(i * K, (i + 1) * K)
        filt = {}
        if tr.smooth is not None:
            st_c = tr.filter_state.index_select(0, g[sl]).contiguous()
            filt = dict(filter=tr.smooth, dt=dt_of[a], state=st_c)
        A.track_step_device(lm[sl], m_c[sl], b_c[sl], (72, 72), (64, 64), (RH, RW), tr.crop_template, tr.template,
                            weights=None if wd is None else wd[sl], lm_frame=lmf[sl], m_align=ma[sl], m_next=mn[sl],
                            boxes_next=bn[sl], status=st[sl], **tr.limits, **filt)
        if tr.smooth is not None:
            tr.filter_state.index_copy_(0, g[sl], st_c)
    aligned = A.warp_frames_device(ring, ma, 112, 112, frame_index_dev=idx, boxes_dev=b_c, samples=tr.samples,
                                   fmt=tr.aligned_format, src=ff)
    tr.m_crop.index_copy_(0, g, mn)
    tr.boxes.index_copy_(0, g, bn)
    tr.status.index_copy_(0, g, st)
    if tr.best_shot is not None:
        qrec = A.face_quality_device(aligned, tr.aligned_format, tr.best_shot.quality)
        names = ("best_q", "gallery", "best_frame", "best_M", "best_landmarks", "best_rec", "_best_reset")
        c = {nm: getattr(tr, nm).index_select(0, g).contiguous() for nm in names}
        bq_out = torch.empty_like(c["best_q"])
        A.track_best_update_device(aligned, qrec, lmf, c["best_q"], bq_out, c["gallery"], c["best_frame"], frame_id, status=st,
                                   reset=c["_best_reset"], weights=wd, m=ma, opts=tr.best_shot, best_m=c["best_M"],
                                   best_lm=c["best_landmarks"], best_rec=c["best_rec"])
        c["best_q"] = bq_out
        c["_best_reset"].zero_()
        for nm in names:
            getattr(tr, nm).index_copy_(0, g, c[nm])
    tr._steps += 1
    return aligned, ma, lmf, st, g.to(torch.int32)


@pytest.mark.parametrize("best_shot", [None, True])
@pytest.mark.parametrize("smooth", [None, True])
@pytest.mark.parametrize("source", ["bgr", "nv12"])
def test_a_schedule_of_streams_is_the_sequence_made_by_hand(mods, rings, model, source, smooth, best_shot):
    """(b) and (c): six ticks on which streams sit out, each stream on its own dt, an update with a birth in a stream
    that sits the next two ticks out, a re-seed -- with host arguments, and with `active`, `frame_index` and `dt` on the
    device inside sync-debug "error" -- against the sequence made by hand, after every tick, on every tensor."""
    L, A, P = mods
    ring, ff = rings[source]
    hand, host, devc = [make_tracker(mods, model, ff, smooth, best_shot) for _ in range(3)]
    trackers = (hand, host, devc)
    for tr in trackers:
        for i, (slots, faces) in SEEDS.items():
            tr.seed(slots, faces, stream=i)
    last = [None] * S
    alive = 0
    for t, active in enumerate(SCHEDULE):
        fi = [RING_SLOT(t, i) for i in range(S)]
        dts = [(1 if last[i] is None else t - last[i]) / 30.0 for i in range(S)]     # the ticks since the stream's last frame
        for i in active:
            last[i] = t
        fid = 1000 + 7 * t if best_shot and t % 2 else None
        before = state_of(hand)
        exp = hand_tick(mods, hand, model, ring, ff, fi, active, dts, hand._steps if fid is None else fid)
        # host forms: the entries of the streams that sit out are None
        kw = {} if fid is None else dict(frame_id=fid)
        if smooth:
            kw["dt"] = [dts[i] if i in active else None for i in range(S)]
        got = host.step_active(ring, [fi[i] if i in active else None for i in range(S)], active, **kw)
        # device forms: nothing is transferred, nothing synchronises
        act_d, fi_d = dev(np.asarray(active, np.int32)), dev(np.asarray(fi, np.int32))
        if smooth:
            kw["dt"] = dev(np.asarray(dts, f64))
        with sync_error(probe=fi_d if t == 0 else None):
            got_d = devc.step_active(ring, fi_d, act_d, **kw)
        for how, res, tr in (("host", got, host), ("device", got_d, devc)):
            assert len(res) == 5
            for a, b in zip(res, exp):
                assert same(a, b), (how, t)
            assert_state(state_of(tr), state_of(hand), (how, t))
            assert tr._steps == hand._steps == t + 1
        # the streams that sat out kept every bit
        after = state_of(host)
        rows = [i * K + j for i in range(S) if i not in active for j in range(K)]
        for name in after:
            assert same(after[name][rows], before[name][rows]), (name, t)
        alive += int((exp[3] == 0).sum())
        if t == 0:                       # a detection in stream 1, which sits the next two ticks out: a birth in its free slot
            for tr in trackers:
                if best_shot:
                    tr.best_q[BORN] = 9.0                    # (more than any face reaches: only a reset lets one in)
                up = tr.update([None, [(50, 10, 90, 50)], None])
            assert up[2][1].tolist()[:2] == [0, 1] and int(up[0][1][0]) == BORN
        if best_shot and t in (1, 2):    # the pending reset survives the ticks its stream sits out ...
            assert int(host._best_reset[BORN]) == 1 and float(host.best_q[BORN]) == 9.0
        if best_shot and t == 3:         # ... and takes effect on the stream's next frame
            assert int(host._best_reset[BORN]) == 0 and float(host.best_q[BORN]) != 9.0
        if t == 3:
            for tr in trackers:
                tr.seed([1], FACES[1:2], stream=2)
    assert alive > 0
    print(source, smooth, best_shot, "rows alive over the schedule:", alive, "status:", host.status.tolist())


@pytest.mark.parametrize("best_shot", [None, True])
@pytest.mark.parametrize("smooth", [None, True])
def test_one_stream_active_is_step(mods, rings, model, smooth, best_shot):
    """(d): streams=1 with active=[0] equals `step`; an empty `active` launches nothing; the two may be mixed."""
    L, A, P = mods
    ring, ff = rings["nv12"]
    one, two = [make_tracker(mods, model, ff, smooth, best_shot, streams=1, capacity=4) for _ in range(2)]
    for tr in (one, two):
        tr.seed([0, 2, 1], FACES[:3])
    for t, fi in enumerate((1, 0, 5, 2)):
        exp = [x.clone() for x in one.step(ring, fi)]
        if t == 2:
            got = two.step(ring, fi)                         # mixed freely
        else:
            got = two.step_active(ring, fi if t else [fi], [0])
            assert torch.equal(got[4].cpu(), torch.arange(4, dtype=torch.int32))
        for a, b in zip(got[:4], exp):
            assert same(a, b), t
        assert_state(state_of(one), state_of(two), (t,))
    before = state_of(two)
    with sync_error():
        res = two.step_active(ring, [0], [])
    assert [tuple(x.shape)[0] for x in res] == [0] * 5 and res[0].shape[1:] == exp[0].shape[1:] and two._steps == 4
    assert_state(state_of(two), before, ("empty",))
