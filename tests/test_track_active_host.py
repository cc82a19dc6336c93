"""CPU-side checks of stepping a subset of the streams (flm_track_gather_streams, flm_track_step_rows,
flm_track_best_update_rows, their wrappers in alignment, FaceTracker.step_active): the symbols, every argument check
answered before any launch (so without a GPU), the Python rejections, the compiler's metadata of the new kernels, the
monotone workspace, and -- on the references alone -- the reason for the feature: a camera that delivered nothing must
not be stepped with its stale frame."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import flm_amd  # noqa: F401
from flm_amd import _lib, alignment, prediction

import face_quality_ref as qref
import track_filter_ref as fref
import track_ref
import track_rows_ref as rref

NAN, INF = float("nan"), float("inf")
IN, GRID, FH, FW = 64, 72, 270, 480
SC = IN / GRID
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "face-landmark-detector_amd", "csrc")


def test_library_exports_the_three_calls():
    lib = C.CDLL(_lib.LIB_PATH)
    for name in ("flm_track_gather_streams", "flm_track_step_rows", "flm_track_best_update_rows"):
        assert hasattr(lib, name) and name in _lib.EXPORTS, name
    L = _lib.load()
    assert L.flm_abi_version() == 2                                   # purely additive
    assert len(L.flm_track_step_rows.argtypes) == len(L.flm_track_step_filtered.argtypes) + 4
    assert len(L.flm_track_best_update_rows.argtypes) == len(L.flm_track_best_update.argtypes) + 2
    assert len(L.flm_track_gather_streams.argtypes) == 18
    assert C.sizeof(_lib.TrackOpts) == 32 and C.sizeof(_lib.TrackFilter) == 32 and C.sizeof(_lib.BestOpts) == 24


P = C.c_void_p(0x1000)        # never dereferenced: every call below is rejected before a launch
err = lambda: _lib.load().flm_last_error().decode()


def _gather(**kw):
    a = dict(active=P, a=2, s=3, k=4, fi=P, dt=P, m=P, boxes=P, bq=P, reset=P, slot_c=P, m_c=P, boxes_c=P, fi_c=P, dt_c=P,
             bq_c=P, reset_c=P)
    a.update(kw)
    return _lib.load().flm_track_gather_streams(None, *[a[n] for n in ("active", "a", "s", "k", "fi", "dt", "m", "boxes", "bq",
                                                                        "reset", "slot_c", "m_c", "boxes_c", "fi_c", "dt_c",
                                                                        "bq_c", "reset_c")])


def test_gather_argument_checks_answer_without_a_gpu():
    who = "flm_track_gather_streams"
    for name in ("active", "m", "boxes", "slot_c", "m_c", "boxes_c", "fi_c"):
        assert _gather(**{name: None}) == -1 and "null" in err() and who in err(), name
    for name in ("dt", "dt_c", "bq", "bq_c", "reset", "reset_c"):      # an output without its input, or the reverse
        assert _gather(**{name: None}) == -1 and "go together" in err() and who in err(), name
    for kw in (dict(a=0), dict(a=-1), dict(s=0), dict(k=0), dict(k=-3)):
        assert _gather(**kw) == -2 and "1 <= a" in err(), kw
    for kw in (dict(a=16384, k=4, s=1), dict(a=1, s=16384, k=4), dict(a=2 ** 31 - 1, s=1, k=2 ** 31 - 1), dict(a=1, s=65536, k=1),
               dict(a=65536, s=1, k=1)):
        assert _gather(**kw) == -2 and "65535" in err(), kw


def _step(filt="default", **kw):
    a = dict(lm=P, ls=2, w=P, ws=1, m=P, boxes=P, n=4, c=68, sx=SC, sy=SC, in_h=IN, in_w=IN, fh=FH, fw=FW, tc=P, ta=P, opts=None,
             lmf=P, ma=P, mn=C.c_void_p(0x100000), bn=C.c_void_p(0x200000), st=C.c_void_p(0x300000), dt=1 / 30, state=P, raw=P,
             slot=P, n_slots=9, dtr=None, str_=C.c_void_p(0x400000))
    a.update(kw)
    fo = _lib.TrackFilter.make() if isinstance(filt, str) else filt
    o = a["opts"]
    return _lib.load().flm_track_step_rows(
        None, a["lm"], a["ls"], a["w"], a["ws"], a["m"], a["boxes"], a["n"], a["c"], a["sx"], a["sy"], a["in_h"], a["in_w"],
        a["fh"], a["fw"], a["tc"], a["ta"], None if o is None else C.byref(o), a["lmf"], a["ma"], a["mn"], a["bn"], a["st"],
        None if fo is None else C.byref(fo), a["dt"], a["state"], a["raw"], a["slot"], a["n_slots"], a["dtr"], a["str_"])


def test_step_rows_argument_checks_answer_without_a_gpu():
    who = "flm_track_step_rows"
    for name in ("lm", "m", "boxes", "tc", "lmf", "mn", "bn", "st", "slot", "str_", "state"):
        assert _step(**{name: None}) == -1 and "null" in err() and who in err(), name
    assert _step(ta=None) == -1 and "go together" in err()
    assert _step(ma=None) == -1 and "go together" in err()
    o = _lib.TrackOpts.make()
    o.struct_size -= 8
    assert _step(opts=o) == -1 and "struct_size" in err()
    assert _step(opts=_lib.TrackOpts.make(min_points=1)) == -1 and "min_points" in err()
    for kw in (dict(min_score=NAN), dict(min_side=NAN), dict(max_side=NAN)):
        assert _step(opts=_lib.TrackOpts.make(**kw)) == -1 and "NaN" in err()
    # the filter's own
    f = _lib.TrackFilter.make()
    f.struct_size -= 8
    assert _step(filt=f) == -1 and "struct_size" in err()
    f = _lib.TrackFilter.make()
    f.reserved = 1
    assert _step(filt=f) == -1 and "reserved" in err()
    for kw, word in ((dict(min_cutoff=0.0), "min_cutoff"), (dict(min_cutoff=NAN), "min_cutoff"), (dict(beta=-1.0), "beta"),
                     (dict(beta=INF), "beta"), (dict(d_cutoff=0.0), "d_cutoff"), (dict(d_cutoff=INF), "d_cutoff")):
        assert _step(filt=_lib.TrackFilter.make(**kw)) == -1 and word in err(), kw
    for dt in (0.0, -1.0, NAN, INF):                                  # the scalar dt is checked only without dt_dev
        assert _step(dt=dt) == -1 and "dt=" in err()
        assert _step(dt=dt, dtr=P, n=0) == -2 and "1 <= n" in err()
    # without a filter: the filter's tensors must be absent, and dt is not read
    for kw in (dict(), dict(raw=None), dict(state=None, raw=None, dtr=P)):
        assert _step(filt=None, **kw) == -1 and "go with filt" in err(), kw
    assert _step(filt=None, state=None, raw=None, dt=NAN, n=0) == -2 and "1 <= n" in err()
    # overlaps of the compact inputs with what is written at the slots
    for kw in (dict(mn=P), dict(bn=P), dict(st=P, str_=P)):
        assert _step(**kw) == -1 and "overlap" in err(), kw
    # shapes
    for n in (0, -1, 65536):
        assert _step(n=n) == -2 and "1 <= n <= 65535" in err()
    for n_slots in (0, -5, 65536):
        assert _step(n_slots=n_slots) == -2 and "1 <= n_slots <= 65535" in err()
    for c in (0, 1025):
        assert _step(c=c) == -2 and "1 <= c <= 1024" in err()
    for kw in (dict(in_h=0), dict(in_w=-1), dict(fh=0), dict(fw=0)):
        assert _step(**kw) == -2 and "in_h, in_w, fh, fw >= 1" in err()
    assert _step(ls=1) == -2 and "lm_stride >= 2" in err()
    assert _step(ws=0) == -2 and "w_stride >= 1" in err()
    for kw in (dict(sx=0.0), dict(sy=-1.0), dict(sx=NAN)):
        assert _step(**kw) == -2 and "sx, sy > 0" in err()
    # what is allowed reaches the last check (c): the most rows and slots, no weights, no aligned pair, no lm_raw, dt_dev
    for kw in (dict(n=65535, n_slots=65535, mn=C.c_void_p(0x10000000), bn=C.c_void_p(0x20000000)), dict(w=None),
               dict(ta=None, ma=None), dict(raw=None), dict(dtr=P, dt=NAN), dict(n_slots=1, n=7)):
        assert _step(c=0, **kw) == -2 and "1 <= c" in err() and who in err(), kw
    assert _step(filt=None, state=None, raw=None, c=0) == -2 and "1 <= c" in err()


def _best(**kw):
    a = dict(faces=C.c_void_p(0x100000), fb=105, n=4, rec=P, st=P, reset=P, lm=P, ls=2, w=P, ws=1, c=68, factor=P, m=P, fid=7,
             opts=None, slot=P, n_slots=9, bq_c=P, bq=C.c_void_p(0x2000), gal=C.c_void_p(0x200000), bf=P, bm=P, blm=P, brec=P)
    a.update(kw)
    o = a["opts"]
    return _lib.load().flm_track_best_update_rows(
        None, a["faces"], a["fb"], a["n"], a["rec"], a["st"], a["reset"], a["lm"], a["ls"], a["w"], a["ws"], a["c"], a["factor"],
        a["m"], a["fid"], None if o is None else C.byref(o), a["slot"], a["n_slots"], a["bq_c"], a["bq"], a["gal"], a["bf"],
        a["bm"], a["blm"], a["brec"])


def test_best_update_rows_argument_checks_answer_without_a_gpu():
    who = "flm_track_best_update_rows"
    for name in ("faces", "rec", "lm", "slot", "bq_c", "bq", "gal", "bf"):
        assert _best(**{name: None}) == -1 and "null" in err() and who in err(), name
    assert _best(m=None) == -1 and "best_m_dev needs m_dev" in err()
    o = _lib.BestOpts.make()
    o.struct_size -= 8
    assert _best(opts=o) == -1 and "struct_size" in err()
    o = _lib.BestOpts.make()
    o.reserved = 1
    assert _best(opts=o) == -1 and "reserved" in err()
    for v in (0.0, -1.0, NAN):
        assert _best(opts=_lib.BestOpts.make(sharp_ref=v)) == -1 and "sharp_ref" in err()
    assert _best(opts=_lib.BestOpts.make(min_exposed=NAN)) == -1 and "min_exposed" in err()
    for n in (0, -1, 65536):
        assert _best(n=n) == -2 and "1 <= n <= 65535" in err()
    for n_slots in (0, -1, 65536):
        assert _best(n_slots=n_slots) == -2 and "1 <= n_slots <= 65535" in err()
    assert _best(c=0) == -2 and "c >= 1" in err()
    assert _best(fb=0) == -2 and "face_bytes" in err()
    assert _best(ls=1) == -2 and "lm_stride" in err()
    assert _best(ws=0) == -2 and "w_stride" in err()
    assert _best(bq=P) == -1 and "best_q_c and best_q overlap" in err()
    assert _best(bq=C.c_void_p(0x1000 + 8 * 3)) == -1 and "overlap" in err()          # (the snapshot's last entry)
    assert _best(gal=C.c_void_p(0x100000 + 105 * 3)) == -1 and "faces_dev and gallery_dev overlap" in err()
    assert _best(faces=C.c_void_p(0x200000 + 105 * 8)) == -1 and "faces_dev and gallery_dev overlap" in err()
    # every optional pointer absent reaches the last check
    assert _best(st=None, reset=None, w=None, ws=0, factor=None, m=None, bm=None, blm=None, brec=None,
                 gal=C.c_void_p(0x100000 + 105 * 3)) == -1 and "gallery_dev overlap" in err()


# ---- the Python rejections ---------------------------------------------------------------------------------------------
class _Model:
    n_classes, input_height, input_width, output_height, output_width = 68, 64, 64, 72, 72
    max_batch = 1024


class _HostRing(alignment.FrameFormat):
    """A frame format whose ring needs no device: 8 slots of the tracker's frames."""

    def ring(self, frames):
        return 8, FH, FW, FH * FW * 3


def test_step_active_rejects_what_it_must_on_the_host():
    mk = lambda **kw: prediction.FaceTracker(_Model(), (FH, FW), 6, streams=3, frame_format=_HostRing.bgr(), **kw)
    tr = mk(smooth=True, best_shot=True)
    fi = [0, 1, 2]
    for bad in ([0, 0], [1, 2, 1], [3], [-1], [0, 3], [0.5], [True], 1, None):          # duplicate, out of range, not a list
        with pytest.raises(ValueError, match="active"):
            tr.step_active(None, fi, bad)
    for bad in (torch.zeros(2, dtype=torch.int32), torch.zeros(2, dtype=torch.int64)):   # (not on the device)
        with pytest.raises(ValueError, match="active"):
            tr.step_active(None, fi, bad)
    for bad in (3, [1], [0, 1], [0, 1, 2, 3]):
        with pytest.raises(ValueError, match="sequence of 3"):
            tr.step_active(None, bad, [0])
    for bad, act in (([0, 8, 0], [1]), ([None, 0, 0], [0]), ([0, 0, -1], [2, 0]), ([0.5, 0, 0], [0]), ([True, 0, 0], [0])):
        with pytest.raises(ValueError, match=r"\[0, 8\)"):
            tr.step_active(None, bad, act)
    with pytest.raises(ValueError, match="CUDA int32"):
        tr.step_active(None, torch.zeros(3, dtype=torch.int32), [0])
    for bad in ([1 / 30], [1 / 30] * 4, "ab", torch.ones(3, dtype=torch.float64)):
        with pytest.raises(ValueError, match="sequence of 3 numbers"):
            tr.step_active(None, fi, [0], dt=bad)
    for bad, act in (([0.0, 1, 1], [0]), ([1, -1.0, 1], [1]), ([1, 1, NAN], [2]), ([INF, 1, 1], [1, 0]), ([None, 1, 1], [0])):
        with pytest.raises(ValueError, match="dt of stream"):
            tr.step_active(None, fi, act, dt=bad)
    for bad in (0.0, -0.1, NAN, INF):
        with pytest.raises(ValueError, match="dt must be finite"):
            tr.step_active(None, fi, [0], dt=bad)
    for bad in (1.5, True, 2 ** 63):
        with pytest.raises(ValueError, match="frame_id"):
            tr.step_active(None, fi, [0], frame_id=bad)
    with pytest.raises(ValueError, match="dt goes with smooth"):
        mk().step_active(None, fi, [0], dt=1 / 30)
    with pytest.raises(ValueError, match="frame_id goes with best_shot"):
        mk(smooth=True).step_active(None, fi, [0], frame_id=3)

    class _OtherRing(alignment.FrameFormat):
        def ring(self, frames):
            return 8, FH + 2, FW, 0

    with pytest.raises(ValueError, match="the ring holds"):
        prediction.FaceTracker(_Model(), (FH, FW), 6, streams=3, frame_format=_OtherRing.bgr()).step_active(None, fi, [0])


def test_wrappers_reject_what_they_must_on_the_host():
    A = alignment
    m, boxes = torch.zeros((6, 2, 3)), torch.zeros((6, 4), dtype=torch.int32)
    with pytest.raises(ValueError, match="active"):                    # (not on the device)
        A.track_gather_streams_device(torch.zeros(2, dtype=torch.int32), m, boxes, 3)
    with pytest.raises(ValueError, match="active"):
        A.track_gather_streams_device([0, 1], m, boxes, 3)
    lm = torch.zeros((2, 5, 2), dtype=torch.float64)
    with pytest.raises(ValueError, match="go with filter"):
        A.track_step_rows_device(lm, m, boxes, None, (72, 72), (64, 64), (FH, FW), None, m, boxes, None, dt=0.1)
    with pytest.raises(ValueError, match="LandmarkFilter"):
        A.track_step_rows_device(lm, m, boxes, None, (72, 72), (64, 64), (FH, FW), None, m, boxes, None, filter="yes")
    with pytest.raises(ValueError, match="opts"):
        A.track_best_update_rows_device(m, None, lm, None, None, None, None, None, 0, opts="sharp")
    with pytest.raises(ValueError, match="frame_id"):
        A.track_best_update_rows_device(m, None, lm, None, None, None, None, None, 0.5)


# ---- the compiler's metadata of the kernels this feature adds --------------------------------------------------------
NEW_KERNELS = ("track_gather_streams_kernel", "track_step_rows_kernelILb0E", "track_step_rows_kernelILb1E",
               "track_best_rows_kernel")


def _metadata(src, tmp):
    """name -> dict of the integer fields of the kernel's metadata, as tests/test_build_hygiene.py reads them."""
    out = os.path.join(tmp, src + ".s")
    cmd = ["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
           "-I", CSRC, "-S", "--cuda-device-only", os.path.join(CSRC, src), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels = {}
    for block in open(out).read().split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        kernels[name] = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\n", block)}
    return kernels


def test_new_kernels_compile_for_gfx950_without_scratch(tmp_path):
    md = {}
    for src in ("flm_track.hip", "flm_quality.hip"):
        md.update(_metadata(src, str(tmp_path)))
    for want in NEW_KERNELS:
        names = [n for n in md if want in n]
        assert len(names) == 1, (want, sorted(md))
        k = md[names[0]]
        print(want, {f: k[f] for f in ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")})
        assert k["private_segment_fixed_size"] == 0, (want, k)
    # the kernels whose body is now shared keep theirs at 0 too
    shared = [n for n in md if "track_step_kernel" in n or "track_best_kernel" in n]
    assert len(shared) == 3 and all(md[n]["private_segment_fixed_size"] == 0 for n in shared)
    # the rows kernels are the shared body plus the row map: no more vector registers than the kernels they extend
    for a, b in (("track_step_rows_kernelILb0E", "track_step_kernelILb0E"), ("track_step_rows_kernelILb1E", "track_step_kernelILb1E"),
                 ("track_best_rows_kernel", "track_best_kernel")):
        va = [md[n]["vgpr_count"] for n in md if a in n][0]
        vb = [md[n]["vgpr_count"] for n in md if b in n][0]
        assert va <= vb + 8, (a, va, vb)


def test_workspace_bytes_do_not_decrease_with_the_batch():
    """What lets FaceTracker.step_active run every batch in one workspace sized for the largest."""
    from flm_amd.networks import LANDMARKS_MODELS
    for hw, sizes in ((64, range(1, 19)), (256, [16 * a for a in (1, 4, 16, 32, 64)] + [1, 7, 255, 257, 1023])):
        m = LANDMARKS_MODELS["fcn_8"](68, input_height=hw, input_width=hw, dtype="bf16")
        for out in ("landmarks", "landmark_stats"):
            b = [m.workspace_bytes(n, out, n_points=4) for n in sorted(sizes)]
            assert all(x <= y for x, y in zip(b, b[1:])), (hw, out, b)
            assert b[0] < b[-1]


# ---- the references alone ----------------------------------------------------------------------------------------------
def _bits(a, b):
    u = {1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(u), np.ascontiguousarray(b).view(u))


def _points(c, t, cx, cy):
    tc = alignment.canonical_template(c, IN, IN)
    return (tc - (IN - 1) / 2.0) * 1.2 + np.array([cx + 2.5 * t, cy + 1.5 * t])


def test_a_stale_frame_must_not_be_stepped():
    """Two streams of one slot; stream 1 delivers every other tick.  Stepped with its stale frame its filter sees the
    same raw points again -- the state changes, the velocity estimate shrinks -- and its face is offered to the best shot
    a second time; left out of `active`, every bit of it stays."""
    c, dt = 8, 1.0 / 30.0
    tc, ta = alignment.canonical_template(c, IN, IN), alignment.canonical_template(c, 112, 112)
    boxes = np.array([[100, 60, 180, 140], [200, 80, 280, 160]], np.int32)
    m, st = track_ref.seed(boxes, IN, IN, FH, FW)
    state = fref.empty_state(2, c)
    filt = dict(fref.DEFAULTS)
    glob = dict(m_next=m, boxes_next=boxes, status=st, state=state)
    pts = lambda t: np.stack([_points(c, t, 140, 100), _points(c, t, 240, 120)])

    def tick(glob, frames, active, dts):
        """One step of the rows `active`; frames[i]: the time of the frame stream i shows."""
        lm = np.stack([track_ref.apply(glob["m_next"][i], pts(frames[i])[i]) / SC for i in active])
        r = rref.step_rows(lm, None, glob["m_next"][active], glob["boxes_next"][active], active, SC, SC, IN, IN, FH, FW, tc, ta,
                           glob["m_next"], glob["boxes_next"], glob["status"], state=glob["state"], dt=np.asarray(dts, np.float64),
                           filt=filt)
        return r, {k: r[k] for k in glob}

    _, g1 = tick(glob, [0, 0], [0, 1], [dt, dt])
    r2, g2 = tick(g1, [1, 1], [0, 1], [dt, dt])                       # both delivered: stream 1 moves
    v2 = np.hypot(g2["state"][1, :, 2], g2["state"][1, :, 3])
    assert (g2["status"] == 0).all() and (v2 > 1.0).all()
    # tick 3, stream 1 has nothing new.  (a) stepped anyway, with frame 1 again and the tick's dt:
    _, stale = tick(g2, [2, 1], [0, 1], [dt, dt])
    vs = np.hypot(stale["state"][1, :, 2], stale["state"][1, :, 3])
    assert not _bits(stale["state"][1], g2["state"][1]) and not _bits(stale["m_next"][1], g2["m_next"][1])
    assert (vs < 0.9 * v2).all()                                      # the same raw point again: the velocity decays
    # (b) left out: stream 1 keeps every bit, stream 0 is what it was in (a)
    r3, skip = tick(g2, [2, 1], [0], [dt])
    for name in ("m_next", "boxes_next", "status", "state"):
        assert _bits(skip[name][1], g2[name][1]) and _bits(skip[name][0], stale[name][0]), name

    # the best shot: one face per stream, offered at tick 2 (frame_id 2); stream 1's slot was born before tick 3
    faces = np.random.default_rng(0).integers(0, 256, (2, 12, 12, 3)).astype(np.uint8)
    rec = qref.record(faces, ("nhwc", "uint8", "bgr", (1, 1, 1), (0, 0, 0)))
    best = qref.new_state(faces, 2, c)
    kw = dict(sharp_ref=1.0, min_exposed=0.0)
    both = np.array([0, 1], np.int32)
    taken = rref.best_update_rows(best, faces, rec, r2["lm_frame"], both, best["best_q"].copy(), 2, status_rows=r2["status_rows"], **kw)
    assert taken.all() and best["best_frame"].tolist() == [2, 2]
    reset = np.array([0, 1], np.int32)                                # a pending reset of stream 1's slot
    snap = rref.gather_streams([0, 1], 2, 1, g2["m_next"], g2["boxes_next"], best_q=best["best_q"], reset=reset)
    twice = {k: v.copy() for k, v in best.items()}
    t = rref.best_update_rows(twice, faces, rec, r2["lm_frame"], snap["slot"], snap["best_q"], 3, reset_c=snap["reset"], **kw)
    assert t.tolist() == [False, True] and twice["best_frame"].tolist() == [2, 3]      # the stale face again, as frame 3's
    assert not snap["reset_global"].any()                                              # ... and the reset is spent on it
    snap = rref.gather_streams([0], 2, 1, g2["m_next"], g2["boxes_next"], best_q=best["best_q"], reset=reset)
    once = {k: v.copy() for k, v in best.items()}
    t = rref.best_update_rows(once, faces[:1], rec[:1], r3["lm_frame"], snap["slot"], snap["best_q"], 3, reset_c=snap["reset"], **kw)
    assert not t.any() and all(_bits(once[k], best[k]) for k in best)
    assert snap["reset_global"].tolist() == [0, 1]                                     # the reset waits for the stream's frame


def test_identity_rows_are_the_plain_references():
    import track_filter_cases as cases
    for k, c, weighted in ((3, 5, False), (6, 17, True)):
        seq = cases.sequence(k, c, weighted, steps=3)
        slot = np.arange(k, dtype=np.int32)
        for s in seq["steps"]:
            junk = np.full(k, 777, np.int32)
            r = rref.step_rows(s["lm"], s["w"], s["m_crop"], s["boxes"], slot, SC, SC, IN, IN, FH, FW, seq["tc"], seq["ta"],
                               s["m_crop"], s["boxes"], junk, state=s["state"], dt=cases.DT, filt=dict(fref.DEFAULTS))
            for name in ("lm_frame", "m_align", "m_next", "boxes_next", "status", "state", "lm_raw"):
                assert _bits(r[name], s["exp"][name]), name
            assert _bits(r["status_rows"], s["exp"]["status"])
            p = track_ref.step(s["lm"], s["w"], s["m_crop"], s["boxes"], SC, SC, IN, IN, FH, FW, seq["tc"], seq["ta"])
            r = rref.step_rows(s["lm"], s["w"], s["m_crop"], s["boxes"], slot, SC, SC, IN, IN, FH, FW, seq["tc"], seq["ta"],
                               s["m_crop"], s["boxes"], junk)
            for name in ("lm_frame", "m_align", "m_next", "boxes_next", "status"):
                assert _bits(r[name], p[name]), name
        # the best update
        rng = np.random.default_rng(k)
        faces = rng.integers(0, 256, (k, 9, 11, 3)).astype(np.uint8)
        rec = qref.record(faces, ("nhwc", "uint8", "bgr", (1, 1, 1), (0, 0, 0)))
        lm = seq["steps"][0]["exp"]["lm_frame"]
        a, b = qref.new_state(faces, k, c), qref.new_state(faces, k, c)
        a["best_q"][:] = b["best_q"][:] = rng.choice([-1.0, 0.0, 0.5, 2.0], k)
        reset = rng.integers(0, 2, k).astype(np.int32)
        st = seq["steps"][0]["exp"]["status"]
        m = seq["steps"][0]["exp"]["m_align"]
        ta_ = qref.best_update(a, faces, rec, lm, 5, status=st, reset=reset, m=m, sharp_ref=1.0)
        tb_ = rref.best_update_rows(b, faces, rec, lm, slot, b["best_q"].copy(), 5, status_rows=st, reset_c=reset, m=m, sharp_ref=1.0)
        assert np.array_equal(ta_, tb_) and all(_bits(a[n], b[n]) for n in a)
    # the gather of every stream in order is the state itself
    m = rng.normal(0, 1, (6, 2, 3)).astype(np.float32)
    bx = rng.integers(0, 99, (6, 4)).astype(np.int32)
    g = rref.gather_streams([0, 1, 2], 3, 2, m, bx, frame_idx_stream=[5, 6, 7], dt_stream=[0.1, 0.2, 0.3])
    assert _bits(g["m"], m) and _bits(g["boxes"], bx) and g["slot"].tolist() == list(range(6))
    assert g["frame_index"].tolist() == [5, 5, 6, 6, 7, 7] and g["dt"].tolist() == [0.1, 0.1, 0.2, 0.2, 0.3, 0.3]
