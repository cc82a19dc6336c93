"""CPU-side checks of finished tracks (flm_track_retire, alignment.TrackExits / track_retire_device / exit_rows,
FaceTracker(exits=...)): the symbols, every argument check answered before any launch (so without a GPU), the Python
rejections, exit_rows against a replay of the ring, the compiler's metadata of the two kernels, and -- on
tests/track_exit_ref.py alone -- the contract of include/flm.h on cases written out by hand."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import flm_amd  # noqa: F401
from flm_amd import _lib, alignment, prediction

import track_exit_ref as xref

NAN, INF = float("nan"), float("inf")
FH, FW = 270, 480
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "face-landmark-detector_amd", "csrc")


def test_library_exports_the_call():
    lib = C.CDLL(_lib.LIB_PATH)
    for name in ("flm_exit_opts_init", "flm_track_retire"):
        assert hasattr(lib, name) and name in _lib.EXPORTS, name
    L = _lib.load()
    assert L.flm_abi_version() == 2                                   # purely additive
    assert len(L.flm_track_retire.argtypes) == 29
    o = _lib.ExitOpts.make()
    assert o.struct_size == C.sizeof(_lib.ExitOpts) == 16 and o.reserved == 0 and o.min_q == 0.0
    text = open(os.path.join(ROOT, "include", "flm.h")).read()
    assert re.search(r"#define FLM_EXIT_META (\d+)", text).group(1) == "8" and alignment.EXIT_META == 8


err = lambda: _lib.load().flm_last_error().decode()
ORDER = ("boxes", "status", "k", "fh", "fw", "best_q", "gallery", "face_bytes", "best_frame", "best_m", "best_lm", "c", "best_rec",
         "frame_id", "flush", "opts", "born", "track_id", "born_frame", "head", "q", "x_gallery", "x_meta", "x_q", "x_m", "x_lm",
         "x_rec", "exit_row")
POINTERS = [n for n in ORDER if n not in ("k", "fh", "fw", "face_bytes", "c", "frame_id", "flush", "opts", "q")]
# never dereferenced: every call below is rejected before a launch.  1 GiB apart: no two of them overlap at any size here
FAKE = {n: C.c_void_p((i + 1) << 30) for i, n in enumerate(POINTERS)}


def _retire(**kw):
    a = dict(FAKE, k=4, fh=FH, fw=FW, face_bytes=37, c=5, frame_id=7, flush=0, opts=None, q=2)
    a.update(kw)
    if isinstance(a["opts"], _lib.ExitOpts):
        a["opts"] = C.byref(a["opts"])
    return _lib.load().flm_track_retire(None, *[a[n] for n in ORDER])


def test_retire_argument_checks_answer_without_a_gpu():
    who = "flm_track_retire"
    for name in ("boxes", "status", "best_q", "gallery", "best_frame", "born", "track_id", "born_frame", "head", "x_gallery",
                 "x_meta", "x_q", "exit_row"):
        assert _retire(**{name: None}) == -1 and "null" in err() and who in err(), name
    for name in ("best_m", "x_m", "best_lm", "x_lm", "best_rec", "x_rec"):     # a source without its ring buffer, or the reverse
        assert _retire(**{name: None}) == -1 and "both or neither" in err() and who in err(), name
    short = _lib.ExitOpts.make()
    short.struct_size = 8
    assert _retire(opts=short) == -1 and "struct_size" in err() and who in err()
    res = _lib.ExitOpts.make()
    res.reserved = 1
    assert _retire(opts=res) == -1 and "reserved" in err() and who in err()
    for bad in (-1e-300, -1.0, -INF, NAN):
        assert _retire(opts=_lib.ExitOpts.make(bad)) == -1 and "min_q" in err() and who in err(), bad
        assert _retire(opts=_lib.ExitOpts.make(bad), k=0) == -1, bad          # the options come before the sizes
    for k in (0, -1, 65536, 2 ** 31 - 1):
        assert _retire(k=k) == -2 and "1 <= k <= 65535" in err() and who in err(), k
    for q in (0, -1, 65536, 2 ** 31 - 1):
        assert _retire(q=q) == -2 and "1 <= q <= 65535" in err() and who in err(), q
    for c in (0, -1, 1025):
        assert _retire(c=c) == -2 and "1 <= c <= 1024" in err() and who in err(), c
    assert _retire(face_bytes=0) == -2 and "face_bytes >= 1" in err() and who in err()
    for kw in (dict(fh=0), dict(fw=0), dict(fh=-1), dict(fw=-7)):
        assert _retire(**kw) == -2 and "fh, fw >= 1" in err() and who in err(), kw
    # what is allowed reaches the last size check (fh): the limits, good options, and every optional pair absent
    none3 = dict(best_m=None, x_m=None, best_lm=None, x_lm=None, best_rec=None, x_rec=None)
    for kw in (dict(k=65535, q=65535, c=1024), dict(k=1, q=1, c=1, face_bytes=1), dict(opts=_lib.ExitOpts.make(0.0)),
               dict(opts=_lib.ExitOpts.make(INF)), dict(opts=_lib.ExitOpts.make(0.25)), none3, dict(flush=1),
               dict(best_m=None, x_m=None), dict(best_lm=None, x_lm=None), dict(best_rec=None, x_rec=None)):
        assert _retire(fh=0, **kw) == -2 and "fh, fw >= 1" in err() and who in err(), kw
    # no two arguments may overlap: the last check, after every size
    base = FAKE["born"].value
    for other, off in (("track_id", 0), ("exit_row", 15), ("head", 8), ("x_q", 4)):    # born is 4*4 = 16 bytes here
        assert _retire(**{other: C.c_void_p(base + off)}) == -1 and "overlap" in err() and "born_dev" in err(), other
    assert _retire(x_gallery=C.c_void_p(FAKE["gallery"].value + 4 * 37 - 1)) == -1 and "gallery_dev and x_gallery" in err()
    assert _retire(x_lm=C.c_void_p(FAKE["x_rec"].value - 2 * 5 * 16 + 1)) == -1 and "x_lm and x_rec" in err()
    assert _retire(fh=0, x_gallery=C.c_void_p(FAKE["gallery"].value + 4 * 37)) == -2             # adjacent: two buffers


# ---- the Python rejections ---------------------------------------------------------------------------------------------
class _Model:
    n_classes, input_height, input_width, output_height, output_width = 68, 64, 64, 72, 72
    max_batch = 1024


class _HostRing(alignment.FrameFormat):
    def ring(self, frames):
        return 8, FH, FW, FH * FW * 3


def test_track_exits_rejects_what_it_must():
    for bad in (0, -1, 65536, 2.5, True, 2 ** 40):
        with pytest.raises(ValueError, match="capacity"):
            alignment.TrackExits(capacity=bad)
    for bad in (-0.1, NAN, -INF):
        with pytest.raises(ValueError, match="min_q"):
            alignment.TrackExits(min_q=bad)
    x = alignment.TrackExits(7, 0.25)
    assert (x.capacity, x.min_q) == (7, 0.25) and "TrackExits(capacity=7, min_q=0.25)" == repr(x)
    assert alignment.TrackExits(65535).capacity == 65535 and alignment.TrackExits().min_q == 0.0
    s = x.struct()
    assert s.min_q == 0.25 and s.reserved == 0 and s.struct_size == 16


def test_face_tracker_rejects_exits_it_cannot_serve():
    mk = lambda **kw: prediction.FaceTracker(_Model(), (FH, FW), 6, frame_format=_HostRing.bgr(), **kw)
    for bad in (4, alignment.TrackExits(4)):
        with pytest.raises(ValueError, match="exits needs best_shot"):
            mk(exits=bad)
        with pytest.raises(ValueError, match="exits needs best_shot"):
            mk(exits=bad, smooth=True, pose=True)
    for bad in (0, -3, 65536):                                         # Q outside the range
        with pytest.raises(ValueError, match="capacity"):
            mk(best_shot=True, exits=bad)
    for bad in (True, 2.0, "8", [8]):
        with pytest.raises(ValueError, match="exits must be"):
            mk(best_shot=True, exits=bad)
    tr = mk(best_shot=True, exits=5)
    assert isinstance(tr.exit_opts, alignment.TrackExits) and tr.exit_opts.capacity == 5 and tr.track_id is None
    assert mk(best_shot=True, exits=alignment.TrackExits(9, 0.5)).exit_opts.min_q == 0.5
    plain = mk(best_shot=True)
    assert plain.exit_opts is None
    for call in (plain.exits, plain.retire):
        with pytest.raises(ValueError, match="needs a tracker made with exits"):
            call()
    for bad in (1.5, True, 2 ** 63):
        with pytest.raises(ValueError, match="frame_id"):
            tr.retire(frame_id=bad)


def test_wrapper_rejects_what_it_must_on_the_host():
    k, q = 4, 2
    t = dict(boxes=torch.zeros((k, 4), dtype=torch.int32), status=torch.zeros(k, dtype=torch.int32))
    with pytest.raises(ValueError, match="boxes"):                     # (not on the device)
        alignment.track_retire_device(t["boxes"], t["status"], (FH, FW), None, None, None, None, None, None, None, None, None,
                                      None, None, 0)
    with pytest.raises(ValueError, match="boxes"):
        alignment.track_retire_device([0, 1], t["status"], (FH, FW), None, None, None, None, None, None, None, None, None, None,
                                      None, 0)
    with pytest.raises(ValueError, match="opts"):
        alignment.track_retire_device(t["boxes"], t["status"], (FH, FW), None, None, None, None, None, None, None, None, None,
                                      None, None, 0, opts=3)
    with pytest.raises(ValueError, match="frame_id"):
        alignment.track_retire_device(t["boxes"], t["status"], (FH, FW), None, None, None, None, None, None, None, None, None,
                                      None, None, 1.5)
    with pytest.raises(ValueError, match="frame_hw"):
        alignment.track_retire_device(t["boxes"], t["status"], (0, FW), None, None, None, None, None, None, None, None, None,
                                      None, None, 1)


# ---- exit_rows ---------------------------------------------------------------------------------------------------------
def test_exit_rows_against_a_replay_of_the_ring():
    for q in (1, 2, 3, 7):
        for seq in range(0, 4 * q + 2):
            for cursor in range(0, seq + 1):
                rows, lost = alignment.exit_rows(seq, cursor, q)
                want_rows, want_lost = xref.exit_rows_brute(seq, cursor, q)
                assert rows.dtype == np.int64 and rows.tolist() == want_rows and lost == want_lost, (q, seq, cursor)
                assert len(rows) + lost == seq - cursor and len(rows) <= q
    q = 7
    for base in (0, 5, 3 * q):
        assert alignment.exit_rows(base, base, q)[0].tolist() == [] and alignment.exit_rows(base, base, q)[1] == 0
        rows, lost = alignment.exit_rows(base + q, base, q)            # exactly Q new: all there, none lost
        assert rows.tolist() == [(base + i) % q for i in range(q)] and lost == 0
        rows, lost = alignment.exit_rows(base + q + 1, base, q)        # Q+1: the oldest is gone
        assert rows.tolist() == [(base + 1 + i) % q for i in range(q)] and lost == 1
    assert alignment.exit_rows(2 ** 40 + 3, 2 ** 40, 64)[0].tolist() == [(2 ** 40 + i) % 64 for i in range(3)]
    for bad in (dict(seq=3, cursor=4, capacity=2), dict(seq=3, cursor=-1, capacity=2), dict(seq=3, cursor=0, capacity=0),
                dict(seq=3, cursor=0, capacity=65536), dict(seq=2.5, cursor=0, capacity=2), dict(seq=3, cursor=True, capacity=2)):
        with pytest.raises(ValueError):
            alignment.exit_rows(**bad)


# ---- the compiler's metadata of the kernels this feature adds -----------------------------------------------------------
def test_the_new_kernels_compile_for_gfx950_without_scratch(tmp_path):
    out = os.path.join(str(tmp_path), "flm_track_exit.s")
    cmd = ["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
           "-I", CSRC, "-S", "--cuda-device-only", os.path.join(CSRC, "flm_track_exit.hip"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    md = {}
    for block in open(out).read().split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        md[name] = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\n", block)}
    decide = [n for n in md if "track_exit_decide_kernel" in n]
    copy = [n for n in md if "track_exit_copy_kernel" in n]
    assert len(decide) == 1 and len(copy) == 1 and len(md) == 2, sorted(md)     # "at most two launches"
    d, c = md[decide[0]], md[copy[0]]
    for k in (d, c):
        print({f: k[f] for f in ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")})
        assert k["private_segment_fixed_size"] == 0 and k["wavefront_size"] == 64, k
    assert d["max_flat_workgroup_size"] == 1024 and c["max_flat_workgroup_size"] == 256
    assert d["group_segment_fixed_size"] <= 192 and c["group_segment_fixed_size"] == 0      # 3 x 16 wave totals
    assert d["vgpr_count"] <= 128, d        # one workgroup of 1024 threads must be resident
    text = open(os.path.join(CSRC, "flm_track_exit.hip")).read() + open(os.path.join(CSRC, "flm_track_exit_dev.h")).read()
    assert "atomic" not in text.replace("No atomics", "") and "hipMalloc" not in text and "Synchronize" not in text


# ---- the restatement against cases written out by hand: K = 4, Q = 2 ---------------------------------------------------
LIVE, DEAD = (10, 10, 60, 60), (0, 0, 0, 0)
FB, NC = 6, 3


def _hand(boxes, status, best_q, track_id, born, head, born_frame=(100, 101, 102, 103), best_frame=(40, 41, 42, 43)):
    s = xref.new_state(4, 2, FB, NC)
    s["boxes"][:] = boxes
    s["status"][:] = status
    s["best_q"][:] = best_q
    s["track_id"][:] = track_id
    s["born"][:] = born
    s["head"][:] = head
    s["born_frame"][:] = born_frame
    s["best_frame"][:] = best_frame
    s["gallery"][:] = np.arange(4 * FB, dtype=np.uint8).reshape(4, FB) + 1
    s["best_m"][:] = np.arange(24, dtype=np.float32).reshape(4, 2, 3)
    s["best_lm"][:] = np.arange(4 * NC * 2, dtype=np.float64).reshape(4, NC, 2)
    s["best_rec"][:] = np.arange(32, dtype=np.int64).reshape(4, 8) * 3
    return s


def _row_is(s, row, t, src):
    return (np.array_equal(s["x_gallery"][row], src["gallery"][t]) and s["x_q"][row] == src["best_q"][t]
            and np.array_equal(s["x_m"][row], src["best_m"][t]) and np.array_equal(s["x_lm"][row], src["best_lm"][t])
            and np.array_equal(s["x_rec"][row], src["best_rec"][t]))


def test_three_exits_in_one_call_into_a_ring_of_two():
    s = _hand([DEAD] * 4, [16, 2, 4, 64], [0.5, 0.6, -1.0, 0.7], [10, 11, 12, 13], [0] * 4, [0, 14, 0, 0])
    src = {k: v.copy() for k, v in s.items()}
    d = xref.retire(s, FH, FW, frame_id=9)
    assert d["E"] == 3 and d["B"] == 0
    assert s["exit_row"].tolist() == [-3, 1, -2, 0]                    # rank 0 overrun, ranks 1, 2 -> rows 1 % 2, 2 % 2
    assert s["head"].tolist() == [3, 14, 1, 1]
    assert s["track_id"].tolist() == [-1] * 4 and s["born"].tolist() == [0] * 4
    assert s["born_frame"].tolist() == [100, 101, 102, 103]
    assert s["x_meta"].tolist() == [[13, 3, 103, 9, 43, 64, 2, 0], [11, 1, 101, 9, 41, 2, 1, 0]]
    assert _row_is(s, 1, 1, src) and _row_is(s, 0, 3, src)
    # a second call finds nothing: no slot holds a track
    before = {k: v.copy() for k, v in s.items()}
    d = xref.retire(s, FH, FW, frame_id=10)
    assert d["E"] == 0 and s["exit_row"].tolist() == [-1] * 4
    assert all(np.array_equal(s[k], before[k]) for k in s if k != "exit_row")


def test_the_sequence_wraps_the_ring_over_two_calls():
    s = _hand([DEAD, LIVE, LIVE, LIVE], [16, 0, 0, 0], [0.5, 0.6, 0.2, 0.7], [0, 1, 2, 3], [0] * 4, [1, 4, 0, 0])
    xref.retire(s, FH, FW, frame_id=5)
    assert s["exit_row"].tolist() == [1, -1, -1, -1] and s["head"].tolist() == [2, 4, 0, 0]        # seq 1 -> row 1
    assert s["x_meta"][1].tolist() == [0, 0, 100, 5, 40, 16, 1, 0] and (s["x_meta"][0] == -77).all()   # row 0: the sentinel
    assert (s["x_gallery"][0] == 0xA5).all() and s["x_q"][0] == -7.5
    s["boxes"][1] = s["boxes"][3] = DEAD
    s["status"][[1, 3]] = (8, 32)
    xref.retire(s, FH, FW, frame_id=6)
    assert s["exit_row"].tolist() == [-1, 0, -1, 1] and s["head"].tolist() == [4, 4, 0, 0]         # seq 2, 3 -> rows 0, 1
    assert s["x_meta"].tolist() == [[1, 1, 101, 6, 41, 8, 2, 0], [3, 3, 103, 6, 43, 32, 3, 0]]
    assert s["track_id"].tolist() == [-1, -1, 2, -1]
    rows, lost = alignment.exit_rows(4, 1, 2)                          # a consumer that looked before the first call
    assert rows.tolist() == [0, 1] and lost == 1


def test_a_replacement_ends_the_old_track_and_names_the_new_one():
    # slot 0: restarted while live; slot 1: born into an empty slot; slot 2: born with an empty box; slot 3: untouched
    s = _hand([LIVE, LIVE, DEAD, LIVE], [0, 0, 1, 0], [0.5, -1.0, 0.3, 0.7], [7, -1, -1, 8], [1, 5, 1, 0], [20, 9, 2, 3])
    src = {k: v.copy() for k, v in s.items()}
    d = xref.retire(s, FH, FW, frame_id=30)
    assert d["E"] == 1 and d["B"] == 2
    assert s["exit_row"].tolist() == [0, -1, -1, -1]                   # seq 20 -> row 0
    assert s["x_meta"][0].tolist() == [7, 0, 100, 30, 40, -1, 20, 0] and _row_is(s, 0, 0, src)
    assert s["track_id"].tolist() == [9, 10, -1, 8] and s["born_frame"].tolist() == [30, 30, 102, 103]
    assert s["head"].tolist() == [21, 11, 2, 3] and s["born"].tolist() == [0] * 4
    # a held slot that was born with an empty box: its old track ends (end = -1) and the slot holds none
    s = _hand([DEAD, LIVE, LIVE, LIVE], [1, 0, 0, 0], [0.5, 0.1, 0.1, 0.1], [7, 1, 2, 3], [1, 0, 0, 0], [0, 9, 0, 0])
    xref.retire(s, FH, FW, frame_id=31)
    assert s["x_meta"][0].tolist() == [7, 0, 100, 31, 40, -1, 0, 0]
    assert s["track_id"].tolist() == [-1, 1, 2, 3] and s["head"].tolist() == [1, 9, 0, 0]


def test_a_flush_ends_every_held_track():
    # slot 0 live and held; slot 1 dead and held; slot 2 born, live and held; slot 3 holds no track
    s = _hand([LIVE, DEAD, LIVE, LIVE], [0, 18, 0, 0], [0.5, 0.6, 0.7, 0.9], [4, 5, 6, -1], [0, 0, 1, 0], [0, 7, 0, 0])
    d = xref.retire(s, FH, FW, frame_id=50, flush=True)
    assert d["E"] == 3 and s["exit_row"].tolist() == [-3, 1, 0, -1]
    assert s["x_meta"].tolist() == [[6, 2, 102, 50, 42, -1, 2, 0], [5, 1, 101, 50, 41, 18, 1, 0]]
    assert s["track_id"].tolist() == [-1, -1, 7, -1] and s["head"].tolist() == [3, 8, 0, 1]        # the birth is still named
    s = _hand([LIVE] * 4, [0] * 4, [0.5, 0.6, 0.7, 0.9], [4, 5, -1, -1], [0] * 4, [0, 7, 0, 0])
    xref.retire(s, FH, FW, frame_id=51, flush=True)
    assert s["x_meta"][:, 5].tolist() == [-2, -2] and s["track_id"].tolist() == [-1] * 4           # live, not born: -2


def test_a_track_without_a_good_enough_best_is_discarded():
    s = _hand([DEAD] * 4, [1, 1, 1, 1], [-1.0, NAN, 0.25, 0.24999], [0, 1, 2, 3], [0] * 4, [6, 4, 10, 0])
    xref.retire(s, FH, FW, frame_id=3, min_q=0.25)
    assert s["exit_row"].tolist() == [-2, -2, 0, -2]                   # equal to min_q counts
    assert s["head"].tolist() == [7, 4, 13, 0] and s["track_id"].tolist() == [-1] * 4
    assert (s["x_meta"][1] == -77).all() and s["x_meta"][0, [0, 6]].tolist() == [2, 6]
    s = _hand([DEAD] * 4, [1, 1, 1, 1], [-1.0, NAN, 0.0, -0.0], [0, 1, 2, 3], [0] * 4, [0, 4, 0, 0])
    xref.retire(s, FH, FW, frame_id=3)                                 # the default min_q = 0: only "no best" is dropped
    assert s["exit_row"].tolist() == [-2, -2, 0, 1] and s["head"].tolist() == [2, 4, 2, 0]


def test_live_is_the_clip_of_the_tracking_section():
    boxes = [(0, 0, 1, 1), (-5, -5, 0, 9), (FW, 0, FW + 9, 9), (FW - 1, FH - 1, FW + 9, FH + 9), (5, 9, 50, 9), (60, 5, 50, 9),
             (-2 ** 31, -2 ** 31, 2 ** 31 - 1, 2 ** 31 - 1), (3, FH, 9, FH + 4)]
    assert xref.live_of(np.array(boxes, np.int64).astype(np.int32), FH, FW).tolist() == [True, False, False, True, False, False,
                                                                                        True, False]
