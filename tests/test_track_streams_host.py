"""CPU-side checks of the association of several streams in one tracker (flm_track_associate_streams,
alignment.track_associate_streams_device, FaceTracker(streams=S)): the symbol, every argument check answered before any
launch (so without a GPU), the Python wrappers' own checks, and -- on the references alone -- the reason for the
feature: two cameras with a face at the same pixels are one face to a tracker that knows no streams, and two faces to
one that does."""
import ctypes as C

import numpy as np
import pytest
import torch

import flm_amd  # noqa: F401
from flm_amd import _lib, alignment, prediction

import track_assoc_ref as ref
import track_ref
import track_streams_ref as sref

NAN = float("nan")
IN, FH, FW = 64, 270, 480


def test_library_exports_the_streams_call():
    lib = C.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "flm_track_associate_streams")
    assert "flm_track_associate_streams" in _lib.EXPORTS
    assert _lib.load().flm_abi_version() == 2          # purely additive
    assert C.sizeof(_lib.TrackAssocOpts) == 40         # (the options are reused unchanged)
    assert len(_lib.load().flm_track_associate_streams.argtypes) == len(_lib.load().flm_track_associate.argtypes) + 1


def _call(lib, p, **kw):
    """flm_track_associate_streams with every argument valid (never launched: each caller breaks one)."""
    a = dict(det=p, n=p, s=3, d=5, k=4, c=68, in_h=64, in_w=64, fh=270, fw=480, opts=None, m=p, boxes=p, st=p, mis=p,
             state=p, ds=p, sd=p, cnt=p)
    a.update(kw)
    o = a["opts"]
    return lib.flm_track_associate_streams(None, a["det"], a["n"], a["s"], a["d"], a["k"], a["c"], a["in_h"], a["in_w"],
                                           a["fh"], a["fw"], None if o is None else C.byref(o), a["m"], a["boxes"], a["st"],
                                           a["mis"], a["state"], a["ds"], a["sd"], a["cnt"])


def test_argument_checks_answer_without_a_gpu():
    lib = _lib.load()
    p = C.c_void_p(0x1000)        # never dereferenced: every call below is rejected before a launch
    err = lambda: lib.flm_last_error().decode()
    for name in ("det", "m", "boxes", "st", "mis", "ds", "sd", "cnt"):
        assert _call(lib, p, **{name: None}) == -1, name
        assert "null" in err() and "flm_track_associate_streams" in err()
    o = _lib.TrackAssocOpts.make()
    o.struct_size -= 8
    assert _call(lib, p, opts=o) == -1 and "struct_size" in err()
    o = _lib.TrackAssocOpts.make()
    o.reserved = 1
    assert _call(lib, p, opts=o) == -1 and "reserved" in err()
    for s in (0, -1):
        assert _call(lib, p, s=s) == -2 and "1 <= s" in err()
    for s, k in ((65536, 1), (64, 1024), (16384, 4), (2 ** 31 - 1, 1024)):
        assert _call(lib, p, s=s, k=k) == -2 and "s*k <= 65535" in err(), (s, k)
    for k in (0, 1025):
        assert _call(lib, p, k=k) == -2 and "1 <= k <= 1024" in err()
    for d in (0, 1025):
        assert _call(lib, p, d=d) == -2 and "1 <= d <= 1024" in err()
    for c in (0, 1025):
        assert _call(lib, p, c=c) == -2 and "1 <= c <= 1024" in err()
    for kw in (dict(in_h=0), dict(in_w=-1), dict(fh=0), dict(fw=0)):
        assert _call(lib, p, **kw) == -2 and "in_h, in_w, fh, fw >= 1" in err()
    for fh, fw in ((32768, 32769), (1, 2 ** 30 + 1), (2 ** 30 + 1, 1), (2 ** 31 - 1, 2 ** 31 - 1)):
        assert _call(lib, p, fh=fh, fw=fw) == -2 and "2^30" in err()
    assert _call(lib, p, opts=_lib.TrackAssocOpts.make(max_misses=-1)) == -2 and "max_misses" in err()
    for kw in (dict(match_iou=NAN), dict(dup_iou=NAN), dict(refresh_iou=NAN)):
        assert _call(lib, p, opts=_lib.TrackAssocOpts.make(**kw)) == -2 and "NaN" in err()
    # what is allowed reaches the last check (a NaN threshold): the most streams, the most slots, no count, no state
    last = dict(match_iou=NAN)
    for kw in (dict(s=65535, k=1), dict(s=63, k=1024, d=1024), dict(s=1, k=1, d=1), dict(n=None), dict(state=None, c=0),
               dict(fh=32768, fw=32768), dict(opts=dict(dup_iou=2.0, refresh_iou=float("inf"), max_misses=2 ** 31 - 1))):
        o = _lib.TrackAssocOpts.make(**dict(kw.pop("opts", {}), **last))
        assert _call(lib, p, opts=o, **kw) == -2 and "NaN" in err() and "flm_track_associate_streams" in err(), kw


class _Model:
    n_classes, input_height, input_width, output_height, output_width = 68, 64, 64, 72, 72


class _HostRing(alignment.FrameFormat):
    """A frame format whose ring needs no device: 8 slots of the tracker's frames (what `step` asks before it looks at
    frame_index)."""

    def ring(self, frames):
        return 8, FH, FW, FH * FW * 3


def test_python_wrappers_reject_what_they_must_on_the_host():
    A = alignment
    for streams in (0, -1, 5, 4, 1.5, True):                       # outside [1, capacity], or not a divisor of 6
        with pytest.raises(ValueError, match="streams"):
            prediction.FaceTracker(_Model(), (FH, FW), 6, streams=streams)
    for streams, k in ((1, 6), (2, 3), (3, 2), (6, 1)):
        tr = prediction.FaceTracker(_Model(), (FH, FW), 6, streams=streams)
        assert (tr.streams, tr.slots_per_stream, tr.capacity) == (streams, k, 6)
    assert prediction.FaceTracker(_Model(), (FH, FW), 6).streams == 1
    # track_associate_streams_device: ranks, types and shapes of det and n_det
    m = torch.zeros((6, 2, 3), dtype=torch.float32)
    boxes, st, mis = torch.zeros((6, 4), dtype=torch.int32), torch.zeros(6, dtype=torch.int32), torch.zeros(6, dtype=torch.int32)
    det = torch.zeros((2, 5, 4), dtype=torch.int32)
    args = (m, boxes, st, mis, 3, (64, 64), (FH, FW))
    with pytest.raises(ValueError, match="assoc"):
        A.track_associate_streams_device(det, *args, assoc="loose")
    for bad in (det[0], det.long(), torch.zeros((2, 5, 5), dtype=torch.int32), det.numpy(), det):   # (the last: not on the device)
        with pytest.raises(ValueError, match="det"):
            A.track_associate_streams_device(bad, *args)
    for bad in (torch.zeros(3, dtype=torch.int32), torch.zeros(2, dtype=torch.int64), torch.zeros((2, 1), dtype=torch.int32),
                torch.zeros(1, dtype=torch.int32), [5, 5]):
        with pytest.raises(ValueError, match="n_det"):
            A.track_associate_streams_device(det, *args, n_det=bad)
    # FaceTracker(streams=2): frame_index and detections given on the host
    tr = prediction.FaceTracker(_Model(), (FH, FW), 6, streams=2, frame_format=_HostRing.bgr())
    for bad in (3, [1], [1, 2, 3], (0,)):
        with pytest.raises(ValueError, match="sequence of 2"):
            tr.step(None, bad)
    for bad in ([0, 8], [-1, 0], [0.5, 1], [True, 1]):
        with pytest.raises(ValueError, match=r"\[0, 8\)"):
            tr.step(None, bad)
    for bad in (torch.zeros(2, dtype=torch.int32), torch.zeros(2, dtype=torch.int64)):              # (not on the device)
        with pytest.raises(ValueError, match="CUDA int32"):
            tr.step(None, bad)
    for bad in ([[[0, 0, 10, 10]]], [[], [], []], []):
        with pytest.raises(ValueError, match="one entry per stream"):
            tr.update(bad)
    with pytest.raises(ValueError, match="boxes"):
        tr.update([[[0.5, 0, 10, 10]], None])
    with pytest.raises(ValueError, match="boxes"):
        tr.update([[[0, 0, 10]], []])
    with pytest.raises(ValueError, match="int32"):
        tr.update([[[0, 0, 10, 2 ** 31]], []])
    with pytest.raises(ValueError, match="n goes with"):
        tr.update([[], []], n=[1, 1])
    with pytest.raises(ValueError, match="1024"):
        tr.update([np.zeros((1025, 4), np.int32), None])
    for bad in (torch.zeros((5, 4), dtype=torch.int32), torch.zeros((3, 5, 4), dtype=torch.int32),
                torch.zeros((2, 5, 4), dtype=torch.int64)):
        with pytest.raises(ValueError, match=r"\[2,D,4\]"):
            tr.update(bad)
    with pytest.raises(ValueError, match="n must be"):
        tr.update(torch.zeros((2, 5, 4), dtype=torch.int32), n=[1, 1])
    with pytest.raises(ValueError, match="1024"):
        prediction.FaceTracker(_Model(), (FH, FW), 2050, streams=2).update([[], []])
    for kw in (dict(stream=2), dict(stream=-1), dict(stream=0.5)):
        with pytest.raises(ValueError, match="stream"):
            tr.seed([0], [[0, 0, 10, 10]], **kw)
    with pytest.raises(ValueError, match="slots of a stream"):
        tr.seed([3], [[0, 0, 10, 10]], stream=1)


# ---- the references alone ----------------------------------------------------------------------------------------------
def _two_cameras(k):
    """Two streams of k slots: each follows a face at the same pixels in slot 0 and saw it again in detection 0."""
    face = [100, 60, 160, 120]
    boxes = np.zeros((2 * k, 4), np.int32)
    boxes[0] = boxes[k] = face
    m, st = track_ref.seed([face], IN, IN, FH, FW)
    mc = np.tile(track_ref.IDENTITY, (2 * k, 1, 1)).astype(np.float32)
    mc[0] = mc[k] = m[0]
    status = np.full(2 * k, track_ref.DEAD, np.int32)
    status[0] = status[k] = st[0]
    det = np.tile(np.asarray(face, np.int32), (2, 1, 1))            # [2,1,4]
    return det, mc, boxes, status, np.zeros(2 * k, np.int32)


def test_two_cameras_with_a_face_at_the_same_pixels():
    k = 3
    det, mc, boxes, status, misses = _two_cameras(k)
    # one tracker that knows no streams: 2K slots, both cameras' detections in one list
    one = ref.associate(det.reshape(-1, 4), None, mc, boxes, status, misses, None, IN, IN, FH, FW, square=False)
    assert one["status"][k] & ref.DUPLICATE and not one["boxes"][k].any()       # camera 1's track ends as a duplicate
    assert one["counts"][3] == 1
    assert one["det_slot"].tolist() == [0, 1]                                   # camera 1's detection lands in camera 0's slots
    # per stream: both tracks live, each detection stays in its stream
    two = sref.associate_streams(det, None, mc, boxes, status, misses, None, k, IN, IN, FH, FW, square=False)
    assert two["status"][[0, k]].tolist() == [0, 0] and np.array_equal(two["boxes"], boxes)
    assert two["det_slot"].tolist() == [[0], [k]] and two["slot_det"].tolist() == [0, -1, -1, 0, -1, -1]
    assert two["counts"].tolist() == [[1, 0, 0, 0, 0, 0, 0, 0]] * 2


def _junk(n, c, seed):
    rng = np.random.default_rng(seed)
    m = rng.normal(0, 3, (n, 2, 3)).astype(np.float32)
    status = rng.choice([0, 0, 1, 8, 32, 64], n).astype(np.int32)
    misses = rng.integers(0, 3, n).astype(np.int32)
    state = rng.normal(50, 40, (n, c, 6))
    state[rng.random((n, c, 6)) < 0.1] = np.nan
    boxes = rng.integers(0, 200, (n, 4)).astype(np.int32)
    boxes[:, 2:] += boxes[:, :2] + 5
    boxes[::4] = 0
    return m, boxes, status, misses, state


def _same_bits(a, b):
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(u), np.ascontiguousarray(b).view(u))


def test_one_stream_is_the_single_association():
    rng = np.random.default_rng(3)
    m, boxes, status, misses, state = _junk(9, 2, 1)
    det = boxes[rng.permutation(9)[:7]] + rng.integers(-4, 5, (7, 4)).astype(np.int32)
    opts = dict(max_misses=2, refresh_iou=0.9, square=False)
    for n in (None, 4, 0):
        a = ref.associate(det, n, m, boxes, status, misses, state, IN, IN, FH, FW, **opts)
        b = sref.associate_streams(det[None], None if n is None else [n], m, boxes, status, misses, state, 9, IN, IN, FH, FW, **opts)
        for name in sref.NAMES:
            assert _same_bits(a[name], b[name].reshape(a[name].shape)), (name, n)
        assert (a["counts"][0] > 0) == (n != 0)


def test_a_skipped_stream_is_not_touched():
    m, boxes, status, misses, state = _junk(12, 2, 2)
    det = np.stack([boxes[0:3], boxes[5:8], boxes[9:12]])
    r = sref.associate_streams(det, [3, -1, -2 ** 31], m, boxes, status, misses, state, 4, IN, IN, FH, FW, max_misses=1, square=False)
    for name, x in (("m_crop", m), ("boxes", boxes), ("status", status), ("misses", misses), ("state", state)):
        assert _same_bits(r[name][4:], x[4:]), name                              # NaNs included
    assert any(not _same_bits(r[name][:4], x[:4]) for name, x in (("status", status), ("misses", misses), ("m_crop", m)))
    assert (r["det_slot"][1:] == -1).all() and (r["slot_det"][4:] == -1).all() and not r["counts"][1:].any()
    assert r["counts"][0].any()
    # and n = 0 is not a skip: the detector ran and found nothing, the live slots count a miss
    r0 = sref.associate_streams(det, [0, 0, 0], m, boxes, status, misses, state, 4, IN, IN, FH, FW, dup_iou=2.0, square=False)
    live = np.array([not ref.empty(ref.clip(b, FH, FW)) for b in boxes])
    assert live.sum() > 6 and np.array_equal(r0["misses"][live], misses[live] + 1) and (r0["det_slot"] == -1).all()
