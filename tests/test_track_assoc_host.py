"""CPU-side checks of the association of detector boxes with live tracks (flm_track_associate,
alignment.TrackAssociation, alignment.track_associate_device, FaceTracker.update): the symbols, the struct and its
defaults, every argument check answered before any launch (so without a GPU), the Python wrappers' own checks, the
reference's box maths against prediction.face_boxes, and a scenario on the reference alone (tests/track_assoc_ref.py over
tests/track_ref.py's step) in which tracks are confirmed, merged, given up and born."""
import ctypes as C

import numpy as np
import pytest
import torch

import flm_amd  # noqa: F401
from flm_amd import _lib, alignment, prediction

import track_assoc_ref as ref
import track_ref

NAN = float("nan")


def test_library_exports_the_association():
    lib = C.CDLL(_lib.LIB_PATH)
    for name in ("flm_track_assoc_opts_init", "flm_track_associate"):
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTS
    assert _lib.load().flm_abi_version() == 2          # purely additive
    assert C.sizeof(_lib.TrackOpts) == 32              # (the options of the step did not grow)
    o = _lib.TrackAssocOpts.make()
    assert o.struct_size == C.sizeof(_lib.TrackAssocOpts) == 40
    assert (o.max_misses, o.square, o.reserved, o.match_iou, o.dup_iou, o.refresh_iou) == (0, 1, 0, 0.3, 0.7, 0.0)
    a = alignment.TrackAssociation()
    assert (a.match_iou, a.dup_iou, a.refresh_iou, a.max_misses, a.square) == (0.3, 0.7, 0.0, 0, True)
    old = (_lib.TRACK_DEAD, _lib.TRACK_FEW_POINTS, _lib.TRACK_LOW_SCORE, _lib.TRACK_SCALE, _lib.TRACK_OUTSIDE)
    new = (_lib.TRACK_DUPLICATE, _lib.TRACK_UNCONFIRMED)
    assert new == (32, 64) == (ref.DUPLICATE, ref.UNCONFIRMED)
    assert all(bin(b).count("1") == 1 for b in old + new) and len(set(old + new)) == 7


def _call(lib, p, **kw):
    """flm_track_associate with every argument valid (never launched: each caller breaks one)."""
    a = dict(det=p, n=p, d=5, k=4, c=68, in_h=64, in_w=64, fh=270, fw=480, opts=None, m=p, boxes=p, st=p, mis=p, state=p,
             ds=p, sd=p, cnt=p)
    a.update(kw)
    o = a["opts"]
    return lib.flm_track_associate(None, a["det"], a["n"], a["d"], a["k"], a["c"], a["in_h"], a["in_w"], a["fh"], a["fw"],
                                   None if o is None else C.byref(o), a["m"], a["boxes"], a["st"], a["mis"], a["state"],
                                   a["ds"], a["sd"], a["cnt"])


def test_argument_checks_answer_without_a_gpu():
    lib = _lib.load()
    p = C.c_void_p(0x1000)        # never dereferenced: every call below is rejected before a launch
    err = lambda: lib.flm_last_error().decode()
    for name in ("det", "m", "boxes", "st", "mis", "ds", "sd", "cnt"):
        assert _call(lib, p, **{name: None}) == -1, name
        assert "null" in err() and "flm_track_associate" in err()
    o = _lib.TrackAssocOpts.make()
    o.struct_size -= 8
    assert _call(lib, p, opts=o) == -1 and "struct_size" in err()
    o = _lib.TrackAssocOpts.make()
    o.reserved = 1
    assert _call(lib, p, opts=o) == -1 and "reserved" in err()
    for k in (0, -1, 1025):
        assert _call(lib, p, k=k) == -2 and "1 <= k <= 1024" in err()
    for d in (0, -7, 1025):
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
    # what is allowed reaches the last check (a NaN threshold): no count, no state (c is then not read), the caps, the
    # largest frames, thresholds beyond [0, 1], the largest max_misses
    last = dict(match_iou=NAN)
    for kw in (dict(n=None), dict(state=None, c=0), dict(k=1024, d=1024), dict(k=1, d=1), dict(fh=1, fw=2 ** 30),
               dict(fh=32768, fw=32768), dict(opts=dict(dup_iou=2.0, refresh_iou=float("inf"), max_misses=2 ** 31 - 1)),
               dict(opts=dict(dup_iou=-1.0, square=False))):
        o = _lib.TrackAssocOpts.make(**dict(kw.pop("opts", {}), **last))
        assert _call(lib, p, opts=o, **kw) == -2 and "NaN" in err(), kw


class _Model:
    n_classes, input_height, input_width, output_height, output_width = 68, 64, 64, 72, 72


def test_python_wrappers_reject_what_they_must_on_the_host():
    A = alignment
    for kw in (dict(match_iou=NAN), dict(dup_iou=NAN), dict(refresh_iou=NAN), dict(max_misses=-1), dict(max_misses=1.5)):
        with pytest.raises(ValueError, match=list(kw)[0]):
            A.TrackAssociation(**kw)
    a = A.TrackAssociation(match_iou=0.5, dup_iou=2.0, refresh_iou=0.4, max_misses=3, square=False)
    assert (a.match_iou, a.dup_iou, a.refresh_iou, a.max_misses, a.square) == (0.5, 2.0, 0.4, 3, False)
    s = a.struct()
    assert (s.match_iou, s.dup_iou, s.refresh_iou, s.max_misses, s.square) == (0.5, 2.0, 0.4, 3, 0)
    # track_associate_device: host tensors, wrong types, wrong shapes
    det = torch.zeros((3, 4), dtype=torch.int32)
    m = torch.zeros((2, 2, 3), dtype=torch.float32)
    boxes, st, mis = torch.zeros((2, 4), dtype=torch.int32), torch.zeros(2, dtype=torch.int32), torch.zeros(2, dtype=torch.int32)
    with pytest.raises(ValueError, match="assoc"):
        A.track_associate_device(det, m, boxes, st, mis, (64, 64), (270, 480), assoc="loose")
    with pytest.raises(ValueError, match="det"):
        A.track_associate_device(det, m, boxes, st, mis, (64, 64), (270, 480))          # not on the device
    with pytest.raises(ValueError, match="det"):
        A.track_associate_device(det.long(), m, boxes, st, mis, (64, 64), (270, 480))
    with pytest.raises(ValueError, match="det"):
        A.track_associate_device(torch.zeros((3, 5), dtype=torch.int32), m, boxes, st, mis, (64, 64), (270, 480))
    # FaceTracker
    with pytest.raises(ValueError, match="associate"):
        prediction.FaceTracker(_Model(), (270, 480), 4, associate=dict(match_iou=0.3))
    tr = prediction.FaceTracker(_Model(), (270, 480), 1025)
    with pytest.raises(ValueError, match="1024"):
        tr.update([[0, 0, 10, 10]])
    tr = prediction.FaceTracker(_Model(), (270, 480), 4, associate=a)
    assert tr.associate is a
    with pytest.raises(ValueError, match="1024"):
        tr.update(np.zeros((1025, 4), np.int32))
    with pytest.raises(ValueError, match="boxes"):
        tr.update([[0.5, 0, 10, 10]])
    with pytest.raises(ValueError, match="boxes"):
        tr.update([[0, 0, 10]])
    with pytest.raises(ValueError, match="n must be"):
        tr.update([[0, 0, 10, 10]], n=1)


def test_reference_box_maths_is_face_boxes():
    rng = np.random.default_rng(7)
    boxes = []
    for lim in (40, 600, 2 ** 28):
        b = rng.integers(-lim, lim + 1, (4000, 4))
        boxes += b.tolist()                                          # (half of them inverted in x, half in y)
    for dh in range(-9, 10):                                         # every small difference of both signs, odd and even
        for w in (1, 2, 7, 10):
            boxes.append([5, 3, 5 + w, 3 + w + dh])
    boxes += [[2 ** 28, 2 ** 28, -2 ** 28, -2 ** 28], [-2 ** 28, -2 ** 28, 2 ** 28, 2 ** 28], [-2 ** 28, 2 ** 28, 2 ** 28, -2 ** 28],
              [0, 0, 0, 0], [3, 3, 3, 9], [3, 3, 9, 3]]
    exp = prediction.face_boxes([list(b) for b in boxes])
    diffs = set()
    for b, e in zip(boxes, exp):
        got = ref.square_box(b)
        assert got == [int(v) for v in e], (b, got, e)
        d = (b[3] - b[1]) - (b[2] - b[0])
        diffs.add((d > 0, d < 0, abs(d) & 1))
    assert diffs >= {(True, False, 0), (True, False, 1), (False, True, 0), (False, True, 1), (False, False, 0)}


# ---- a scenario on the reference alone ----------------------------------------------------------------------------------
IN, GRID, FH, FW, CL = 64, 72, 270, 480, 12
SC = IN / GRID


def _scene(t):
    """The faces in frame t as (cx, cy, side): A and B from the start, C enters the frame at t = 8."""
    faces = {"A": (80.0 + 3.0 * t, 90.0 + 1.0 * t, 60.0), "B": (400.0 - 4.0 * t, 150.0, 72.0)}
    if t >= 8:
        faces["C"] = (30.0 + 5.0 * (t - 8), 200.0, 50.0)
    return faces


def _detector(face):
    """The box a detector would report for a face, such that the reference's box maths lands on the face's square."""
    cx, cy, side = face
    x0, y0, s = int(round(cx - side / 2)), int(round(cy - side / 2)), int(side)
    return [x0, y0 - int(abs(s * 0.1)), x0 + s, y0 - int(abs(s * 0.1)) + s]


class _Sim:
    """`cap` slots followed with track_ref.step on synthetic landmarks: a slot whose box holds a face's centre sees
    that face (its landmarks are the crop template laid over the face's square), any other live slot sees the template
    where it is (a texture that looks like a face to the network and stands still)."""

    def __init__(self, cap, **assoc):
        self.cap, self.assoc = cap, assoc
        self.tmpl = alignment.canonical_template(CL, IN, IN)
        self.m = np.tile(track_ref.IDENTITY, (cap, 1, 1))
        self.boxes = np.zeros((cap, 4), np.int32)
        self.status = np.full(cap, track_ref.DEAD, np.int32)
        self.misses = np.zeros(cap, np.int32)

    def put(self, slot, box):
        m, st = track_ref.seed([box], IN, IN, FH, FW)
        self.m[slot], self.status[slot], self.boxes[slot], self.misses[slot] = m[0], st[0], box, 0

    def step(self, t):
        lm = np.zeros((self.cap, CL, 2))
        for s in range(self.cap):
            x0, y0, x1, y1 = self.boxes[s]
            under = [f for f in _scene(t).values() if x0 <= f[0] < x1 and y0 <= f[1] < y1]
            if under:
                cx, cy, side = min(under, key=lambda f: abs(f[0] - (x0 + x1) / 2) + abs(f[1] - (y0 + y1) / 2))
                pts = self.tmpl / IN * side + [cx - side / 2, cy - side / 2]
                lm[s] = np.maximum(track_ref.apply(self.m[s], pts) / SC, 0.0)
            else:
                lm[s] = self.tmpl / SC
        r = track_ref.step(lm, None, self.m, self.boxes, SC, SC, IN, IN, FH, FW, self.tmpl)
        self.m, self.boxes, self.status = r["m_next"], r["boxes_next"], r["status"]

    def update(self, det):
        r = ref.associate(det, None, self.m, self.boxes, self.status, self.misses, None, IN, IN, FH, FW, **self.assoc)
        self.m, self.boxes, self.status, self.misses = r["m_crop"], r["boxes"], r["status"], r["misses"]
        return r

    def live(self):
        return [s for s in range(self.cap) if not track_ref.box_empty(self.boxes[s], FH, FW)]


def test_scenario_on_the_reference():
    sim = _Sim(5, max_misses=2)
    f = _scene(0)
    r = sim.update([_detector(f["A"]), _detector(f["B"])])
    assert r["det_slot"].tolist() == [0, 1] and r["slot_det"].tolist() == [0, 1, -1, -1, -1]
    assert r["counts"].tolist() == [0, 2, 0, 0, 0, 0, 0, 0] and sim.live() == [0, 1]
    # a second track steered onto A, and one onto a patch of the frame that holds no face
    ax, ay, _ = f["A"]
    sim.put(2, [int(ax) - 24, int(ay) - 33, int(ax) + 36, int(ay) + 27])
    sim.put(3, [200, 20, 250, 70])
    for t in range(1, 6):
        sim.step(t)
        assert sim.live() == [0, 1, 2, 3] and not sim.status[:4].any(), t        # nothing stops the two tracks on A
    i = ref.inter(ref.clip(sim.boxes[0], FH, FW), ref.clip(sim.boxes[2], FH, FW))
    assert i > 0.9 * ref.area(ref.clip(sim.boxes[0], FH, FW))                 # (they have drifted onto one another)
    f = _scene(5)
    r = sim.update([_detector(f["B"]), _detector(f["A"])])
    assert r["slot_det"].tolist() == [1, 0, -1, -1, -1] and r["det_slot"].tolist() == [1, 0]
    assert sim.status[:4].tolist() == [0, 0, ref.DUPLICATE, 0]                 # the higher slot on A ends
    assert sim.live() == [0, 1, 3] and sim.misses.tolist() == [0, 0, 0, 1, 0]  # the track on no face: one miss, alive
    assert r["counts"].tolist() == [2, 0, 0, 1, 0, 0, 0, 0]
    for t in range(6, 11):
        sim.step(t)
    assert sim.live() == [0, 1, 3]
    f = _scene(10)
    r = sim.update([_detector(f["A"]), _detector(f["B"]), _detector(f["C"])])
    assert sim.status[3] == ref.UNCONFIRMED and sim.misses[3] == 0            # after exactly max_misses updates
    assert r["det_slot"].tolist() == [0, 1, 2] and r["slot_det"].tolist() == [0, 1, 2, -1, -1]   # C: the lowest dead slot
    assert r["counts"].tolist() == [2, 1, 0, 0, 1, 0, 0, 0] and sim.live() == [0, 1, 2]
    for t in range(11, 16):
        sim.step(t)
    assert sim.live() == [0, 1, 2] and not sim.status[:3].any()
    f = _scene(15)
    spurious = [[300, 10, 330, 40], [350, 10, 380, 40], [420, 200, 450, 230]]
    r = sim.update([_detector(f["A"])] + spurious + [_detector(f["C"]), _detector(f["B"])])
    assert r["det_slot"].tolist() == [0, 3, 4, -2, 2, 1]                       # one detection more than free slots
    assert r["counts"].tolist() == [3, 2, 0, 0, 0, 1, 0, 0] and sim.live() == [0, 1, 2, 3, 4]
    assert not sim.status.any() and not sim.misses.any()
    # a tracker that never gives up (max_misses = 0) keeps the track on no face
    keep = _Sim(2)
    keep.put(0, [200, 20, 250, 70])
    for n in range(1, 4):
        keep.update([[0, 0, 5, 5]] if n == 1 else [[-10 ** 9, 0, 5, 5]])
        assert keep.misses[0] == n and keep.status[0] == 0
