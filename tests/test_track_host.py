"""CPU-side checks of the tracking calls (flm_track_seed, flm_landmarks_from_crop, flm_track_step,
prediction.FaceTracker): the symbols exist, every argument check answers before any launch (so without a GPU),
flm_track.hip compiles for gfx950 without a private segment, the Python wrappers reject what they cannot run, and the
arithmetic the header states (tests/track_ref.py) follows a synthetic face over a sequence of frames and gives it up
for each of the reasons it names."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import flm_amd  # noqa: F401
from flm_amd import _lib, alignment, prediction

import track_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "face-landmark-detector_amd", "csrc")
NAMES = ("flm_track_seed", "flm_landmarks_from_crop", "flm_track_step")


def _build_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("_flm_build", os.path.join(ROOT, "face-landmark-detector_amd", "build.py"))
    bld = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bld)
    return bld


def test_library_exports_the_tracking_entry_points():
    lib = C.CDLL(_lib.LIB_PATH)
    for name in NAMES + ("flm_track_opts_init",):
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTS
    assert _lib.load().flm_abi_version() == 2          # purely additive
    assert "flm_track.hip" in _build_module().SOURCES
    o = _lib.TrackOpts.make()
    assert o.struct_size == C.sizeof(_lib.TrackOpts) == 32
    assert (o.min_points, o.min_score, o.min_side, o.max_side) == (2, 0.0, 0.0, float("inf"))
    assert (_lib.TRACK_DEAD, _lib.TRACK_FEW_POINTS, _lib.TRACK_LOW_SCORE, _lib.TRACK_SCALE, _lib.TRACK_OUTSIDE) == \
        (track_ref.DEAD, track_ref.FEW_POINTS, track_ref.LOW_SCORE, track_ref.SCALE, track_ref.OUTSIDE) == (1, 2, 4, 8, 16)


def _step(lib, p, **kw):
    """flm_track_step with every argument valid (never launched: each caller breaks one)."""
    a = dict(lm=p, ls=2, w=None, ws=1, m=p, boxes=p, k=4, c=68, sx=64 / 72, sy=64 / 72, in_h=64, in_w=64, fh=270, fw=480,
             tc=p, ta=p, opts=None, lmf=p, ma=p, mn=p, bn=p, st=p)
    a.update(kw)
    o = a["opts"]
    return lib.flm_track_step(None, a["lm"], a["ls"], a["w"], a["ws"], a["m"], a["boxes"], a["k"], a["c"], a["sx"], a["sy"],
                              a["in_h"], a["in_w"], a["fh"], a["fw"], a["tc"], a["ta"], None if o is None else C.byref(o),
                              a["lmf"], a["ma"], a["mn"], a["bn"], a["st"])


def test_argument_checks_answer_without_a_gpu():
    lib = _lib.load()
    p = C.c_void_p(0x1000)        # never dereferenced: every call below is rejected before a launch
    err = lambda: lib.flm_last_error().decode()
    # flm_track_seed
    assert lib.flm_track_seed(None, None, 1, 64, 64, 270, 480, p, p) == -1
    assert lib.flm_track_seed(None, p, 1, 64, 64, 270, 480, None, p) == -1
    assert lib.flm_track_seed(None, p, 1, 64, 64, 270, 480, p, None) == -1
    for k in (0, 65536):
        assert lib.flm_track_seed(None, p, k, 64, 64, 270, 480, p, p) == -2
        assert "1 <= k <= 65535" in err()
    for sizes in ((0, 64, 270, 480), (64, 0, 270, 480), (64, 64, 0, 480), (64, 64, 270, -1)):
        assert lib.flm_track_seed(None, p, 1, *sizes, p, p) == -2
        assert "in_h, in_w, fh, fw >= 1" in err()
    # flm_landmarks_from_crop
    assert lib.flm_landmarks_from_crop(None, None, 2, p, 1, 68, 1.0, 1.0, p) == -1
    assert lib.flm_landmarks_from_crop(None, p, 2, None, 1, 68, 1.0, 1.0, p) == -1
    assert lib.flm_landmarks_from_crop(None, p, 2, p, 1, 68, 1.0, 1.0, None) == -1
    for k in (0, 65536):
        assert lib.flm_landmarks_from_crop(None, p, 2, p, k, 68, 1.0, 1.0, p) == -2
        assert "1 <= k <= 65535" in err()
    for c in (0, 1025):
        assert lib.flm_landmarks_from_crop(None, p, 2, p, 1, c, 1.0, 1.0, p) == -2
        assert "1 <= c <= 1024" in err()
    assert lib.flm_landmarks_from_crop(None, p, 1, p, 1, 68, 1.0, 1.0, p) == -2
    assert "lm_stride >= 2" in err()
    for sx, sy in ((0.0, 1.0), (1.0, -1.0), (float("nan"), 1.0)):
        assert lib.flm_landmarks_from_crop(None, p, 2, p, 1, 68, sx, sy, p) == -2
        assert "sx, sy > 0" in err()
    # flm_track_step: null pointers (the weights and the aligned pair are optional)
    for name in ("lm", "m", "boxes", "tc", "lmf", "mn", "bn", "st"):
        assert _step(lib, p, **{name: None}) == -1, name
        assert "null" in err()
    assert _step(lib, p, ta=None) == -1 and "both or neither" in err()
    assert _step(lib, p, ma=None) == -1 and "both or neither" in err()
    # the option struct
    o = _lib.TrackOpts.make()
    o.struct_size -= 8
    assert _step(lib, p, opts=o) == -1 and "struct_size" in err()
    for mp in (1, 0, -3):
        assert _step(lib, p, opts=_lib.TrackOpts.make(min_points=mp)) == -1 and "min_points >= 2" in err()
    nan = float("nan")
    for kw in (dict(min_score=nan), dict(min_side=nan), dict(max_side=nan)):
        assert _step(lib, p, opts=_lib.TrackOpts.make(**kw)) == -1 and "NaN" in err()
    # sizes
    for k in (0, -1, 65536):
        assert _step(lib, p, k=k) == -2 and "1 <= k <= 65535" in err()
    for c in (0, 1025):
        assert _step(lib, p, c=c) == -2 and "1 <= c <= 1024" in err()
    assert _step(lib, p, ls=1) == -2 and "lm_stride >= 2" in err()
    assert _step(lib, p, w=p, ws=0) == -2 and "w_stride >= 1" in err()
    for kw in (dict(in_h=0), dict(in_w=0), dict(fh=0), dict(fw=-5)):
        assert _step(lib, p, **kw) == -2 and "in_h, in_w, fh, fw >= 1" in err()
    for kw in (dict(sx=0.0), dict(sy=-2.0), dict(sx=nan)):
        assert _step(lib, p, **kw) == -2 and "sx, sy > 0" in err()


def test_track_source_compiles_without_scratch(tmp_path):
    """The method of tests/test_frames_host.py (metadata fields only): no kernel of flm_track.hip has a private segment,
    and none takes more than 128 VGPRs."""
    bld = _build_module()
    assert "-ffp-contract=off" in bld.FLAGS
    out = str(tmp_path / "flm_track.s")
    cmd = [bld._hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off",
           *bld.FILE_FLAGS.get("flm_track.hip", []), "-I", os.path.join(ROOT, "include"), "-I", CSRC, "-S",
           "--cuda-device-only", os.path.join(CSRC, "flm_track.hip"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    text = open(out).read()
    kernels = {}
    for m in re.finditer(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)", text):
        kernels[m.group(1)] = (int(m.group(2)), int(m.group(3)))
    print(kernels)
    for name in ("track_seed_kernel", "landmarks_from_crop_kernel", "track_step_kernel"):
        assert any(name in k for k in kernels), name
    bad = {k: v for k, v in kernels.items() if v[0] != 0}
    assert not bad, "kernels with a private segment (scratch): %s" % bad
    assert all(v[1] <= 128 for v in kernels.values()), kernels


class _Model:
    n_classes, input_height, input_width, output_height, output_width = 68, 64, 64, 72, 72


def test_python_wrappers_reject_bad_arguments_on_the_host():
    lm = torch.zeros((2, 68, 2), dtype=torch.float64)
    m = torch.zeros((2, 2, 3), dtype=torch.float32)
    boxes = torch.zeros((2, 4), dtype=torch.int32)
    t = torch.zeros((68, 2), dtype=torch.float64)
    A = alignment
    for bad in (boxes, boxes.to(torch.int64), boxes[0], boxes[:, :3]):      # host memory, dtype, rank, shape
        with pytest.raises(ValueError):
            A.track_seed_device(bad, (64, 64), (270, 480))
    for bad in (lm, lm.to(torch.float32), lm[0], lm[..., :1]):
        with pytest.raises(ValueError):
            A.landmarks_from_crop_device(bad, m, (72, 72), (64, 64))
        with pytest.raises(ValueError):
            A.track_step_device(bad, m, boxes, (72, 72), (64, 64), (270, 480), t)
    tr = prediction.FaceTracker(_Model(), (270, 480), 4)            # (no device state before the first seed or step)
    assert tr.capacity == 4 and tr.m_crop is None
    for slots in ([4], [-1], [0, 0], [0, 1]):                       # outside capacity, repeated, one box for two slots
        with pytest.raises(ValueError):
            tr.seed(slots, [(10, 10, 60, 60)])
    with pytest.raises(ValueError):                                 # not a box
        tr.seed([0], [(10, 10, 60)])
    ring = torch.zeros((2, 270, 480, 3), dtype=torch.uint8)
    for bad in (ring, ring.to(torch.float32), ring[0], [ring[0], ring[1]]):   # host memory, dtype, rank, a list
        with pytest.raises(ValueError):
            tr.step(bad, 0)
    for w in ("scores", 1.0, torch.ones((4, 68), dtype=torch.float64)):
        with pytest.raises(ValueError):
            prediction.FaceTracker(_Model(), (270, 480), 4, weights=w)
    for kw in (dict(capacity=0), dict(capacity=65536), dict(frame_hw=(270, 1)), dict(out_size=(0, 112)), dict(samples=3),
               dict(crop_samples=8), dict(min_points=1), dict(min_side=float("nan")), dict(template=np.zeros((5, 2))),
               dict(crop_template=np.zeros((68, 3))), dict(aligned_format="nchw"), dict(frame_format="nv12")):
        args = dict(model=_Model(), frame_hw=(270, 480), capacity=4)
        args.update(kw)
        with pytest.raises(ValueError):
            prediction.FaceTracker(**args)


# ---- the closed loop on the reference alone ---------------------------------------------------------------------------
IN, GRID, FH, FW, NC = 64, 72, 270, 480, 68
SC = IN / GRID                                    # grid px -> input px
TMPL = alignment.canonical_template(NC, IN, IN)   # crop_template


def pose(scale, deg, cx, cy):
    """The frame landmarks of the template under a similarity about the template's centre, moved to (cx, cy)."""
    th = np.deg2rad(deg)
    r = scale * np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
    return (TMPL - (IN - 1) / 2.0) @ r.T + np.array([cx, cy])


def on_grid(m_crop, pts):
    """What a perfect network would decode: the frame points in the current crop, in output-grid px."""
    return track_ref.apply(m_crop, pts) / SC


def seed_from(pts):
    lo, hi = np.floor(pts.min(0)).astype(int), np.ceil(pts.max(0)).astype(int)
    side = int(max(hi - lo)) + 8
    x0, y0 = int((lo[0] + hi[0] - side) // 2), int((lo[1] + hi[1] - side) // 2)
    boxes = np.array([[x0, y0, x0 + side, y0 + side]], np.int32)
    m, st = track_ref.seed(boxes, IN, IN, FH, FW)
    assert st[0] == 0
    return m, boxes


def one_step(m_crop, boxes, pts, w=None, lm=None, **limits):
    lm = on_grid(m_crop[0], pts)[None] if lm is None else lm
    return track_ref.step(lm, w, m_crop, boxes, SC, SC, IN, IN, FH, FW, TMPL, None, **limits)


def test_reference_follows_a_face_and_gives_it_up():
    n = 8
    scales = np.geomspace(0.5, 2.0, n)              # 0.5x .. 2x
    angles = np.linspace(-20.0, 20.0, n)            # 40 degrees in all
    cxs, cys = np.linspace(200.0, 270.0, n), np.linspace(120.0, 150.0, n)
    m_crop, boxes = seed_from(pose(scales[0], angles[0], cxs[0], cys[0]))
    worst = 0.0
    for t in range(n):
        pts = pose(scales[t], angles[t], cxs[t], cys[t])
        r = one_step(m_crop, boxes, pts)
        assert r["status"][0] == 0, (t, r["status"])
        err = float(np.abs(track_ref.apply(r["m_next"][0], pts) - TMPL).max())
        worst = max(worst, err)
        # float32 entries of M: relative 2^-24 on products with frame coordinates < 2^11 at scales <= 8, and on the
        # translation -- below 1e-3 px a term; the float64 fit itself is exact to 1e-10 on noise-free points
        assert err <= 0.01, (t, err)
        side = IN * scales[t]
        b = r["boxes_next"][0]
        assert not track_ref.box_empty(b, FH, FW) and b[2] - b[0] >= side - 1 and b[3] - b[1] >= side - 1
        assert b[0] <= cxs[t] <= b[2] and b[1] <= cys[t] <= b[3]
        m_crop, boxes = r["m_next"], r["boxes_next"]
    print("closed loop: max |M_next(landmarks) - crop_template| = %.3e px over %d frames" % (worst, n))
    last = pose(scales[-1], angles[-1], cxs[-1], cys[-1])
    # the centre leaves the frame (to the right: coordinates stay positive, so no point is rejected)
    r = one_step(m_crop, boxes, pose(scales[-1], angles[-1], FW + 20.0, cys[-1]))
    assert r["status"][0] == track_ref.OUTSIDE
    assert r["boxes_next"][0].tolist() == [0, 0, 0, 0] and np.array_equal(r["m_next"][0], track_ref.IDENTITY)
    assert track_ref.box_empty(r["boxes_next"][0], FH, FW)
    # ... and a step from that state is dead, with every landmark rejected
    d = one_step(r["m_next"], r["boxes_next"], last)
    assert d["status"][0] & track_ref.DEAD and (d["lm_frame"] == -1.0).all() and d["boxes_next"][0].tolist() == [0, 0, 0, 0]
    # all but one point rejected
    lm = on_grid(m_crop[0], last)[None].copy()
    lm[0, 1:] = -1.0
    r = one_step(m_crop, boxes, last, lm=lm)
    assert r["status"][0] == track_ref.FEW_POINTS and r["boxes_next"][0].tolist() == [0, 0, 0, 0]
    # scores below min_score (and the same scores above it)
    w = np.full((1, NC), 0.1)
    r = one_step(m_crop, boxes, last, w=w, min_score=0.5)
    assert r["status"][0] == track_ref.LOW_SCORE and np.array_equal(r["m_next"][0], track_ref.IDENTITY)
    assert one_step(m_crop, boxes, last, w=w, min_score=0.05)["status"][0] == 0
    # a face smaller than min_side: the 2x face covers 128 px, the 0.5x face 32
    assert one_step(m_crop, boxes, last, min_side=40.0)["status"][0] == 0
    small = pose(0.5, angles[-1], cxs[-1], cys[-1])
    r = one_step(m_crop, boxes, small, min_side=40.0)
    assert r["status"][0] == track_ref.SCALE and r["boxes_next"][0].tolist() == [0, 0, 0, 0]
    assert one_step(m_crop, boxes, last, max_side=100.0)["status"][0] == track_ref.SCALE
