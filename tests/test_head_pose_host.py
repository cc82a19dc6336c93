"""CPU-side checks of the head-pose call (flm_head_pose, alignment.HeadModel / HeadPose, FaceTracker(pose=)): the
exports, every argument check of the C call (each answers before any launch, so without a GPU), tests/head_pose_ref.py
against poses it is given exactly -- which pins the sign conventions --, the degenerate point sets, and the Python
validation."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

import flm_amd  # noqa: F401
from flm_amd import _lib, alignment, prediction

import head_pose_ref as ref

f64 = np.float64
P = C.c_void_p(0x1000)        # never dereferenced: every call below is rejected before a launch


def err():
    return _lib.load().flm_last_error().decode()


def _codes():
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "flm.h")).read()
    return {n: int(v) for n, v in re.findall(r"(FLM_ERR_\w+)\s*=\s*(-?\d+)", text)}


ARG, SHAPE = _codes()["FLM_ERR_ARG"], _codes()["FLM_ERR_SHAPE"]


# ---- export and ABI -------------------------------------------------------------------------------------------------------
def test_exports_and_defaults():
    lib = C.CDLL(_lib.LIB_PATH)
    for name in ("flm_pose_opts_init", "flm_head_pose"):
        assert hasattr(lib, name) and name in _lib.EXPORTS, name
    assert _lib.load().flm_abi_version() == 2          # purely additive
    o = _lib.PoseOpts.make()
    assert (o.struct_size, o.reserved, o.min_volume, o.min_frontal) == (C.sizeof(_lib.PoseOpts), 0, 1e-6, 0.0)
    assert o.struct_size == 24 and _lib.POSE_REC == 18 == alignment.POSE_REC == ref.REC
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "flm.h")).read()
    assert re.search(r"#define FLM_POSE_REC 18\b", text)


# ---- argument checks ------------------------------------------------------------------------------------------------------
def pose_call(**kw):
    # lm [2,68] records of 6 doubles at 0x10000 (6528 bytes), weights inside them; everything else far away
    a = dict(lm=C.c_void_p(0x10000), ls=6, w=C.c_void_p(0x10010), ws=6, n=2, c=68, idx=C.c_void_p(0x20000),
             xyz=C.c_void_p(0x21000), p=6, opts=None, slot=None, n_slots=0, pose=C.c_void_p(0x30000),
             factor=C.c_void_p(0x40000))
    a.update(kw)
    return _lib.load().flm_head_pose(None, a["lm"], a["ls"], a["w"], a["ws"], a["n"], a["c"], a["idx"], a["xyz"], a["p"],
                                     None if a["opts"] is None else C.byref(a["opts"]), a["slot"], a["n_slots"], a["pose"],
                                     a["factor"])


def test_argument_errors():
    O = _lib.PoseOpts
    for name in ("lm", "idx", "xyz", "pose"):
        assert pose_call(**{name: None}) == ARG, name
        assert "null" in err() and "flm_head_pose" in err()
    small = O.make()
    small.struct_size = 16
    res = O.make()
    res.reserved = 1
    nan, inf = float("nan"), float("inf")
    for kw, word in [(dict(opts=small), "struct_size"), (dict(opts=res), "reserved"),
                     (dict(opts=O.make(min_volume=nan)), "min_volume >= 0"), (dict(opts=O.make(min_volume=-1e-9)), "min_volume >= 0"),
                     (dict(opts=O.make(min_frontal=nan)), "min_frontal <= 1"), (dict(opts=O.make(min_frontal=-0.1)), "min_frontal <= 1"),
                     (dict(opts=O.make(min_frontal=1.5)), "min_frontal <= 1"), (dict(opts=O.make(min_frontal=inf)), "min_frontal <= 1"),
                     # outputs over inputs: the landmarks' last double ends at 0x10000 + ((2*68-1)*6 + 2)*8 = 0x10000 + 6496
                     (dict(pose=C.c_void_p(0x10000 + 6488)), "overlaps lm_dev"),
                     (dict(pose=C.c_void_p(0x10000 - 2 * 18 * 8 + 8)), "overlaps lm_dev"),
                     (dict(factor=C.c_void_p(0x10000 + 6488)), "overlaps lm_dev"),
                     (dict(lm=C.c_void_p(0x50000), pose=C.c_void_p(0x10010 + 135 * 48)), "overlaps w_dev"),
                     (dict(pose=C.c_void_p(0x20000 + 20)), "overlaps idx_dev"),
                     (dict(factor=C.c_void_p(0x21000 + 6 * 24 - 8)), "overlaps xyz_dev"),
                     (dict(slot=C.c_void_p(0x60000), n_slots=4, factor=C.c_void_p(0x60004)), "overlaps slot_dev"),
                     (dict(factor=C.c_void_p(0x30000 + 2 * 18 * 8 - 8)), "pose_dev and factor_out overlap"),
                     # with slot the record tensor has n_slots rows
                     (dict(slot=C.c_void_p(0x60000), n_slots=100, factor=C.c_void_p(0x30000 + 99 * 144)), "pose_dev and factor_out")]:
        assert pose_call(**kw) == ARG, kw
        assert word in err() and "flm_head_pose" in err(), (kw, err())
    for kw, word in [(dict(n=0), "1 <= n <= 65535"), (dict(n=65536), "1 <= n <= 65535"), (dict(c=0), "1 <= c <= 1024"),
                     (dict(c=1025), "1 <= c <= 1024"), (dict(p=3), "4 <= p <= 256"), (dict(p=257), "4 <= p <= 256"),
                     (dict(ls=1), "lm_stride >= 2"), (dict(ws=0), "w_stride >= 1"),
                     (dict(slot=P, n_slots=0), "1 <= n_slots <= 65535"), (dict(slot=P, n_slots=65536), "1 <= n_slots <= 65535")]:
        assert pose_call(**kw) == SHAPE, kw
        assert word in err(), (kw, err())


# ---- the restatement recovers the pose it is given ------------------------------------------------------------------------
def test_angle_recovery():
    rng = np.random.default_rng(11)
    idx, xyz = np.array(ref.DEFAULT_INDICES), np.array(ref.DEFAULT_POINTS)
    worst = np.zeros(5)
    for _ in range(2000):
        yaw, pitch = rng.uniform(-1.0, 1.0, 2)
        roll = rng.uniform(-3.0, 3.0)
        scale = rng.uniform(0.05, 3.0)
        w = rng.uniform(0.1, 1.0, 68)
        lm = np.full((68, 2), -1.0)
        lm[idx] = ref.project(xyz, ref.rotation(yaw, pitch, roll), scale, 2000.0, 1500.0)
        assert lm[idx].min() >= 0.0
        rec = ref.fit_one(lm, w, idx, xyz)
        assert rec[14] == 1.0 and rec[13] == 6.0
        got = np.array([rec[15] - yaw, rec[16] - pitch, rec[17] - roll, rec[9] / scale - 1.0, rec[12]])
        worst = np.maximum(worst, np.abs(got))
    print("worst yaw, pitch, roll, relative scale, rms:", worst)
    assert (worst < 1e-9).all(), worst


def test_sign_conventions():
    idx, xyz = np.array(ref.DEFAULT_INDICES), np.array(ref.DEFAULT_POINTS)
    lm = np.full((68, 2), -1.0)
    lm[idx] = xyz[:, :2] + 500.0                            # the model seen frontally at scale 1
    rec = ref.fit_one(lm, None, idx, xyz)
    assert np.allclose(rec[:9].reshape(3, 3), np.eye(3), atol=1e-12) and abs(rec[9] - 1.0) < 1e-12 and rec[8] > 0.999999
    assert np.allclose(rec[10:12], lm[idx].mean(0)) and np.allclose(rec[15:], 0.0, atol=1e-12)
    # a positive yaw turns the nose (Z = 0, nearest the camera) towards image-left of the eyes' midpoint
    lm[idx] = ref.project(xyz, ref.rotation(0.5, 0.0, 0.0), 1.0, 500.0, 500.0)
    rec = ref.fit_one(lm, None, idx, xyz)
    assert abs(rec[15] - 0.5) < 1e-12 and lm[30, 0] < (lm[36, 0] + lm[45, 0]) / 2
    # a positive pitch moves the nose down (Y down: larger y) against the eyes; a positive roll is clockwise in the image
    lm[idx] = ref.project(xyz, ref.rotation(0.0, 0.4, 0.0), 1.0, 500.0, 500.0)
    front = xyz[0, 1] - xyz[2, 1]
    assert abs(ref.fit_one(lm, None, idx, xyz)[16] - 0.4) < 1e-12 and lm[30, 1] - lm[36, 1] > front
    lm[idx] = ref.project(xyz, ref.rotation(0.0, 0.0, 0.3), 1.0, 500.0, 500.0)
    assert abs(ref.fit_one(lm, None, idx, xyz)[17] - 0.3) < 1e-12 and lm[45, 1] > lm[36, 1]
    assert np.array_equal(ref.factor(rec[None], 0.0), [rec[8]]) and ref.factor(rec[None], 0.95)[0] == 0.0


# ---- degenerate sets ------------------------------------------------------------------------------------------------------
def test_degenerate_sets():
    idx, xyz = np.array(ref.DEFAULT_INDICES), np.array(ref.DEFAULT_POINTS)
    full = np.full((68, 2), -1.0)
    full[idx] = ref.project(xyz, ref.rotation(0.3, -0.2, 0.1), 0.7, 900.0, 700.0)
    info = {}
    assert ref.fit_one(full, None, idx, xyz, info=info)[14] == 1.0 and 0.9 < info["vol"] < 0.95
    coplanar = (2, 3, 4, 5)                                  # the eye and mouth corners: Z = 135, 135, 125, 125 on a plane
    vols = []
    for k in (4, 5):
        for keep in itertools.combinations(range(6), k):
            lm = np.full((68, 2), -1.0)
            lm[idx[list(keep)]] = full[idx[list(keep)]]
            rec = ref.fit_one(lm, None, idx, xyz, info=info)
            assert rec[13] == k
            if keep == coplanar:
                assert info["vol"] == 0.0 and np.array_equal(rec, ref.not_ok(4)), (keep, info)
            else:
                assert rec[14] == 1.0, (keep, info)
                vols.append(info["vol"])
                assert np.abs(rec[15:] - [0.3, -0.2, 0.1]).max() < 1e-9
    print("smallest vol of a non-planar subset:", min(vols))
    assert 6e-3 < min(vols) < 7e-3                           # three orders above the default threshold of 1e-6
    for keep in itertools.combinations(range(6), 3):
        lm = np.full((68, 2), -1.0)
        lm[idx[list(keep)]] = full[idx[list(keep)]]
        assert np.array_equal(ref.fit_one(lm, None, idx, xyz), ref.not_ok(3))
    assert np.array_equal(ref.fit_one(np.full((68, 2), -1.0), None, idx, xyz), ref.not_ok(0))
    assert np.array_equal(ref.fit_one(full, np.zeros(68), idx, xyz), ref.not_ok(0))
    w = np.ones(68)
    w[[30, 8]] = [np.nan, -1.0]                              # a NaN and a negative weight leave their points out
    assert np.array_equal(ref.fit_one(full, w, idx, xyz), ref.not_ok(4))    # ... and the coplanar four remain


# ---- the Python validation ------------------------------------------------------------------------------------------------
def test_head_model_validation():
    A = alignment
    pts = [[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]]
    m = A.HeadModel([0, 1, 2, 3], pts)
    assert len(m) == 4 and m.indices.dtype == np.int32 and m.points.dtype == np.float64
    with pytest.raises(ValueError, match="distinct"):
        A.HeadModel([0, 1, 2, 2], pts)
    with pytest.raises(ValueError, match="4 to 256"):
        A.HeadModel([0, 1, 2], pts[:3])
    with pytest.raises(ValueError, match="4 to 256"):
        A.HeadModel(list(range(257)), np.zeros((257, 3)))
    for bad in (np.nan, np.inf):
        with pytest.raises(ValueError, match="finite"):
            A.HeadModel([0, 1, 2, 3], [[bad, 0, 0]] + pts[1:])
    with pytest.raises(ValueError):
        A.HeadModel([0, 1, 2, -3], pts)
    with pytest.raises(ValueError):
        A.HeadModel([0, 1, 2, 3], pts[:3])
    with pytest.raises(ValueError, match="68 landmarks"):
        A.HeadModel.default(67)
    d = A.HeadModel.default(68)
    assert d.indices.tolist() == ref.DEFAULT_INDICES and d.points.tolist() == ref.DEFAULT_POINTS


def test_python_argument_checks():
    A = alignment
    for kw in (dict(min_volume=-1.0), dict(min_volume=float("nan")), dict(min_frontal=-0.1), dict(min_frontal=1.1),
               dict(min_frontal=float("nan")), dict(model="default")):
        with pytest.raises(ValueError):
            A.HeadPose(**kw)
    h = A.HeadPose(min_volume=1e-3, min_frontal=0.5)
    s = h.struct()
    assert (s.min_volume, s.min_frontal, s.reserved) == (1e-3, 0.5, 0) and h.model_for(68).indices.tolist() == ref.DEFAULT_INDICES
    with pytest.raises(ValueError, match="68 landmarks"):
        h.model_for(5)
    import torch
    lm = torch.zeros((2, 68, 2), dtype=torch.float64)
    with pytest.raises(ValueError, match="HeadModel"):
        A.head_pose_device(lm, None)
    with pytest.raises(ValueError, match="HeadPose"):
        A.head_pose_device(lm, A.HeadModel.default(68), opts=object())
    with pytest.raises(ValueError, match="CUDA"):
        A.head_pose_device(lm, A.HeadModel.default(68))
    with pytest.raises(ValueError, match="pose"):
        prediction.FaceTracker(None, (270, 480), 2, pose="yes")
    with pytest.raises(ValueError, match="pose"):
        prediction.head_pose(np.zeros((1, 68, 2)), pose=object())
    with pytest.raises(ValueError, match="68 landmarks"):
        prediction.head_pose(np.zeros((1, 5, 2)))
    with pytest.raises(ValueError, match=r"\[N,C,2\]"):
        prediction.head_pose(np.zeros((68, 2)))


# ---- the compiler's metadata of the kernel ---------------------------------------------------------------------------------
def test_kernel_compiles_for_gfx950_without_scratch(tmp_path):
    import shutil
    import subprocess
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "face-landmark-detector_amd", "csrc")
    out = str(tmp_path / "flm_pose.s")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(root, "include"),
           "-I", csrc, "-S", "--cuda-device-only", os.path.join(csrc, "flm_pose.hip"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    blocks = [b for b in open(out).read().split("  - .agpr_count:")[1:] if "head_pose_kernel" in b]
    assert len(blocks) == 1
    k = {n: int(v) for n, v in re.findall(r"\.(\w+):\s+(\d+)\n", blocks[0])}
    print({f: k[f] for f in ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")})
    assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0
    assert k["group_segment_fixed_size"] <= 16 * 1024          # 256 staged points of six doubles, the sums and the means
