"""CPU-side checks of the piecewise-affine warp over the landmark mesh (flm_mesh_map, flm_mesh_affines,
flm_warp_mesh_frames, alignment.FaceMesh): the default mesh is a Delaunay triangulation that covers the aligned
rectangle, the constructor rejects what the device must never see, every argument check of the three calls answers
before any launch (so without a GPU), the new source compiles for gfx950 without a private segment, and the Python
wrappers reject what they cannot run."""
import ctypes as C
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest
import torch

import flm_amd  # noqa: F401
from flm_amd import _lib, alignment, prediction

import mesh_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "face-landmark-detector_amd", "csrc")
NEW = ("flm_mesh_map", "flm_mesh_affines", "flm_warp_mesh_frames")
FaceMesh = alignment.FaceMesh


def test_library_exports_the_mesh_entry_points():
    lib = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTS
    assert _lib.load().flm_abi_version() == _lib.ABI_VERSION          # purely additive


# ---- the default mesh -----------------------------------------------------------------------------------------------
def area2(pts, tri):
    a, b, c = pts[tri[:, 0]], pts[tri[:, 1]], pts[tri[:, 2]]
    return (b[:, 0] - a[:, 0]) * (c[:, 1] - a[:, 1]) - (b[:, 1] - a[:, 1]) * (c[:, 0] - a[:, 0])


@pytest.mark.parametrize("hw", [(112, 112), (24, 20)])
def test_default_mesh_is_a_delaunay_cover(hw):
    h, w = hw
    mesh = FaceMesh.default(68, h, w)
    pts, tri = mesh.points, mesh.triangles
    assert (mesh.n_points, mesh.n_anchors, mesh.n_landmarks) == (76, 8, 68) and 1 <= mesh.n_triangles <= 255
    assert pts.dtype == np.float64 and tri.dtype == np.int32
    assert np.array_equal(pts[:68], alignment.canonical_template(68, h, w))
    anchors = {(0.0, 0.0), (w - 1.0, 0.0), (w - 1.0, h - 1.0), (0.0, h - 1.0), ((w - 1) / 2, 0.0), (w - 1.0, (h - 1) / 2),
               ((w - 1) / 2, h - 1.0), (0.0, (h - 1) / 2)}
    assert {tuple(p) for p in pts[68:]} == anchors
    ar = area2(pts, tri)
    assert (ar > 0).all()                                            # positively oriented
    assert abs(ar.sum() / 2 - (w - 1) * (h - 1)) <= 1e-9 * (w - 1) * (h - 1)
    # Euler: a triangulation of 76 points of which 8 lie on the hull has 2*76 - 2 - 8 triangles
    assert mesh.n_triangles == 2 * 76 - 2 - 8
    # the empty-circumcircle property, in exact rational arithmetic on the float64 coordinates: no point lies deeper
    # inside a triangle's circumcircle than 1e-9 of its squared radius (cocircular points, of which the mirror-symmetric
    # template has many, lie on it up to the rounding of their coordinates)
    fp = [(Fraction(float(x)), Fraction(float(y))) for x, y in pts]
    slack = Fraction(1, 10 ** 9)
    for t in tri:
        (ax, ay), (bx, by), (cx, cy) = fp[t[0]], fp[t[1]], fp[t[2]]
        d = 2 * (ax * (by - cy) + bx * (cy - ay) + cx * (ay - by))
        a2, b2, c2 = ax * ax + ay * ay, bx * bx + by * by, cx * cx + cy * cy
        ux = (a2 * (by - cy) + b2 * (cy - ay) + c2 * (ay - by)) / d
        uy = (a2 * (cx - bx) + b2 * (ax - cx) + c2 * (bx - ax)) / d
        r2 = (ax - ux) ** 2 + (ay - uy) ** 2
        for i, (qx, qy) in enumerate(fp):
            if i in t:
                continue
            assert (qx - ux) ** 2 + (qy - uy) ** 2 >= r2 * (1 - slack), (t, i)
    # the reference map leaves no pixel without a triangle
    tmap = mesh_ref.mesh_map_ref(pts, tri, h, w)
    assert tmap.dtype == np.uint8 and tmap.shape == (h, w) and (tmap != 255).all() and tmap.max() < mesh.n_triangles
    # deterministic, and other landmark counts work
    again = FaceMesh.default(68, h, w)
    assert np.array_equal(again.triangles, tri) and np.array_equal(again.points, pts)
    five = FaceMesh.default(5, h, w)
    assert five.n_points == 13 and (mesh_ref.mesh_map_ref(five.points, five.triangles, h, w) != 255).all()


def test_reference_map_ties_and_holes():
    pts = np.array([[0, 0], [8, 0], [8, 8], [0, 8]], np.float64)
    tri = np.array([[0, 1, 2], [0, 2, 3]])
    m = mesh_ref.mesh_map_ref(pts, tri, 9, 9)
    assert m[4, 4] == 0 and m[0, 0] == 0 and m[8, 8] == 0           # the shared diagonal and its ends: the lowest index
    assert m[2, 6] == 0 and m[6, 2] == 1
    assert (mesh_ref.mesh_map_ref(pts, tri[::-1], 9, 9)[[4, 0, 8], [4, 0, 8]] == 0).all()
    hole = mesh_ref.mesh_map_ref(pts, tri[1:], 9, 9)
    assert hole[2, 6] == 255 and hole[6, 2] == 0 and hole[4, 4] == 0


def test_reference_affines_rigid_and_fallback():
    mesh = FaceMesh.default(68, 112, 112)
    m = np.array([[[0.2, -0.05, 10.0], [0.05, 0.2, -20.0]]], np.float32)
    lm = mesh_ref.anchor_source_ref(m, mesh.points[:68])             # the landmarks exactly M^-1 of the template
    aff = mesh_ref.mesh_affines_ref(lm, m, mesh.points, mesh.triangles, 8)
    assert aff.shape == (1, mesh.n_triangles, 2, 3) and aff.dtype == np.float32
    assert np.abs(aff[0] - m[0]).max() < 1e-4
    lm2 = lm.copy()
    lm2[0, 30] = np.nan
    aff2 = mesh_ref.mesh_affines_ref(lm2, m, mesh.points, mesh.triangles, 8)
    uses = (mesh.triangles == 30).any(1)
    assert uses.any() and (aff2[0, uses].view(np.uint32) == m[0].view(np.uint32)).all()
    assert (aff2[0, ~uses].view(np.uint32) == aff[0, ~uses].view(np.uint32)).all()


# ---- the constructor ------------------------------------------------------------------------------------------------
def test_constructor_normalises_and_rejects():
    pts = np.array([[0, 0], [10, 0], [10, 10], [0, 10]], np.float64)
    good = FaceMesh(pts, [[0, 2, 1], [0, 2, 3]], 0)                   # the first is negatively oriented: turned
    assert (area2(good.points, good.triangles) > 0).all() and good.triangles.tolist() == [[0, 1, 2], [0, 2, 3]]
    assert good.n_anchors == 0 and good.n_landmarks == 4 and "FaceMesh" in repr(good)
    assert FaceMesh(pts, np.array([[0, 1, 2]], np.int64), 4).n_landmarks == 0
    many = np.stack([np.arange(257.0), np.arange(257.0) ** 2], 1)
    bad = [
        (many, [[0, 1, 2]], 0),                                       # P > 256
        (pts[:2], [[0, 1, 1]], 0),                                    # P < 3
        (pts, [[0, 1, 2]] * 256, 0),                                  # T > 255
        (pts, np.zeros((0, 3), np.int32), 0),                         # T < 1
        (pts, [[0, 1, 4]], 0),                                        # an index outside [0,P)
        (pts, [[0, 1, -1]], 0),
        (pts, [[0, 1, 1]], 0),                                        # a repeated vertex
        (pts, [[2, 1, 2]], 0),
        (np.array([[0, 0], [5, 5], [10, 10], [0, 10]], np.float64), [[0, 1, 2]], 0),          # collinear: area 0
        (np.array([[0, 0], [1e-5, 0], [0, 1e-5], [0, 10]], np.float64), [[0, 1, 2]], 0),      # doubled area 1e-10 < 1e-9
        (pts, [[0, 1, 2]], 5), (pts, [[0, 1, 2]], -1), (pts, [[0, 1, 2]], 1.5),               # n_anchors
        (pts, [[0.0, 1.0, 2.0]], 0),                                  # float indices
        (pts.reshape(2, 4), [[0, 1, 2]], 0), (pts, [0, 1, 2], 0),     # shapes
        (np.array([[0, 0], [np.nan, 0], [10, 10], [0, 10]]), [[0, 1, 2]], 0),
    ]
    for p, t, a in bad:
        with pytest.raises(ValueError):
            FaceMesh(p, t, a)
    assert FaceMesh(np.array([[0, 0], [4e-5, 0], [0, 4e-5], [0, 10]], np.float64), [[0, 1, 2]], 0).n_triangles == 1
    for args in ((68, 1, 112), (68, 112, 1), (0, 112, 112)):
        with pytest.raises(ValueError):
            FaceMesh.default(*args)


# ---- the C calls ------------------------------------------------------------------------------------------------------
def nv12(**kw):
    f = _lib.FrameFormat()
    _lib.load().flm_frame_format_init(C.byref(f))
    f.pixel = _lib.FRAME_NV12
    for k, v in kw.items():
        setattr(f, k, v)
    return f


def test_argument_checks_answer_without_a_gpu():
    lib = _lib.load()
    p = C.c_void_p(0x1000)        # never dereferenced: every call below is rejected before a launch
    err = lambda: lib.flm_last_error().decode()
    r = C.byref
    fh, fw = 1080, 1920

    def mmap(pts=p, tris=p, np_=76, nt=142, hd=112, wd=112, out=p):
        return lib.flm_mesh_map(None, pts, tris, np_, nt, hd, wd, out)

    def affs(lm=p, ls=2, m=p, pts=p, tris=p, np_=76, na=8, nt=142, k=1, min_det=1e-6, out=p):
        return lib.flm_mesh_affines(None, lm, ls, m, pts, tris, np_, na, nt, k, min_det, out)

    def warp(frames=p, stride=fh * fw * 3, nf=8, fh=fh, fw=fw, idx=None, boxes=None, lm=p, ls=2, m=p, pts=p, tris=p, np_=76,
             na=8, nt=142, tmap=p, k=1, dst=p, hd=112, wd=112, samples=1, f=None, src=None, min_det=1e-6, aff=None):
        return lib.flm_warp_mesh_frames(None, frames, stride, nf, fh, fw, idx, boxes, lm, ls, m, pts, tris, np_, na, nt,
                                        tmap, k, dst, hd, wd, samples, f, src, min_det, aff)

    # null pointers -> FLM_ERR_ARG
    for kw in (dict(pts=None), dict(tris=None), dict(out=None)):
        assert mmap(**kw) == -1 and "null" in err(), kw
    for kw in (dict(lm=None), dict(m=None), dict(pts=None), dict(tris=None), dict(out=None)):
        assert affs(**kw) == -1 and "null" in err(), kw
    for kw in (dict(frames=None), dict(lm=None), dict(m=None), dict(pts=None), dict(tris=None), dict(tmap=None), dict(dst=None)):
        assert warp(**kw) == -1 and "null" in err(), kw
    # the mesh's sizes -> FLM_ERR_ARG
    for call in (mmap, affs, warp):
        for nt in (0, 256, -1):
            assert call(nt=nt) == -1 and "1 <= t <= 255" in err(), nt
        for np_ in (2, 257, 0):
            assert call(np_=np_) == -1 and "3 <= p <= 256" in err(), np_
    for call in (affs, warp):
        for na in (-1, 77):
            assert call(na=na) == -1 and "0 <= a <= p" in err(), na
        assert call(ls=1) == -1 and "lm_stride >= 2" in err()
        assert call(min_det=-1.0) == -1 and "min_det" in err()
        assert call(min_det=float("nan")) == -1 and "min_det" in err()
        assert call(k=0) == -2 and "1 <= k <= 65535" in err()
        assert call(k=65536) == -2 and "1 <= k <= 65535" in err()
    assert mmap(hd=0) == -2 and mmap(wd=0) == -2 and "hd, wd >= 1" in err()
    assert mmap(hd=16384, wd=16384) == -2 and "hd*wd*3*4 < 2^31" in err()
    # what flm_warp_affine_frames_src answers, with its codes
    for s in (3, 0, 8, -1):
        assert warp(samples=s) == -1 and "samples" in err()
    bad_fmt = alignment.AlignedFormat().struct()
    bad_fmt.layout = 5
    assert warp(f=r(bad_fmt)) == -1 and "layout" in err()
    f16 = alignment.AlignedFormat.matcher().struct()
    assert warp(dst=C.c_void_p(0x1001), f=r(f16)) == -1 and "aligned" in err()
    assert warp(dst=C.c_void_p(0x1002)) == -1                          # fmt NULL is float32: 4-byte elements
    short = nv12()
    short.struct_size = C.sizeof(_lib.FrameFormat) - 4
    assert warp(src=r(short)) == -1 and "struct_size" in err()
    assert warp(src=r(nv12(pixel=2))) == -1 and "pixel" in err()
    assert warp(src=r(nv12(matrix=2))) == -1 and "matrix" in err()
    # BGR24 ring (src NULL and an explicit BGR24 format alike)
    bgr = nv12(pixel=_lib.FRAME_BGR24)
    for src in (None, r(bgr)):
        assert warp(src=src, nf=0) == -2 and "nframes >= 1" in err()
        assert warp(src=src, stride=fh * fw * 3 - 1) == -2 and "frame_stride >= fh*fw*3" in err()
        assert warp(src=src, stride=1080 * 3, fw=1) == -2 and "fw >= 2" in err()
        assert warp(src=src, fh=0) == -2
        assert warp(src=src, fh=32768, fw=32768, stride=1 << 40) == -2 and "fh*fw*3 < 2^31" in err()
        assert warp(src=src, hd=0) == -2 and warp(src=src, hd=16384, wd=16384) == -2 and "hd*wd*3*4 < 2^31" in err()
    assert warp(src=r(nv12(pixel=_lib.FRAME_BGR24, y_pitch=1920 * 3))) == -2 and "dense" in err()
    # NV12 ring
    full = fh * fw * 3 // 2
    ok = nv12()
    assert warp(src=r(ok), stride=full, fh=1079) == -2 and "even" in err()
    assert warp(src=r(nv12(y_pitch=1919)), stride=full) == -2 and "y_pitch >= fw" in err()
    assert warp(src=r(nv12(y_pitch=2048, uv_pitch=1918)), stride=1 << 23) == -2 and "uv_pitch >= fw" in err()
    assert warp(src=r(ok), stride=full - 1) == -2 and "frame_stride >= flm_frame_format_bytes" in err()
    assert warp(src=r(ok), stride=full, nf=0) == -2 and "nframes >= 1" in err()
    assert warp(src=r(ok), stride=full, hd=0) == -2


def test_mesh_source_compiles_without_scratch(tmp_path):
    """The method of tests/test_frames_nv12_host.py for csrc/flm_mesh.hip: built by build.py, compiles for gfx950 with the
    build's flags, no kernel has a private segment, and the warps keep four waves per SIMD (128 registers) with the
    per-pixel matrix in vector registers."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("_flm_build", os.path.join(ROOT, "face-landmark-detector_amd", "build.py"))
    bld = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bld)
    assert "flm_mesh.hip" in bld.SOURCES
    assert "-ffp-contract=off" in bld.FLAGS
    out = str(tmp_path / "flm_mesh.s")
    cmd = [bld._hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off",
           *bld.FILE_FLAGS.get("flm_mesh.hip", []), "-I", os.path.join(ROOT, "include"), "-I", CSRC, "-S",
           "--cuda-device-only", os.path.join(CSRC, "flm_mesh.hip"), "-o", out]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    text = open(out).read()
    kernels = {}
    for m in re.finditer(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)", text):
        kernels[m.group(1)] = (int(m.group(2)), int(m.group(3)))
    print(kernels)
    assert any("mesh_map_kernel" in k for k in kernels) and any("mesh_affines_kernel" in k for k in kernels)
    for nv in (0, 1):
        for s, unr in ((1, 4), (2, 2), (4, 1)):
            for layout in (0, 1):
                for typ in (0, 1, 2, 3):
                    tag = "warp_mesh_kernelILb%dELi%dELi%dELi%dELi%dE" % (nv, s, unr, layout, typ)
                    assert any(tag in k for k in kernels), tag
    bad = {k: v for k, v in kernels.items() if v[0] != 0}
    assert not bad, "kernels with a private segment (scratch): %s" % bad
    assert all(v[1] <= 128 for v in kernels.values()), kernels


# ---- Python ---------------------------------------------------------------------------------------------------------
def test_python_wrappers_reject_bad_arguments_on_the_host():
    mesh = FaceMesh.default(68, 24, 20)
    ring = torch.zeros((2, 48, 64, 3), dtype=torch.uint8)
    lm = torch.zeros((2, 68, 2), dtype=torch.float64)
    m = torch.zeros((2, 2, 3), dtype=torch.float32)
    with pytest.raises(ValueError):      # host memory
        alignment.warp_mesh_frames_device(ring, lm, m, mesh, 24, 20)
    with pytest.raises(ValueError):
        alignment.mesh_affines_device(lm, m, mesh)
    with pytest.raises(ValueError):
        alignment.mesh_map_device(mesh, 24, 20, out=torch.zeros((24, 20), dtype=torch.uint8))
    with pytest.raises(ValueError):      # not a mesh
        alignment.mesh_map_device("default", 24, 20)
    with pytest.raises(ValueError):
        alignment.mesh_map_device(mesh, 0, 20)
    with pytest.raises(ValueError):
        alignment.mesh_affines_device(lm, m, mesh, min_det=-1.0)
    with pytest.raises(ValueError):      # not a FrameFormat / AlignedFormat
        alignment.warp_mesh_frames_device(ring, lm, m, mesh, 24, 20, src="nv12")
    with pytest.raises(ValueError):
        alignment.warp_mesh_frames_device(ring, lm, m, mesh, 24, 20, fmt="float16")
    with pytest.raises(ValueError):
        prediction.normalize_frames(ring, lm, m, mesh="default")
    with pytest.raises(ValueError):
        prediction.normalize_frames(ring, lm, m, samples=3)
