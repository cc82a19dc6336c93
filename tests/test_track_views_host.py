"""CPU-side checks of the pose-binned best shots (flm_track_views_update, flm_track_exit_views, alignment.PoseViews /
track_views_update_device / track_exit_views_device, FaceTracker(views=...)): the symbols, every argument check answered
before any launch (so without a GPU), the Python rejections, the degree -> edge conversion, the compiler's metadata of the
three kernels, the sign convention of u and v from a rotated head model, and -- on tests/track_views_ref.py alone -- the
contract of include/flm.h on cases written out by hand."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import flm_amd  # noqa: F401
from flm_amd import _lib, alignment, prediction

import head_pose_ref as pref
import track_views_ref as vref

NAN, INF = float("nan"), float("inf")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "face-landmark-detector_amd", "csrc")
S20 = math.sin(math.radians(20.0))


def test_library_exports_the_calls():
    lib = C.CDLL(_lib.LIB_PATH)
    text = open(os.path.join(ROOT, "include", "flm.h")).read()
    for name in ("flm_views_opts_init", "flm_track_views_update", "flm_track_exit_views"):
        assert hasattr(lib, name) and name in _lib.EXPORTS, name
        assert re.search(r"\b%s\(" % name, text), name                 # header and EXPORTS agree
    L = _lib.load()
    assert L.flm_abi_version() == 2 and "#define FLM_ABI_VERSION 2" in text          # purely additive
    assert len(L.flm_track_views_update.argtypes) == 25 and len(L.flm_track_exit_views.argtypes) == 19
    # the prototypes of the header have as many parameters as the argtypes
    for name, fn in (("flm_track_views_update", L.flm_track_views_update), ("flm_track_exit_views", L.flm_track_exit_views)):
        proto = re.search(r"int %s\((.*?)\);" % name, text, re.S).group(1)
        assert len(re.sub(r"/\*.*?\*/", "", proto, flags=re.S).split(",")) == len(fn.argtypes), name
    assert re.search(r"#define FLM_VIEWS_MAX_EDGES (\d+)", text).group(1) == "7" and alignment.VIEWS_MAX_EDGES == 7
    o = _lib.ViewsOpts.make()
    assert o.struct_size == C.sizeof(_lib.ViewsOpts) == 144 and o.reserved == 0
    assert (o.sharp_ref, o.min_exposed, o.n_u, o.n_v) == (100.0, 0.5, 2, 0)
    assert list(o.u_edge)[:2] == [-S20, S20]                           # the C default is PoseViews' default, to the bit
    s = alignment.PoseViews().struct()
    assert bytes(s) == bytes(o)


err = lambda: _lib.load().flm_last_error().decode()
ORDER = ("faces", "face_bytes", "n", "rec", "status", "reset", "lm", "lm_stride", "w", "w_stride", "c", "m", "frame_id", "opts",
         "slot", "n_slots", "pose", "view_q", "view_frame", "view_gallery", "view_m", "view_lm", "view_pose", "take")
SCALARS = ("face_bytes", "n", "lm_stride", "w_stride", "c", "frame_id", "opts", "n_slots")
POINTERS = [n for n in ORDER if n not in SCALARS]
# never dereferenced: every call below is rejected before a launch.  1 GiB apart: no two of them overlap at any size here
FAKE = {n: C.c_void_p((i + 1) << 30) for i, n in enumerate(POINTERS)}
INPUTS = ("faces", "rec", "status", "reset", "lm", "w", "m", "slot", "pose")
OUTPUTS = ("view_q", "view_frame", "view_gallery", "view_m", "view_lm", "view_pose", "take")


def _update(**kw):
    a = dict(FAKE, face_bytes=37, n=4, lm_stride=2, w_stride=1, c=5, frame_id=7, opts=None, n_slots=6)
    a.update(kw)
    if isinstance(a["opts"], _lib.ViewsOpts):
        a["opts"] = C.byref(a["opts"])
    return _lib.load().flm_track_views_update(None, *[a[n] for n in ORDER])


def _opts(u=(-0.3, 0.3), v=(), **kw):
    o = _lib.ViewsOpts.make(list(u), list(v))
    for k, val in kw.items():
        setattr(o, k, val)
    return o


def test_update_argument_checks_answer_without_a_gpu():
    who = "flm_track_views_update"
    for name in ("faces", "rec", "lm", "pose", "view_q", "view_frame", "view_gallery", "take"):
        assert _update(**{name: None}) == -1 and "null" in err() and who in err(), name
    assert _update(m=None) == -1 and "view_m needs m_dev" in err() and who in err()
    assert _update(opts=_opts(struct_size=136)) == -1 and "struct_size" in err() and who in err()
    assert _update(opts=_opts(reserved=1)) == -1 and "reserved" in err() and who in err()
    for bad in (0.0, -1.0, NAN):
        assert _update(opts=_opts(sharp_ref=bad)) == -1 and "sharp_ref" in err() and who in err(), bad
    assert _update(opts=_opts(min_exposed=NAN)) == -1 and "min_exposed" in err() and who in err()
    for axis in ("u", "v"):
        for bad in (-1, 8, 2 ** 31 - 1):
            assert _update(opts=_opts(**{"n_" + axis: bad})) == -1 and "n_%s" % axis in err() and "<= 7" in err(), (axis, bad)
        for edges, what in (((0.3, 0.3), "ascending"), ((0.3, -0.3), "ascending"), ((-1.0, 0.3), "(-1, 1)"),
                            ((0.0, 1.0), "(-1, 1)"), ((NAN,), "(-1, 1)"), ((INF,), "(-1, 1)"), ((-INF, 0.0), "(-1, 1)"),
                            ((0.0, NAN), "(-1, 1)")):
            o = _opts(**{axis: edges}) if axis == "u" else _opts(v=edges)
            assert _update(opts=o) == -1 and what in err() and "%s_edge" % axis in err() and who in err(), (axis, edges)
            assert _update(opts=o, n=0) == -1, (axis, edges)             # the options come before the sizes
    # an edge past the count is not read
    o = _opts(u=(0.25,))
    o.u_edge[1] = NAN
    assert _update(opts=o, lm_stride=1) == -2
    for n in (0, -1, 65536, 2 ** 31 - 1):
        assert _update(n=n) == -2 and "1 <= n <= 65535" in err() and who in err(), n
    for ns in (0, -1, 65536):
        assert _update(n_slots=ns) == -2 and "1 <= n_slots <= 65535" in err() and who in err(), ns
        assert _update(n_slots=ns, slot=None, lm_stride=1) == -2 and "lm_stride" in err(), ns    # not read without slot_dev
    for c in (0, -1, 1025):
        assert _update(c=c) == -2 and "1 <= c <= 1024" in err() and who in err(), c
    assert _update(face_bytes=0) == -2 and "face_bytes >= 1" in err() and who in err()
    for kw in (dict(lm_stride=1), dict(lm_stride=0), dict(w_stride=0)):
        assert _update(**kw) == -2 and "lm_stride >= 2 and w_stride >= 1" in err() and who in err(), kw
    # what is allowed reaches the last size check (the strides): the limits, good options, every optional argument absent
    full = _opts(u=[-0.9 + 0.25 * i for i in range(7)], v=[-0.9 + 0.25 * i for i in range(7)])
    for kw in (dict(n=65535, n_slots=65535, c=1024), dict(n=1, n_slots=1, c=1, face_bytes=1), dict(opts=full),
               dict(opts=_opts(u=(), v=())), dict(opts=_opts(min_exposed=INF)), dict(opts=_opts(min_exposed=-INF)),
               dict(status=None, reset=None, w=None, m=None, view_m=None, slot=None, view_lm=None, view_pose=None),
               dict(w=None, w_stride=0, lm_stride=1)):
        assert _update(**dict(dict(lm_stride=1), **kw)) == -2 and "lm_stride" in err() and who in err(), kw
    # no output may overlap an input or another output: the last check, after every size.  n=4, n_slots=6, B=3, c=5
    sizes = dict(faces=4 * 37, rec=4 * 64, status=16, reset=16, lm=(19 * 2 + 2) * 8, w=20 * 8, m=96, slot=16, pose=6 * 144,
                 view_q=144, view_frame=144, view_gallery=18 * 37, view_m=18 * 24, view_lm=18 * 80, view_pose=18 * 144, take=16)
    for out in OUTPUTS:
        for other in INPUTS + tuple(o for o in OUTPUTS if o != out):
            at = C.c_void_p(FAKE[other].value + sizes[other] - 1)        # the last byte of `other`
            assert _update(**{out: at}) == -1 and "overlap" in err() and who in err(), (out, other)
            at = C.c_void_p(FAKE[other].value + sizes[other])            # adjacent: two buffers
            assert _update(lm_stride=1, **{out: at}) == -2, (out, other)
    base = FAKE["take"].value
    assert _update(view_q=C.c_void_p(base - 143)) == -1 and "view_q and take_dev" in err()
    assert _update(view_q=C.c_void_p(base - 144), lm_stride=1) == -2
    # inputs may share memory with each other (status and reset, say)
    assert _update(reset=FAKE["status"], lm_stride=1) == -2 and "lm_stride" in err()


XORDER = ("exit_row", "k", "q", "bins", "face_bytes", "c", "view_q", "view_frame", "view_gallery", "view_m", "view_lm",
          "view_pose", "x_view_q", "x_view_frame", "x_view_gallery", "x_view_m", "x_view_lm", "x_view_pose")
XPOINTERS = [n for n in XORDER if n not in ("k", "q", "bins", "face_bytes", "c")]
XFAKE = {n: C.c_void_p((i + 1) << 30) for i, n in enumerate(XPOINTERS)}


def _exit(**kw):
    a = dict(XFAKE, k=4, q=2, bins=3, face_bytes=37, c=5)
    a.update(kw)
    return _lib.load().flm_track_exit_views(None, *[a[n] for n in XORDER])


def test_exit_views_argument_checks_answer_without_a_gpu():
    who = "flm_track_exit_views"
    for name in ("exit_row", "view_q", "view_frame", "view_gallery", "x_view_q", "x_view_frame", "x_view_gallery"):
        assert _exit(**{name: None}) == -1 and "null" in err() and who in err(), name
    for name in ("view_m", "x_view_m", "view_lm", "x_view_lm", "view_pose", "x_view_pose"):
        assert _exit(**{name: None}) == -1 and "both or neither" in err() and who in err(), name
    for k in (0, -1, 65536):
        assert _exit(k=k) == -2 and "1 <= k <= 65535" in err() and who in err(), k
    for q in (0, -1, 65536):
        assert _exit(q=q) == -2 and "1 <= q <= 65535" in err() and who in err(), q
    for b in (0, -1, 65):
        assert _exit(bins=b) == -2 and "1 <= bins <= 64" in err() and who in err(), b
    for c in (0, -1, 1025):
        assert _exit(c=c) == -2 and "1 <= c <= 1024" in err() and who in err(), c
    assert _exit(face_bytes=0) == -2 and "face_bytes >= 1" in err() and who in err()
    # the limits and the absent pairs pass every check but the last size check
    for kw in (dict(k=65535, q=65535, bins=1, c=1), dict(k=1, q=1, bins=64, c=1024),
               dict(view_m=None, x_view_m=None, view_lm=None, x_view_lm=None, view_pose=None, x_view_pose=None)):
        assert _exit(face_bytes=0, **kw) == -2 and "face_bytes" in err(), kw
    # overlaps: the last check.  k=4, q=2, B=3
    base = XFAKE["view_q"].value                                       # 4*3*8 = 96 bytes
    for other in ("x_view_q", "exit_row", "x_view_pose", "view_frame"):
        assert _exit(**{other: C.c_void_p(base + 95)}) == -1 and "overlap" in err() and "view_q" in err() and who in err(), other
    assert _exit(x_view_gallery=C.c_void_p(XFAKE["view_gallery"].value + 12 * 37 - 1)) == -1 and \
        "view_gallery and x_view_gallery" in err()
    assert _exit(face_bytes=0, x_view_gallery=C.c_void_p(XFAKE["view_gallery"].value + 12 * 37)) == -2    # adjacent


# ---- PoseViews -------------------------------------------------------------------------------------------------------
def test_pose_views_conversions_and_bins():
    v = alignment.PoseViews()
    assert v.u_edges == (-S20, S20) and v.v_edges == () and v.bins == 3 and (v.sharp_ref, v.min_exposed) == (100.0, 0.5)
    v = alignment.PoseViews(yaw=(-45, -15, 15, 45), pitch=(-10.0, 10.0), sharp_ref=50, min_exposed=0.25)
    assert v.u_edges == tuple(math.sin(math.radians(d)) for d in (-45.0, -15.0, 15.0, 45.0))
    assert v.v_edges == (math.sin(math.radians(-10.0)), math.sin(math.radians(10.0))) and v.bins == 15
    s = v.struct()
    assert (s.n_u, s.n_v, s.sharp_ref, s.min_exposed) == (4, 2, 50.0, 0.25)
    assert list(s.u_edge)[:4] == list(v.u_edges) and list(s.v_edge)[:2] == list(v.v_edges)
    assert alignment.PoseViews(yaw=(), pitch=()).bins == 1
    assert alignment.PoseViews(yaw=range(-30, 40, 10)).bins == 8 and alignment.PoseViews(yaw=range(-30, 40, 10), pitch=range(-30, 40, 10)).bins == 64
    r = alignment.PoseViews.from_edges((-0.5, 0.0, 0.25), (0.125,))
    assert r.u_edges == (-0.5, 0.0, 0.25) and r.v_edges == (0.125,) and r.bins == 8
    assert "from_edges((-0.5, 0.0, 0.25), (0.125,)" in repr(r)
    for bad in (dict(yaw=(20, -20)), dict(yaw=(20, 20)), dict(yaw=(-90, 0)), dict(pitch=(0, 90)), dict(yaw=(NAN,)),
                dict(yaw=(INF,)), dict(yaw=range(-40, 40, 10)), dict(pitch=range(-40, 40, 10)), dict(yaw=3), dict(yaw=("a",)),
                dict(sharp_ref=0), dict(sharp_ref=NAN), dict(min_exposed=NAN)):
        with pytest.raises(ValueError):
            alignment.PoseViews(**bad)
    for bad in (dict(u_edges=(0.3, 0.3)), dict(u_edges=(0.3, -0.3)), dict(u_edges=(-1.0,)), dict(u_edges=(1.0,)),
                dict(u_edges=(NAN,)), dict(u_edges=(), v_edges=(INF,)), dict(u_edges=[0.1 * i for i in range(8)]),
                dict(u_edges=(), v_edges=[0.1 * i for i in range(8)]), dict(u_edges=(), sharp_ref=-1.0), dict(u_edges=None)):
        with pytest.raises(ValueError):
            alignment.PoseViews.from_edges(**bad)


# ---- the Python rejections ---------------------------------------------------------------------------------------------
class _Model:
    n_classes, input_height, input_width, output_height, output_width = 68, 64, 64, 72, 72
    max_batch = 1024


class _HostRing(alignment.FrameFormat):
    def ring(self, frames):
        return 8, 270, 480, 270 * 480 * 3


def test_face_tracker_rejects_views_it_cannot_serve():
    mk = lambda **kw: prediction.FaceTracker(_Model(), (270, 480), 6, frame_format=_HostRing.bgr(), **kw)
    for kw in (dict(), dict(best_shot=True), dict(pose=True), dict(best_shot=True, exits=4), dict(best_shot=False, pose=True)):
        for v in (True, alignment.PoseViews()):
            with pytest.raises(ValueError, match="views needs both best_shot and pose"):
                mk(views=v, **kw)
    for bad in (3, 2.0, "yes", (-20, 20), False):
        with pytest.raises(ValueError, match="views must be"):
            mk(best_shot=True, pose=True, views=bad)
    import inspect
    assert list(inspect.signature(prediction.FaceTracker.__init__).parameters)[-2:] == ["exits", "views"]
    tr = mk(best_shot=True, pose=True, views=True)
    assert isinstance(tr.view_opts, alignment.PoseViews) and tr.view_opts.bins == 3 and tr.view_q is None
    with pytest.raises(ValueError, match="needs a tracker made with exits"):
        tr.exit_views()
    plain = mk(best_shot=True, pose=True, exits=4)
    assert plain.view_opts is None
    for call in (plain.views, plain.exit_views):
        with pytest.raises(ValueError, match="needs a tracker made with views"):
            call()
    custom = alignment.PoseViews.from_edges((0.0,), (0.0,))
    assert mk(best_shot=True, pose=True, exits=4, views=custom).view_opts is custom


def test_wrappers_reject_what_they_must_on_the_host():
    n, b, c = 4, 3, 5
    t = dict(faces=torch.zeros((n, 2, 2, 3)), rec=torch.zeros((n, 8), dtype=torch.int64), lm=torch.zeros((n, c, 2), dtype=torch.float64),
             pose=torch.zeros((n, 18), dtype=torch.float64), view_q=torch.zeros((n, b), dtype=torch.float64),
             view_frame=torch.zeros((n, b), dtype=torch.int64), view_gallery=torch.zeros((n, b, 2, 2, 3)),
             take=torch.zeros(n, dtype=torch.int32))
    args = lambda **kw: [dict(t, **kw)[k] for k in ("faces", "rec", "lm", "pose", "view_q", "view_frame", "view_gallery", "take")]
    with pytest.raises(ValueError, match="opts"):
        alignment.track_views_update_device(*args(), 0, opts=alignment.BestShot())
    with pytest.raises(ValueError, match="frame_id"):
        alignment.track_views_update_device(*args(), 1.5)
    with pytest.raises(ValueError, match="faces"):                     # (not on the device)
        alignment.track_views_update_device(*args(), 0)
    with pytest.raises(ValueError, match="faces"):
        alignment.track_views_update_device(*args(faces=[1, 2]), 0)
    x = dict(exit_row=torch.zeros(n, dtype=torch.int32), view_q=t["view_q"], view_frame=t["view_frame"],
             view_gallery=t["view_gallery"], x_view_q=torch.zeros((2, b), dtype=torch.float64),
             x_view_frame=torch.zeros((2, b), dtype=torch.int64), x_view_gallery=torch.zeros((2, b, 2, 2, 3)))
    xargs = lambda **kw: [dict(x, **kw)[k] for k in ("exit_row", "view_q", "view_frame", "view_gallery", "x_view_q",
                                                     "x_view_frame", "x_view_gallery")]
    with pytest.raises(ValueError, match="view_q"):                    # (not on the device)
        alignment.track_exit_views_device(*xargs())
    with pytest.raises(ValueError, match="view_q"):
        alignment.track_exit_views_device(*xargs(view_q=torch.zeros((n,), dtype=torch.float64)))
    with pytest.raises(ValueError, match="view_q"):
        alignment.track_exit_views_device(*xargs(view_q=torch.zeros((n, 65), dtype=torch.float64)))


def test_the_overlap_check_on_host_tensors():
    """alignment._check_no_overlap, the check of both wrappers that no two tensors share a byte, on views of one buffer
    (tests/test_gpu_track_views.py runs the wrappers themselves, on the device)."""
    buf = torch.zeros(64, dtype=torch.float64)
    ok = lambda *named: alignment._check_no_overlap(list(named))
    ok((buf[0:8], "a"), (buf[8:16], "b"), (buf[16:24], "c"))           # adjacent: three buffers
    ok((buf[16:24], "c"), (buf[0:8], "a"), (None, "n"), (buf[8:16], "b"))   # in any order, None skipped
    ok((buf[0:8], "a"), (buf[4:4], "empty"), (buf[8:16], "b"))         # an empty tensor shares no byte
    ok((buf[0:8], "a"), (buf[8:16].view(torch.int64), "b"), (buf[16:17].view(torch.int32), "c"))
    for named, what in ((((buf[0:8], "a"), (buf[7:15], "b")), "a and b"),                   # one element shared
                        (((buf[7:15], "b"), (buf[0:8], "a")), "a and b"),                   # named in address order
                        (((buf[0:32], "a"), (buf[8:16], "b")), "a and b"),                  # one inside the other
                        (((buf[0:8], "a"), (buf[0:8], "b")), "a and b"),                    # the same tensor twice
                        (((buf[0:8], "a"), (buf[40:48], "c"), (buf[7:9].view(torch.int32)[1:3], "b")), "a and b"),   # four bytes
                        (((buf[0:8], "a"), (buf[8:16], "b"), (buf[15:20], "c")), "b and c")):
        with pytest.raises(ValueError, match="%s must be two buffers that do not overlap" % what):
            alignment._check_no_overlap(list(named))
    # the gallery check refuses what is not on the device before it looks at anything else
    with pytest.raises(ValueError, match="view_gallery must be a contiguous CUDA tensor \\[4,3,...\\]"):
        alignment._check_view_faces(torch.zeros((4, 3, 2, 2, 3)), (4, 3), torch.zeros((4, 2, 2, 3)), "view_gallery")


# ---- the compiler's metadata of the kernels this feature adds -----------------------------------------------------------
def test_the_new_kernels_compile_for_gfx950_without_scratch(tmp_path):
    out = os.path.join(str(tmp_path), "flm_track_views.s")
    cmd = ["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
           "-I", CSRC, "-S", "--cuda-device-only", os.path.join(CSRC, "flm_track_views.hip"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    md = {}
    for block in open(out).read().split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        md[name] = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\n", block)}
    for want in ("track_views_decide_kernel", "track_views_copy_kernel", "track_exit_views_kernel"):
        assert len([n for n in md if want in n]) == 1, (want, sorted(md))
    assert len(md) == 3, sorted(md)                                    # two launches for the update, one for the exits
    for name, k in md.items():
        print(name, {f: k[f] for f in ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")})
        assert k["private_segment_fixed_size"] == 0 and k["wavefront_size"] == 64, (name, k)
        assert k["group_segment_fixed_size"] == 0, (name, k)
    text = "".join(open(os.path.join(CSRC, f)).read() for f in ("flm_track_views.hip", "flm_track_views_dev.h", "flm_copy_dev.h",
                                                                "flm_best_dev.h"))
    assert "atomic" not in text.replace("no atomics", "") and "hipMalloc" not in text and "Synchronize" not in text
    build = open(os.path.join(ROOT, "face-landmark-detector_amd", "build.py")).read()
    assert '"flm_track_views.hip"' in build


# ---- the sign convention of u and v, from a head model rotated by a known angle -----------------------------------------
def _record_of(yaw, pitch):
    idx, xyz = pref.DEFAULT_INDICES, np.asarray(pref.DEFAULT_POINTS, np.float64)
    pts = pref.project(xyz, pref.rotation(yaw, pitch, 0.0), 0.2, 240.0, 135.0)
    lm = np.full((68, 2), -1.0)
    lm[idx] = pts
    return pref.fit_one(lm, None, idx, xyz), lm


def test_u_is_positive_for_a_face_turned_to_the_images_left():
    edges = alignment.PoseViews().u_edges
    front, lm0 = _record_of(0.0, 0.0)
    nose_dx = lambda lm: lm[30, 0] - 0.5 * (lm[36, 0] + lm[45, 0])     # the nose tip against the midpoint of the eye corners
    nose_dy = lambda lm: lm[30, 1] - 0.5 * (lm[36, 1] + lm[45, 1])
    assert front[14] == 1.0 and abs(front[6]) < 1e-12 and vref.bin_of(front, edges, ()) == 1
    for deg in (25.0, 40.0, 60.0):
        a = math.radians(deg)
        left, lm = _record_of(a, 0.0)                                  # yaw > 0
        assert left[14] == 1.0 and abs(-left[6] - math.sin(a)) < 1e-9 and abs(left[15] - a) < 1e-9
        assert nose_dx(lm) < nose_dx(lm0) - 1.0                        # the nose points to the image's LEFT (smaller x)
        assert vref.bin_of(left, edges, ()) == 2
        right, lm = _record_of(-a, 0.0)
        assert abs(-right[6] + math.sin(a)) < 1e-9 and nose_dx(lm) > nose_dx(lm0) + 1.0 and vref.bin_of(right, edges, ()) == 0
    for deg in (10.0, 19.0):                                           # inside the frontal bin on both sides
        for sgn in (1.0, -1.0):
            assert vref.bin_of(_record_of(sgn * math.radians(deg), 0.0)[0], edges, ()) == 1
    # v = sin(pitch) > 0: the face looks DOWN in the image (its nose moves down against its eyes: Y points down)
    down, lm = _record_of(0.0, math.radians(25.0))
    assert abs(down[7] - math.sin(math.radians(25.0))) < 1e-9 and nose_dy(lm) > nose_dy(lm0) + 1.0
    assert vref.bin_of(down, (), (0.0,)) == 1 and vref.bin_of(_record_of(0.0, -0.3)[0], (), (0.0,)) == 0
    # a yaw edge is exact at pitch 0 only: u = cos(pitch) * sin(yaw)
    both = _record_of(math.radians(21.0), math.radians(30.0))[0]
    assert abs(-both[6] - math.cos(math.radians(30.0)) * math.sin(math.radians(21.0))) < 1e-9
    assert vref.bin_of(both, edges, ()) == 1 and vref.bin_of(_record_of(math.radians(21.0), 0.0)[0], edges, ()) == 2


# ---- the restatement against cases written out by hand: 2 slots, B = 3, faces of 6 bytes ----------------------------------
UE = alignment.PoseViews.from_edges((-0.3, 0.3)).u_edges          # the edges as the product hands them to the C call


def _rec(sharp, exposed_percent):
    """A record whose sharpness is `sharp` and whose exposed share is exposed_percent / 100 (n_lap = 64, S_L = 0)."""
    return [100, 0, 0, 64, 0, int(64 * 256 * sharp), 100 - exposed_percent, 0]


def _pose(u, ok=1.0, v=0.0):
    p = np.zeros(18)
    p[14], p[6], p[7] = ok, -u, v
    p[9] = 3.0                                                         # something to recognise in view_pose
    return p


def test_the_restatement_on_cases_written_out_by_hand():
    assert UE == (-0.3, 0.3) and alignment.PoseViews.from_edges(UE).bins == 3
    s = vref.new_state(2, 3, (6,), np.uint8, 2)
    faces = lambda k: (np.arange(12, dtype=np.uint8).reshape(2, 6) + 20 * k)
    lm = lambda k: np.arange(8, dtype=np.float64).reshape(2, 2, 2) + 100.0 * k
    m = lambda k: np.arange(12, dtype=np.float32).reshape(2, 2, 3) + 10 * k
    # frame 1: slot 0 lies ON the upper edge (-> bin 2) with q = 0.5 * 1.0; slot 1 is frontal with q = 0.5 * 0.5
    pose = np.stack([_pose(0.3), _pose(0.0)])
    rec = np.array([_rec(50, 100), _rec(50, 50)], np.int64)
    take = vref.update(s, faces(1), rec, lm(1), pose, 11, UE, (), m=m(1))
    assert take.tolist() == [2, 1]
    assert s["view_q"].tolist() == [[-1.0, -1.0, 0.5], [-1.0, 0.25, -1.0]] and s["view_frame"].tolist() == [[-1, -1, 11], [-1, 11, -1]]
    assert np.array_equal(s["view_gallery"][0, 2], faces(1)[0]) and np.array_equal(s["view_gallery"][1, 1], faces(1)[1])
    assert np.array_equal(s["view_m"][0, 2], m(1)[0]) and np.array_equal(s["view_lm"][1, 1], lm(1)[1])
    assert np.array_equal(s["view_pose"][0, 2], pose[0]) and (s["view_gallery"][0, :2] == 0).all()
    # frame 2: a tie in slot 0 (the earlier frame stays); slot 1's pose is not ok
    before = {k: v.copy() for k, v in s.items()}
    take = vref.update(s, faces(2), rec, lm(2), np.stack([_pose(0.9), _pose(0.0, ok=0.0)]), 12, UE, (), m=m(2))
    assert take.tolist() == [-1, -1] and all(np.array_equal(s[k], before[k]) for k in s)
    # frame 3: slot 0 turned right, a blurred face (q = 0.25) -- its own bin is empty, so it is taken although the track has
    # a better face elsewhere; slot 1: status != 0, e below min_exposed, a NaN u -- none is taken
    take = vref.update(s, faces(3), np.array([_rec(25, 100), _rec(200, 100)], np.int64), lm(3),
                       np.stack([_pose(-0.31), _pose(0.0)]), 13, UE, (), m=m(3), status=np.array([0, 2], np.int32))
    assert take.tolist() == [0, -1] and s["view_q"][0].tolist() == [0.25, -1.0, 0.5] and s["view_frame"][0].tolist() == [13, -1, 11]
    for kw in (dict(rec=np.array([_rec(25, 100), _rec(200, 49)], np.int64)), dict(pose=np.stack([_pose(-0.31), _pose(NAN)])),
               dict(pose=np.stack([_pose(-0.31), _pose(0.0, v=NAN)]))):
        a = dict(rec=np.array([_rec(25, 100), _rec(200, 100)], np.int64), pose=np.stack([_pose(-0.31), _pose(0.0)]))
        a.update(kw)
        assert vref.update(s, faces(3), a["rec"], lm(3), a["pose"], 13, UE, (), m=m(3)).tolist() == [-1, -1], kw
    # frame 4: a better face in slot 1's bin replaces it (sharpness saturates at sharp_ref: q = 1.0 * 0.5)
    take = vref.update(s, faces(4), np.array([_rec(25, 100), _rec(200, 50)], np.int64), lm(4),
                       np.stack([_pose(-0.31), _pose(0.0)]), 14, UE, (), m=m(4))
    assert take.tolist() == [-1, 1] and s["view_q"][1].tolist() == [-1.0, 0.5, -1.0] and s["view_frame"][1, 1] == 14
    assert np.array_equal(s["view_gallery"][1, 1], faces(4)[1])
    # frame 5: a reset in slot 0 empties all three bins first -- and nothing else -- then the face goes into its bin
    gal = s["view_gallery"].copy()
    take = vref.update(s, faces(5), np.array([_rec(10, 100), _rec(1, 50)], np.int64), lm(5),
                       np.stack([_pose(0.0), _pose(0.0)]), 15, UE, (), m=m(5), reset=np.array([1, 0], np.int32))
    assert take.tolist() == [1, -1] and s["view_q"][0].tolist() == [-1.0, 0.1, -1.0]
    assert s["view_frame"][0].tolist() == [13, 15, 11]                 # the emptied bins keep their other entries
    assert np.array_equal(s["view_gallery"][0, [0, 2]], gal[0, [0, 2]]) and np.array_equal(s["view_gallery"][0, 1], faces(5)[0])
    # the rows form: row 0 -> slot 1, row 1 inert; slot 0 is named by no row
    before = {k: v.copy() for k, v in s.items()}
    take = vref.update(s, faces(6), np.array([_rec(200, 100), _rec(200, 100)], np.int64), lm(6),
                       np.stack([_pose(0.0), _pose(0.5)]), 16, UE, (), m=m(6), slot=np.array([1, 2], np.int32))
    assert take.tolist() == [2, -1]                                    # read at the SLOT's pose: u = 0.5
    assert np.array_equal(s["view_gallery"][1, 2], faces(6)[0]) and s["view_q"][1].tolist() == [-1.0, 0.5, 1.0]
    assert all(np.array_equal(s[k][0], before[k][0]) for k in s)
    # the exits: slot 0 -> ring row 1, slot 1 discarded; the empty bins of slot 0 leave the ring's bytes alone
    ring = {"x_" + k: np.full((2,) + v.shape[1:], 7, v.dtype) for k, v in s.items()}
    vref.exit_views(s, ring, np.array([1, -2], np.int32))
    assert ring["x_view_q"].tolist() == [[7.0] * 3, [-1.0, 0.1, -1.0]] and ring["x_view_frame"][1].tolist() == [13, 15, 11]
    assert np.array_equal(ring["x_view_gallery"][1, 1], s["view_gallery"][0, 1]) and (ring["x_view_gallery"][1, [0, 2]] == 7).all()
    assert np.array_equal(ring["x_view_pose"][1, 1], s["view_pose"][0, 1]) and (ring["x_view_lm"][1, 0] == 7).all()
    assert all((v[0] == 7).all() for v in ring.values())
    vref.exit_views(s, ring, np.array([-1, -3], np.int32))
    assert all((v[0] == 7).all() for v in ring.values())
