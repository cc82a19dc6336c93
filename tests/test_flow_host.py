"""CPU-side checks of the landmark flow (flm_flow_pyramid, flm_landmark_flow, alignment.LandmarkFlow,
FaceTracker.step_flow): the exports, every argument check of the three calls answered before any launch (so without a
GPU), the Python rejections, the new source compiled for gfx950 without a private segment, and the properties of the
numpy reference (tests/flow_ref.py) alone on a synthetic multi-scale texture."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import flm_amd  # noqa: F401
from flm_amd import _lib, alignment, prediction

import flow_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "face-landmark-detector_amd", "csrc")
NEW = ("flm_flow_pyramid_bytes", "flm_flow_pyramid", "flm_flow_opts_init", "flm_landmark_flow")


def test_library_exports_the_flow_entry_points():
    lib = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTS
    assert _lib.load().flm_abi_version() == _lib.ABI_VERSION == 2      # purely additive
    o = _lib.FlowOpts.make()
    assert C.sizeof(_lib.FlowOpts) == 56 == o.struct_size
    assert (o.levels, o.radius, o.max_iter, o.eps, o.min_eig, o.max_err, o.max_move) == (4, 7, 10, 0.03, 0.5, 12.0, 64.0)
    assert (o.reserved, o.pad) == (0, 0)
    f = alignment.LandmarkFlow()
    assert (f.levels, f.radius, f.max_iter, f.eps, f.min_eig, f.max_err, f.max_move) == (4, 7, 10, 0.03, 0.5, 12.0, 64.0)


def test_pyramid_bytes():
    lib = _lib.load()
    assert lib.flm_flow_pyramid_bytes(64, 64, 3) == 64 * 64 + 32 * 32 + 16 * 16 == flow_ref.pyramid_bytes(64, 64, 3)
    assert lib.flm_flow_pyramid_bytes(32, 48, 2) == 32 * 48 + 16 * 24
    assert lib.flm_flow_pyramid_bytes(256, 256, 4) == 87040 == alignment.LandmarkFlow().pyramid_bytes(256, 256)
    for bad in ((0, 64, 3), (64, 0, 3), (64, 64, 0), (64, 64, 7), (-4, 64, 1)):
        assert lib.flm_flow_pyramid_bytes(*bad) == 0


def test_argument_checks_answer_without_a_gpu():
    lib = _lib.load()
    p, q = C.c_void_p(0x10000000), C.c_void_p(0x20000000)   # never dereferenced: every call is rejected before a launch
    err = lambda: lib.flm_last_error().decode()

    def pyr(src=p, n=2, h=64, w=64, ch=3, levels=3, out=q):
        return lib.flm_flow_pyramid(None, src, n, h, w, ch, levels, out)

    assert pyr(src=None) == -1 and pyr(out=None) == -1 and "null" in err()
    assert pyr(n=0) == -2 and "1 <= n <= 131070" in err()
    assert pyr(n=131071) == -2
    assert pyr(ch=2) == -2 and "ch" in err()
    assert pyr(ch=4) == -2
    assert pyr(levels=0) == -2 and "1 <= levels <= 6" in err()
    assert pyr(levels=7) == -2
    assert pyr(h=60, levels=4) == -2 and "multiples of 2^(levels-1) = 8" in err()
    assert pyr(w=66) == -2
    assert pyr(h=4, w=4, levels=3) == -2 and "at least 8" in err()       # (h >> 2) == 1
    assert pyr(h=32772, w=8) == -2 and "32768" in err()
    assert pyr(out=C.c_void_p(0x10000000 + 100)) == -1 and "overlaps" in err()
    assert pyr(n=131070, h=32768, w=32768, levels=1) == -2 and "2^31" in err()

    def flow(pp=p, pc=q, k=2, h=64, w=64, lm=C.c_void_p(0x30000000), wp=None, m=C.c_void_p(0x40000000), c=68, opts=True,
             lo=C.c_void_p(0x50000000), wo=None, eo=None, fo=C.c_void_p(0x60000000), **kw):
        o = None
        if opts:
            o = _lib.FlowOpts.make(levels=3)
            for name, v in kw.items():
                setattr(o, name, v)
            o = C.byref(o)
        return lib.flm_landmark_flow(None, pp, pc, k, h, w, lm, wp, m, c, o, lo, wo, eo, fo)

    for name in ("pp", "pc", "lm", "m", "lo", "fo"):
        assert flow(**{name: None}) == -1 and "null" in err(), name
    assert flow(struct_size=8) == -1 and "struct_size" in err()
    assert flow(reserved=1) == -1 and "reserved" in err()
    assert flow(pad=1) == -1 and "pad" in err()
    for name, bad, word in (("eps", (0.0, -1.0, float("nan")), "eps > 0"), ("min_eig", (-0.5, float("nan")), "min_eig >= 0"),
                            ("max_err", (-1.0, float("nan")), "max_err >= 0"),
                            ("max_move", (0.0, -2.0, float("nan")), "max_move > 0")):
        for v in bad:
            assert flow(**{name: v}) == -1 and word in err(), (name, v)
    assert flow(k=0) == -2 and flow(k=65536) == -2 and "1 <= k <= 65535" in err()
    assert flow(c=0) == -2 and flow(c=1025) == -2 and "1 <= c <= 1024" in err()
    assert flow(levels=0) == -2 and flow(levels=7) == -2 and "1 <= levels <= 6" in err()
    assert flow(radius=0) == -2 and flow(radius=8) == -2 and "1 <= radius <= 7" in err()
    assert flow(max_iter=0) == -2 and flow(max_iter=65) == -2 and "1 <= max_iter <= 64" in err()
    assert flow(h=62) == -2 and "multiples" in err()
    assert flow(w=4, levels=3) == -2
    assert flow(opts=False, h=60) == -2 and "= 8" in err()               # NULL opts: the defaults, four levels
    near = lambda a, off: C.c_void_p(a + off)
    assert flow(lo=near(0x30000000, 16)) == -1 and "lm_out_dev overlaps lm_prev_dev" in err()
    assert flow(fo=near(0x50000000, 8)) == -1 and "lm_out_dev overlaps flags_out_dev" in err()
    assert flow(wp=C.c_void_p(0x70000000), wo=near(0x70000000, 8)) == -1 and "w_out_dev overlaps w_prev_dev" in err()
    assert flow(eo=near(0x10000000, 64)) == -1 and "err_out_dev overlaps pyr_prev_dev" in err()


def test_flow_source_compiles_without_scratch(tmp_path):
    """The method of tests/test_mesh_host.py for csrc/flm_flow.hip: built by build.py, compiles for gfx950 with the build's
    flags, and the pyramid kernel has no private segment.  The one landmark-flow kernel, which flm_landmark_flow runs
    too, is landmark_flow_rows_kernel of csrc/flm_flow_rows.hip (tests/test_flow_rows_host.py holds it to the same
    bars); no second one is left here."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("_flm_build", os.path.join(ROOT, "face-landmark-detector_amd", "build.py"))
    bld = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bld)
    assert "flm_flow.hip" in bld.SOURCES
    assert "-ffp-contract=off" in bld.FLAGS
    out = str(tmp_path / "flm_flow.s")
    cmd = [bld._hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off",
           *bld.FILE_FLAGS.get("flm_flow.hip", []), "-I", os.path.join(ROOT, "include"), "-I", CSRC, "-S",
           "--cuda-device-only", os.path.join(CSRC, "flm_flow.hip"), "-o", out]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    text = open(out).read()
    kernels = {}
    for m in re.finditer(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)", text):
        kernels[m.group(1)] = (int(m.group(2)), int(m.group(3)))
    print(kernels)
    assert any("flow_pyramid_kernel" in k for k in kernels)
    assert not any("landmark_flow" in k for k in kernels), kernels
    bad = {k: v for k, v in kernels.items() if v[0] != 0}
    assert not bad, "kernels with a private segment (scratch): %s" % bad
    assert all(v[1] <= 128 for v in kernels.values()), kernels          # four waves per SIMD


# ---- Python ---------------------------------------------------------------------------------------------------------
class _Model:
    n_classes, input_height, input_width, output_height, output_width = 68, 64, 64, 72, 72
    max_batch = 1024


def test_landmark_flow_options_reject_bad_values():
    for bad in (dict(levels=0), dict(levels=7), dict(levels=2.5), dict(levels=True), dict(radius=0), dict(radius=8),
                dict(max_iter=0), dict(max_iter=65), dict(eps=0.0), dict(eps=float("nan")), dict(min_eig=-1.0),
                dict(max_err=-1.0), dict(max_err=float("nan")), dict(max_move=0.0)):
        with pytest.raises(ValueError):
            alignment.LandmarkFlow(**bad)
    f = alignment.LandmarkFlow(levels=3, radius=3)
    f.check_crop(64, 64)
    for hw in ((62, 64), (64, 4), (4, 64)):
        with pytest.raises(ValueError, match="no pyramid of 3 levels"):
            f.check_crop(*hw)
    assert "levels=3" in repr(f)


def test_python_wrappers_reject_bad_arguments_on_the_host():
    flow = alignment.LandmarkFlow(levels=3)
    with pytest.raises(ValueError, match="crops must be"):
        alignment.flow_pyramid_device(torch.zeros((2, 64, 64, 3), dtype=torch.float32), 3)
    with pytest.raises(ValueError, match="crops must be"):
        alignment.flow_pyramid_device(torch.zeros((2, 64, 64, 2), dtype=torch.uint8), 3)
    with pytest.raises(ValueError, match="crops must be"):
        alignment.flow_pyramid_device(torch.zeros((2, 64, 64, 3), dtype=torch.uint8), 3)      # (not on the device)
    with pytest.raises(ValueError, match="levels must be"):
        alignment.flow_pyramid_device(torch.zeros((2, 64, 64, 3), dtype=torch.uint8), 0)
    with pytest.raises(ValueError, match="no pyramid"):
        alignment.flow_pyramid_device(torch.zeros((2, 62, 64, 3), dtype=torch.uint8), 3)
    nb = flow.pyramid_bytes(64, 64)
    pyr = torch.zeros((2, nb), dtype=torch.uint8)
    lm = torch.zeros((2, 68, 2), dtype=torch.float64)
    m = torch.zeros((2, 2, 3), dtype=torch.float32)
    with pytest.raises(ValueError, match="flow must be"):
        alignment.landmark_flow_device(pyr, pyr, lm, m, (64, 64), None)
    with pytest.raises(ValueError, match="lm_prev must be"):
        alignment.landmark_flow_device(pyr, pyr, lm[..., :1], m, (64, 64), flow)
    with pytest.raises(ValueError, match="lm_prev must be"):
        alignment.landmark_flow_device(pyr, pyr, lm.float(), m, (64, 64), flow)
    with pytest.raises(ValueError, match="no pyramid"):
        alignment.landmark_flow_device(pyr, pyr, lm, m, (64, 62), flow)
    for bad in (dict(flow=True), dict(flow=3)):
        with pytest.raises(ValueError):
            prediction.landmark_flow(np.zeros((1, 64, 64), np.uint8), np.zeros((1, 64, 64), np.uint8),
                                     np.zeros((1, 5, 2)), **bad)
    with pytest.raises(ValueError, match="one shape"):
        prediction.landmark_flow(np.zeros((1, 64, 64), np.uint8), np.zeros((1, 64, 32), np.uint8), np.zeros((1, 5, 2)))
    with pytest.raises(ValueError, match="points must be"):
        prediction.landmark_flow(np.zeros((1, 64, 64), np.uint8), np.zeros((1, 64, 64), np.uint8), np.zeros((2, 5, 2)))
    with pytest.raises(ValueError, match="no pyramid"):
        prediction.landmark_flow(np.zeros((1, 60, 64), np.uint8), np.zeros((1, 60, 64), np.uint8), np.zeros((1, 5, 2)))


class _HostRing(alignment.FrameFormat):      # lets the host checks of a step run without a ring on the device
    def ring(self, frames):
        return 2, 96, 128, 96 * 128 * 3


def test_face_tracker_rejects_flow_it_cannot_serve():
    mk = lambda hw=(96, 128), **kw: prediction.FaceTracker(_Model(), hw, 4, frame_format=_HostRing.bgr(), **kw)
    for bad in (3, "yes", alignment.LandmarkFilter()):
        with pytest.raises(ValueError, match="flow must be"):
            mk(flow=bad)
    with pytest.raises(ValueError, match="no pyramid of 6 levels"):          # 64 >> 5 == 2 is fine; 7 levels do not exist
        prediction.FaceTracker(type("M", (_Model,), dict(input_height=48))(), (96, 128), 4, flow=alignment.LandmarkFlow(levels=6))
    assert mk().flow is None and mk(flow=False).flow is None and isinstance(mk(flow=True).flow, alignment.LandmarkFlow)
    ring = torch.zeros((2, 96, 128, 3), dtype=torch.uint8)
    with pytest.raises(ValueError, match="step_flow needs a tracker made with flow"):
        mk().step_flow(ring, 0)
    tr = mk(flow=True, streams=2)
    with pytest.raises(ValueError, match="may follow only step or step_flow"):   # a new tracker has no history
        tr.step_flow(ring, [0, 1])

    def poke(call):     # without a GPU the call stops at the device state, after it has cleared the flag
        try:
            call()
        except _lib.FlmError:
            pass

    for call in (lambda: tr.seed([0], [[10, 10, 50, 50]]), lambda: tr.update([[[10, 10, 50, 50]], None]),
                 lambda: tr.step_active(ring, [0, 1], [0]), lambda: tr.step_live(ring, [0, 1], 2)):
        tr._flow_ok = True
        poke(call)
        assert tr._flow_ok is False
        with pytest.raises(ValueError, match="may follow only step or step_flow"):
            tr.step_flow(ring, [0, 1])
    tr._flow_ok = True     # as after a step: the ring and the indices are judged before anything is launched
    other = mk(hw=(96, 64), flow=True)
    other._flow_ok = True
    with pytest.raises(ValueError, match="the ring holds 96x128 frames, the tracker was made for 96x64"):
        other.step_flow(ring, 0)
    with pytest.raises(ValueError, match="frame_index must name ring slots"):
        tr.step_flow(ring, [0, 2])
    with pytest.raises(ValueError, match="dt goes with smooth"):
        tr.step_flow(ring, [0, 1], dt=0.1)
    one = mk(flow=True)
    one._flow_ok = True
    with pytest.raises(ValueError, match="frame_index must name a ring slot"):
        one.step_flow(ring, 2)
    import inspect
    assert list(inspect.signature(prediction.FaceTracker.step_flow).parameters) == ["self", "ring", "frame_index", "dt", "frame_id"]


# ---- the reference alone --------------------------------------------------------------------------------------------
O3 = flow_ref.options(levels=3)
IDENT = np.array([[1, 0, 0], [0, 1, 0]], np.float32)


def _points(seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(10.0, 53.0, (68, 2))


def _run(a, b, pts, o=O3):
    pa, pb = flow_ref.pyramid(a, o["levels"]), flow_ref.pyramid(b, o["levels"])
    out = [flow_ref.flow_point(pa, pb, IDENT, x, y, o) for x, y in pts]
    return np.array([(q[0], q[1]) for q in out]), np.array([q[2] for q in out]), np.array([q[3] for q in out])


@pytest.fixture(scope="module")
def tex():
    return flow_ref.texture(64, 64, 11)


def test_reference_returns_the_points_of_an_unmoved_image(tex):
    a = flow_ref.shifted(tex, 0.0, 0.0)
    pts = _points(1)
    q, err, flags = _run(a, a, pts)
    assert (flags == 0).all() and (err == 0).all()
    assert (q.view(np.uint64) == ((pts + 0.5) - 0.5).view(np.uint64)).all()       # p_0 = (p0 + 0.5)/1 - 0.5, exactly
    assert np.abs(q - pts).max() < 1e-13


@pytest.mark.parametrize("shift", [(1.25, -0.75), (3.3, -2.6)])
def test_reference_recovers_a_translation(tex, shift):
    a, b = flow_ref.shifted(tex, 0.0, 0.0), flow_ref.shifted(tex, *shift)
    pts = _points(2)
    q, err, flags = _run(a, b, pts)
    d = np.abs(q - (pts + np.asarray(shift))).max()
    print("shift", shift, "worst", d, "rejected", int((flags != 0).sum()))
    assert (flags == 0).all()
    assert d <= 0.1


def test_reference_flags(tex):
    a, b = flow_ref.shifted(tex, 0.0, 0.0), flow_ref.shifted(tex, 3.3, -2.6)
    pts = _points(3)
    flat = np.full((64, 64), 90, np.uint8)
    _, _, flags = _run(flat, flat, pts)
    assert (flags & flow_ref.LOW_TEXTURE).all()
    q, err, flags = _run(a, b, np.array([[-1.0, -1.0], [np.nan, 4.0], [5.0, np.inf]]))
    assert (flags == flow_ref.NO_HISTORY).all() and (err == -1).all() and (q == -1.0).all()
    _, _, flags = _run(a, b, pts, flow_ref.options(levels=3, max_move=1.0))
    assert (flags == flow_ref.MOVED).all()
    _, _, flags = _run(a, b, np.array([[62.0, 32.0], [30.0, 1.0]]))         # the match lies at x = 65.3, at y = -1.6
    assert (flags & flow_ref.OUTSIDE).all()
    big = IDENT.copy()
    big[0, 2] = 3.0e6
    pa = flow_ref.pyramid(a, 3)
    assert flow_ref.flow_point(pa, pa, big, 5.0, 5.0, O3)[3] == flow_ref.NOT_FINITE
