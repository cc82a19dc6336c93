"""CPU-side checks of the flow tick on rows (flm_track_gather_flow, flm_landmark_flow_rows, flm_track_flow_history_put,
alignment.LandmarkFlow(max_fb=...), FaceTracker.step_flow_live): the exports, every argument check of the three calls
answered before any launch (so without a GPU), the Python rejections, and the new source compiled for gfx950 without a
private segment."""
import ctypes as C
import os
import re
import subprocess

import pytest
import torch

import flm_amd  # noqa: F401
from flm_amd import _lib, alignment, prediction

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "face-landmark-detector_amd", "csrc")
NEW = ("flm_track_gather_flow", "flm_landmark_flow_rows", "flm_track_flow_history_put")
P = lambda a: C.c_void_p(a)


def test_library_exports_the_rows_entry_points():
    lib = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTS
    assert _lib.load().flm_abi_version() == _lib.ABI_VERSION == 2      # purely additive
    assert C.sizeof(_lib.FlowOpts) == 56                                # max_fb is an argument, not a field
    assert alignment.FLOW_FB == _lib.FLOW_FB == 64
    text = open(os.path.join(ROOT, "include", "flm.h")).read()
    assert "#define FLM_FLOW_FB 64" in text and all(("int %s(" % n) in text for n in NEW)
    assert "flow_ready[g] == 1 exactly when" in text                   # the history rule is stated in the header


def test_gather_flow_argument_checks_answer_without_a_gpu():
    lib = _lib.load()
    err = lambda: lib.flm_last_error().decode()
    base = dict(on=None, s=2, k=4, fh=1080, fw=1920, n=3, fi=None, dts=None, dt=0.0, m=P(0x10000000), boxes=P(0x11000000),
                bq=None, reset=None, age=None, cursor=None, frame=P(0x12000000), ready=P(0x13000000), slot=P(0x20000000),
                mc=P(0x21000000), bc=P(0x22000000), fic=P(0x23000000), pfc=P(0x24000000), dtc=None, bqc=None, rc=None,
                counts=P(0x25000000))
    order = list(base)

    def call(**kw):
        a = dict(base)
        a.update(kw)
        return lib.flm_track_gather_flow(None, *[a[k] for k in order])

    for name in ("m", "boxes", "frame", "ready", "slot", "mc", "bc", "fic", "pfc", "counts"):
        assert call(**{name: None}) == -1 and "null" in err(), name
    assert call(age=P(0x30000000)) == -1 and "go together" in err()
    assert call(bqc=P(0x30000000)) == -1 and call(reset=P(0x30000000)) == -1 and "go together" in err()
    assert call(dts=P(0x30000000)) == -1 and "goes with age_dev" in err()
    for dt in (0.0, -1.0, float("nan"), float("inf")):
        assert call(age=P(0x30000000), dtc=P(0x31000000), dt=dt) == -1 and "finite dt > 0" in err(), dt
    assert call(n=0) == -2 and call(n=65536) == -2 and "1 <= n <= 65535" in err()
    assert call(s=0) == -2 and call(k=0) == -2 and call(s=256, k=256) == -2 and "s*k <= 65535" in err()
    assert call(fh=0) == -2 and call(fw=0) == -2 and "fh, fw >= 1" in err()
    assert call(pfc=P(0x23000000 + 4)) == -1 and "frame_idx_c overlaps prev_frame_idx_c" in err()
    assert call(ready=P(0x12000000 + 8)) == -1 and "flow_ready_dev overlaps flow_frame_dev" in err()
    assert call(counts=P(0x11000000 + 16)) == -1 and "counts_dev overlaps boxes_dev" in err()


def test_flow_rows_argument_checks_answer_without_a_gpu():
    lib = _lib.load()
    err = lambda: lib.flm_last_error().decode()

    def flow(pp=P(0x10000000), pc=P(0x20000000), n=2, h=64, w=64, slot=P(0x28000000), n_slots=4, lm=P(0x30000000), wp=None,
             m=P(0x40000000), c=68, opts=True, max_fb=1.0, lo=P(0x50000000), wo=None, eo=None, fb=P(0x58000000),
             fo=P(0x60000000), **kw):
        o = None
        if opts:
            o = _lib.FlowOpts.make(levels=3)
            for name, v in kw.items():
                setattr(o, name, v)
            o = C.byref(o)
        return lib.flm_landmark_flow_rows(None, pp, pc, n, h, w, slot, n_slots, lm, wp, m, c, o, max_fb, lo, wo, eo, fb, fo)

    for name in ("pp", "pc", "slot", "lm", "m", "lo", "fb", "fo"):
        assert flow(**{name: None}) == -1 and "null" in err(), name
    assert flow(struct_size=8) == -1 and "struct_size" in err()
    assert flow(reserved=1) == -1 and flow(pad=1) == -1 and "pad" in err()
    for name, bad, word in (("eps", (0.0, float("nan")), "eps > 0"), ("min_eig", (-0.5, float("nan")), "min_eig >= 0"),
                            ("max_err", (-1.0, float("nan")), "max_err >= 0"), ("max_move", (0.0, float("nan")), "max_move > 0")):
        for v in bad:
            assert flow(**{name: v}) == -1 and word in err(), (name, v)
    for v in (-0.5, float("nan"), float("inf")):
        assert flow(max_fb=v) == -1 and "max_fb" in err(), v
    assert flow(n=0) == -2 and flow(n=65536) == -2 and "1 <= n <= 65535" in err()
    assert flow(n_slots=0) == -2 and flow(n_slots=65536) == -2 and "1 <= n_slots <= 65535" in err()
    assert flow(c=0) == -2 and flow(c=1025) == -2 and "1 <= c <= 1024" in err()
    assert flow(levels=0) == -2 and flow(levels=7) == -2 and "1 <= levels <= 6" in err()
    assert flow(radius=0) == -2 and flow(radius=8) == -2 and "1 <= radius <= 7" in err()
    assert flow(max_iter=0) == -2 and flow(max_iter=65) == -2 and "1 <= max_iter <= 64" in err()
    assert flow(h=62) == -2 and "multiples" in err()
    assert flow(opts=False, h=60) == -2 and "= 8" in err()
    assert flow(lo=P(0x30000000 + 16)) == -1 and "lm_out_dev overlaps lm_prev_dev" in err()
    # the history store has n_slots entries, not n: an output past n rows of it still overlaps
    assert flow(fo=P(0x30000000 + 3 * 68 * 16)) == -1 and "flags_out_dev overlaps lm_prev_dev" in err()
    assert flow(fb=P(0x50000000 + 8)) == -1 and "lm_out_dev overlaps fb_out_dev" in err()
    assert flow(wp=P(0x70000000), wo=P(0x70000000 + 8)) == -1 and "w_out_dev overlaps w_prev_dev" in err()
    assert flow(eo=P(0x28000000 + 4)) == -1 and "err_out_dev overlaps slot_dev" in err()


def test_history_put_argument_checks_answer_without_a_gpu():
    lib = _lib.load()
    err = lambda: lib.flm_last_error().decode()

    def put(slot=P(0x10000000), st=P(0x11000000), fi=P(0x12000000), lm=P(0x20000000), wr=P(0x21000000), n=3, n_slots=8, c=68,
            hl=P(0x30000000), hw=P(0x31000000), frame=P(0x40000000), ready=P(0x41000000)):
        return lib.flm_track_flow_history_put(None, slot, st, fi, lm, wr, n, n_slots, c, hl, hw, frame, ready)

    for name in ("slot", "st", "fi", "frame", "ready"):
        assert put(**{name: None}) == -1 and "null" in err(), name
    assert put(lm=None) == -1 and put(hl=None) == -1 and put(wr=None) == -1 and put(hw=None) == -1 and "go together" in err()
    assert put(lm=None, hl=None) == -1 and "w_rows_dev goes with lm_rows_dev" in err()
    assert put(n=0) == -2 and put(n=65536) == -2 and "1 <= n <= 65535" in err()
    assert put(n_slots=0) == -2 and put(n_slots=65536) == -2 and "1 <= n_slots <= 65535" in err()
    assert put(c=0) == -2 and put(c=1025) == -2 and "1 <= c <= 1024" in err()
    assert put(hl=P(0x20000000 + 64)) == -1 and "hist_lm_dev overlaps lm_rows_dev" in err()
    assert put(ready=P(0x40000000 + 4)) == -1 and "flow_frame_dev overlaps flow_ready_dev" in err()
    assert put(frame=P(0x10000000 + 8)) == -1 and "flow_frame_dev overlaps slot_dev" in err()


def test_rows_source_compiles_without_scratch(tmp_path):
    """The method of tests/test_flow_host.py for csrc/flm_flow_rows.hip: built by build.py without contraction, compiles
    for gfx950 with the build's flags, and none of the kernels has a private segment; the fused two-pass flow kernel,
    the one landmark-flow kernel body (instantiated for flm_landmark_flow_rows and for flm_landmark_flow), stays within
    128 VGPRs, four waves per SIMD, in both instantiations."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("_flm_build", os.path.join(ROOT, "face-landmark-detector_amd", "build.py"))
    bld = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bld)
    assert "flm_flow_rows.hip" in bld.SOURCES and "-ffp-contract=off" in bld.FLAGS
    out = str(tmp_path / "flm_flow_rows.s")
    cmd = [bld._hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off",
           *bld.FILE_FLAGS.get("flm_flow_rows.hip", []), "-I", os.path.join(ROOT, "include"), "-I", CSRC, "-S",
           "--cuda-device-only", os.path.join(CSRC, "flm_flow_rows.hip"), "-o", out]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    text = open(out).read()
    kernels = {}
    for m in re.finditer(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)", text):
        kernels[m.group(1)] = (int(m.group(2)), int(m.group(3)))
    print(kernels)
    for name in ("track_gather_flow_kernel", "landmark_flow_rows_kernel", "flow_history_put_kernel"):
        assert any(name in k for k in kernels), name
    flow_kernels = [k for k in kernels if "landmark_flow" in k]      # one body: its rows and its all-slots instantiation
    assert len(flow_kernels) == 2 and all("landmark_flow_rows_kernelI" in k for k in flow_kernels), kernels
    src = open(os.path.join(CSRC, "flm_flow_rows.hip")).read()
    assert len(re.findall(r"__global__[^;{]*landmark_flow", src)) == 1
    bad = {k: v for k, v in kernels.items() if v[0] != 0}
    assert not bad, "kernels with a private segment (scratch): %s" % bad
    assert all(v[1] <= 128 for v in kernels.values()), kernels


# ---- Python ---------------------------------------------------------------------------------------------------------
class _Model:
    n_classes, input_height, input_width, output_height, output_width = 68, 64, 64, 72, 72
    max_batch = 1024


class _HostRing(alignment.FrameFormat):      # lets the host checks of a step run without a ring on the device
    def ring(self, frames):
        return 2, 96, 128, 96 * 128 * 3


def test_max_fb_is_off_by_default_and_checked():
    f = alignment.LandmarkFlow()
    assert f.max_fb is None and "max_fb" not in repr(f)
    assert (f.levels, f.radius, f.max_iter, f.eps, f.min_eig, f.max_err, f.max_move) == (4, 7, 10, 0.03, 0.5, 12.0, 64.0)
    g = alignment.LandmarkFlow(max_fb=1)
    assert g.max_fb == 1.0 and "max_fb=1.0" in repr(g)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="max_fb"):
            alignment.LandmarkFlow(max_fb=bad)
    assert "not been measured on real faces" in " ".join(alignment.LandmarkFlow.__doc__.split())


def test_python_wrappers_reject_bad_arguments_on_the_host():
    flow = alignment.LandmarkFlow(levels=3)
    nb = flow.pyramid_bytes(64, 64)
    pyr = torch.zeros((2, nb), dtype=torch.uint8)
    lm = torch.zeros((4, 68, 2), dtype=torch.float64)
    m = torch.zeros((2, 2, 3), dtype=torch.float32)
    slot = torch.zeros((2,), dtype=torch.int32)
    with pytest.raises(ValueError, match="flow must be"):
        alignment.landmark_flow_rows_device(pyr, pyr, slot, lm, m, (64, 64), None)
    with pytest.raises(ValueError, match="lm_prev must be"):
        alignment.landmark_flow_rows_device(pyr, pyr, slot, lm[..., :1], m, (64, 64), flow)
    with pytest.raises(ValueError, match="lm_prev must be"):
        alignment.landmark_flow_rows_device(pyr, pyr, slot, lm, m, (64, 64), flow)      # (not on the device)
    with pytest.raises(ValueError, match="no pyramid"):
        alignment.landmark_flow_rows_device(pyr, pyr, slot, lm, m, (64, 62), flow)
    i4 = torch.zeros((4,), dtype=torch.int32)
    with pytest.raises(ValueError, match="slot must be"):
        alignment.track_flow_history_device(None, slot, slot, i4, i4)
    with pytest.raises(ValueError, match="slot must be"):
        alignment.track_flow_history_device(slot.view(1, 2), slot, slot, i4, i4)
    with pytest.raises(ValueError, match="must be a contiguous CUDA int32"):
        alignment.track_gather_flow_device(m, None, None, None, 2, (96, 128), 2)


def test_step_flow_live_needs_flow_and_checks_as_step_live():
    mk = lambda **kw: prediction.FaceTracker(_Model(), (96, 128), 4, frame_format=_HostRing.bgr(), streams=2, **kw)
    ring = torch.zeros((2, 96, 128, 3), dtype=torch.uint8)
    with pytest.raises(ValueError, match="step_flow_live needs a tracker made with flow"):
        mk().step_flow_live(ring, [0, 1], 2)
    tr = mk(flow=alignment.LandmarkFlow(levels=3, max_fb=1.0))
    for bad in (0, 5, 2.5, True):
        with pytest.raises(ValueError, match="budget must be"):
            tr.step_flow_live(ring, [0, 1], bad)
    with pytest.raises(ValueError, match="active must be"):
        tr.step_flow_live(ring, [0, 1], 2, active=[0, 0])
    with pytest.raises(ValueError, match="frame_index must"):
        tr.step_flow_live(ring, [0, 7], 2)
    with pytest.raises(ValueError, match="dt goes with smooth"):
        tr.step_flow_live(ring, [0, 1], 2, dt=0.04)
    with pytest.raises(ValueError, match="the ring holds"):
        prediction.FaceTracker(_Model(), (48, 128), 4, frame_format=_HostRing.bgr(), flow=True).step_flow_live(ring, 0, 2)
