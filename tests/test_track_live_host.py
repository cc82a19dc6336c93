"""CPU-side checks of stepping only the live slots (flm_track_gather_live, alignment.track_gather_live_device,
FaceTracker.step_live): the symbol, every argument check answered before any launch (so without a GPU), the Python
rejections, the compiler's metadata of the new kernel, and -- on tests/track_live_ref.py alone -- the properties the row
map is there for: every live slot served once and in order, fairness over consecutive calls, ages that add up to the time
waited, a stream that is off left alone."""
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

import track_live_ref as lref

NAN, INF = float("nan"), float("inf")
FH, FW = 270, 480
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "face-landmark-detector_amd", "csrc")


def test_library_exports_the_call():
    lib = C.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "flm_track_gather_live") and "flm_track_gather_live" in _lib.EXPORTS
    L = _lib.load()
    assert L.flm_abi_version() == 2                                   # purely additive
    assert len(L.flm_track_gather_live.argtypes) == 24
    assert len(L.flm_track_gather_streams.argtypes) == 18


P = C.c_void_p(0x1000)        # never dereferenced: every call below is rejected before a launch
err = lambda: _lib.load().flm_last_error().decode()
ORDER = ("on", "s", "k", "fh", "fw", "n", "fi", "dts", "dt", "m", "boxes", "bq", "reset", "age", "cursor", "slot_c", "m_c",
         "boxes_c", "fi_c", "dt_c", "bq_c", "reset_c", "counts")


def _live(**kw):
    a = dict(on=P, s=3, k=4, fh=FH, fw=FW, n=5, fi=P, dts=P, dt=0.0, m=P, boxes=P, bq=P, reset=P, age=P, cursor=P, slot_c=P,
             m_c=P, boxes_c=P, fi_c=P, dt_c=P, bq_c=P, reset_c=P, counts=P)
    a.update(kw)
    return _lib.load().flm_track_gather_live(None, *[a[n] for n in ORDER])


def test_gather_live_argument_checks_answer_without_a_gpu():
    who = "flm_track_gather_live"
    for name in ("m", "boxes", "slot_c", "m_c", "boxes_c", "fi_c", "counts"):
        assert _live(**{name: None}) == -1 and "null" in err() and who in err(), name
    for name in ("age", "dt_c", "bq", "bq_c", "reset", "reset_c"):     # an output without its input, or the reverse
        assert _live(**{name: None}, dts=None, dt=0.1) == -1 and "go together" in err() and who in err(), name
    assert _live(age=None, dt_c=None) == -1 and "dt_stream_dev goes with age_dev" in err()
    for dt in (0.0, -1.0, NAN, INF, -INF):                             # the scalar dt counts only without dt_stream_dev
        assert _live(dts=None, dt=dt) == -1 and "dt=" in err() and who in err(), dt
        assert _live(dt=dt, n=0) == -2 and "1 <= n" in err(), dt
        assert _live(dts=None, age=None, dt_c=None, dt=dt, n=0) == -2, dt      # ... and only with age_dev
    for n in (0, -1, 65536, 2 ** 31 - 1):
        assert _live(n=n) == -2 and "1 <= n <= 65535" in err() and who in err(), n
    for kw in (dict(s=0), dict(s=-1), dict(k=0), dict(k=-3)):
        assert _live(**kw) == -2 and "1 <= s, 1 <= k" in err(), kw
    for kw in (dict(s=16384, k=4), dict(s=65536, k=1), dict(s=1, k=65536), dict(s=2 ** 31 - 1, k=2 ** 31 - 1)):
        assert _live(**kw) == -2 and "s*k <= 65535" in err(), kw
    for kw in (dict(fh=0), dict(fw=0), dict(fh=-1), dict(fw=-7)):
        assert _live(**kw) == -2 and "fh, fw >= 1" in err(), kw
    # what is allowed reaches the last check (fh): the limits, and every optional pointer absent
    for kw in (dict(n=65535, s=65535, k=1), dict(n=1, s=1, k=65535), dict(on=None), dict(fi=None), dict(cursor=None),
               dict(dts=None, dt=0.04), dict(bq=None, bq_c=None), dict(reset=None, reset_c=None),
               dict(dts=None, age=None, dt_c=None, dt=NAN),
               dict(on=None, fi=None, dts=None, bq=None, reset=None, age=None, cursor=None, dt_c=None, bq_c=None, reset_c=None)):
        assert _live(fh=0, **kw) == -2 and "fh, fw >= 1" in err() and who in err(), kw


# ---- the Python rejections ---------------------------------------------------------------------------------------------
class _Model:
    n_classes, input_height, input_width, output_height, output_width = 68, 64, 64, 72, 72
    max_batch = 1024


class _HostRing(alignment.FrameFormat):
    """A frame format whose ring needs no device: 8 slots of the tracker's frames."""

    def ring(self, frames):
        return 8, FH, FW, FH * FW * 3


def test_step_live_rejects_what_it_must_on_the_host():
    mk = lambda **kw: prediction.FaceTracker(_Model(), (FH, FW), 6, streams=3, frame_format=_HostRing.bgr(), **kw)
    tr = mk(smooth=True, best_shot=True)
    fi = [0, 1, 2]
    for bad in (0, -1, 7, 2.5, True, 2 ** 40):                         # a budget outside [1, capacity]
        with pytest.raises(ValueError, match="budget"):
            tr.step_live(None, fi, bad)
    with pytest.raises(ValueError, match="dt goes with smooth"):
        mk().step_live(None, fi, 6, dt=1 / 30)
    with pytest.raises(ValueError, match="frame_id goes with best_shot"):
        mk(smooth=True).step_live(None, fi, 6, frame_id=3)
    for bad in ([0, 0], [1, 2, 1], [3], [-1], [0, 3], [0.5], [True], 1):       # duplicate, out of range, not a list
        with pytest.raises(ValueError, match="active"):
            tr.step_live(None, fi, 6, active=bad)
    for bad in (torch.zeros(3, dtype=torch.int32), torch.zeros(3, dtype=torch.int64)):   # (not on the device)
        with pytest.raises(ValueError, match="active"):
            tr.step_live(None, fi, 6, active=bad)
    for bad in (3, [1], [0, 1], [0, 1, 2, 3]):
        with pytest.raises(ValueError, match="sequence of 3"):
            tr.step_live(None, bad, 6)
    for bad, act in (([0, 8, 0], [1]), ([None, 0, 0], [0]), ([0, 0, -1], [2, 0]), ([0.5, 0, 0], [0]), ([True, 0, 0], [0]),
                     ([0, None, 0], None), ([0, 0, 8], None)):         # without `active` every entry counts
        with pytest.raises(ValueError, match=r"\[0, 8\)"):
            tr.step_live(None, bad, 6, active=act)
    with pytest.raises(ValueError, match="CUDA int32"):
        tr.step_live(None, torch.zeros(3, dtype=torch.int32), 6)
    for bad in ([1 / 30], [1 / 30] * 4, "ab", torch.ones(3, dtype=torch.float64)):
        with pytest.raises(ValueError, match="sequence of 3 numbers"):
            tr.step_live(None, fi, 6, dt=bad)
    for bad, act in (([0.0, 1, 1], [0]), ([1, -1.0, 1], [1]), ([1, 1, NAN], [2]), ([INF, 1, 1], [1, 0]), ([None, 1, 1], [0]),
                     ([1, 1, 0.0], None), ([1, None, 1], None)):
        with pytest.raises(ValueError, match="dt of stream"):
            tr.step_live(None, fi, 6, active=act, dt=bad)
    for bad in (0.0, -0.1, NAN, INF):
        with pytest.raises(ValueError, match="dt must be finite"):
            tr.step_live(None, fi, 6, dt=bad)
    for bad in (1.5, True, 2 ** 63):
        with pytest.raises(ValueError, match="frame_id"):
            tr.step_live(None, fi, 6, frame_id=bad)

    class _OtherRing(alignment.FrameFormat):
        def ring(self, frames):
            return 8, FH + 2, FW, 0

    with pytest.raises(ValueError, match="the ring holds"):
        prediction.FaceTracker(_Model(), (FH, FW), 6, streams=3, frame_format=_OtherRing.bgr()).step_live(None, fi, 6)


def test_wrapper_rejects_what_it_must_on_the_host():
    m, boxes = torch.zeros((6, 2, 3)), torch.zeros((6, 4), dtype=torch.int32)
    with pytest.raises(ValueError, match="m_crop"):                    # (not on the device)
        alignment.track_gather_live_device(m, boxes, 3, (FH, FW), 4)
    with pytest.raises(ValueError, match="m_crop"):
        alignment.track_gather_live_device([0, 1], boxes, 3, (FH, FW), 4)


# ---- the compiler's metadata of the kernel this feature adds ------------------------------------------------------------
def _metadata(src, tmp):
    """name -> dict of the integer fields of the kernel's metadata, as tests/test_track_active_host.py reads them."""
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


def test_the_new_kernel_compiles_for_gfx950_without_scratch(tmp_path):
    md = _metadata("flm_track.hip", str(tmp_path))
    names = [n for n in md if "track_gather_live_kernel" in n]
    assert len(names) == 1, sorted(md)
    k = md[names[0]]
    print({f: k[f] for f in ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")})
    assert k["private_segment_fixed_size"] == 0, k
    assert k["max_flat_workgroup_size"] == 1024 and k["wavefront_size"] == 64, k
    assert k["group_segment_fixed_size"] <= 128, k                     # sixteen wave totals and one slot
    # one workgroup of 1024 threads must be resident: at most 128 vector registers a thread
    assert k["vgpr_count"] <= 128, k


# ---- the reference alone -----------------------------------------------------------------------------------------------
def _state(s, k, live, seed=0):
    """s*k slots of which `live` hold a box with pixels; the others are empty in every way a box can be."""
    rng = np.random.default_rng(seed)
    n = s * k
    boxes = np.zeros((n, 4), np.int32)
    empties = [(0, 0, 0, 0), (-40, 10, 0, 60), (FW, 10, FW + 30, 60), (10, FH, 60, FH + 9), (50, 50, 50, 90), (90, 40, 60, 80)]
    for g in range(n):
        boxes[g] = (20 + g % 7, 10, 80 + g % 5, 70) if g in live else empties[g % len(empties)]
    m = rng.normal(0, 1, (n, 2, 3)).astype(np.float32)
    return m, boxes


def test_with_room_every_live_slot_is_served_once_in_order_from_the_cursor():
    s, k = 5, 4
    live = {1, 2, 7, 8, 13, 19}
    m, boxes = _state(s, k, live)
    for cursor in (None, 0, 2, 8, 14, 19, 20, -3):
        c0 = cursor if cursor is not None and 0 <= cursor < s * k else 0
        for n in (6, 7, 20):
            r = lref.gather_live(m, boxes, s, k, FH, FW, n, cursor=cursor)
            got = r["slot"][:6].tolist()
            assert sorted(got) == sorted(live) and (r["slot"][6:] == -1).all()
            assert got == sorted(live, key=lambda g: (g - c0) % (s * k))                 # ascending from the cursor
            assert r["counts"].tolist() == [6, 6, 0, c0]                                 # E <= N: the cursor stays
            for row, g in enumerate(got):
                assert np.array_equal(r["m"][row], m[g]) and np.array_equal(r["boxes"][row], boxes[g])
            assert (r["boxes"][6:] == 0).all() and (r["m"][6:] == np.float32([[1, 0, 0], [0, 1, 0]])).all()


def test_over_the_budget_every_live_slot_is_served_within_ceil_e_over_n_calls():
    s, k = 4, 8
    rng = np.random.default_rng(4)
    for e, n, cursor in ((5, 2, 0), (9, 4, 30), (32, 5, 17), (7, 6, 31), (3, 1, 9)):
        live = set(rng.permutation(s * k)[:e].tolist())
        m, boxes = _state(s, k, live)
        calls = math.ceil(e / n)
        for start in range(3):                                         # from any call on, not only the first
            seen, cur = [], cursor
            for t in range(start + calls):
                r = lref.gather_live(m, boxes, s, k, FH, FW, n, cursor=cur)
                assert r["counts"].tolist()[:3] == [e, n, e - n]
                rows = r["slot"].tolist()
                assert len(set(rows)) == n and set(rows) <= live
                cur = r["cursor_global"]
                assert cur == (rows[-1] + 1) % (s * k) == r["counts"][3]
                if t >= start:
                    seen += rows
            assert set(seen) == live, (e, n, start)
        # without a cursor the order starts at slot 0 every time: the same rows again
        a, b = [lref.gather_live(m, boxes, s, k, FH, FW, n) for _ in range(2)]
        assert a["slot"].tolist() == b["slot"].tolist() == sorted(live)[:n] and a["cursor_global"] is None


def test_the_ages_add_up_to_the_time_each_slot_waited():
    s, k, n = 3, 4, 2
    live = {0, 3, 5, 6, 10}
    m, boxes = _state(s, k, live)
    age = np.zeros(s * k)
    age[[1, 2]] = 7.0                                                  # a dead slot's stale age is cleared, not served
    cur, clock, last = 0, 0.0, {g: 0.0 for g in live}
    served_all = []
    for t in range(9):
        dts = np.array([0.03, 0.05, 0.04]) * (1 + t % 3)               # every stream on its own clock
        # (all streams tick together here, so the time a slot waited is the sum of ITS stream's steps since it was served)
        r = lref.gather_live(m, boxes, s, k, FH, FW, n, dt_stream=dts, age=age, cursor=cur)
        waited = {g: last[g] + dts[g // k] for g in live}
        for row, g in enumerate(r["slot"].tolist()):
            assert g in live and abs(r["dt"][row] - waited[g]) < 1e-12, (t, g)
            assert r["age_global"][g] == 0.0
            last[g] = 0.0
            served_all.append(g)
        for g in live - set(r["slot"].tolist()):
            assert abs(r["age_global"][g] - waited[g]) < 1e-12
            last[g] = waited[g]
        assert not r["age_global"][sorted(set(range(s * k)) - live)].any()
        age, cur = r["age_global"], r["cursor_global"]
    assert set(served_all) == live
    # a time step that is not > 0 and finite: a served slot gets it as it is, a waiting slot's age is NaN from then on, and
    # the NaN reaches dt when the slot is served -- which restarts the filter (flm_track_step_rows, rule 2)
    for bad in (0.0, -0.1, NAN, INF):
        r = lref.gather_live(m, boxes, s, k, FH, FW, n, dt_stream=np.array([bad, 0.04, 0.04]), age=np.full(s * k, 0.5), cursor=0)
        assert r["slot"].tolist() == [0, 3] and all(np.array_equal(v, np.float64(bad), equal_nan=True) for v in r["dt"])
        assert r["age_global"][[5, 6, 10]].tolist() == [0.5 + 0.04] * 3
        r = lref.gather_live(m, boxes, s, k, FH, FW, n, dt_stream=np.array([0.04, bad, 0.04]), age=np.full(s * k, 0.5), cursor=0)
        assert r["dt"].tolist() == [0.04 + 0.5] * 2 and np.isnan(r["age_global"][[5, 6]]).all() and r["age_global"][10] == 0.5 + 0.04
        r2 = lref.gather_live(m, boxes, s, k, FH, FW, n, dt=0.04, age=r["age_global"], cursor=r["cursor_global"])
        assert r2["slot"].tolist() == [5, 6] and np.isnan(r2["dt"]).all() and not r2["age_global"][[5, 6]].any()


def test_a_stream_that_is_off_is_untouched():
    s, k, n = 4, 3, 4
    live = {0, 2, 3, 4, 7, 9, 11}
    m, boxes = _state(s, k, live)
    rng = np.random.default_rng(1)
    age, reset, bq = rng.uniform(0, 1, s * k), rng.integers(1, 5, s * k).astype(np.int32), rng.uniform(0, 1, s * k)
    on = np.array([1, 0, -5, 0], np.int32)                             # any non-zero value is on
    r = lref.gather_live(m, boxes, s, k, FH, FW, n, stream_on=on, frame_idx_stream=[4, 5, 6, 7], dt=0.1, best_q=bq, reset=reset,
                         age=age, cursor=5)
    assert r["slot"].tolist() == [7, 0, 2, -1] and r["frame_index"].tolist() == [6, 4, 4, 0]
    assert r["counts"].tolist() == [3, 3, 0, 5]
    off = [3, 4, 5, 9, 10, 11]
    assert np.array_equal(r["age_global"][off], age[off]) and np.array_equal(r["reset_global"][off], reset[off])
    assert r["reset"].tolist() == reset[[7, 0, 2]].tolist() + [0] and not r["reset_global"][[7, 0, 2]].any()
    assert np.array_equal(r["reset_global"][[1, 6, 8]], reset[[1, 6, 8]])              # dead slots of streams that are on
    assert r["best_q"].tolist() == bq[[7, 0, 2]].tolist() + [-1.0]
    # a box full of junk in a stream that is off is not even looked at: it cannot become a row
    boxes2 = boxes.copy()
    boxes2[10] = (5, 5, 50, 50)
    r2 = lref.gather_live(m, boxes2, s, k, FH, FW, n, stream_on=on, cursor=5)
    assert r2["slot"].tolist() == r["slot"].tolist()
    # every stream off: nothing is served, nothing changes
    r3 = lref.gather_live(m, boxes, s, k, FH, FW, n, stream_on=np.zeros(s, np.int32), dt=0.1, reset=reset, age=age, cursor=5)
    assert (r3["slot"] == -1).all() and r3["counts"].tolist() == [0, 0, 0, 5]
    assert np.array_equal(r3["age_global"], age) and np.array_equal(r3["reset_global"], reset)
