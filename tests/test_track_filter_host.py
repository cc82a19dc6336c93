"""CPU-side checks of the filtered track step (flm_track_step_filtered, alignment.LandmarkFilter,
FaceTracker(smooth=...)): the symbols and the defaults, every argument check answered before any launch (so without a
GPU), the Python wrappers' own checks, and the arithmetic the header states (tests/track_filter_ref.py): its two
identities against tests/track_ref.py, the lag of a steadily moving point and the noise of a resting one."""
import ctypes as C

import numpy as np
import pytest
import torch

import flm_amd  # noqa: F401
from flm_amd import _lib, alignment, prediction

import track_filter_cases as cases
import track_filter_ref
import track_ref

INF, NAN = float("inf"), float("nan")


def test_library_exports_the_filtered_step():
    lib = C.CDLL(_lib.LIB_PATH)
    for name in ("flm_track_filter_init", "flm_track_step_filtered"):
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTS
    assert _lib.load().flm_abi_version() == 2          # purely additive
    o = _lib.TrackFilter.make()
    assert o.struct_size == C.sizeof(_lib.TrackFilter) == 32 and o.reserved == 0
    assert (o.min_cutoff, o.beta, o.d_cutoff) == (1.0, 15.0, 1.0)
    assert C.sizeof(_lib.TrackOpts) == 32              # (the options of the plain step did not grow)
    f = alignment.LandmarkFilter()
    assert (f.min_cutoff, f.beta, f.d_cutoff, f.fps) == (1.0, 15.0, 1.0, 30.0)
    assert (track_filter_ref.DEFAULTS["min_cutoff"], track_filter_ref.DEFAULTS["beta"],
            track_filter_ref.DEFAULTS["d_cutoff"]) == (1.0, 15.0, 1.0)


def _step(lib, p, **kw):
    """flm_track_step_filtered with every argument valid (never launched: each caller breaks one)."""
    a = dict(lm=p, ls=2, w=None, ws=1, m=p, boxes=p, k=4, c=68, sx=64 / 72, sy=64 / 72, in_h=64, in_w=64, fh=270, fw=480,
             tc=p, ta=p, opts=None, lmf=p, ma=p, mn=p, bn=p, st=p, filt=_lib.TrackFilter.make(), dt=1 / 30, state=p, raw=p)
    a.update(kw)
    o, f = a["opts"], a["filt"]
    return lib.flm_track_step_filtered(
        None, a["lm"], a["ls"], a["w"], a["ws"], a["m"], a["boxes"], a["k"], a["c"], a["sx"], a["sy"], a["in_h"], a["in_w"],
        a["fh"], a["fw"], a["tc"], a["ta"], None if o is None else C.byref(o), a["lmf"], a["ma"], a["mn"], a["bn"], a["st"],
        None if f is None else C.byref(f), a["dt"], a["state"], a["raw"])


def test_filter_argument_checks_answer_without_a_gpu():
    lib = _lib.load()
    p = C.c_void_p(0x1000)        # never dereferenced: every call below is rejected before a launch
    err = lambda: lib.flm_last_error().decode()
    assert _step(lib, p, filt=None) == -1 and "filt" in err()
    assert _step(lib, p, state=None) == -1 and "state_dev" in err()
    f = _lib.TrackFilter.make()
    f.struct_size -= 8
    assert _step(lib, p, filt=f) == -1 and "struct_size" in err()
    f = _lib.TrackFilter.make()
    f.reserved = 1
    assert _step(lib, p, filt=f) == -1 and "reserved" in err()
    for field, bad in (("min_cutoff", (0.0, -1.0, NAN, -INF)), ("beta", (-0.5, NAN, INF)),
                       ("d_cutoff", (0.0, -2.0, NAN, INF))):
        for v in bad:
            assert _step(lib, p, filt=_lib.TrackFilter.make(**{field: v})) == -1, (field, v)
            assert field in err() and "flm_track_step_filtered" in err(), (field, v, err())
    for dt in (0.0, -1 / 30, NAN, INF):
        assert _step(lib, p, dt=dt) == -1 and "dt" in err(), dt
    # what is allowed reaches the size checks, which come last: +inf as min_cutoff, beta = 0, no lm_raw
    for kw in (dict(filt=_lib.TrackFilter.make(min_cutoff=INF)), dict(filt=_lib.TrackFilter.make(beta=0.0)), dict(raw=None)):
        assert _step(lib, p, k=0, **kw) == -2 and "1 <= k <= 65535" in err()


def test_every_error_of_the_plain_step_is_answered_by_the_filtered_one():
    lib = _lib.load()
    p = C.c_void_p(0x1000)
    err = lambda: lib.flm_last_error().decode()
    for name in ("lm", "m", "boxes", "tc", "lmf", "mn", "bn", "st"):
        assert _step(lib, p, **{name: None}) == -1, name
        assert "null" in err()
    assert _step(lib, p, ta=None) == -1 and "both or neither" in err()
    assert _step(lib, p, ma=None) == -1 and "both or neither" in err()
    o = _lib.TrackOpts.make()
    o.struct_size -= 8
    assert _step(lib, p, opts=o) == -1 and "struct_size" in err()
    for mp in (1, 0, -3):
        assert _step(lib, p, opts=_lib.TrackOpts.make(min_points=mp)) == -1 and "min_points >= 2" in err()
    for kw in (dict(min_score=NAN), dict(min_side=NAN), dict(max_side=NAN)):
        assert _step(lib, p, opts=_lib.TrackOpts.make(**kw)) == -1 and "NaN" in err()
    for k in (0, -1, 65536):
        assert _step(lib, p, k=k) == -2 and "1 <= k <= 65535" in err()
    for c in (0, 1025):
        assert _step(lib, p, c=c) == -2 and "1 <= c <= 1024" in err()
    assert _step(lib, p, ls=1) == -2 and "lm_stride >= 2" in err()
    assert _step(lib, p, w=p, ws=0) == -2 and "w_stride >= 1" in err()
    for kw in (dict(in_h=0), dict(in_w=0), dict(fh=0), dict(fw=-5)):
        assert _step(lib, p, **kw) == -2 and "in_h, in_w, fh, fw >= 1" in err()
    for kw in (dict(sx=0.0), dict(sy=-2.0), dict(sx=NAN)):
        assert _step(lib, p, **kw) == -2 and "sx, sy > 0" in err()
        assert "flm_track_step_filtered" in err()


class _Model:
    n_classes, input_height, input_width, output_height, output_width = 68, 64, 64, 72, 72


def test_python_wrappers_reject_bad_filters_on_the_host():
    A = alignment
    for kw, field in ((dict(min_cutoff=0.0), "min_cutoff"), (dict(min_cutoff=-1.0), "min_cutoff"), (dict(min_cutoff=NAN), "min_cutoff"),
                      (dict(beta=-1.0), "beta"), (dict(beta=INF), "beta"), (dict(beta=NAN), "beta"),
                      (dict(d_cutoff=0.0), "d_cutoff"), (dict(d_cutoff=INF), "d_cutoff"), (dict(d_cutoff=NAN), "d_cutoff"),
                      (dict(fps=0.0), "fps"), (dict(fps=-30.0), "fps"), (dict(fps=INF), "fps"), (dict(fps=NAN), "fps")):
        with pytest.raises(ValueError, match=field):
            A.LandmarkFilter(**kw)
    assert A.LandmarkFilter(min_cutoff=INF).min_cutoff == INF and A.LandmarkFilter(beta=0).beta == 0.0
    filt = A.LandmarkFilter(fps=25.0)
    assert filt.time_step() == 1.0 / 25.0 and filt.time_step(0.5) == 0.5
    # track_step_device: the filter's own arguments are checked before any tensor is looked at
    lm = torch.zeros((2, 68, 2), dtype=torch.float64)
    m = torch.zeros((2, 2, 3), dtype=torch.float32)
    boxes = torch.zeros((2, 4), dtype=torch.int32)
    t = torch.zeros((68, 2), dtype=torch.float64)
    state = torch.full((2, 68, 6), -1.0, dtype=torch.float64)
    args = (lm, m, boxes, (72, 72), (64, 64), (270, 480), t)
    with pytest.raises(ValueError, match="LandmarkFilter"):
        A.track_step_device(*args, filter=True, state=state)
    with pytest.raises(ValueError, match="LandmarkFilter"):
        A.track_step_device(*args, filter=(1.0, 15.0, 1.0), state=state)
    for dt in (0.0, -0.1, NAN, INF):
        with pytest.raises(ValueError, match="dt must be"):
            A.track_step_device(*args, filter=filt, dt=dt, state=state)
    for bad in (None, state.to(torch.float32), state[0], state[..., :5], state.numpy()):   # missing, dtype, rank, shape, type
        with pytest.raises(ValueError, match="state must be"):
            A.track_step_device(*args, filter=filt, state=bad)
    for kw in (dict(dt=1 / 30), dict(state=state), dict(lm_raw=lm)):                       # these go with a filter
        with pytest.raises(ValueError, match="go with filter"):
            A.track_step_device(*args, **kw)
    # FaceTracker
    for bad in (False, 1.0, "one-euro", (1.0, 15.0, 1.0)):
        with pytest.raises(ValueError, match="smooth"):
            prediction.FaceTracker(_Model(), (270, 480), 4, smooth=bad)
    tr = prediction.FaceTracker(_Model(), (270, 480), 4, smooth=True)
    assert isinstance(tr.smooth, A.LandmarkFilter) and tr.smooth.beta == 15.0 and tr.filter_state is None
    assert prediction.FaceTracker(_Model(), (270, 480), 4, smooth=filt).smooth is filt
    ring = torch.zeros((2, 270, 480, 3), dtype=torch.uint8)
    for dt in (0.0, -1.0, NAN):
        with pytest.raises(ValueError, match="dt must be"):
            tr.step(ring, 0, dt=dt)
    plain = prediction.FaceTracker(_Model(), (270, 480), 4)
    assert plain.smooth is None and plain.filter_state is None
    with pytest.raises(ValueError, match="dt goes with smooth"):
        plain.step(ring, 0, dt=1 / 30)


# ---- the reference against tests/track_ref.py -------------------------------------------------------------------------
def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(u), b.view(u))


FIVE = ("lm_frame", "m_align", "m_next", "boxes_next", "status")


def _plain(s, seq):
    return track_ref.step(s["lm"], s["w"], s["m_crop"], s["boxes"], cases.SC, cases.SC, cases.IN, cases.IN, cases.FH,
                          cases.FW, seq["tc"], seq["ta"])


@pytest.mark.parametrize("weighted", [False, True])
def test_reference_without_history_is_the_plain_step(weighted):
    """Six frames of the closed loop; at every one of them the filtered step from an empty state is track_ref.step."""
    seq = cases.sequence(8, 68, weighted, steps=6)
    smoothed = 0
    for t, s in enumerate(seq["steps"]):
        exp = _plain(s, seq)
        got = track_filter_ref.step(s["lm"], s["w"], s["m_crop"], s["boxes"], cases.SC, cases.SC, cases.IN, cases.IN, cases.FH,
                                    cases.FW, seq["tc"], seq["ta"], track_filter_ref.empty_state(8, 68), cases.DT)
        for n in FIVE:
            assert _bits(got[n], exp[n]), (t, n)
        assert _bits(got["lm_raw"], exp["lm_frame"])
        # ... while the sequence's own state, which has a history from step 2 on, gives other points
        assert _bits(s["exp"]["lm_raw"], exp["lm_frame"])
        smoothed += int((s["exp"]["lm_frame"] != exp["lm_frame"]).sum())
        if t == 0:
            assert all(_bits(s["exp"][n], exp[n]) for n in FIVE)
    assert smoothed > 1000


@pytest.mark.parametrize("weighted", [False, True])
def test_reference_with_an_infinite_cutoff_is_the_plain_step(weighted):
    seq = cases.sequence(8, 68, weighted, steps=6, filt=dict(min_cutoff=INF, beta=15.0, d_cutoff=1.0))
    histories = 0
    for t, s in enumerate(seq["steps"]):
        exp = _plain(s, seq)
        for n in FIVE:
            assert _bits(s["exp"][n], exp[n]), (t, n)
        histories += int((s["state"][..., 0] >= 0).sum())
    assert histories > 1000                               # (the filter ran with a history, and changed nothing)


def test_the_sequences_hold_what_they_promise():
    """A condition on the inputs of the GPU test: its largest case loses, re-seeds, rejects and poisons as described."""
    seq = cases.sequence(70, 68, True)
    kinds = np.array(seq["kinds"])
    st = np.stack([s["exp"]["status"] for s in seq["steps"]])
    alive = np.isin(kinds, (cases.PLAIN, cases.ROLLED, cases.SMALL))
    assert (st[:, alive] == 0).all()
    assert (st[:, kinds == cases.DEAD] & track_ref.DEAD).all()
    lost = kinds == cases.LOST
    assert (st[:2, lost] == 0).all() and (st[2, lost] == track_ref.OUTSIDE).all() and (st[3:, lost] == 0).all()
    s4 = seq["steps"][3]
    assert (s4["state"][lost] == -1).all() and _bits(s4["exp"]["lm_frame"][lost], s4["exp"]["lm_raw"][lost])
    # rejected points lose their history and restart: out = raw at the step they return
    for t, back in ((3, range(3, 67, 4)), (4, range(1, 67, 4))):     # (point 67 is never rejected: it is poisoned)
        e = seq["steps"][t - 1]["exp"]
        for i in back:
            assert (seq["steps"][t - 1]["state"][alive, i, 0] == -1).all()
            assert _bits(e["lm_frame"][alive, i], e["lm_raw"][alive, i]) and (e["lm_raw"][alive, i] >= 0).all()
    # the poisoned entry: that point restarts too, its neighbour does not
    i, _ = cases.poisoned(68)
    s3 = seq["steps"][2]
    assert np.isnan(s3["state"][0, i]).sum() == 1
    assert _bits(s3["exp"]["lm_frame"][0, i], s3["exp"]["lm_raw"][0, i])
    assert (s3["exp"]["lm_frame"][0, i - 1] != s3["exp"]["lm_raw"][0, i - 1]).all()
    assert np.isfinite(s3["exp"]["state"]).all()


# ---- what the filter does to a moving and to a resting point ----------------------------------------------------------
@pytest.mark.parametrize("v", [0.25, 1.0, 4.0])
def test_lag_of_a_steady_ramp(v):
    """A noise-free point moving at v crop sides per second, 30 frames/s, 300 frames.  Once the velocity estimate has
    settled (0.827^300) the filter is a fixed first-order low-pass of cutoff fc = min_cutoff + beta*v, whose lag behind a
    ramp of V px/s is V/(2 pi fc)."""
    side, fps, n = 256.0, 30.0, 300
    mc, beta = 1.0, 15.0
    d = np.array([np.cos(0.3), np.sin(0.3)])                    # (neither axis: the speed is the vector's length)
    state = track_filter_ref.empty_state(1)
    for t in range(n):
        raw = (np.array([50.0, 40.0]) + d * (v * side * t / fps))[None]
        out, state = track_filter_ref.one_euro(raw, state, side, 1.0 / fps, mc, beta, 1.0)
    lag = float(np.hypot(*(raw - out)[0]))
    steady = side * v / (2 * np.pi * (mc + beta * v))
    print("v = %.2f sides/s: lag %.9f px, steady state %.9f px, bound %.9f px" % (v, lag, steady, side / (2 * np.pi * beta)))
    assert lag <= side / (2 * np.pi * beta) * (1 + 1e-9)
    assert abs(lag - steady) <= 1e-6


def test_noise_of_a_resting_point():
    """White noise of 0.3 px on a resting point, 2,000 frames at 30 frames/s: the arithmetic predicts about 0.33 of the
    input's standard deviation (0.31 for a fixed a = 0.173, a little more once the noise's own speed raises the cutoff);
    0.5 is a cap that only an unfiltered output would break."""
    rng = np.random.default_rng(7)
    n, side = 2000, 256.0
    raw = np.array([300.0, 200.0]) + rng.normal(0, 0.3, (n, 2))
    state = track_filter_ref.empty_state(1)
    out = np.zeros_like(raw)
    for t in range(n):
        o, state = track_filter_ref.one_euro(raw[t][None], state, side, 1.0 / 30.0)
        out[t] = o[0]
    ratio = out.std(0) / raw.std(0)
    print("output / input standard deviation per axis: %s" % ratio)
    assert (ratio < 0.5).all()
