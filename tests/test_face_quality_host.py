"""CPU-side checks of the best-shot calls (flm_face_quality, flm_track_best_update, alignment.QualityOptions / BestShot,
FaceTracker(best_shot=)): tests/face_quality_ref.py against values worked out by hand, the rules of the update (tie,
reset, status, NaN), every argument check of the two C calls (each answers before any launch, so without a GPU) and the
Python validation."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import flm_amd  # noqa: F401
from flm_amd import _lib, alignment, prediction

import face_quality_ref as ref

f32, f64 = np.float32, np.float64
P = C.c_void_p(0x1000)        # never dereferenced: every call below is rejected before a launch
PLAIN = ("nhwc", "uint8", "bgr", (1.0,) * 3, (0.0,) * 3)


def err():
    return _lib.load().flm_last_error().decode()


def gray(a):
    """uint8 [h,w] -> a uint8 NHWC face [1,h,w,3] with B = G = R."""
    a = np.asarray(a, np.uint8)
    return np.repeat(a[None, :, :, None], 3, axis=3)


# ---- the reference against values worked out by hand -------------------------------------------------------------------
def test_one_laplacian_pixel():
    # B = G = R = x gives Y = (16384*16x + 8192) >> 14 = 16x.  Centre 10, its four neighbours 20, 30, 40, 50, corners 0:
    # L = 16 * (20+30+40+50 - 40) = 1600.
    a = [[0, 20, 0], [30, 10, 40], [0, 50, 0]]
    rec = ref.record(gray(a), PLAIN)
    s = 16 * 150
    ss = 256 * (100 + 400 + 900 + 1600 + 2500)
    assert rec.tolist() == [[9, s, ss, 1, 1600, 1600 * 1600, 5, 0]]       # (dark, below level 16: the corners and the centre)
    # one sample: the variance of the Laplacian is 0
    assert ref.sharpness(rec[0]) == 0.0


def test_luma_weights_by_channel_order():
    face = np.zeros((1, 1, 1, 3), np.uint8)
    face[0, 0, 0] = (255, 0, 0)                         # output channel 0
    assert ref.record(face, PLAIN)[0, 1] == (1868 * 4080 + 8192) >> 14                       # BGR: it is B
    assert ref.record(face, ("nhwc", "uint8", "rgb", (1.0,) * 3, (0.0,) * 3))[0, 1] == (4899 * 4080 + 8192) >> 14   # RGB: R
    planar = np.ascontiguousarray(face.transpose(0, 3, 1, 2))
    assert ref.record(planar, ("nchw", "uint8", "bgr", (1.0,) * 3, (0.0,) * 3))[0, 1] == (1868 * 4080 + 8192) >> 14


def test_constant_face():
    rec = ref.record(gray(np.full((6, 9), 100)), PLAIN)
    assert rec.tolist() == [[54, 54 * 1600, 54 * 1600 * 1600, 28, 0, 0, 0, 0]]
    assert ref.sharpness(rec[0]) == 0.0
    # no interior: n_lap = 0 and the slot can never be eligible
    rec = ref.record(gray(np.full((2, 7), 100)), PLAIN)
    assert rec[0, 3] == 0 and rec[0, 4] == 0 and rec[0, 5] == 0
    q, ok = ref.quality(rec, np.zeros((1, 1, 2)))
    assert not ok[0]


def test_checkerboard_is_the_extreme():
    h, w = 8, 10
    yy, xx = np.mgrid[0:h, 0:w]
    a = np.where((yy + xx) % 2 == 0, 255, 0)
    rec = ref.record(gray(a), PLAIN)[0]
    n_lap = (h - 2) * (w - 2)
    # every interior pixel: |L| = 4 * 4080, the largest a Laplacian can be; the signs alternate
    assert rec[3] == n_lap and rec[5] == n_lap * (4 * 4080) ** 2 and rec[4] == 0
    assert rec[6] == h * w // 2 and rec[7] == h * w // 2
    assert ref.sharpness(rec) == (4 * 255.0) ** 2
    # with h, w at the call's limit (h*w*12 < 2^31) the sum stays below 2^56
    assert (2 ** 31 // 12) * (4 * 4080) ** 2 < 2 ** 56


def test_blur_lowers_sharpness():
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (40, 36, 3)).astype(f32)
    sharp = ref.record(img[None], ("nhwc", "float32", "bgr", (1.0,) * 3, (0.0,) * 3))
    soft = ref.record(ref.box_blur(img)[None], ("nhwc", "float32", "bgr", (1.0,) * 3, (0.0,) * 3))
    assert 0.0 < ref.sharpness(soft[0]) < ref.sharpness(sharp[0])


def test_quantise_edges():
    one = f32(1.0)
    x = np.array([[np.nan, np.inf, -np.inf], [300.0, -5.0, 0.03125], [0.09375, 254.96875, 255.0]], f32)
    p = ref.quantise(x, f32(0.0), one)
    # NaN -> 0; the infinities clamp; 0.5 and 1.5 sixteenths round to even
    assert p.tolist() == [[0, 4080, 0], [4080, 0, 0], [2, 4080, 4080]]
    # the matcher's format stores (x/127.5 - 1): undone in two float32 operations
    sc, bi = f32(1.0 / 127.5), f32(-1.0)
    stored = (np.arange(256, dtype=f32) * sc).astype(f32) + bi
    back = ref.quantise(stored.astype(f32), bi, (one / sc).astype(f32))
    assert np.abs(back - 16 * np.arange(256)).max() <= 1      # float32 rounding moves a value by at most one sixteenth


def _one_slot():
    rng = np.random.default_rng(2)
    face = rng.integers(0, 256, (1, 8, 8, 3)).astype(np.uint8)
    return face, ref.record(face, PLAIN), np.zeros((1, 2, 2))


def test_update_rules():
    face, rec, lm = _one_slot()
    st = ref.new_state(face, 1, 2)
    assert ref.best_update(st, face, rec, lm, 7).tolist() == [True]
    q0 = st["best_q"][0]
    assert q0 > 0 and st["best_frame"][0] == 7 and np.array_equal(st["gallery"], face)
    # a tie: the earlier frame stays
    other = face[:, ::-1].copy()                       # the same sums, other bytes
    assert ref.best_update(st, other, rec, lm, 8).tolist() == [False]
    assert st["best_frame"][0] == 7 and np.array_equal(st["gallery"], face) and st["best_q"][0] == q0
    # status != 0: not eligible
    assert ref.best_update(st, other, rec, lm, 9, factor=np.array([2.0]), status=np.array([4], np.int32)).tolist() == [False]
    # a NaN factor: not eligible; a negative one neither
    assert ref.best_update(st, other, rec, lm, 9, factor=np.array([np.nan])).tolist() == [False]
    assert ref.best_update(st, other, rec, lm, 9, factor=np.array([-1.0])).tolist() == [False]
    assert st["best_q"][0] == q0 and st["best_frame"][0] == 7
    # reset with an ineligible face: the slot holds no best (-1), its gallery bytes stay
    assert ref.best_update(st, other, rec, lm, 10, factor=np.array([np.nan]), reset=np.array([1], np.int32)).tolist() == [False]
    assert st["best_q"][0] == -1.0 and np.array_equal(st["gallery"], face)
    # q = 0 beats "no best"
    assert ref.best_update(st, other, rec, lm, 11, factor=np.array([0.0])).tolist() == [True]
    assert st["best_q"][0] == 0.0 and st["best_frame"][0] == 11 and np.array_equal(st["gallery"], other)


def test_wbar_skips_rejected_landmarks():
    face, rec, _ = _one_slot()
    lm = np.array([[[3.0, 4.0], [-1.0, -1.0], [5.0, -1.0]]])
    w = np.array([[0.5, 100.0, 0.25]])
    q1, _ = ref.quality(rec, lm)
    qw, ok = ref.quality(rec, lm, w)
    assert ok[0] and qw[0] == q1[0] * ((0.5 + 0.25) / 2)
    q0, ok = ref.quality(rec, np.full((1, 3, 2), -1.0), w)
    assert q0[0] == 0.0 and ok[0]                       # no landmark took part: wbar = 0, q = 0
    # exposure: a black face is all dark -> e = 0 < min_exposed
    black = np.zeros((1, 8, 8, 3), np.uint8)
    _, ok = ref.quality(ref.record(black, PLAIN), lm)
    assert not ok[0]


def test_quality_scalars():
    a = [[0, 20, 0], [30, 10, 40], [0, 50, 0]]
    rec = ref.record(gray(np.kron(np.array(a), np.ones((2, 2), int))), PLAIN)
    sc = alignment.quality_scalars(rec)
    assert sc.shape == (1, 4) and sc.dtype == np.float64
    y = ref.luma(gray(np.kron(np.array(a), np.ones((2, 2), int))), PLAIN)[0] / 16.0
    lap = ref.laplacian(ref.luma(gray(np.kron(np.array(a), np.ones((2, 2), int))), PLAIN))[0] / 16.0
    assert np.allclose(sc[0], [lap.var(), y.mean(), y.std(), (y >= 16).mean()], rtol=1e-12)
    t = alignment.quality_scalars(torch.from_numpy(rec))
    assert isinstance(t, torch.Tensor) and np.array_equal(t.numpy(), sc)
    assert alignment.quality_scalars(ref.record(gray(np.full((2, 7), 100)), PLAIN))[0, 0] == 0.0
    with pytest.raises(ValueError):
        alignment.quality_scalars(np.zeros((1, 7), np.int64))


# ---- the C ABI ----------------------------------------------------------------------------------------------------------
def test_exports_and_defaults():
    lib = C.CDLL(_lib.LIB_PATH)
    for name in ("flm_quality_opts_init", "flm_face_quality", "flm_best_opts_init", "flm_track_best_update"):
        assert hasattr(lib, name) and name in _lib.EXPORTS, name
    assert _lib.load().flm_abi_version() == 2          # purely additive
    q = _lib.QualityOpts.make()
    assert (q.struct_size, q.dark, q.bright) == (C.sizeof(_lib.QualityOpts), 16, 239) and q.struct_size == 12
    b = _lib.BestOpts.make()
    assert (b.struct_size, b.reserved, b.sharp_ref, b.min_exposed) == (C.sizeof(_lib.BestOpts), 0, 100.0, 0.5)
    assert b.struct_size == 24 and _lib.QUALITY_REC == 8


def fmt_struct(**kw):
    f = _lib.ImageFormat()
    _lib.load().flm_image_format_init(C.byref(f))
    for k, v in kw.items():
        if k in ("scale", "bias"):
            for c in range(3):
                getattr(f, k)[c] = v[c]
        else:
            setattr(f, k, v)
    return f


def quality_call(faces=P, k=1, h=112, w=112, fmt=None, opts=None, rec=P):
    return _lib.load().flm_face_quality(None, faces, k, h, w, None if fmt is None else C.byref(fmt),
                                        None if opts is None else C.byref(opts), rec)


def test_face_quality_argument_errors():
    QualityOpts = _lib.QualityOpts
    cases = [
        (dict(faces=None), "null"), (dict(rec=None), "null"),
        (dict(fmt=fmt_struct(struct_size=8)), "struct_size"),
        (dict(fmt=fmt_struct(layout=2)), "layout"), (dict(fmt=fmt_struct(type=4)), "pixel type"),
        (dict(fmt=fmt_struct(reverse_channels=2)), "reverse_channels"),
        (dict(fmt=fmt_struct(scale=(1.0, float("inf"), 1.0))), "finite"),
        (dict(fmt=fmt_struct(bias=(float("nan"), 0.0, 0.0))), "finite"),
        (dict(fmt=fmt_struct(scale=(1.0, 0.0, 1.0))), "scale != 0"),
        (dict(fmt=fmt_struct(type=_lib.PIX_F16), faces=C.c_void_p(0x1001)), "2-byte"),
        (dict(faces=C.c_void_p(0x1002)), "4-byte"),
        (dict(opts=QualityOpts.make(dark=-1)), "[0, 255]"), (dict(opts=QualityOpts.make(bright=256)), "[0, 255]"),
    ]
    small = QualityOpts.make()
    small.struct_size = 8
    cases.append((dict(opts=small), "struct_size"))
    for kw, word in cases:
        rc = quality_call(**kw)
        assert rc != 0 and rc == _arg_code(), (kw, rc)
        assert word in err() and "flm_face_quality" in err(), (kw, err())
    for kw, word in [(dict(k=0), "65535"), (dict(k=65536), "65535"), (dict(h=0), "h, w >= 1"), (dict(w=0), "h, w >= 1"),
                     (dict(h=13378, w=13378), "2^31")]:
        rc = quality_call(**kw)
        assert rc == _shape_code(), (kw, rc)
        assert word in err(), (kw, err())
    assert 13377 * 13377 * 12 < 2 ** 31 <= 13378 * 13378 * 12


def _codes():
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "flm.h")).read()
    return {n: int(v) for n, v in re.findall(r"(FLM_ERR_\w+)\s*=\s*(-?\d+)", text)}


def _arg_code():
    return _codes()["FLM_ERR_ARG"]


def _shape_code():
    return _codes()["FLM_ERR_SHAPE"]


def best_call(**kw):
    a = dict(faces=P, face_bytes=192, k=2, rec=P, status=None, reset=None, lm=P, ls=2, w=None, ws=1, c=5, factor=None, m=None,
             frame_id=0, opts=None, q_in=C.c_void_p(0x2000), q_out=C.c_void_p(0x3000), gallery=C.c_void_p(0x9000),
             frame=P, best_m=None, best_lm=None, best_rec=None)
    a.update(kw)
    return _lib.load().flm_track_best_update(
        None, a["faces"], a["face_bytes"], a["k"], a["rec"], a["status"], a["reset"], a["lm"], a["ls"], a["w"], a["ws"],
        a["c"], a["factor"], a["m"], a["frame_id"], None if a["opts"] is None else C.byref(a["opts"]), a["q_in"], a["q_out"],
        a["gallery"], a["frame"], a["best_m"], a["best_lm"], a["best_rec"])


def test_track_best_update_argument_errors():
    B = _lib.BestOpts
    for name in ("faces", "rec", "lm", "q_in", "q_out", "gallery", "frame"):
        assert best_call(**{name: None}) == _arg_code(), name
        assert "null" in err() and "flm_track_best_update" in err()
    small = B.make()
    small.struct_size = 16
    res = B.make()
    res.reserved = 1
    for kw, word in [(dict(best_m=P), "needs m_dev"), (dict(opts=small), "struct_size"), (dict(opts=res), "reserved"),
                     (dict(opts=B.make(sharp_ref=0.0)), "sharp_ref > 0"), (dict(opts=B.make(sharp_ref=float("nan"))), "sharp_ref > 0"),
                     (dict(opts=B.make(min_exposed=float("nan"))), "NaN"),
                     (dict(q_out=C.c_void_p(0x2000)), "overlap"), (dict(q_out=C.c_void_p(0x2008)), "overlap"),
                     (dict(q_in=C.c_void_p(0x3008)), "overlap"),
                     (dict(gallery=C.c_void_p(0x1000 + 383)), "gallery_dev overlap")]:
        assert best_call(**kw) == _arg_code(), kw
        assert word in err(), (kw, err())
    for kw, word in [(dict(k=0), "65535"), (dict(k=65536), "65535"), (dict(c=0), "c >= 1"), (dict(face_bytes=0), "face_bytes"),
                     (dict(ls=1), "lm_stride >= 2"), (dict(w=P, ws=0), "w_stride >= 1")]:
        assert best_call(**kw) == _shape_code(), kw
        assert word in err(), (kw, err())
    # adjacent buffers do not overlap
    assert "overlap" not in (err() if best_call(q_out=C.c_void_p(0x2010), k=0) else "")


# ---- the Python validation -----------------------------------------------------------------------------------------------
def test_python_argument_checks():
    A = alignment
    for kw in (dict(dark=-1), dict(bright=256), dict(dark=1.5), dict(dark=True)):
        with pytest.raises(ValueError):
            A.QualityOptions(**kw)
    for kw in (dict(sharp_ref=0.0), dict(sharp_ref=float("nan")), dict(min_exposed=float("nan")), dict(bright=300)):
        with pytest.raises(ValueError):
            A.BestShot(**kw)
    b = A.BestShot(sharp_ref=50, min_exposed=0.25, dark=10, bright=200)
    assert (b.sharp_ref, b.min_exposed, b.dark, b.bright) == (50.0, 0.25, 10, 200)
    assert (A.QualityOptions().dark, A.QualityOptions().bright) == (16, 239)
    faces = torch.zeros((2, 8, 8, 3))
    with pytest.raises(ValueError, match="opts"):
        A.face_quality_device(faces, opts=object())
    with pytest.raises(ValueError, match="AlignedFormat"):
        A.face_quality_device(faces, fmt="nchw")
    with pytest.raises(ValueError, match="float16"):
        A.face_quality_device(faces, fmt=A.AlignedFormat.matcher())          # float32 faces for a float16 format
    with pytest.raises(ValueError, match="shape"):
        A.face_quality_device(torch.zeros((2, 8, 8, 3), dtype=torch.float16), fmt=A.AlignedFormat.matcher())   # not planar
    with pytest.raises(ValueError, match="scale of 0"):
        A.face_quality_device(faces, fmt=A.AlignedFormat(scale=(1.0, 0.0, 1.0)))
    with pytest.raises(ValueError, match="CUDA"):
        A.face_quality_device(faces)
    with pytest.raises(ValueError, match="BestShot"):
        A.track_best_update_device(faces, None, None, None, None, None, None, 0, opts=object())
    with pytest.raises(ValueError, match="frame_id"):
        A.track_best_update_device(faces, None, None, None, None, None, None, 1.5)
    with pytest.raises(ValueError, match="CUDA"):
        A.track_best_update_device(faces, None, None, None, None, None, None, 0)
    with pytest.raises(ValueError, match="best_shot"):
        prediction.FaceTracker(None, (270, 480), 2, best_shot="yes")
    with pytest.raises(ValueError, match="bfloat16"):
        prediction.face_quality(np.zeros((1, 3, 8, 8), np.uint16), A.AlignedFormat("nchw", "bfloat16"))
