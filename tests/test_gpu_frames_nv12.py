"""GPU parity of the NV12 frame source: flm_frames_to_bgr against tests/nv12_ref.py, and flm_crop_resize_frames_src /
flm_warp_affine_frames_src / prediction.align_frames(frame_format=...) on the NV12 ring against the existing BGR calls
on the reference's BGR ring.  Every comparison is exact (torch.equal): the contract of include/flm.h is "the bits of
the BGR call on the converted frame".  No test here tries to provoke an out-of-slot read; tests/test_nv12_taps_host.py
catches those on the host.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import nv12_ref

pytestmark = pytest.mark.gpu
f32 = np.float32
FH, FW, PITCH, UV_ROW, ROWS, NF = 48, 64, 80, 56, 84, 3     # 24 U,V rows from row 56, 4 slack rows per slot
MATRICES = ["bt601", "bt709"]


@pytest.fixture(scope="module")
def mods():
    import flm_amd  # noqa: F401
    from flm_amd import _lib, alignment, prediction
    _lib.load()
    return _lib, alignment, prediction


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def saturated(bgr):
    return float(((bgr == 0) | (bgr == 255)).any(-1).mean())


def make_rings(matrix):
    """The padded ring of the module docstring and its reference BGR ring, a dense 48x64 ring, a dense 2x2 frame and a
    dense 6x40 frame (a width that is no multiple of the converter's 16-pixel segment)."""
    rng = np.random.default_rng(MATRICES.index(matrix) + 71)
    ring = rng.integers(0, 256, (NF, ROWS, PITCH), dtype=np.uint8)             # padding and slack rows: junk
    for f in range(2):                                                         # slots 0, 1: white noise, forward transform
        y, uv = nv12_ref.bgr_to_nv12(rng.integers(0, 256, (FH, FW, 3), dtype=np.uint8), matrix)
        ring[f] = nv12_ref.pack_slot(y, uv, PITCH, UV_ROW, ROWS, rng)
    # slot 2 stays uniformly random bytes: most of its pixels saturate a channel
    bgr = np.stack([nv12_ref.nv12_to_bgr_ref(ring[f].reshape(-1), FH, FW, PITCH, UV_ROW * PITCH, PITCH, matrix)
                    for f in range(NF)])
    dense = np.ascontiguousarray(np.concatenate([ring[:, :FH, :FW], ring[:, UV_ROW:UV_ROW + FH // 2, :FW]], 1))
    tiny = rng.integers(0, 256, (1, 3, 2), dtype=np.uint8)
    ragged = rng.integers(0, 256, (2, 9, 40), dtype=np.uint8)
    return dict(matrix=matrix, ring=ring, bgr=bgr, dense=dense, tiny=tiny, ragged=ragged,
                tiny_bgr=nv12_ref.nv12_to_bgr_ref(tiny[0].reshape(-1), 2, 2, 2, 4, 2, matrix)[None],
                ragged_bgr=np.stack([nv12_ref.nv12_to_bgr_ref(ragged[f].reshape(-1), 6, 40, 40, 240, 40, matrix) for f in range(2)]))


@pytest.fixture(scope="module", params=MATRICES)
def data(request, mods):
    L, A, _ = mods
    d = make_rings(request.param)
    d["nv"] = A.FrameFormat.nv12(FH, FW, matrix=request.param, uv_row=UV_ROW)
    for k in ("ring", "bgr", "dense", "tiny", "ragged", "tiny_bgr", "ragged_bgr"):
        d[k + "_d"] = dev(d[k])
    return d


def dense_format(L, matrix, pixel=None):
    """A flm_frame_format with every pitch and offset 0 (the defaults: y_pitch = fw, uv_pitch = y_pitch, uv_offset = y_pitch*fh)."""
    s = L.FrameFormat()
    L.load().flm_frame_format_init(C.byref(s))
    s.pixel = L.FRAME_NV12 if pixel is None else pixel
    s.matrix = MATRICES.index(matrix)
    return s


# ---- the C calls on a raw ring (the Python wrappers always pass the tensor's pitch) -----------------------------------
def raw_to_bgr(L, ring, fh, fw, src):
    nf = int(ring.shape[0])
    out = torch.empty((nf, fh, fw, 3), dtype=torch.uint8, device="cuda")
    L.check(L.load().flm_frames_to_bgr(L.stream_ptr(), L.ptr(ring), ring[0].numel(), nf, fh, fw, C.byref(src), L.ptr(out)), "to_bgr")
    return out


def raw_crop(L, ring, fh, fw, boxes, idx, oh, ow, src=None):
    """src None: flm_crop_resize_frames on a BGR ring."""
    nf, k = int(ring.shape[0]), int(boxes.shape[0])
    out = torch.full((k, oh, ow, 3), 99, dtype=torch.uint8, device="cuda")
    lib = L.load()
    if src is None:
        L.check(lib.flm_crop_resize_frames(L.stream_ptr(), L.ptr(ring), ring[0].numel(), nf, fh, fw, L.ptr(boxes), L.ptr(idx), k,
                                           L.ptr(out), oh, ow), "crop")
    else:
        L.check(lib.flm_crop_resize_frames_src(L.stream_ptr(), L.ptr(ring), ring[0].numel(), nf, fh, fw, L.ptr(boxes), L.ptr(idx), k,
                                               L.ptr(out), oh, ow, C.byref(src)), "crop_src")
    return out


def raw_warp(L, ring, fh, fw, idx, boxes, m, hd, wd, samples, src):
    nf, k = int(ring.shape[0]), int(m.shape[0])
    out = torch.full((k, hd, wd, 3), 777.0, dtype=torch.float32, device="cuda")
    L.check(L.load().flm_warp_affine_frames_src(L.stream_ptr(), L.ptr(ring), ring[0].numel(), nf, fh, fw,
                                                None if idx is None else L.ptr(idx), None if boxes is None else L.ptr(boxes),
                                                L.ptr(m), k, L.ptr(out), hd, wd, samples, None, C.byref(src)), "warp_src")
    return out


# ---- 1. the converter ----------------------------------------------------------------------------------------------
def test_input_condition_and_frames_to_bgr(mods, data):
    L, A, P = mods
    sat = [saturated(data["bgr"][f]) for f in range(NF)]
    print("saturated pixels per slot (%s): %s" % (data["matrix"], np.round(sat, 3)))
    assert max(sat[:2]) <= 0.15                      # a condition on the input: slots 0, 1 mostly inside the clamps
    assert sat[2] >= 0.5                             # slot 2 exercises them
    got = P.frames_to_bgr_device(data["ring_d"], data["nv"])
    assert got.dtype == torch.uint8 and tuple(got.shape) == (NF, FH, FW, 3) and got.is_cuda
    assert torch.equal(got, data["bgr_d"])
    out = torch.empty_like(got)
    assert P.frames_to_bgr_device(data["ring_d"], data["nv"], out=out).data_ptr() == out.data_ptr() and torch.equal(out, got)
    # dense rings, every pitch and offset 0
    z = dense_format(L, data["matrix"])
    assert torch.equal(raw_to_bgr(L, data["dense_d"], FH, FW, z), data["bgr_d"])
    assert torch.equal(raw_to_bgr(L, data["tiny_d"], 2, 2, z), data["tiny_bgr_d"])
    assert torch.equal(raw_to_bgr(L, data["ragged_d"], 6, 40, z), data["ragged_bgr_d"])
    # an output that is not 16-byte aligned takes the element stores
    buf = torch.zeros(NF * FH * FW * 3 + 16, dtype=torch.uint8, device="cuda")
    view = buf[3:3 + NF * FH * FW * 3].view(NF, FH, FW, 3)
    P.frames_to_bgr_device(data["ring_d"], data["nv"], out=view)
    assert torch.equal(view, data["bgr_d"]) and not buf[:3].any() and not buf[3 + NF * FH * FW * 3:].any()
    # the slack rows and the padding are not part of the frame
    junk = data["ring_d"].clone()
    junk[:, FH:UV_ROW] ^= 0xFF
    junk[:, UV_ROW + FH // 2:] ^= 0xFF
    junk[:, :, FW:] ^= 0xFF
    assert torch.equal(P.frames_to_bgr_device(junk, data["nv"]), data["bgr_d"])


# ---- 2. crop / resize ------------------------------------------------------------------------------------------------
CROP_BOXES = np.array([[5, 7, 37, 39],          # odd origin
                       [4, 8, 36, 40],          # even origin
                       [-10, -6, 30, 34],       # poking out
                       [70, 10, 100, 40],       # missing the frame
                       [3, 5, 51, 37],          # 48x32: exact 2x of 16x24 at an odd origin
                       [4, 6, 52, 38],          # the same at an even origin
                       [20, 20, 29, 29],        # a 9x9 upscale
                       [0, 0, 64, 48],          # the whole frame
                       [5, 7, 37, 39],          # slot 2: saturated pixels
                       [1, 1, 63, 47],          # slot 2
                       [5, 7, 37, 39],          # a slot index outside the ring
                       [5, 7, 37, 39]], np.int32)
CROP_SLOTS = np.array([0, 1, 0, 1, 0, 1, 1, 0, 2, 2, 3, -1], np.int32)


@pytest.mark.parametrize("out_hw", [(32, 32), (16, 24)])
def test_crop_resize_from_nv12(mods, data, out_hw):
    L, A, P = mods
    oh, ow = out_hw
    boxes, idx = dev(CROP_BOXES), dev(CROP_SLOTS)
    exp = raw_crop(L, data["bgr_d"], FH, FW, boxes, idx, oh, ow)
    assert not exp[3].any() and not exp[10].any() and not exp[11].any() and exp[0].any() and exp[8].any()
    got = raw_crop(L, data["ring_d"], FH, FW, boxes, idx, oh, ow, data["nv"].struct(data["ring_d"]))
    assert torch.equal(got, exp)
    # the dense ring with every pitch 0
    assert torch.equal(raw_crop(L, data["dense_d"], FH, FW, boxes, idx, oh, ow, dense_format(L, data["matrix"])), exp)
    # a BGR24 source through the _src call is the old call
    assert torch.equal(raw_crop(L, data["bgr_d"], FH, FW, boxes, idx, oh, ow, dense_format(L, data["matrix"], L.FRAME_BGR24)), exp)
    # the 2x2 frame: whole, and its last pixel
    tb, ti = dev(np.array([[0, 0, 2, 2], [1, 1, 2, 2], [0, 0, 2, 2]], np.int32)), dev(np.array([0, 0, 0], np.int32))
    for th, tw in ((oh, ow), (1, 1)):                # (1x1 from 2x2 is the exact-2x area path)
        assert torch.equal(raw_crop(L, data["tiny_d"], 2, 2, tb, ti, th, tw, dense_format(L, data["matrix"])),
                           raw_crop(L, data["tiny_bgr_d"], 2, 2, tb, ti, th, tw))


def test_crop_frames_device_from_nv12(mods, data):
    """The Python entry point: detector boxes squared on the host, one upload, the NV12 ring direct."""
    L, A, P = mods
    faces = [[[6, 5, 38, 40], [30, 2, 70, 44]], [[-4, 10, 30, 46]], [[9, 9, 41, 37]]]
    exp = P.crop_frames_device(data["bgr_d"], faces, 32, 48, frame_index=[2, 0, 1], return_device=True)
    got = P.crop_frames_device(data["ring_d"], faces, 32, 48, frame_index=[2, 0, 1], return_device=True, frame_format=data["nv"])
    assert torch.equal(got[0], exp[0]) and got[1] == exp[1] and torch.equal(got[2], exp[2]) and torch.equal(got[3], exp[3])
    assert got[0].any()
    same = P.crop_frames_device(data["bgr_d"], faces, 32, 48, frame_index=[2, 0, 1], frame_format=A.FrameFormat.bgr())
    assert torch.equal(same[0], exp[0])


# ---- 3. the warp -----------------------------------------------------------------------------------------------------
def sims(hd, wd):
    """12 maps frame px -> aligned px: strong down-scales, near-unit scale, rotations, centres at and beyond the border,
    the identity (every column from fw-1 on is xs = fw-1 exactly where wd >= fw) and the shifted identity whose last
    pixel is (fw-1, fh-1)."""
    spec = [(0.07, 0.3, 32, 24), (0.11, -2.0, 30, 20), (0.22, 1.2, 5, 40), (0.45, 0.0, 63, 47), (0.97, 0.02, 32, 24),
            (1.0, 0.0, 0, 0), (1.03, -0.01, 64, 48), (1.7, 0.8, 20, 30), (2.6, -2.4, 50, 10), (3.5, 3.1, -3, 50)]
    m = np.zeros((12, 2, 3), f32)
    for i, (s, th, cx, cy) in enumerate(spec):
        a, b = s * np.cos(th), s * np.sin(th)
        m[i] = [[a, -b, wd / 2 - (a * cx - b * cy)], [b, a, hd / 2 - (b * cx + a * cy)]]
    m[10] = [[1, 0, 0], [0, 1, 0]]
    m[11] = [[1, 0, wd - FW], [0, 1, hd - FH]]
    return m


WARP_SLOTS = np.array([0, 1, 2, 0, 1, 2, 2, 1, 5, 0, 1, 2], np.int32)                   # face 8: a slot outside the ring
WARP_BOXES = np.tile(np.array([[5, 5, 40, 40]], np.int32), (12, 1))
WARP_BOXES[3] = [70, 10, 100, 40]                                                       # face 3: an empty clipped box


@pytest.fixture(scope="module")
def warp_args():
    return {hw: dev(sims(*hw)) for hw in ((112, 112), (7, 5))}, dev(WARP_SLOTS), dev(WARP_BOXES)


@pytest.mark.parametrize("out_hw", [(112, 112), (7, 5)])
@pytest.mark.parametrize("samples", [1, 2, 4])
def test_warp_from_nv12_plain(mods, data, warp_args, out_hw, samples):
    L, A, P = mods
    hd, wd = out_hw
    ms, idx, boxes = warp_args
    m = ms[out_hw]
    exp = A.warp_frames_device(data["bgr_d"], m, hd, wd, frame_index_dev=idx, boxes_dev=boxes, samples=samples)
    assert not exp[3].any() and not exp[8].any() and exp[0].any() and exp[2].any()
    if samples == 1:                                 # x0 = fw-1, y0 = fh-1 are in the data
        assert exp[11, -1, -1].tolist() == data["bgr"][2, -1, -1].astype(f32).tolist()
    got = A.warp_frames_device(data["ring_d"], m, hd, wd, frame_index_dev=idx, boxes_dev=boxes, samples=samples, src=data["nv"])
    assert got.dtype == torch.float32 and tuple(got.shape) == (12, hd, wd, 3)
    assert torch.equal(got, exp)
    out = torch.full_like(got, 777.0)
    r = A.warp_frames_device(data["ring_d"], m, hd, wd, frame_index_dev=idx, boxes_dev=boxes, samples=samples, src=data["nv"], out=out)
    assert r.data_ptr() == out.data_ptr() and torch.equal(out, exp)
    # without boxes and without slots (every face reads slot 0)
    assert torch.equal(A.warp_frames_device(data["ring_d"], m, hd, wd, samples=samples, src=data["nv"]),
                       A.warp_frames_device(data["bgr_d"], m, hd, wd, samples=samples))
    # the dense ring with every pitch 0, and the 2x2 frame
    z = dense_format(L, data["matrix"])
    assert torch.equal(raw_warp(L, data["dense_d"], FH, FW, idx, boxes, m, hd, wd, samples, z), exp)
    tm = dev(np.array([[[1, 0, 0], [0, 1, 0]], [[2.5, 0, 0.5], [0, 3.0, 0.25]], [[0.9, -0.5, 2], [0.5, 0.9, 1]],
                       [[1, 0, wd - 2], [0, 1, hd - 2]]], f32))
    assert torch.equal(raw_warp(L, data["tiny_d"], 2, 2, None, None, tm, hd, wd, samples, z),
                       A.warp_frames_device(data["tiny_bgr_d"], tm, hd, wd, samples=samples))
    # a BGR24 source through the _src call is the old call
    assert torch.equal(A.warp_frames_device(data["bgr_d"], m, hd, wd, frame_index_dev=idx, boxes_dev=boxes, samples=samples,
                                            src=A.FrameFormat.bgr()), exp)


@pytest.mark.parametrize("out_hw", [(112, 112), (7, 5)])
def test_warp_from_nv12_formats(mods, data, warp_args, out_hw):
    L, A, P = mods
    hd, wd = out_hw
    ms, idx, boxes = warp_args
    m = ms[out_hw]
    cases = [(A.AlignedFormat(layout, dtype, "rgb", scale=(0.5, 1.0 / 127.5, 1.25), bias=(-1.0, 0.25, 3.0)), 1)
             for layout in ("nhwc", "nchw") for dtype in ("float32", "float16", "bfloat16", "uint8")]
    cases += [(A.AlignedFormat.matcher("float16"), 2), (A.AlignedFormat.matcher("float16"), 4),
              (A.AlignedFormat.matcher("bfloat16"), 4)]
    for fmt, s in cases:
        exp = A.warp_frames_device(data["bgr_d"], m, hd, wd, frame_index_dev=idx, boxes_dev=boxes, samples=s, fmt=fmt)
        got = A.warp_frames_device(data["ring_d"], m, hd, wd, frame_index_dev=idx, boxes_dev=boxes, samples=s, fmt=fmt, src=data["nv"])
        assert got.dtype == fmt.torch_dtype and tuple(got.shape) == fmt.shape(12, hd, wd)
        assert not torch.isnan(exp.float()).any()
        assert torch.equal(got, exp), (fmt, s)
        same = A.warp_frames_device(data["bgr_d"], m, hd, wd, frame_index_dev=idx, boxes_dev=boxes, samples=s, fmt=fmt,
                                    src=A.FrameFormat.bgr())
        assert torch.equal(same, exp), (fmt, s)
    # a destination that is a slice of a larger buffer, aligned to its element only
    fmt = A.AlignedFormat.matcher("float16")
    n = 12 * 3 * hd * wd
    buf = torch.zeros(n + 8, dtype=torch.float16, device="cuda")
    view = buf[1:1 + n].view(12, 3, hd, wd)
    A.warp_frames_device(data["ring_d"], m, hd, wd, frame_index_dev=idx, boxes_dev=boxes, fmt=fmt, src=data["nv"], out=view)
    assert torch.equal(view, A.warp_frames_device(data["bgr_d"], m, hd, wd, frame_index_dev=idx, boxes_dev=boxes, fmt=fmt))
    assert not buf[:1].any() and not buf[1 + n:].any()


# ---- 5. end to end ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_model():
    from flm_amd.networks import LANDMARKS_MODELS
    from flm_amd.weights import synth_fcn8_weights
    model = LANDMARKS_MODELS["fcn_8"](68, input_height=64, input_width=96, dtype="bf16")
    model.load_weights(synth_fcn8_weights(68, seed=2))
    return model


def test_align_frames_from_nv12(mods, data, small_model):
    L, A, P = mods
    faces = [[[6, 5, 38, 40], [30, 2, 70, 44]], [[-4, 10, 30, 46]], [[9, 9, 41, 37]]]
    slots = [2, 0, 1]
    exp = P.align_frames(data["bgr_d"], faces, small_model, out_size=(112, 112), frame_index=slots, samples=2)
    got = P.align_frames(data["ring_d"], faces, small_model, out_size=(112, 112), frame_index=slots, samples=2,
                         frame_format=data["nv"])
    assert len(got) == len(exp) == 4
    for a, b in zip(got, exp):
        assert a.dtype == b.dtype and a.is_cuda and torch.equal(a, b)
    assert exp[0].abs().max() > 0 and (exp[2] >= 0).any()
    # with the matcher's format and the score weights: five tensors, all equal
    fmt = A.AlignedFormat.matcher("float16")
    exp = P.align_frames(data["bgr_d"], faces, small_model, frame_index=slots, weights="score", aligned_format=fmt)
    got = P.align_frames(data["ring_d"], faces, small_model, frame_index=slots, weights="score", aligned_format=fmt,
                         frame_format=data["nv"])
    assert len(got) == len(exp) == 5 and got[0].dtype == torch.float16
    for a, b in zip(got, exp):
        assert torch.equal(a, b)
    # no faces: shapes only
    e = P.align_frames(data["ring_d"], [[], [], []], small_model, out_size=(96, 80), frame_format=data["nv"])
    assert [tuple(t.shape) for t in e[:3]] == [(0, 96, 80, 3), (0, 2, 3), (0, 68, 2)]
    # what the host checks of an NV12 call need a CUDA ring to reach
    with pytest.raises(ValueError):      # slot outside the ring
        P.align_frames(data["ring_d"], faces, small_model, frame_format=data["nv"], frame_index=[0, 1, 3])
    with pytest.raises(ValueError):      # one slot per entry
        P.align_frames(data["ring_d"], faces, small_model, frame_format=data["nv"], frame_index=[0, 1])
    with pytest.raises(ValueError):
        P.align_frames(data["ring_d"], faces, small_model, frame_format=data["nv"], samples=3)
    with pytest.raises(ValueError):
        A.warp_frames_device(data["ring_d"], exp[1], 112, 112, samples=3, src=data["nv"])
    with pytest.raises(ValueError):
        P.crop_frames_device(data["ring_d"], faces, 64, 96, frame_index=[0, 1, 3], frame_format=data["nv"])
