"""CPU-side checks of the frame annotation (flm_frames_annotate, flm_bgr_to_yuv, alignment.FrameAnnotation /
annotate_frames_device, prediction.annotate_frames, FaceTracker.annotate): the symbols, the struct and its defaults, every
argument check answered before any launch (so without a GPU), the Python rejections, the colour conversion against the
restatement, the compiler's metadata of the four kernels, and -- on tests/annotate_ref.py alone -- the contract of
include/flm.h on cases written out by hand and the marks layer against utils.plots.draw_marks."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import flm_amd  # noqa: F401
from flm_amd import _lib, alignment, prediction
from flm_amd.utils import plots

import annotate_ref as aref

NAN, INF = float("nan"), float("inf")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "face-landmark-detector_amd", "csrc")
NAMES = ("flm_annotate_opts_init", "flm_bgr_to_yuv", "flm_frames_annotate")
GREEN = (0, 255, 0)


def test_library_exports_the_calls():
    lib = C.CDLL(_lib.LIB_PATH)
    text = open(os.path.join(ROOT, "include", "flm.h")).read()
    for name in NAMES:
        assert hasattr(lib, name) and name in _lib.EXPORTS, name
        assert re.search(r"\b%s\(" % name, text), name                 # header and EXPORTS agree
    L = _lib.load()
    assert L.flm_abi_version() == 2 and "#define FLM_ABI_VERSION 2" in text          # purely additive
    proto = re.search(r"int flm_frames_annotate\((.*?)\);", text, re.S).group(1)
    assert len(re.sub(r"/\*.*?\*/", "", proto, flags=re.S).split(",")) == len(L.flm_frames_annotate.argtypes) == 14
    o = _lib.AnnotateOpts.make()
    assert o.struct_size == C.sizeof(_lib.AnnotateOpts) == 56
    assert (o.marks, o.box, o.redact) == (1, 0, 0) and list(o.margin) == [0.1, 0.35, 0.1, 0.1]
    assert tuple(o.mark_bgr) == GREEN and tuple(o.box_bgr) == GREEN and tuple(o.reserved) == (0, 0)
    assert bytes(alignment.FrameAnnotation().struct()) == bytes(o)     # the C default is FrameAnnotation's, to the bit
    assert tuple(aref.DEFAULT_MARGIN) == (0.1, 0.35, 0.1, 0.1)
    junk = _lib.AnnotateOpts()
    C.memset(C.byref(junk), 0xA5, C.sizeof(junk))
    L.flm_annotate_opts_init(C.byref(junk))
    assert bytes(junk) == bytes(o)                                     # init writes every byte, the padding included
    L.flm_annotate_opts_init(None)                                     # tolerated, as the other *_init calls


err = lambda: _lib.load().flm_last_error().decode()
ORDER = ("frames", "frame_stride", "nframes", "fh", "fw", "src", "frame_idx", "lm", "lm_stride", "k", "c", "opts", "regions")
FAKE = dict(frames=C.c_void_p(1 << 30), frame_idx=C.c_void_p(2 << 30), lm=C.c_void_p(3 << 30), regions=C.c_void_p(4 << 30))
WHO = "flm_frames_annotate"


def _call(**kw):
    """Never dereferenced: every call here is rejected before a launch.  The defaults are a valid BGR call on a ring of 3
    frames of 48x64."""
    a = dict(FAKE, frame_stride=48 * 64 * 3, nframes=3, fh=48, fw=64, src=None, lm_stride=2, k=5, c=68, opts=None)
    a.update(kw)
    for key in ("src", "opts"):
        if isinstance(a[key], C.Structure):
            a[key] = C.byref(a[key])
    return _lib.load().flm_frames_annotate(None, *[a[n] for n in ORDER])


def _opts(**kw):
    o = _lib.AnnotateOpts.make()
    for k, v in kw.items():
        if k == "margin":
            for i, m in enumerate(v):
                o.margin[i] = m
        else:
            setattr(o, k, v)
    return o


def _nv12(fw=64, fh=48, pitch=80, uv_row=50, matrix=0, **kw):
    f = _lib.FrameFormat()
    f.struct_size, f.pixel, f.matrix = C.sizeof(f), _lib.FRAME_NV12, matrix
    f.y_pitch, f.uv_pitch, f.uv_offset = pitch, pitch, uv_row * pitch
    for k, v in kw.items():
        setattr(f, k, v)
    return f


def test_argument_checks_answer_without_a_gpu():
    passes = lambda **kw: _call(frame_stride=0, **kw) == -2 and "frame_stride" in err() and WHO in err()
    assert passes()                                                    # the sentinel: everything before the stride holds
    for name in ("frames", "lm", "regions"):
        assert _call(**{name: None}) == -1 and "null" in err() and WHO in err(), name
    assert passes(frame_idx=None) and passes(opts=_opts()) and passes(src=_nv12())
    # the options: FLM_ERR_ARG, before the sizes
    assert _call(opts=_opts(struct_size=48)) == -1 and "struct_size" in err() and WHO in err()
    for bad in (-1, 2, 2 ** 31 - 1):
        assert _call(opts=_opts(marks=bad), k=0) == -1 and "marks" in err() and WHO in err(), bad
    for bad in (-1, 17, 2 ** 31 - 1):
        assert _call(opts=_opts(box=bad), k=0) == -1 and "box" in err() and "<= 16" in err(), bad
    for bad in (-2, 1, 3, 63, 65, 66, 2 ** 31 - 1):
        assert _call(opts=_opts(redact=bad), k=0) == -1 and "redact" in err() and "even" in err(), bad
    for i in range(4):
        for bad in (NAN, -1e-9, 4.000001, INF, -INF):
            m = [0.1, 0.35, 0.1, 0.1]
            m[i] = bad
            assert _call(opts=_opts(margin=m), k=0) == -1 and "margin[%d]" % i in err() and WHO in err(), (i, bad)
    for good in (dict(marks=0), dict(box=16), dict(redact=2), dict(redact=64), dict(margin=[0.0, 4.0, 0.0, 4.0]),
                 dict(marks=0, box=0, redact=0)):
        assert passes(opts=_opts(**good)), good
    # the frame format: unknown values are FLM_ERR_ARG
    assert _call(src=_nv12(struct_size=8)) == -1 and "struct_size" in err() and WHO in err()
    assert _call(src=_nv12(pixel=2)) == -1 and "pixel" in err()
    assert _call(src=_nv12(matrix=2)) == -1 and "matrix" in err()
    # the sizes: FLM_ERR_SHAPE, the limit named
    for k in (0, -1, 65536, 2 ** 31 - 1):
        assert _call(k=k) == -2 and "1 <= k <= 65535" in err() and WHO in err(), k
    assert passes(k=65535) and passes(k=4096, opts=_opts(redact=8)) and passes(k=4097)
    for k in (4097, 65535):
        assert _call(k=k, opts=_opts(redact=8)) == -2 and "k <= 4096" in err() and WHO in err(), k
    for c in (0, -1, 1025):
        assert _call(c=c) == -2 and "1 <= c <= 1024" in err() and WHO in err(), c
    assert passes(c=1) and passes(c=1024)
    for s in (0, 1):
        assert _call(lm_stride=s) == -2 and "lm_stride >= 2" in err() and WHO in err(), s
    assert passes(lm_stride=6)
    # the frame geometry of flm_warp_affine_frames_src, BGR24 ...
    assert _call(nframes=0) == -2 and "nframes >= 1" in err() and WHO in err()
    assert _call(fh=0) == -2 and "fh >= 1 and fw >= 2" in err()
    assert _call(fw=1, frame_stride=1 << 20) == -2 and "fh >= 1 and fw >= 2" in err()
    assert _call(fh=32768, fw=32768, frame_stride=1 << 40) == -2 and "fh*fw*3 < 2^31" in err()
    assert _call(frame_stride=48 * 64 * 3 - 1) == -2 and "frame_stride >= fh*fw*3" in err()
    bgr_pitch = _nv12(pixel=_lib.FRAME_BGR24)
    assert _call(src=bgr_pitch) == -2 and "dense" in err() and WHO in err()
    assert _call(src=bgr_pitch, opts=_opts(box=17)) == -1              # an option out of range comes first
    # ... and NV12
    nv = lambda **kw: _call(**dict(dict(src=_nv12(), frame_stride=62 * 80), **kw))
    assert nv(frame_stride=0) == -2 and "frame_stride" in err()
    assert nv(frame_stride=50 * 80 + 23 * 80 + 64 - 1) == -2 and "flm_frame_format_bytes" in err()
    assert nv(frame_stride=0, fh=47) == -2 and "even" in err() and nv(fw=63) == -2 and "even" in err()
    assert nv(src=_nv12(pitch=62)) == -2 and "y_pitch" in err()
    assert nv(src=_nv12(uv_pitch=62)) == -2 and "uv_pitch" in err()
    assert nv(src=_nv12(uv_row=47)) == -2 and "uv_offset" in err()
    assert nv(nframes=0) == -2 and "nframes" in err()


def test_bgr_to_yuv_matches_the_restatement():
    lib = _lib.load()
    assert aref.yuv_coefficients("bt601") == [[6416, 33039, 16829], [28784, -19071, -9714], [-4681, -24103, 28784]]
    assert aref.yuv_coefficients("bt709") == [[4064, 40254, 11966], [28784, -22189, -6596], [-2639, -26145, 28784]]
    text = open(os.path.join(ROOT, "include", "flm.h")).read()
    for matrix in ("bt601", "bt709"):                                  # the header quotes the same numbers
        for row in aref.yuv_coefficients(matrix):
            assert "(%d, %d, %d)" % tuple(row) in text, (matrix, row)
    rng = np.random.default_rng(7)
    corners = np.array([[b, g, r] for b in (0, 255) for g in (0, 255) for r in (0, 255)], np.uint8)
    colours = np.concatenate([corners, rng.integers(0, 256, (4000, 3), dtype=np.uint8)])
    for code, matrix in ((_lib.YUV_BT601_LIMITED, "bt601"), (_lib.YUV_BT709_LIMITED, "bt709")):
        want = aref.bgr_to_yuv(colours, matrix)
        got = np.zeros_like(colours)
        for i, col in enumerate(colours):
            src, dst = (C.c_uint8 * 3)(*col.tolist()), (C.c_uint8 * 3)()
            assert lib.flm_bgr_to_yuv(code, src, dst) == 0
            got[i] = list(dst)
        assert np.array_equal(got, want), matrix
        assert want[0].tolist() == [16, 128, 128] and want[7].tolist() == [235, 128, 128], matrix     # black and white
        assert want[:, 0].min() >= 16 and want[:, 0].max() <= 235 and want[:, 1:].min() >= 16 and want[:, 1:].max() <= 240
    assert aref.bgr_to_yuv(np.array(GREEN, np.uint8), "bt601").tolist() == [145, 54, 34]     # the well-known green
    px = (C.c_uint8 * 3)()
    assert lib.flm_bgr_to_yuv(2, px, px) == -1 and "matrix" in err()
    assert lib.flm_bgr_to_yuv(0, None, px) == -1 and lib.flm_bgr_to_yuv(0, px, None) == -1 and "null" in err()


# ---- the Python rejections ---------------------------------------------------------------------------------------------
def test_frame_annotation_validates_its_options():
    a = alignment.FrameAnnotation()
    assert (a.marks, a.box, a.redact, a.margin, a.mark_color, a.box_color) == (True, 0, 0, (0.1, 0.35, 0.1, 0.1), GREEN, GREEN)
    a = alignment.FrameAnnotation(marks=False, box=16, redact=64, margin=[0, 4, 0.5, 1], mark_color=[1, 2, 3], box_color=(255, 0, 9))
    s = a.struct()
    assert (s.marks, s.box, s.redact, list(s.margin), tuple(s.mark_bgr), tuple(s.box_bgr)) == \
        (0, 16, 64, [0.0, 4.0, 0.5, 1.0], (1, 2, 3), (255, 0, 9))
    assert "redact=64" in repr(a)
    assert "measured" in alignment.FrameAnnotation.__doc__             # the margins are guesses, and the docstring says so
    for bad in (dict(marks=1), dict(marks=None), dict(box=-1), dict(box=17), dict(box=1.0), dict(box=True), dict(redact=1),
                dict(redact=3), dict(redact=66), dict(redact=-2), dict(redact="8"), dict(margin=(0.1, 0.1, 0.1)),
                dict(margin=(0.1, 0.1, 0.1, NAN)), dict(margin=(0.1, 0.1, 0.1, -0.1)), dict(margin=(4.1, 0, 0, 0)),
                dict(margin=0.1), dict(margin=("a", 0, 0, 0)), dict(mark_color=(0, 256, 0)), dict(mark_color=(0, 0)),
                dict(box_color=(0, -1, 0)), dict(box_color=(0.5, 0, 0)), dict(box_color=7)):
        with pytest.raises(ValueError):
            alignment.FrameAnnotation(**bad)


class _Model:
    n_classes, input_height, input_width, output_height, output_width = 68, 64, 64, 72, 72
    max_batch = 1024


def test_wrappers_reject_what_they_must_on_the_host():
    ring = torch.zeros((2, 8, 8, 3), dtype=torch.uint8)
    lm = torch.zeros((3, 5, 2), dtype=torch.float64)
    with pytest.raises(ValueError, match="opts must be None or a FrameAnnotation"):
        alignment.annotate_frames_device(ring, lm, opts=dict(box=1))
    with pytest.raises(ValueError, match="frame format"):
        alignment.annotate_frames_device(ring, lm, src="nv12")
    with pytest.raises(ValueError, match="frames must be a contiguous CUDA uint8"):          # (not on the device)
        alignment.annotate_frames_device(ring, lm)
    with pytest.raises(ValueError, match="NV12 ring"):
        alignment.annotate_frames_device(ring, lm, src=alignment.FrameFormat.nv12(8, 8))
    with pytest.raises(ValueError, match="redact"):
        prediction.annotate_frames(ring, lm, redact=5)
    with pytest.raises(ValueError, match="frame_format"):
        prediction.annotate_frames(ring, lm, frame_format="bgr")
    with pytest.raises(TypeError):
        prediction.annotate_frames(ring, lm, colour=GREEN)
    with pytest.raises(ValueError, match="landmarks must be a CUDA"):
        prediction.annotate_frames(ring, lm, frame_index=[0, 1, 1])
    # the tracker's method: a new method, the constructor is as it was
    assert list(inspect.signature(prediction.FaceTracker.__init__).parameters)[-2:] == ["exits", "views"]
    assert list(inspect.signature(prediction.FaceTracker.annotate).parameters) == ["self", "ring", "landmarks", "frame_index",
                                                                                  "annotation"]
    tr = prediction.FaceTracker(_Model(), (8, 8), 3)
    with pytest.raises(ValueError, match="annotation must be None or an alignment.FrameAnnotation"):
        tr.annotate(ring, lm, annotation=dict(box=1))
    with pytest.raises(ValueError, match="frames must be a contiguous CUDA uint8"):
        tr.annotate(ring, lm)
    for doc in (prediction.FaceTracker.annotate.__doc__,):
        assert "step_active" in doc and "WRITES" in doc and "frames_to_bgr_device" in doc and "set_sync_debug_mode" in doc


# ---- the restatement against cases written out by hand -----------------------------------------------------------------
def _changed(a, b):
    """The (x, y) of the pixels of two [H,W,3] frames that differ."""
    ys, xs = np.nonzero((a != b).any(-1))
    return sorted(zip(xs.tolist(), ys.tolist()))


def test_the_restatement_on_one_landmark():
    frames = np.full((1, 12, 16, 3), 7, np.uint8)
    lm = np.array([[[5.9, 4.2]]])
    out, reg = aref.annotate_bgr(frames, lm)
    assert reg.tolist() == [[5, 4, 7, 6]]                              # floor, and ceil + 1; side = 0: the margins add nothing
    disc = sorted((5 + dx, 4 + dy) for dx, dy in [(-1, -2), (0, -2), (1, -2), (-1, 2), (0, 2), (1, 2)] +
                  [(dx, dy) for dy in (-1, 0, 1) for dx in range(-2, 3)])
    assert len(disc) == 21 and _changed(out[0], frames[0]) == disc and (out[0, 4, 5] == GREEN).all()
    # at the corner the disc is clipped to 3 + 3 + 2 pixels ... and just past the frame the face takes no part at all
    out, reg = aref.annotate_bgr(frames, np.array([[[15.0, 11.0]]]))
    assert reg.tolist() == [[15, 11, 16, 12]] and len(_changed(out[0], frames[0])) == 8
    out, reg = aref.annotate_bgr(frames, np.array([[[16.0, 5.0]]]))
    assert reg.tolist() == [[16, 5, 17, 6]] and np.array_equal(out, frames)
    # the box of one landmark: t = 1 paints R itself (2 x 2 here); nothing with every layer off; a rejected point is no face
    out, _ = aref.annotate_bgr(frames, lm, marks=0, box=1, box_bgr=(9, 8, 7))
    assert _changed(out[0], frames[0]) == [(5, 4), (5, 5), (6, 4), (6, 5)] and out[0, 5, 6].tolist() == [9, 8, 7]
    out, reg = aref.annotate_bgr(frames, lm, marks=0)
    assert np.array_equal(out, frames) and reg.tolist() == [[5, 4, 7, 6]]
    for bad in ((-1.0, -1.0), (NAN, 3.0), (3.0, INF), (2.0 ** 30 + 1, 3.0)):
        out, reg = aref.annotate_bgr(frames, np.array([[bad]]), box=2, redact=2)
        assert reg.tolist() == [[0, 0, 0, 0]] and np.array_equal(out, frames), bad
    # a frame index outside the ring: the region is still reported
    for fi in (-1, 1):
        out, reg = aref.annotate_bgr(frames, lm, frame_idx=[fi], box=1, redact=2)
        assert reg.tolist() == [[5, 4, 7, 6]] and np.array_equal(out, frames)


def test_the_restatement_on_a_face_half_outside_the_frame():
    frames = np.zeros((1, 8, 8, 3), np.uint8)
    lm = np.array([[[0.0, 2.0], [3.0, 5.0], [-1.0, -1.0]]])
    out, reg = aref.annotate_bgr(frames, lm, marks=0, box=1, margin=(1.0, 0.0, 0.0, 0.0), box_bgr=(1, 2, 3))
    assert reg.tolist() == [[-3, 2, 4, 6]]                             # side = 3: the left margin reaches past the border
    want = sorted({(x, 2) for x in range(4)} | {(x, 5) for x in range(4)} | {(3, y) for y in range(2, 6)})
    assert _changed(out[0], frames[0]) == want                         # top, bottom and right edge; no edge along the border
    # t = 16 is thicker than half the region: it fills P
    out, _ = aref.annotate_bgr(frames, lm, marks=0, box=16, margin=(1.0, 0.0, 0.0, 0.0))
    assert _changed(out[0], frames[0]) == sorted((x, y) for x in range(4) for y in range(2, 6))


def test_the_restatement_on_two_faces_sharing_cells():
    rng = np.random.default_rng(3)
    frames = rng.integers(0, 256, (2, 8, 10, 3), dtype=np.uint8)
    lm = np.array([[[1.0, 1.0], [2.0, 2.0]], [[3.0, 3.0], [5.0, 5.0]], [[1.0, 1.0], [2.0, 2.0]]])
    out, reg = aref.annotate_bgr(frames, lm, frame_idx=[0, 0, 1], marks=0, redact=4, margin=(0, 0, 0, 0))
    assert reg.tolist() == [[1, 1, 3, 3], [3, 3, 6, 6], [1, 1, 3, 3]]
    want = frames.copy()
    mean = lambda blk: (blk.astype(np.int64).sum((0, 1)) + (blk.shape[0] * blk.shape[1] >> 1)) // (blk.shape[0] * blk.shape[1])
    for cy in (0, 1):
        for cx in (0, 1):                                              # the four cells of slot 0, each ONCE from the original
            want[0, 4 * cy:4 * cy + 4, 4 * cx:4 * cx + 4] = mean(frames[0, 4 * cy:4 * cy + 4, 4 * cx:4 * cx + 4])
    want[1, 0:4, 0:4] = mean(frames[1, 0:4, 0:4])                      # the same pixels named in another slot: that slot alone
    assert np.array_equal(out, want)
    # in any order of the faces
    out2, _ = aref.annotate_bgr(frames, lm[::-1], frame_idx=[1, 0, 0], marks=0, redact=4, margin=(0, 0, 0, 0))
    assert np.array_equal(out2, want)
    # a cell at the frame's edge is narrower: columns 8..9
    out, _ = aref.annotate_bgr(frames, np.array([[[9.0, 7.0]]]), marks=0, redact=4)
    want = frames.copy()
    want[0, 4:8, 8:10] = mean(frames[0, 4:8, 8:10])
    assert np.array_equal(out, want)
    # the layers in order: the outline over the mosaic, the marks over both
    out, reg = aref.annotate_bgr(frames, np.array([[[1.0, 1.0], [6.0, 6.0]]]), box=1, redact=4, margin=(0, 0, 0, 0),
                                 box_bgr=(1, 1, 1), mark_bgr=(2, 2, 2))
    assert reg.tolist() == [[1, 1, 7, 7]]
    assert out[0, 1, 1].tolist() == [2, 2, 2] and out[0, 1, 4].tolist() == [1, 1, 1]       # a mark; the top edge beside it
    assert out[0, 3, 4].tolist() == mean(frames[0, 0:4, 4:8]).tolist()                     # inside: the cell's mean


def test_the_restatement_on_an_odd_region_on_nv12():
    fh, fw, pitch, uv_row, rows = 8, 8, 10, 9, 13
    rng = np.random.default_rng(5)
    ring = rng.integers(0, 256, (1, rows, pitch), dtype=np.uint8)
    lm = np.array([[[3.5, 3.5]]])
    y, u, v = 145, 54, 34                                              # green, BT.601
    out, reg = aref.annotate_nv12(ring, fh, fw, uv_row, "bt601", lm, marks=0, box=1)
    assert reg.tolist() == [[3, 3, 5, 5]]
    want = ring.copy()
    want[0, 3:5, 3:5] = y                                              # four pixels with odd corners ...
    for row in (uv_row + 1, uv_row + 2):                               # ... lie in four 2x2 blocks: the pairs at columns 2 and 4
        want[0, row, 2:6] = [u, v, u, v]
    assert np.array_equal(out, want)
    # the mosaic of the same region, s = 2: four luma cells, each chroma sample its own mean (m = 1): unchanged
    out, _ = aref.annotate_nv12(ring, fh, fw, uv_row, "bt601", lm, marks=0, redact=2)
    want = ring.copy()
    for cy in (1, 2):
        for cx in (1, 2):
            want[0, 2 * cy:2 * cy + 2, 2 * cx:2 * cx + 2] = (int(ring[0, 2 * cy:2 * cy + 2, 2 * cx:2 * cx + 2].astype(int).sum()) + 2) // 4
    assert np.array_equal(out, want)
    # s = 4: one U and one V mean over the 2 x 2 samples under the cell
    out, _ = aref.annotate_nv12(ring, fh, fw, uv_row, "bt601", np.array([[[1.0, 1.0]]]), marks=0, redact=4)
    want = ring.copy()
    want[0, 0:4, 0:4] = (int(ring[0, 0:4, 0:4].astype(int).sum()) + 8) // 16
    uv = ring[0, uv_row:uv_row + 2, 0:4].astype(int)
    want[0, uv_row:uv_row + 2, 0:4:2] = (uv[:, 0::2].sum() + 2) // 4
    want[0, uv_row:uv_row + 2, 1:4:2] = (uv[:, 1::2].sum() + 2) // 4
    assert np.array_equal(out, want)
    # nothing outside the two planes' fw columns ever changes: the padding, the row between the planes, the rows after
    out, _ = aref.annotate_nv12(ring, fh, fw, uv_row, "bt709", np.array([[[0.0, 0.0], [7.0, 7.0]]]), box=3, redact=2, margin=(4, 4, 4, 4))
    assert np.array_equal(out[0, :, fw:], ring[0, :, fw:]) and np.array_equal(out[0, fh:uv_row], ring[0, fh:uv_row])
    assert np.array_equal(out[0, uv_row + fh // 2:], ring[0, uv_row + fh // 2:]) and not np.array_equal(out, ring)


def test_the_marks_layer_is_draw_marks():
    rng = np.random.default_rng(11)
    frames = rng.integers(0, 256, (1, 48, 64, 3), dtype=np.uint8)
    marks = np.stack([rng.integers(0, 64, 68), rng.integers(0, 48, 68)], -1).astype(np.float64)
    marks[:4] = [[0, 0], [63, 47], [63, 0], [0, 47]]                   # the corners: clipped discs
    for colour in (GREEN, (255, 0, 128)):
        out, _ = aref.annotate_bgr(frames, marks[None], mark_bgr=colour)
        assert np.array_equal(out[0], plots.draw_marks(frames[0].copy(), marks, color=colour))
    assert sorted(aref.DISC) == sorted(plots._DISC2)


# ---- the compiler's metadata of the kernels this feature adds -----------------------------------------------------------
def test_the_new_kernels_compile_for_gfx950_without_scratch(tmp_path):
    out = os.path.join(str(tmp_path), "flm_annotate.s")
    cmd = ["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
           "-I", CSRC, "-S", "--cuda-device-only", os.path.join(CSRC, "flm_annotate.hip"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    md = {}
    for block in open(out).read().split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        md[name] = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\n", block)}
    for want in ("annotate_regions_kernel", "annotate_mosaic_kernel", "annotate_outline_kernel", "annotate_marks_kernel"):
        assert len([n for n in md if want in n]) == 1, (want, sorted(md))
    assert len(md) == 4, sorted(md)                                    # at most four launches, one kernel each
    for name, k in md.items():
        print(name, {f: k[f] for f in ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")})
        assert k["private_segment_fixed_size"] == 0 and k["wavefront_size"] == 64, (name, k)
        lds = 4096 * 2 + 4 if "mosaic" in name else 0                  # the list of the faces that share cells, and its count
        assert k["group_segment_fixed_size"] == lds, (name, k)
        assert k["vgpr_count"] <= 64, (name, k)                        # eight waves per SIMD
    text = "".join(open(os.path.join(CSRC, f)).read() for f in ("flm_annotate.hip", "flm_annotate_dev.h"))
    assert "atomic" not in text.replace("no atomics", "").replace("without atomics", "")
    assert "hipMalloc" not in text and "Synchronize" not in text
    from flm_amd import build
    assert "flm_annotate.hip" in build.SOURCES
