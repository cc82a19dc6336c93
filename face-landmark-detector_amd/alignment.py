"""Face alignment: similarity transform from predicted landmarks + bilinear warp, on the device.

The reference states the intent ("predict landmark and align face for Face Match",
README.md:1) but contains no alignment code; this is build-defined (SURVEY.md section 8 row
A8).  The warp follows the shape of the reference's only affine warp
(`skimage.transform.warp(im, tform, mode="edge")`, data/generator.py:192-200): inverse map,
bilinear, edge clamp -- but keeps pixel units (no [0,1] rescale) and float32.
"""
from __future__ import annotations

import math

import numpy as np

from . import _lib


def canonical_template(n_landmarks: int, out_h: int, out_w: int) -> np.ndarray:
    """Deterministic canonical landmark layout, float64 [K,2] (x,y) in output pixels.

    68 landmarks: the iBUG-68 ordering laid out procedurally (jaw 0-16, brows 17-26, nose
    27-35, eyes 36-47, mouth 48-67) inside the unit square; other counts: a centred ellipse.
    No trained model exists for the reference (README.md:4-7), so the template only has to be
    a fixed, well-conditioned target for the similarity fit.
    """
    k = int(n_landmarks)
    pts = np.zeros((k, 2), np.float64)
    if k == 68:
        t = np.linspace(np.pi * 1.05, np.pi * 1.95, 17)       # jaw: lower arc, left to right
        pts[0:17] = np.stack([0.5 + 0.42 * np.cos(t), 0.42 - 0.48 * np.sin(t)], 1)
        pts[17:22] = np.stack([np.linspace(0.18, 0.42, 5), 0.30 - 0.03 * np.sin(np.linspace(0, np.pi, 5))], 1)
        pts[22:27] = np.stack([np.linspace(0.58, 0.82, 5), 0.30 - 0.03 * np.sin(np.linspace(0, np.pi, 5))], 1)
        pts[27:31] = np.stack([np.full(4, 0.5), np.linspace(0.38, 0.56, 4)], 1)
        pts[31:36] = np.stack([np.linspace(0.42, 0.58, 5), 0.62 + 0.015 * np.sin(np.linspace(0, np.pi, 5))], 1)
        for base, cx in ((36, 0.31), (42, 0.69)):
            a = np.linspace(np.pi, -np.pi, 7)[:6]
            pts[base:base + 6] = np.stack([cx + 0.07 * np.cos(a), 0.40 - 0.03 * np.sin(a)], 1)
        a = np.linspace(np.pi, -np.pi, 13)[:12]
        pts[48:60] = np.stack([0.5 + 0.13 * np.cos(a), 0.76 - 0.06 * np.sin(a)], 1)
        a = np.linspace(np.pi, -np.pi, 9)[:8]
        pts[60:68] = np.stack([0.5 + 0.08 * np.cos(a), 0.76 - 0.025 * np.sin(a)], 1)
    else:
        a = np.linspace(0, 2 * np.pi, k, endpoint=False)
        pts = np.stack([0.5 + 0.35 * np.cos(a), 0.5 + 0.40 * np.sin(a)], 1)
    return pts * np.array([out_w - 1, out_h - 1], np.float64)


class AlignedFormat:
    """What the aligned faces look like when they leave the warp (flm_image_format, include/flm.h): the conversion runs
    in the warp's own store, so no float32 [N,h,w,3] copy exists and no launch follows.

    layout   "nhwc" [N,h,w,3] or "nchw" [N,3,h,w], dense
    dtype    "float32", "float16", "bfloat16" or "uint8" (a torch or numpy dtype of those names does too)
    channels "bgr": output channel c is source channel c (the sources of this package are BGR throughout);
             "rgb": output channel c is source channel 2-c
    scale, bias  three numbers each, by OUTPUT channel (one number: all three): stored = convert(v * scale + bias), a
             float32 multiply, then a float32 add, then the rounding the header states per type (float16 / bfloat16:
             nearest even; uint8: rint, clamped to [0,255]).

    The defaults are the format the warps have without one: float32 NHWC BGR, scale 1, bias 0."""
    _LAYOUTS = {"nhwc": _lib.LAYOUT_NHWC, "nchw": _lib.LAYOUT_NCHW}
    _DTYPES = {"float32": _lib.PIX_F32, "float16": _lib.PIX_F16, "bfloat16": _lib.PIX_BF16, "uint8": _lib.PIX_U8}
    _ITEMSIZE = {"float32": 4, "float16": 2, "bfloat16": 2, "uint8": 1}

    def __init__(self, layout="nhwc", dtype="float32", channels="bgr", scale=(1.0, 1.0, 1.0), bias=(0.0, 0.0, 0.0)):
        if not isinstance(layout, str) or layout.lower() not in self._LAYOUTS:
            raise ValueError("layout must be \"nhwc\" or \"nchw\" (got %r)" % (layout,))
        if isinstance(dtype, str):
            name = dtype
        else:
            try:
                name = np.dtype(dtype).name
            except TypeError:   # a torch dtype
                name = str(dtype)
        name = name.lower().replace("torch.", "")
        if name not in self._DTYPES:
            raise ValueError("dtype must be one of %s (got %r)" % (", ".join(sorted(self._DTYPES)), dtype))
        if not isinstance(channels, str) or channels.lower() not in ("bgr", "rgb"):
            raise ValueError("channels must be \"bgr\" or \"rgb\" (got %r)" % (channels,))
        self.layout = layout.lower()
        self.dtype = name
        self.channels = channels.lower()
        self.scale = self._triple("scale", scale)
        self.bias = self._triple("bias", bias)

    @staticmethod
    def _triple(what, v):
        if isinstance(v, (int, float)) and not isinstance(v, bool):
            v = (v, v, v)
        try:
            vals = tuple(float(x) for x in v)
        except (TypeError, ValueError):
            raise ValueError("%s must be three numbers (got %r)" % (what, v))
        if len(vals) != 3:
            raise ValueError("%s must have one value per channel, three in all (got %d)" % (what, len(vals)))
        # the C struct holds float32: a value that is finite only in float64 is not a scale the kernel can apply
        with np.errstate(over="ignore"):
            if not all(np.isfinite(np.float32(x)) for x in vals):
                raise ValueError("%s must be finite in float32 (got %r)" % (what, vals))
        return vals

    @classmethod
    def matcher(cls, dtype="float16"):
        """What face-embedding networks take: planar [N,3,h,w], RGB, (x - 127.5) / 127.5 written as x * (1/127.5) - 1."""
        return cls("nchw", dtype, "rgb", (1.0 / 127.5,) * 3, (-1.0,) * 3)

    @property
    def torch_dtype(self):
        import torch
        return getattr(torch, self.dtype)

    @property
    def numpy_dtype(self):
        """The numpy type of the same bits, None for bfloat16 (numpy has none)."""
        return None if self.dtype == "bfloat16" else np.dtype(self.dtype)

    @property
    def itemsize(self):
        return self._ITEMSIZE[self.dtype]

    def shape(self, n, h, w):
        n, h, w = int(n), int(h), int(w)
        return (n, h, w, 3) if self.layout == "nhwc" else (n, 3, h, w)

    def nbytes(self, n, h, w):
        return int(n) * int(h) * int(w) * 3 * self.itemsize

    def struct(self):
        """The flm_image_format of this format (struct_size set, as flm_image_format_init sets it)."""
        f = _lib.ImageFormat()
        f.struct_size = _lib.C.sizeof(_lib.ImageFormat)
        f.layout = self._LAYOUTS[self.layout]
        f.type = self._DTYPES[self.dtype]
        f.reverse_channels = int(self.channels == "rgb")
        for c in range(3):
            f.scale[c] = self.scale[c]
            f.bias[c] = self.bias[c]
        return f

    def key(self):
        return (self.layout, self.dtype, self.channels, self.scale, self.bias)

    def __eq__(self, other):
        return isinstance(other, AlignedFormat) and self.key() == other.key()

    def __hash__(self):
        return hash(self.key())

    def __repr__(self):
        return "AlignedFormat(layout=%r, dtype=%r, channels=%r, scale=%r, bias=%r)" % self.key()


class FrameFormat:
    """How a ring slot holds its pixels (flm_frame_format, include/flm.h): what the frame-reading calls take as
    `frame_format=` / `src=`.

    FrameFormat.bgr()   the dense ring of today: one contiguous CUDA uint8 [F,H,W,3] tensor.
    FrameFormat.nv12(height, width, matrix="bt601", uv_row=None)
                        a decoder's NV12 surfaces: one contiguous CUDA uint8 [F,rows,pitch] tensor.  Luma is rows
                        0..height-1 of a slot, the interleaved U,V rows start at row `uv_row` (default `height`), both
                        planes use the tensor's pitch, and a slot is rows*pitch bytes.  `matrix`: "bt601" or "bt709",
                        limited range (what the decoder tags; 1080p streams are BT.709).
    The kernels convert a tap with the integer arithmetic the header states and then compute what the BGR calls compute:
    the results have the bits of those calls on `prediction.frames_to_bgr_device(frames, frame_format)`."""
    _MATRICES = {"bt601": _lib.YUV_BT601_LIMITED, "bt709": _lib.YUV_BT709_LIMITED}

    def __init__(self, pixel="bgr", height=None, width=None, matrix="bt601", uv_row=None):
        if pixel not in ("bgr", "nv12"):
            raise ValueError("pixel must be \"bgr\" or \"nv12\" (got %r)" % (pixel,))
        if not isinstance(matrix, str) or matrix.lower() not in self._MATRICES:
            raise ValueError("matrix must be \"bt601\" or \"bt709\" (got %r)" % (matrix,))
        self.pixel = pixel
        self.matrix = matrix.lower()
        self.height = self.width = self.uv_row = None
        if pixel == "nv12":
            height, width = int(height), int(width)
            if height < 2 or width < 2 or height % 2 or width % 2:
                raise ValueError("NV12 frames have even sizes of 2 or more (got %dx%d)" % (height, width))
            uv_row = height if uv_row is None else int(uv_row)
            if uv_row < height:
                raise ValueError("uv_row=%d lies inside the %d luma rows" % (uv_row, height))
            self.height, self.width, self.uv_row = height, width, uv_row

    @classmethod
    def bgr(cls):
        return cls("bgr")

    @classmethod
    def nv12(cls, height, width, matrix="bt601", uv_row=None):
        return cls("nv12", height, width, matrix, uv_row)

    def ring(self, frames):
        """(slots, frame height, frame width, bytes between slots) of the ring tensor `frames`; ValueError for a tensor
        that is not a ring of this format (a list of frames, the wrong rank or type, too few rows, too short a pitch)."""
        import torch
        if self.pixel == "bgr":
            if (not isinstance(frames, torch.Tensor) or frames.dim() != 4 or frames.shape[3] != 3
                    or frames.dtype != torch.uint8 or not frames.is_cuda or not frames.is_contiguous()):
                raise ValueError("frames must be a contiguous CUDA uint8 [F,H,W,3] tensor")
            nf, fh, fw = [int(v) for v in frames.shape[:3]]
            return nf, fh, fw, fh * fw * 3
        if not isinstance(frames, torch.Tensor) or frames.dim() != 3 or frames.dtype != torch.uint8:
            raise ValueError("an NV12 ring is one uint8 [F,rows,pitch] tensor (got %s)" % (
                "a %s" % type(frames).__name__ if not isinstance(frames, torch.Tensor) else
                "%s %s" % (frames.dtype, list(frames.shape))))
        nf, rows, pitch = [int(v) for v in frames.shape]
        if pitch < self.width:
            raise ValueError("the ring's pitch of %d bytes is shorter than the frame width %d" % (pitch, self.width))
        if rows < self.uv_row + self.height // 2:
            raise ValueError("a slot of %d rows does not hold %d U,V rows from row %d" % (rows, self.height // 2, self.uv_row))
        if rows * pitch >= 2 ** 31:
            raise ValueError("a slot of %d bytes is outside the kernels' reach (< 2^31)" % (rows * pitch))
        if not frames.is_cuda or not frames.is_contiguous():
            raise ValueError("frames must be a contiguous CUDA tensor")
        return nf, self.height, self.width, rows * pitch

    def struct(self, frames=None):
        """The flm_frame_format of this format for the ring tensor `frames` (its pitch)."""
        f = _lib.FrameFormat()
        f.struct_size = _lib.C.sizeof(_lib.FrameFormat)
        f.matrix = self._MATRICES[self.matrix]
        if self.pixel == "bgr":
            f.pixel = _lib.FRAME_BGR24
            return f
        pitch = int(frames.shape[2])
        f.pixel = _lib.FRAME_NV12
        f.y_pitch = pitch
        f.uv_pitch = pitch
        f.uv_offset = self.uv_row * pitch
        return f

    def key(self):
        return (self.pixel, self.height, self.width, self.matrix, self.uv_row)

    def __eq__(self, other):
        return isinstance(other, FrameFormat) and self.key() == other.key()

    def __hash__(self):
        return hash(self.key())

    def __repr__(self):
        if self.pixel == "bgr":
            return "FrameFormat.bgr()"
        return "FrameFormat.nv12(%d, %d, matrix=%r, uv_row=%d)" % (self.height, self.width, self.matrix, self.uv_row)


def _check_frame_format(src):
    if not isinstance(src, FrameFormat):
        raise ValueError("the frame format must be an alignment.FrameFormat or None (got %r)" % (src,))


def _check_format(fmt):
    if not isinstance(fmt, AlignedFormat):
        raise ValueError("fmt must be an alignment.AlignedFormat or None (got %r)" % (fmt,))


def _format_out(fmt, out, n, h, w, device):
    """The destination of a formatted warp: a new tensor of the format's dtype and shape, or `out` checked against them."""
    import torch
    shape = fmt.shape(n, h, w)
    if out is None:
        return torch.empty(shape, dtype=fmt.torch_dtype, device=device)
    if not isinstance(out, torch.Tensor) or out.dtype != fmt.torch_dtype or tuple(out.shape) != shape:
        raise ValueError("out must be a %s tensor of shape %s for %r" % (fmt.dtype, list(shape), fmt))
    if not out.is_cuda or not out.is_contiguous():
        raise ValueError("out must be a contiguous CUDA tensor")
    return out


def _uniform_stride(t, inner):
    """Element stride between consecutive points of a [N,K(,inner)] view whose points lie `stride` elements apart, the
    `inner` elements of a point adjacent (rec[..., :2], rec[..., 2] of a landmark record tensor); None when the view has
    no such stride."""
    n, k = int(t.shape[0]), int(t.shape[1])
    st = t.stride()
    if inner > 1 and st[2] != 1:
        return None
    step = st[1] if k > 1 else (st[0] if n > 1 else inner)
    if step < inner or (n > 1 and st[0] != k * step):
        return None
    return int(step)


def _strided(t, inner):
    """(tensor, element stride between points) of a view read in place; a view without a uniform stride is copied."""
    st = _uniform_stride(t, inner)
    return (t.contiguous(), inner) if st is None else (t, st)


def similarity_device(landmarks, template, landmark_scale=(1.0, 1.0), weights=None):
    """landmarks: CUDA float64 [N,K,2]; template: CUDA float64 [K,2] -> CUDA float32 [N,2,3].
    `landmark_scale` (sx, sy) takes the landmarks to the template's pixel units inside the kernel (float64
    products; the decode's reject marker (-1,-1) stays negative, so the fit skips those points).
    `weights`: CUDA float64 [N,K], one weight per landmark (flm_similarity_from_landmarks_weighted: a point takes part
    when its weight is > 0; None = the unweighted fit, unchanged).  Then `landmarks` and `weights` may be views with a
    uniform element stride -- rec[..., :2] and rec[..., 2] of a landmark record tensor -- and are read in place; any
    other layout is copied first."""
    import torch
    lib = _lib.load()
    n, k, _ = landmarks.shape
    if landmarks.dtype != torch.float64 or template.dtype != torch.float64:
        raise ValueError("landmarks and template must be float64")
    if tuple(template.shape) != (k, 2):
        raise ValueError("template must be [K,2]")
    m = torch.empty((n, 2, 3), dtype=torch.float32, device=landmarks.device)
    if weights is not None:
        if (not isinstance(weights, torch.Tensor) or weights.dtype != torch.float64 or tuple(weights.shape) != (n, k)
                or weights.device != landmarks.device):
            raise ValueError("weights must be a float64 [%d,%d] tensor on the landmarks' device" % (n, k))
        if landmarks.shape[2] != 2:
            raise ValueError("landmarks must be [N,K,2]")
        landmarks, ls = _strided(landmarks, 2)
        weights, wst = _strided(weights, 1)
        if n and k:
            _lib.check(lib.flm_similarity_from_landmarks_weighted(_lib.stream_ptr(), _lib.ptr(landmarks), ls,
                                                                  _lib.ptr(weights), wst, _lib.ptr(template.contiguous()),
                                                                  n, k, float(landmark_scale[0]), float(landmark_scale[1]),
                                                                  _lib.ptr(m)),
                       "flm_similarity_from_landmarks_weighted")
        return m
    _lib.check(lib.flm_similarity_from_landmarks_scaled(_lib.stream_ptr(), _lib.ptr(landmarks.contiguous()),
                                                        _lib.ptr(template.contiguous()), n, k,
                                                        float(landmark_scale[0]), float(landmark_scale[1]),
                                                        _lib.ptr(m)),
               "flm_similarity_from_landmarks_scaled")
    return m


def warp_device(src, m, out_h, out_w, out=None, fmt=None):
    """src: CUDA uint8/float32 [N,Hs,Ws,3]; m: CUDA float32 [N,2,3] (source -> aligned).
    `fmt`: an AlignedFormat -- the faces leave the warp in that layout, type, channel order and normalisation
    (flm_warp_affine_fmt; `out`, when given, must have the format's dtype and shape); None: float32 [N,h,w,3] from
    flm_warp_affine, as ever."""
    import torch
    if fmt is not None:
        _check_format(fmt)
    if src.dim() != 4 or src.shape[3] != 3 or src.dtype not in (torch.uint8, torch.float32):
        raise ValueError("src must be uint8/float32 [N,H,W,3]")
    n, hs, ws, _ = [int(v) for v in src.shape]
    if fmt is not None:
        out_h, out_w = int(out_h), int(out_w)
        out = _format_out(fmt, out, n, out_h, out_w, src.device)
        if n:
            lib = _lib.load()
            cf = fmt.struct()
            _lib.check(lib.flm_warp_affine_fmt(_lib.stream_ptr(), _lib.ptr(src.contiguous()), int(src.dtype == torch.uint8),
                                               n, hs, ws, _lib.ptr(m.contiguous()), _lib.ptr(out), out_h, out_w,
                                               _lib.C.byref(cf)), "flm_warp_affine_fmt")
        return out
    lib = _lib.load()
    if out is None:
        out = torch.empty((n, out_h, out_w, 3), dtype=torch.float32, device=src.device)
    _lib.check(lib.flm_warp_affine(_lib.stream_ptr(), _lib.ptr(src.contiguous()), int(src.dtype == torch.uint8),
                                   n, hs, ws, _lib.ptr(m.contiguous()), _lib.ptr(out), out_h, out_w),
               "flm_warp_affine")
    return out


def align_device(crops, landmarks_in, template, out_h, out_w, landmark_scale=(1.0, 1.0), weights=None, fmt=None):
    """crops [N,H,W,3] + landmarks (crop pixel units after `landmark_scale`) -> aligned crops, M.
    `weights`: per-landmark weights of the fit, as similarity_device takes them; `fmt`: the AlignedFormat of the aligned
    crops, as warp_device takes it (M does not depend on it)."""
    if fmt is not None:
        _check_format(fmt)
    m = similarity_device(landmarks_in, template, landmark_scale, weights)
    if fmt is None:
        return warp_device(crops, m, out_h, out_w), m
    return warp_device(crops, m, out_h, out_w, fmt=fmt), m


def _check_boxes(boxes_dev, k):
    import torch
    if (not isinstance(boxes_dev, torch.Tensor) or boxes_dev.dtype != torch.int32 or not boxes_dev.is_cuda
            or not boxes_dev.is_contiguous() or tuple(boxes_dev.shape) != (k, 4)):
        raise ValueError("boxes_dev must be a contiguous CUDA int32 [%d,4] tensor" % k)


def landmarks_to_frame_device(lm, boxes_dev, grid_hw, frame_hw, out=None):
    """lm: CUDA float64 [K,C,2] in output-grid pixels; boxes_dev: CUDA int32 [K,4] (the squared boxes the crops were
    cut from) -> CUDA float64 [K,C,2] in frame pixels (flm_landmarks_to_frame: the box clipped to the frame as the crop
    kernel clips it, then x0 + x * (w / grid_w) in float64; rejected points and faces without pixels stay (-1,-1)).
    `out` may be `lm` itself."""
    import torch
    if not isinstance(lm, torch.Tensor) or lm.dtype != torch.float64 or lm.dim() != 3 or lm.shape[2] != 2 or not lm.is_cuda:
        raise ValueError("lm must be a CUDA float64 [K,C,2] tensor")
    k, c = int(lm.shape[0]), int(lm.shape[1])
    _check_boxes(boxes_dev, k)
    gh, gw = [int(v) for v in grid_hw]
    fh, fw = [int(v) for v in frame_hw]
    if min(gh, gw, fh, fw) < 1:
        raise ValueError("grid_hw and frame_hw must be positive")
    if out is None:
        out = torch.empty_like(lm, memory_format=torch.contiguous_format)
    elif (not isinstance(out, torch.Tensor) or out.dtype != torch.float64 or tuple(out.shape) != (k, c, 2)
          or not out.is_cuda or not out.is_contiguous()):
        raise ValueError("out must be a contiguous CUDA float64 [%d,%d,2] tensor" % (k, c))
    if k and c:
        lib = _lib.load()
        _lib.check(lib.flm_landmarks_to_frame(_lib.stream_ptr(), _lib.ptr(lm.contiguous()), _lib.ptr(boxes_dev), k, c,
                                              gh, gw, fh, fw, _lib.ptr(out)), "flm_landmarks_to_frame")
    return out


def warp_frames_device(frames, m, out_h, out_w, frame_index_dev=None, boxes_dev=None, samples=1, out=None, fmt=None,
                       src=None):
    """frames: contiguous CUDA uint8 [F,H,W,3] ring; m: CUDA float32 [K,2,3] (FRAME pixels -> aligned pixels);
    frame_index_dev: CUDA int32 [K] ring slot of every face (default: slot 0); boxes_dev: CUDA int32 [K,4], faces whose
    clipped box is empty come back as zeros; samples: 1, 2 or 4 bilinear samples per axis and output pixel
    -> CUDA float32 [K,out_h,out_w,3] (flm_warp_affine_frames).
    `fmt`: an AlignedFormat -- the faces leave the warp in that layout, type, channel order and normalisation
    (flm_warp_affine_frames_fmt), e.g. AlignedFormat.matcher() -> CUDA float16 [K,3,out_h,out_w], RGB, in [-1,1];
    `out`, when given, must then have the format's dtype and shape.
    `src`: a FrameFormat -- how the ring holds its pixels (flm_warp_affine_frames_src).  FrameFormat.nv12(H, W, ...):
    `frames` is the decoder's CUDA uint8 [F,rows,pitch] ring and every tap is converted to BGR on its way in; the result
    has the bits of this call on the converted ring.  None: the BGR ring through the calls above, as ever."""
    import torch
    if fmt is not None:
        _check_format(fmt)
    if src is not None:
        _check_frame_format(src)
        ring = src.ring(frames)
    elif (not isinstance(frames, torch.Tensor) or frames.dim() != 4 or frames.shape[3] != 3 or frames.dtype != torch.uint8
            or not frames.is_cuda or not frames.is_contiguous()):
        raise ValueError("frames must be a contiguous CUDA uint8 [F,H,W,3] tensor")
    if not isinstance(m, torch.Tensor) or m.dtype != torch.float32 or m.dim() != 3 or tuple(m.shape[1:]) != (2, 3) or not m.is_cuda:
        raise ValueError("m must be a CUDA float32 [K,2,3] tensor")
    if samples not in (1, 2, 4):
        raise ValueError("samples must be 1, 2 or 4")
    out_h, out_w = int(out_h), int(out_w)
    if out_h < 1 or out_w < 1:
        raise ValueError("out_h and out_w must be positive")
    k = int(m.shape[0])
    if src is not None:
        nf, fh, fw, stride = ring
    else:
        nf, fh, fw = [int(v) for v in frames.shape[:3]]
        stride = fh * fw * 3
    if frame_index_dev is not None and (not isinstance(frame_index_dev, torch.Tensor) or frame_index_dev.dtype != torch.int32
                                        or not frame_index_dev.is_cuda or not frame_index_dev.is_contiguous()
                                        or tuple(frame_index_dev.shape) != (k,)):
        raise ValueError("frame_index_dev must be a contiguous CUDA int32 [%d] tensor" % k)
    if boxes_dev is not None:
        _check_boxes(boxes_dev, k)
    if fmt is not None:
        out = _format_out(fmt, out, k, out_h, out_w, frames.device)
    elif out is None:
        out = torch.empty((k, out_h, out_w, 3), dtype=torch.float32, device=frames.device)
    elif (not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or tuple(out.shape) != (k, out_h, out_w, 3)
          or not out.is_cuda or not out.is_contiguous()):
        raise ValueError("out must be a contiguous CUDA float32 [%d,%d,%d,3] tensor" % (k, out_h, out_w))
    if not k:
        return out
    lib = _lib.load()
    cf = None if fmt is None else fmt.struct()
    head = (_lib.stream_ptr(), _lib.ptr(frames), stride, nf, fh, fw,
            None if frame_index_dev is None else _lib.ptr(frame_index_dev),
            None if boxes_dev is None else _lib.ptr(boxes_dev), _lib.ptr(m.contiguous()), k, _lib.ptr(out), out_h, out_w,
            int(samples))
    if src is not None:     # one call for every ring and format: it dispatches on a NULL fmt and on BGR24 itself
        cs = src.struct(frames)
        _lib.check(lib.flm_warp_affine_frames_src(*head, None if cf is None else _lib.C.byref(cf), _lib.C.byref(cs)),
                   "flm_warp_affine_frames_src")
    elif fmt is not None:   # no frame format: the symbols of before
        _lib.check(lib.flm_warp_affine_frames_fmt(*head, _lib.C.byref(cf)), "flm_warp_affine_frames_fmt")
    else:
        _lib.check(lib.flm_warp_affine_frames(*head), "flm_warp_affine_frames")
    return out


# ---- shape-normalised faces: the piecewise-affine warp over the landmark mesh (include/flm.h) ---------------------------
def _cross2(a, b, c):
    """(bx-ax)*(cy-ay) - (by-ay)*(cx-ax): the doubled signed area of (a, b, c), the edge function of include/flm.h."""
    return (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])


def _in_circumcircle(a, b, c, d):
    """Is d strictly inside the circumcircle of the positively oriented triangle (a, b, c)?  The in-circle determinant
    in float64 against 1e-12 of the sum of its terms' magnitudes: points that are cocircular up to rounding (the
    template is mirror-symmetric, so every isosceles trapezoid of it is) count as outside, whichever way they round."""
    ax, ay, bx, by, cx, cy = a[0] - d[0], a[1] - d[1], b[0] - d[0], b[1] - d[1], c[0] - d[0], c[1] - d[1]
    a2, b2, c2 = ax * ax + ay * ay, bx * bx + by * by, cx * cx + cy * cy
    terms = (ax * by * c2, -ax * cy * b2, -ay * bx * c2, ay * cx * b2, a2 * bx * cy, -a2 * by * cx)
    return sum(terms) > 1e-12 * sum(abs(t) for t in terms)


def _delaunay_in_rectangle(points, corners):
    """Delaunay triangulation (Bowyer-Watson, float64) of `points`, four of which -- `corners`, in order around the
    rectangle -- are the corners of an axis-aligned rectangle that holds all the others.  The rectangle's two triangles
    are the start, so there is no super-triangle to remove; a point on the rectangle's border (exactly collinear with
    two corners) splits the border edge, and the triangle of zero area that the cavity's border edge would make is
    dropped.  -> list of (i, j, k), each positively oriented."""
    pts = [(float(x), float(y)) for x, y in points]
    c0, c1, c2, c3 = corners
    tris = [(c0, c1, c2), (c0, c2, c3)]
    if _cross2(pts[c0], pts[c1], pts[c2]) < 0:
        tris = [(c0, c2, c1), (c0, c3, c2)]
    for i, q in enumerate(pts):
        if i in corners:
            continue
        bad = [t for t in tris if _in_circumcircle(pts[t[0]], pts[t[1]], pts[t[2]], q)]
        if not bad:          # on the border, and cocircular with the triangle there: the triangle that holds the point
            bad = [t for t in tris if min(_cross2(pts[t[0]], pts[t[1]], q), _cross2(pts[t[1]], pts[t[2]], q),
                                          _cross2(pts[t[2]], pts[t[0]], q)) >= 0][:1]
        edges = {}
        for t in bad:
            for e in ((t[0], t[1]), (t[1], t[2]), (t[2], t[0])):
                if (e[1], e[0]) in edges:
                    del edges[(e[1], e[0])]
                else:
                    edges[e] = True
        tris = [t for t in tris if t not in bad]
        for a, b in edges:
            if _cross2(pts[a], pts[b], q) > 0:      # == 0: q lies on the border edge a-b
                tris.append((a, b, i))
    return tris


class FaceMesh:
    """The mesh of the piecewise-affine warp (flm_warp_mesh_frames): `points`, float64 [P,2] template positions in aligned
    pixels -- the first P - n_anchors those of the landmarks, in landmark order, the last `n_anchors` ANCHORS, template
    positions without a landmark that a face places in its frame through the inverse of its similarity M -- and
    `triangles`, int [T,3] of point indices.  3 <= P <= 256, 1 <= T <= 255.  The constructor turns every triangle to
    positive orientation and rejects an index outside [0,P), a repeated vertex and a triangle whose doubled template
    area is below 1e-9.  `points` and `triangles` are the mesh's own read-only copies.  The device tensors and the triangle map of every
    (device, aligned size) are made once, by the first call that needs them, and cached for the callers of every stream:
    that call synchronises its stream once, so that what the cache holds is finished data (a `FaceTracker` does it when
    it allocates its state)."""

    MAX_POINTS, MAX_TRIANGLES, MIN_AREA2 = 256, 255, 1e-9

    def __init__(self, points, triangles, n_anchors=0):
        pts = np.asarray(points, np.float64)
        tri = np.asarray(triangles)
        if pts.ndim != 2 or pts.shape[1] != 2 or tri.ndim != 2 or tri.shape[1] != 3 or tri.dtype.kind not in "iu":
            raise ValueError("a face mesh is float64 [P,2] points and integer [T,3] triangles")
        p, t = int(pts.shape[0]), int(tri.shape[0])
        if not 3 <= p <= self.MAX_POINTS:
            raise ValueError("a face mesh has 3 to %d points (got %d)" % (self.MAX_POINTS, p))
        if not 1 <= t <= self.MAX_TRIANGLES:
            raise ValueError("a face mesh has 1 to %d triangles (got %d)" % (self.MAX_TRIANGLES, t))
        if isinstance(n_anchors, bool) or int(n_anchors) != n_anchors or not 0 <= int(n_anchors) <= p:
            raise ValueError("n_anchors must be an integer in [0, %d] (got %r)" % (p, n_anchors))
        if not np.isfinite(pts).all():
            raise ValueError("the points of a face mesh must be finite")
        if tri.min() < 0 or tri.max() >= p:
            raise ValueError("a triangle names a point outside [0, %d)" % p)
        tri = tri.astype(np.int32)
        if ((tri[:, 0] == tri[:, 1]) | (tri[:, 1] == tri[:, 2]) | (tri[:, 0] == tri[:, 2])).any():
            raise ValueError("a triangle repeats a vertex")
        a, b, c = pts[tri[:, 0]], pts[tri[:, 1]], pts[tri[:, 2]]
        area2 = (b[:, 0] - a[:, 0]) * (c[:, 1] - a[:, 1]) - (b[:, 1] - a[:, 1]) * (c[:, 0] - a[:, 0])
        if (np.abs(area2) < self.MIN_AREA2).any():
            raise ValueError("template triangle %d is degenerate (doubled area below %g)"
                             % (int(np.argmax(np.abs(area2) < self.MIN_AREA2)), self.MIN_AREA2))
        flip = area2 < 0
        tri[flip] = tri[flip][:, [0, 2, 1]]
        self.points = np.array(pts, np.float64, order="C")        # the mesh's own copies, read-only: the device tensors
        self.triangles = np.array(tri, np.int32, order="C")       # and maps cached below are made from them once
        self.points.setflags(write=False)
        self.triangles.setflags(write=False)
        self.n_anchors = int(n_anchors)
        self._dev, self._maps = {}, {}

    @classmethod
    def default(cls, n_landmarks, out_h, out_w):
        """canonical_template(n_landmarks, out_h, out_w) plus eight anchors -- the corners and edge midpoints of
        [0,out_w-1] x [0,out_h-1] -- under their Delaunay triangulation: the mesh covers every output pixel and is
        continuous with the similarity warp at the border."""
        n, h, w = int(n_landmarks), int(out_h), int(out_w)
        if n < 1 or h < 2 or w < 2:
            raise ValueError("the default mesh needs n_landmarks >= 1 and an aligned size of 2 x 2 or more")
        x1, y1 = float(w - 1), float(h - 1)
        anchors = np.array([[0, 0], [x1, 0], [x1, y1], [0, y1], [x1 / 2, 0], [x1, y1 / 2], [x1 / 2, y1], [0, y1 / 2]], np.float64)
        pts = np.concatenate([canonical_template(n, h, w), anchors])
        tris = np.array(sorted(_delaunay_in_rectangle(pts, (n, n + 1, n + 2, n + 3))), np.int32)
        # a triangulation of P points of which the 8 anchors lie on the hull has 2P - 2 - 8 triangles that tile the rectangle
        a, b, c = pts[tris[:, 0]], pts[tris[:, 1]], pts[tris[:, 2]]
        area2 = (b[:, 0] - a[:, 0]) * (c[:, 1] - a[:, 1]) - (b[:, 1] - a[:, 1]) * (c[:, 0] - a[:, 0])
        if len(tris) != 2 * (n + 8) - 10 or not (area2 > 0).all() or abs(area2.sum() / 2 - x1 * y1) > 1e-9 * x1 * y1:
            raise ValueError("the default mesh of %d landmarks at %dx%d does not tile the aligned rectangle (landmark "
                             "positions that coincide or lie on its border?): pass an alignment.FaceMesh" % (n, h, w))
        return cls(pts, tris, 8)

    @property
    def n_points(self):
        return int(self.points.shape[0])

    @property
    def n_triangles(self):
        return int(self.triangles.shape[0])

    @property
    def n_landmarks(self):
        return self.n_points - self.n_anchors

    @staticmethod
    def _device(device):
        """`device` with its index spelled out: "cuda" and "cuda:0" are one cache entry."""
        import torch
        d = torch.device(device)
        if d.type == "cuda" and d.index is None:
            d = torch.device("cuda", torch.cuda.current_device())
        return d

    @staticmethod
    def _finished(device):
        """What the caches below hold is shared by every stream of the device, so it is FINISHED read-only data before
        it gets there: the stream that produced it is synchronised, once per entry, by the caller that made it."""
        import torch
        if device.type == "cuda":
            torch.cuda.current_stream(device).synchronize()

    def tensors(self, device):
        """(points float64 [P,2], triangles int32 [T,3]) on `device`, uploaded and finished at the first call."""
        import torch
        d = self._device(device)
        if d not in self._dev:
            made = (torch.from_numpy(self.points.copy()).to(d), torch.from_numpy(self.triangles.copy()).to(d))
            self._finished(d)
            self._dev[d] = made
        return self._dev[d]

    def map(self, device, out_h, out_w):
        """The triangle map uint8 [out_h,out_w] on `device` (flm_mesh_map), made at the first call of any stream and
        finished -- the launching stream is synchronised once -- before any caller, on any stream, can find it here."""
        d = self._device(device)
        key = (d, int(out_h), int(out_w))
        if key not in self._maps:
            made = mesh_map_device(self, out_h, out_w, d)
            self._finished(d)
            self._maps[key] = made
        return self._maps[key]

    def __repr__(self):
        return "FaceMesh(%d points, %d anchors, %d triangles)" % (self.n_points, self.n_anchors, self.n_triangles)


def _check_mesh(mesh):
    if not isinstance(mesh, FaceMesh):
        raise ValueError("mesh must be an alignment.FaceMesh (got %r)" % (mesh,))


def _check_min_det(min_det):
    min_det = float(min_det)
    if not min_det >= 0.0:
        raise ValueError("min_det must be >= 0 (got %r)" % min_det)
    return min_det


def mesh_map_device(mesh, out_h, out_w, device="cuda", out=None):
    """The triangle of every aligned pixel: CUDA uint8 [out_h,out_w], the lowest triangle of `mesh` whose three edge
    functions at the pixel's integer position are >= 0, 255 where there is none (flm_mesh_map).  FaceMesh.map caches it."""
    import torch
    _check_mesh(mesh)
    out_h, out_w = _sizes((out_h, out_w), "out_h and out_w")
    if out is None:
        out = torch.empty((out_h, out_w), dtype=torch.uint8, device=device)
    else:
        _check_out(out, torch.uint8, (out_h, out_w), "out")
    pts, tris = mesh.tensors(out.device)
    _lib.check(_lib.load().flm_mesh_map(_lib.stream_ptr(), _lib.ptr(pts), _lib.ptr(tris), mesh.n_points, mesh.n_triangles,
                                        out_h, out_w, _lib.ptr(out)), "flm_mesh_map")
    return out


def _mesh_faces(lm, m, mesh):
    """The checks that flm_mesh_affines and flm_warp_mesh_frames share: (lm, its element stride, K)."""
    _check_mesh(mesh)
    lm, ls = _strided_points(lm)
    k, c = int(lm.shape[0]), int(lm.shape[1])
    if c != mesh.n_landmarks:
        raise ValueError("lm has %d landmarks per face, the mesh %d" % (c, mesh.n_landmarks))
    _check_matrices(m, k)
    if m.device != lm.device:
        raise ValueError("lm and m must be on one device")
    return lm, ls, k


def mesh_affines_device(lm, m, mesh, min_det=1e-6, out=None):
    """lm: CUDA float64 [K,C,2] frame-space landmarks (or the x,y view of a landmark record tensor, read in place);
    m: contiguous CUDA float32 [K,2,3], every face's similarity frame px -> aligned px -> CUDA float32 [K,T,2,3], the
    affine frame px -> aligned px of every triangle of every face (flm_mesh_affines; a triangle whose landmarks span
    less than `min_det` doubled area, or hold a NaN, takes the face's m)."""
    import torch
    lm, ls, k = _mesh_faces(lm, m, mesh)
    min_det = _check_min_det(min_det)
    out = _out(out, torch.float32, (k, mesh.n_triangles, 2, 3), "out", lm.device)
    if k:
        pts, tris = mesh.tensors(lm.device)
        _lib.check(_lib.load().flm_mesh_affines(_lib.stream_ptr(), _lib.ptr(lm), ls, _lib.ptr(m), _lib.ptr(pts),
                                                _lib.ptr(tris), mesh.n_points, mesh.n_anchors, mesh.n_triangles, k,
                                                min_det, _lib.ptr(out)), "flm_mesh_affines")
    return out


def warp_mesh_frames_device(frames, lm, m, mesh, out_h, out_w, frame_index_dev=None, boxes_dev=None, samples=1, fmt=None,
                            src=None, out=None, affines_out=None, min_det=1e-6):
    """Shape-normalised faces in one launch (flm_warp_mesh_frames): every triangle of `mesh` is filled from the frame by
    the affine that takes the face's landmarks onto the triangle's template corners, so each landmark's texture lands
    on its template pixel.  frames, frame_index_dev, boxes_dev, samples, fmt, src, out: as warp_frames_device takes them
    (and with its result for a ring slot outside the ring and an empty box: a zero face); lm: CUDA float64 [K,C,2]
    FRAME-space landmarks, C the mesh's landmark count (a view of a landmark record tensor is read in place); m: contiguous
    CUDA float32 [K,2,3], the faces' similarity frame px -> aligned px, which places the mesh's anchors and stands in for
    a triangle whose landmarks collapse; affines_out: None or contiguous CUDA float32 [K,T,2,3], receives the matrices of
    mesh_affines_device.  A pixel of triangle t has the bits warp_frames_device gives with m = affines[:, t]."""
    import torch
    if fmt is not None:
        _check_format(fmt)
    if src is not None:
        _check_frame_format(src)
        ring = src.ring(frames)
    elif (not isinstance(frames, torch.Tensor) or frames.dim() != 4 or frames.shape[3] != 3 or frames.dtype != torch.uint8
            or not frames.is_cuda or not frames.is_contiguous()):
        raise ValueError("frames must be a contiguous CUDA uint8 [F,H,W,3] tensor")
    lm, ls, k = _mesh_faces(lm, m, mesh)
    if lm.device != frames.device:
        raise ValueError("lm and m must be on the device of frames (%s, got %s)" % (frames.device, lm.device))
    if samples not in (1, 2, 4):
        raise ValueError("samples must be 1, 2 or 4")
    min_det = _check_min_det(min_det)
    out_h, out_w = _sizes((out_h, out_w), "out_h and out_w")
    if src is not None:
        nf, fh, fw, stride = ring
    else:
        nf, fh, fw = [int(v) for v in frames.shape[:3]]
        stride = fh * fw * 3
    if frame_index_dev is not None:
        _check_out(frame_index_dev, torch.int32, (k,), "frame_index_dev")
    if boxes_dev is not None:
        _check_boxes(boxes_dev, k)
    if fmt is not None:
        out = _format_out(fmt, out, k, out_h, out_w, frames.device)
    else:
        out = _out(out, torch.float32, (k, out_h, out_w, 3), "out", frames.device)
    if affines_out is not None:
        _check_out(affines_out, torch.float32, (k, mesh.n_triangles, 2, 3), "affines_out")
    if not k:
        return out
    pts, tris = mesh.tensors(frames.device)
    tmap = mesh.map(frames.device, out_h, out_w)
    cf = None if fmt is None else fmt.struct()
    cs = None if src is None else src.struct(frames)
    _lib.check(_lib.load().flm_warp_mesh_frames(
        _lib.stream_ptr(), _lib.ptr(frames), stride, nf, fh, fw, _ptr(frame_index_dev), _ptr(boxes_dev), _lib.ptr(lm), ls,
        _lib.ptr(m), _lib.ptr(pts), _lib.ptr(tris), mesh.n_points, mesh.n_anchors, mesh.n_triangles, _lib.ptr(tmap), k,
        _lib.ptr(out), out_h, out_w, int(samples), None if cf is None else _lib.C.byref(cf),
        None if cs is None else _lib.C.byref(cs), min_det, _ptr(affines_out)), "flm_warp_mesh_frames")
    return out


# ---- tracking: the next frame's crop from this frame's landmarks (include/flm.h, "tracking") --------------------------
def _check_matrices(m, k, what="m"):
    import torch
    if (not isinstance(m, torch.Tensor) or m.dtype != torch.float32 or not m.is_cuda or not m.is_contiguous()
            or m.dim() != 3 or tuple(m.shape[1:]) != (2, 3) or (k is not None and int(m.shape[0]) != k)):
        raise ValueError("%s must be a contiguous CUDA float32 [%s,2,3] tensor" % (what, "K" if k is None else k))


def _check_out(t, dtype, shape, what):
    import torch
    if (not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_cuda
            or not t.is_contiguous()):
        raise ValueError("%s must be a contiguous CUDA %s %s tensor" % (what, str(dtype).replace("torch.", ""), list(shape)))


def _sizes(hw, what):
    h, w = [int(v) for v in hw]
    if h < 1 or w < 1:
        raise ValueError("%s must be positive" % what)
    return h, w

def _check_overlap(a, b, what):
    if (a is not None and b is not None and a.numel() and b.numel()
            and a.data_ptr() < b.data_ptr() + b.numel() * b.element_size()
            and b.data_ptr() < a.data_ptr() + a.numel() * a.element_size()):
        raise ValueError("%s must be two buffers that do not overlap" % what)


def _out(t, dtype, shape, what, device):
    """An output of a call: `t` checked against dtype and shape, or a new tensor for None.  Matrices (every [k,2,3]
    output is one) and boxes go through their own checks, which word the error their way (`_check_boxes` calls every
    box tensor boxes_dev)."""
    if t is None:
        import torch
        return torch.empty(shape, dtype=dtype, device=device)
    if what == "boxes_dev":
        _check_boxes(t, shape[0])
    elif shape[1:] == (2, 3):
        _check_matrices(t, shape[0], what)
    else:
        _check_out(t, dtype, shape, what)
    return t


def _ptr(t):
    """The pointer of an optional tensor: NULL for None."""
    return None if t is None else _lib.ptr(t)


def _frame_id(frame_id):
    """frame_id as the int the C calls take; ValueError for what is no integer of int64."""
    if isinstance(frame_id, bool) or int(frame_id) != frame_id or not -2 ** 63 <= int(frame_id) < 2 ** 63:
        raise ValueError("frame_id must be an integer that fits int64 (got %r)" % (frame_id,))
    return int(frame_id)



def _strided_points(lm, what="lm"):
    """(tensor, element stride) of a CUDA float64 [K,C,2] tensor or view read in place: rec[..., :2] of a landmark
    record tensor keeps its stride of 6, any other non-uniform view is copied."""
    import torch
    if not isinstance(lm, torch.Tensor) or lm.dtype != torch.float64 or lm.dim() != 3 or lm.shape[2] != 2 or not lm.is_cuda:
        raise ValueError("%s must be a CUDA float64 [K,C,2] tensor" % what)
    return _strided(lm, 2)


def _weights_arg(weights, n, c):
    """(weights, element stride) of the optional CUDA float64 [n,c] weights of a call, a view of a landmark record tensor
    read in place; (None, 1) for None."""
    if weights is None:
        return None, 1
    import torch
    if (not isinstance(weights, torch.Tensor) or weights.dtype != torch.float64 or tuple(weights.shape) != (n, c)
            or not weights.is_cuda):
        raise ValueError("weights must be a CUDA float64 [%d,%d] tensor" % (n, c))
    return _strided(weights, 1)


def track_seed_device(boxes_dev, in_hw, frame_hw, m_out=None, status_out=None):
    """boxes_dev: CUDA int32 [K,4] squared detector boxes -> (m CUDA float32 [K,2,3] frame px -> network-input px,
    status CUDA int32 [K]) (flm_track_seed: the matrix under which the uint8 frame warp cuts the box as
    flm_crop_resize does; a box without pixels in the frame gives the identity and TRACK_DEAD)."""
    import torch
    if not isinstance(boxes_dev, torch.Tensor) or boxes_dev.dim() != 2:
        raise ValueError("boxes_dev must be a contiguous CUDA int32 [K,4] tensor")
    k = int(boxes_dev.shape[0])
    _check_boxes(boxes_dev, k)
    ih, iw = _sizes(in_hw, "in_hw")
    fh, fw = _sizes(frame_hw, "frame_hw")
    m_out = _out(m_out, torch.float32, (k, 2, 3), "m_out", boxes_dev.device)
    status_out = _out(status_out, torch.int32, (k,), "status_out", boxes_dev.device)
    if k:
        _lib.check(_lib.load().flm_track_seed(_lib.stream_ptr(), _lib.ptr(boxes_dev), k, ih, iw, fh, fw, _lib.ptr(m_out),
                                              _lib.ptr(status_out)), "flm_track_seed")
    return m_out, status_out


def landmarks_from_crop_device(lm, m, grid_hw, in_hw, out=None):
    """lm: CUDA float64 [K,C,2] in output-grid pixels (rec[..., :2] of a landmark record tensor is read in place);
    m: CUDA float32 [K,2,3], the matrices the crops were cut with (frame px -> input px) -> CUDA float64 [K,C,2] in frame
    pixels (flm_landmarks_from_crop: the float64 inverse of m; rejected points, points that land at a negative frame
    coordinate and the points of a face with a singular matrix are (-1,-1))."""
    import torch
    lm, ls = _strided_points(lm)
    k, c = int(lm.shape[0]), int(lm.shape[1])
    _check_matrices(m, k)
    gh, gw = _sizes(grid_hw, "grid_hw")
    ih, iw = _sizes(in_hw, "in_hw")
    out = _out(out, torch.float64, (k, c, 2), "out", lm.device)
    if k and c:
        _lib.check(_lib.load().flm_landmarks_from_crop(_lib.stream_ptr(), _lib.ptr(lm), ls, _lib.ptr(m), k, c, iw / gw,
                                                       ih / gh, _lib.ptr(out)), "flm_landmarks_from_crop")
    return out


class LandmarkFilter:
    """The One-Euro filter of flm_track_step_filtered (include/flm.h): a low-pass on every tracked landmark whose cutoff
    is min_cutoff [Hz] at rest and rises by beta per crop side and second of speed; d_cutoff [Hz] smooths the velocity;
    fps gives the time step 1/fps where a caller names none.  min_cutoff may be +inf: no smoothing.  The defaults keep
    the lag of a moving point below side/(2 pi beta) = 1.06 % of the crop side and pass 0.31 of white noise at rest."""

    def __init__(self, min_cutoff=1.0, beta=15.0, d_cutoff=1.0, fps=30.0):
        import math
        min_cutoff, beta, d_cutoff, fps = float(min_cutoff), float(beta), float(d_cutoff), float(fps)
        if not min_cutoff > 0.0:
            raise ValueError("min_cutoff must be > 0 (+inf switches the smoothing off), got %r" % min_cutoff)
        if not (beta >= 0.0 and math.isfinite(beta)):
            raise ValueError("beta must be finite and >= 0, got %r" % beta)
        if not (d_cutoff > 0.0 and math.isfinite(d_cutoff)):
            raise ValueError("d_cutoff must be finite and > 0, got %r" % d_cutoff)
        if not (fps > 0.0 and math.isfinite(fps)):
            raise ValueError("fps must be finite and > 0, got %r" % fps)
        self.min_cutoff, self.beta, self.d_cutoff, self.fps = min_cutoff, beta, d_cutoff, fps

    def time_step(self, dt=None):
        """dt in seconds, checked; 1/fps for None."""
        import math
        dt = 1.0 / self.fps if dt is None else float(dt)
        if not (dt > 0.0 and math.isfinite(dt)):
            raise ValueError("dt must be finite and > 0, got %r" % dt)
        return dt

    def __repr__(self):
        return "LandmarkFilter(min_cutoff=%r, beta=%r, d_cutoff=%r, fps=%r)" % (self.min_cutoff, self.beta, self.d_cutoff,
                                                                                 self.fps)


def _track_step(lm, m_crop, boxes, grid_hw, in_hw, frame_hw, tmpl_crop, tmpl_align, weights, min_points, min_score,
                min_side, max_side, lm_frame, m_align, m_next, boxes_next, status, filter, dt, state, lm_raw, rows=False,
                slot=None, status_rows=None, m_what="m_crop", k_what="K"):
    """The one statement of `track_step_device` and, with rows=True, of `track_step_rows_device`: the rows form adds
    slot, n_slots (taken from m_next), a per-row dt tensor, status_rows and the three overlap checks.  m_what, k_what:
    what the caller names the matrices and the size of the tracker's own tensors.  Returns every tensor the call writes:
    (lm_frame, m_align, m_next, boxes_next, status, status_rows)."""
    import torch
    dt_rows = None
    if filter is None:
        if dt is not None or state is not None or lm_raw is not None:
            raise ValueError("dt, state and lm_raw go with filter")
    else:                           # (the filter's own arguments first: they need no tensor to be judged)
        if not isinstance(filter, LandmarkFilter):
            raise ValueError("filter must be None or a LandmarkFilter (got %r)" % (filter,))
        if rows and isinstance(dt, torch.Tensor):
            dt_rows, dt = dt, 0.0
        else:
            dt = filter.time_step(dt)
        if (not isinstance(state, torch.Tensor) or state.dtype != torch.float64 or state.dim() != 3
                or int(state.shape[2]) != 6):
            raise ValueError("state must be a contiguous CUDA float64 [%s,C,6] tensor" % k_what)
    lm, ls = _strided_points(lm)
    n, c = int(lm.shape[0]), int(lm.shape[1])
    n_slots = n
    if rows:                        # the tracker's own tensors are written at the slot: they exist, and give n_slots
        _check_out(slot, torch.int32, (n,), "slot")
        _check_matrices(m_next, None, "m_next")
        n_slots = int(m_next.shape[0])
        if not 1 <= n_slots <= 65535 or n > 65535:
            raise ValueError("at most 65535 slots and 65535 rows, at least one slot (got %d slots, %d rows)" % (n_slots, n))
        _check_boxes(boxes_next, n_slots)
        _check_out(status, torch.int32, (n_slots,), "status")
    if filter is not None:
        _check_out(state, torch.float64, (n_slots, c, 6), "state")
        if dt_rows is not None:
            _check_out(dt_rows, torch.float64, (n,), "dt")
        if lm_raw is not None:
            _check_out(lm_raw, torch.float64, (n, c, 2), "lm_raw")
    _check_matrices(m_crop, n, m_what)
    _check_boxes(boxes, n)
    gh, gw = _sizes(grid_hw, "grid_hw")
    ih, iw = _sizes(in_hw, "in_hw")
    fh, fw = _sizes(frame_hw, "frame_hw")
    _check_out(tmpl_crop, torch.float64, (c, 2), "tmpl_crop")
    if tmpl_align is not None:
        _check_out(tmpl_align, torch.float64, (c, 2), "tmpl_align")
    weights, wst = _weights_arg(weights, n, c)
    if m_align is not None and tmpl_align is None:
        raise ValueError("m_align needs tmpl_align")
    if int(min_points) < 2:
        raise ValueError("min_points must be 2 or more")
    if any(v != v for v in (float(min_score), float(min_side), float(max_side))):
        raise ValueError("min_score, min_side and max_side must not be NaN")
    dev = lm.device
    lm_frame = _out(lm_frame, torch.float64, (n, c, 2), "lm_frame", dev)
    if tmpl_align is not None:
        m_align = _out(m_align, torch.float32, (n, 2, 3), "m_align", dev)
    if rows:
        status_rows = _out(status_rows, torch.int32, (n,), "status_rows", dev)
        _check_overlap(m_crop, m_next, "m_crop_c and m_next")
        _check_overlap(boxes, boxes_next, "boxes_c and boxes_next")
        _check_overlap(status_rows, status, "status_rows and status")
    else:
        m_next = _out(m_next, torch.float32, (n, 2, 3), "m_next", dev)
        boxes_next = _out(boxes_next, torch.int32, (n, 4), "boxes_dev", dev)
        status = _out(status, torch.int32, (n,), "status", dev)
    if n and c:
        lib = _lib.load()
        opts = _lib.TrackOpts.make(min_points, min_score, min_side, max_side)
        fo = None if filter is None else _lib.TrackFilter.make(filter.min_cutoff, filter.beta, filter.d_cutoff)
        args = (_lib.stream_ptr(), _lib.ptr(lm), ls, _ptr(weights), wst, _lib.ptr(m_crop), _lib.ptr(boxes), n, c, iw / gw,
                ih / gh, ih, iw, fh, fw, _lib.ptr(tmpl_crop), _ptr(tmpl_align), _lib.C.byref(opts), _lib.ptr(lm_frame),
                _ptr(m_align), _lib.ptr(m_next), _lib.ptr(boxes_next), _lib.ptr(status))
        if rows:
            _lib.check(lib.flm_track_step_rows(*args, None if fo is None else _lib.C.byref(fo), 0.0 if fo is None else dt,
                                               _ptr(state), _ptr(lm_raw), _lib.ptr(slot), n_slots, _ptr(dt_rows),
                                               _lib.ptr(status_rows)), "flm_track_step_rows")
        elif fo is None:
            _lib.check(lib.flm_track_step(*args), "flm_track_step")
        else:
            _lib.check(lib.flm_track_step_filtered(*args, _lib.C.byref(fo), dt, _lib.ptr(state), _ptr(lm_raw)),
                       "flm_track_step_filtered")
    return lm_frame, m_align, m_next, boxes_next, status, status_rows


def track_step_device(lm, m_crop, boxes_dev, grid_hw, in_hw, frame_hw, tmpl_crop, tmpl_align=None, weights=None,
                      min_points=2, min_score=0.0, min_side=0.0, max_side=float("inf"), lm_frame=None, m_align=None,
                      m_next=None, boxes_next=None, status=None, filter=None, dt=None, state=None, lm_raw=None):
    """The per-frame update of a set of tracks in one launch (flm_track_step; include/flm.h states it line by line).

    lm: CUDA float64 [K,C,2] on the output grid and `weights`: None or CUDA float64 [K,C] (both may be views of a
    landmark record tensor, read in place); m_crop CUDA float32 [K,2,3] and boxes_dev CUDA int32 [K,4]: what this frame's
    crops were cut with; tmpl_crop CUDA float64 [C,2] in input px: where the landmarks should sit in the next crop;
    tmpl_align CUDA float64 [C,2] in aligned px, or None: no aligned fit.
    Returns (lm_frame float64 [K,C,2] frame px, m_align float32 [K,2,3] frame px -> aligned px or None, m_next float32
    [K,2,3] frame px -> input px of the next crop, boxes_next int32 [K,4], status int32 [K]: 0 or TRACK_* bits; a lost
    track has an empty box and the identity as m_next).  The five keyword tensors name where to write; `m_next` may be
    `m_crop` and `boxes_next` may be `boxes_dev`.

    filter: None, or a `LandmarkFilter`: the landmarks pass through its One-Euro filter inside the same launch
    (flm_track_step_filtered), and lm_frame, both fits, the status and the box are those of the filtered points.  Then
    `state` is the CUDA float64 [K,C,6] filter state, read and written (filled with -1: no history), `dt` the seconds
    since the previous step (None: 1/filter.fps), and `lm_raw`, if given, a CUDA float64 [K,C,2] tensor that receives
    the unfiltered points."""
    return _track_step(lm, m_crop, boxes_dev, grid_hw, in_hw, frame_hw, tmpl_crop, tmpl_align, weights, min_points,
                       min_score, min_side, max_side, lm_frame, m_align, m_next, boxes_next, status, filter, dt, state,
                       lm_raw)[:5]


# ---- association: detector boxes against live tracks (include/flm.h, "association") ----------------------------------
ASSOC_MAX = 1024      # slots and detections per flm_track_associate call


class TrackAssociation:
    """How flm_track_associate pairs detector boxes with live tracks (include/flm.h): a detection and a track may pair
    when their IoU is at least match_iou; two live tracks with an IoU of at least dup_iou are one face, and the higher
    slot ends (above 1: never); a matched pair whose IoU is below refresh_iou restarts the track from the detection
    (0: never); a track no detection has matched in max_misses consecutive updates ends (0: never); square: the
    detections pass through the box maths of `prediction.face_boxes` first, as `FaceTracker.seed` does on the host.
    The defaults are the customary gate of box trackers and a guess; none has been tuned against a trained model."""

    def __init__(self, match_iou=0.3, dup_iou=0.7, refresh_iou=0.0, max_misses=0, square=True):
        match_iou, dup_iou, refresh_iou = float(match_iou), float(dup_iou), float(refresh_iou)
        for name, v in (("match_iou", match_iou), ("dup_iou", dup_iou), ("refresh_iou", refresh_iou)):
            if v != v:
                raise ValueError("%s must not be NaN" % name)
        if int(max_misses) != max_misses or int(max_misses) < 0:
            raise ValueError("max_misses must be an integer >= 0 (0 = never), got %r" % (max_misses,))
        self.match_iou, self.dup_iou, self.refresh_iou = match_iou, dup_iou, refresh_iou
        self.max_misses, self.square = int(max_misses), bool(square)

    def struct(self):
        return _lib.TrackAssocOpts.make(self.match_iou, self.dup_iou, self.refresh_iou, self.max_misses, self.square)

    def __repr__(self):
        return "TrackAssociation(match_iou=%r, dup_iou=%r, refresh_iou=%r, max_misses=%r, square=%r)" % (
            self.match_iou, self.dup_iou, self.refresh_iou, self.max_misses, self.square)


def _track_associate(who, det, m_crop, boxes, status, misses, in_hw, frame_hw, n_det, state, assoc, det_slot, slot_det,
                     counts, streams=False, slots_per_stream=None):
    """The one statement of `track_associate_device` and, with streams=True, of `track_associate_streams_device`: the
    single call is the streams call without the S axis -- det is 2-D, n_det has one element, counts is [8] and the slots
    are those of m_crop.  who: the caller's name, for its messages."""
    import torch
    if assoc is None:
        assoc = TrackAssociation()
    elif not isinstance(assoc, TrackAssociation):
        raise ValueError("assoc must be None or a TrackAssociation (got %r)" % (assoc,))
    if streams:
        if not isinstance(det, torch.Tensor) or det.dim() != 3 or det.dtype != torch.int32 or int(det.shape[2]) != 4:
            raise ValueError("det must be a contiguous CUDA int32 [S,D,4] tensor")
        s, d = int(det.shape[0]), int(det.shape[1])
        if n_det is not None and (not isinstance(n_det, torch.Tensor) or n_det.dtype != torch.int32
                                  or tuple(n_det.shape) != (s,)):
            raise ValueError("n_det must be None or a contiguous CUDA int32 [%d] tensor, one count per stream" % s)
        if not det.is_cuda or not det.is_contiguous():
            raise ValueError("det must be a contiguous CUDA int32 [S,D,4] tensor")
        if isinstance(slots_per_stream, bool) or int(slots_per_stream) != slots_per_stream:
            raise ValueError("slots_per_stream must be an integer (got %r)" % (slots_per_stream,))
        k = int(slots_per_stream)
        if s < 1 or not 1 <= d <= ASSOC_MAX or not 1 <= k <= ASSOC_MAX:
            raise ValueError("%s takes 1 or more streams of 1..%d detections and 1..%d slots each "
                             "(got %d streams, %d, %d)" % (who, ASSOC_MAX, ASSOC_MAX, s, d, k))
        n = s * k
        if n > 65535:
            raise ValueError("%d streams of %d slots exceed the tracker's 65535 slots" % (s, k))
        _check_matrices(m_crop, n, "m_crop")
    else:
        if not isinstance(det, torch.Tensor) or det.dim() != 2:
            raise ValueError("det must be a contiguous CUDA int32 [D,4] tensor")
        s, d = 1, int(det.shape[0])
        if (det.dtype != torch.int32 or not det.is_cuda or not det.is_contiguous() or int(det.shape[1]) != 4):
            raise ValueError("det must be a contiguous CUDA int32 [D,4] tensor")
        _check_matrices(m_crop, None, "m_crop")
        n = k = int(m_crop.shape[0])
        if not 1 <= d <= ASSOC_MAX or not 1 <= k <= ASSOC_MAX:
            raise ValueError("%s takes 1..%d detections and 1..%d slots (got %d, %d)" % (who, ASSOC_MAX, ASSOC_MAX, d, k))
    _check_boxes(boxes, n)
    _check_out(status, torch.int32, (n,), "status")
    _check_out(misses, torch.int32, (n,), "misses")
    if n_det is not None:
        if streams:
            _check_out(n_det, torch.int32, (s,), "n_det")
        elif (not isinstance(n_det, torch.Tensor) or n_det.dtype != torch.int32 or not n_det.is_cuda or n_det.numel() != 1
                or not n_det.is_contiguous()):
            raise ValueError("n_det must be None or a CUDA int32 tensor of one element")
    c = 1
    if state is not None:
        if not isinstance(state, torch.Tensor) or state.dim() != 3:
            raise ValueError("state must be a contiguous CUDA float64 [%s,C,6] tensor" % ("S*K" if streams else "K"))
        c = int(state.shape[1])
        _check_out(state, torch.float64, (n, c, 6), "state")
        if not 1 <= c <= 1024:
            raise ValueError("state must have 1..1024 landmarks (got %d)" % c)
    ih, iw = _sizes(in_hw, "in_hw")
    fh, fw = _sizes(frame_hw, "frame_hw")
    if fh * fw > 2 ** 30:
        raise ValueError("frames of %dx%d are outside the association's reach (H*W <= 2^30)" % (fh, fw))
    tensors = [det, m_crop, boxes, status, misses] + [t for t in (n_det, state) if t is not None]
    det_slot = _out(det_slot, torch.int32, (s, d) if streams else (d,), "det_slot", det.device)
    slot_det = _out(slot_det, torch.int32, (n,), "slot_det", det.device)
    counts = _out(counts, torch.int32, (s, 8) if streams else (8,), "counts", det.device)
    if any(t.device != det.device for t in tensors + [det_slot, slot_det, counts]):
        raise ValueError("every tensor of %s must lie on the device of det" % who)
    opts = assoc.struct()
    head = (_lib.stream_ptr(), _lib.ptr(det), _ptr(n_det))
    tail = (d, k, c, ih, iw, fh, fw, _lib.C.byref(opts), _lib.ptr(m_crop), _lib.ptr(boxes), _lib.ptr(status),
            _lib.ptr(misses), _ptr(state), _lib.ptr(det_slot), _lib.ptr(slot_det), _lib.ptr(counts))
    if streams:
        _lib.check(_lib.load().flm_track_associate_streams(*head, s, *tail), "flm_track_associate_streams")
    else:
        _lib.check(_lib.load().flm_track_associate(*head, *tail), "flm_track_associate")
    return det_slot, slot_det, counts


def track_associate_device(det, m_crop, boxes, status, misses, in_hw, frame_hw, n_det=None, state=None, assoc=None,
                           det_slot=None, slot_det=None, counts=None):
    """Detector boxes against the live tracks of a tracker in one launch (flm_track_associate; include/flm.h states it
    line by line).

    det: CUDA int32 [D,4] boxes (x0,y0,x1,y1), D <= 1024; n_det: None, or a CUDA int32 tensor of one element that says
    how many rows of `det` are valid.  m_crop CUDA float32 [K,2,3], boxes CUDA int32 [K,4], status and misses CUDA int32
    [K], and `state`, None or the CUDA float64 [K,C,6] filter state, are the tracker's own tensors, K <= 1024: read and
    written in place.  assoc: None (the defaults) or a `TrackAssociation`.
    Returns (det_slot int32 [D]: the slot a detection matched or was born into, -1 for a void or unread row, -2 when no
    slot was free; slot_det int32 [K]: the detection of a matched or born slot, else -1; counts int32 [8]: matched,
    born, restarted, duplicates, unconfirmed, dropped, void, 0).  The three keyword tensors name where to write."""
    return _track_associate("track_associate_device", det, m_crop, boxes, status, misses, in_hw, frame_hw, n_det, state,
                            assoc, det_slot, slot_det, counts)


def track_associate_streams_device(det, m_crop, boxes, status, misses, slots_per_stream, in_hw, frame_hw, n_det=None,
                                   state=None, assoc=None, det_slot=None, slot_det=None, counts=None):
    """The association for S streams (cameras) that share one tracker, in one launch of one workgroup per stream
    (flm_track_associate_streams; include/flm.h states it).

    det: CUDA int32 [S,D,4], the boxes of stream i in det[i], D <= 1024; n_det: None, or CUDA int32 [S]: how many rows
    of det[i] are valid -- a negative entry skips the stream (its detector did not run): nothing of its state is read or
    written.  m_crop CUDA float32 [S*K,2,3], boxes CUDA int32 [S*K,4], status and misses CUDA int32 [S*K], and `state`,
    None or CUDA float64 [S*K,C,6], are the tracker's own tensors, stream i owning the slots [i*K, (i+1)*K) with
    K = slots_per_stream <= 1024 and S*K <= 65535: read and written in place.  No pair of two streams is evaluated.
    Returns (det_slot int32 [S,D]: the GLOBAL slot i*K + t a detection matched or was born into, -1 for a void or
    unread row or a skipped stream, -2 when no slot of its stream was free; slot_det int32 [S*K]: the row inside det[i]
    of a matched or born slot, else -1; counts int32 [S,8], per stream as `track_associate_device` lists them, zero for
    a skipped stream).  The three keyword tensors name where to write."""
    return _track_associate("track_associate_streams_device", det, m_crop, boxes, status, misses, in_hw, frame_hw, n_det,
                            state, assoc, det_slot, slot_det, counts, streams=True, slots_per_stream=slots_per_stream)


# ---- the best shot of a track: face quality and gallery (include/flm.h, "the best shot of a track") -------------------
QUALITY_REC = _lib.QUALITY_REC


class QualityOptions:
    """The exposure levels of flm_face_quality: a pixel whose luma lies below `dark` (above `bright`), in 8-bit levels,
    counts as under- (over-) exposed.  Integers in [0, 255]."""

    def __init__(self, dark=16, bright=239):
        for name, v in (("dark", dark), ("bright", bright)):
            if isinstance(v, bool) or int(v) != v or not 0 <= int(v) <= 255:
                raise ValueError("%s must be an integer in [0, 255] (got %r)" % (name, v))
        self.dark, self.bright = int(dark), int(bright)

    def struct(self):
        return _lib.QualityOpts.make(self.dark, self.bright)

    def __repr__(self):
        return "QualityOptions(dark=%r, bright=%r)" % (self.dark, self.bright)


class BestShot:
    """How a tracker picks the best face of a track (flm_face_quality, flm_track_best_update; include/flm.h): the
    quality of a face is min(sharpness / sharp_ref, 1) x the share of well-exposed pixels x the mean landmark score (x a
    factor of the caller's); a face whose exposed share lies below min_exposed never counts.  sharp_ref = 100 is the
    customary blur threshold of the variance of the Laplacian, min_exposed = 0.5 a guess; neither has been tuned
    against real footage.  dark, bright: as `QualityOptions`."""

    def __init__(self, sharp_ref=100.0, min_exposed=0.5, dark=16, bright=239):
        sharp_ref, min_exposed = float(sharp_ref), float(min_exposed)
        if not sharp_ref > 0.0:
            raise ValueError("sharp_ref must be > 0 (got %r)" % sharp_ref)
        if min_exposed != min_exposed:
            raise ValueError("min_exposed must not be NaN")
        self.quality = QualityOptions(dark, bright)
        self.sharp_ref, self.min_exposed = sharp_ref, min_exposed

    @property
    def dark(self):
        return self.quality.dark

    @property
    def bright(self):
        return self.quality.bright

    def struct(self):
        return _lib.BestOpts.make(self.sharp_ref, self.min_exposed)

    def __repr__(self):
        return "BestShot(sharp_ref=%r, min_exposed=%r, dark=%r, bright=%r)" % (self.sharp_ref, self.min_exposed, self.dark,
                                                                                self.bright)


def _faces_of(faces, fmt):
    """(K, h, w) of a CUDA tensor of aligned faces in `fmt` (None: float32 [K,h,w,3]); ValueError otherwise."""
    import torch
    if fmt is None:
        fmt = AlignedFormat()
    else:
        _check_format(fmt)
    if not isinstance(faces, torch.Tensor) or faces.dim() != 4 or faces.dtype != fmt.torch_dtype:
        raise ValueError("faces must be a %s tensor of shape %s for %r" % (
            fmt.dtype, "[K,h,w,3]" if fmt.layout == "nhwc" else "[K,3,h,w]", fmt))
    k = int(faces.shape[0])
    h, w = [int(v) for v in (faces.shape[1:3] if fmt.layout == "nhwc" else faces.shape[2:4])]
    if tuple(faces.shape) != fmt.shape(k, h, w):
        raise ValueError("faces must be a %s tensor of shape %s for %r" % (
            fmt.dtype, "[K,h,w,3]" if fmt.layout == "nhwc" else "[K,3,h,w]", fmt))
    if any(np.float32(s) == 0.0 for s in fmt.scale):    # (the C struct holds float32)
        raise ValueError("a format with a scale of 0 cannot be undone (scale=%r)" % (fmt.scale,))
    if not faces.is_cuda or not faces.is_contiguous():
        raise ValueError("faces must be a contiguous CUDA tensor")
    return fmt, k, h, w


def face_quality_device(faces, fmt=None, opts=None, out=None):
    """faces: CUDA tensor of K aligned faces as the warps store them under `fmt` (an AlignedFormat; None: float32
    [K,h,w,3] BGR) -> CUDA int64 [K,8], the exact quality record of every face (flm_face_quality: n_pix, sum Y, sum Y*Y,
    n_lap, sum L, sum L*L, dark pixels, bright pixels; Y the luma in sixteenths of an 8-bit level, L its 4-neighbour
    Laplacian).  opts: None or a `QualityOptions`; out: where to write.  `faces` may be a slice of a larger buffer."""
    import torch
    if opts is None:
        opts = QualityOptions()
    elif not isinstance(opts, QualityOptions):
        raise ValueError("opts must be None or a QualityOptions (got %r)" % (opts,))
    fmt, k, h, w = _faces_of(faces, fmt)
    out = _out(out, torch.int64, (k, QUALITY_REC), "out", faces.device)
    if k:
        cf, co = fmt.struct(), opts.struct()
        _lib.check(_lib.load().flm_face_quality(_lib.stream_ptr(), _lib.ptr(faces), k, h, w, _lib.C.byref(cf),
                                                _lib.C.byref(co), _lib.ptr(out)), "flm_face_quality")
    return out


def quality_scalars(rec):
    """rec: int64 [K,8] quality records (a tensor on any device, or a numpy array) -> float64 [K,4] of the same kind:
    sharpness (the variance of the Laplacian in 8-bit levels squared; 0 for a face without interior), mean luma and luma
    standard deviation in 8-bit levels, and the share of pixels that are neither dark nor bright."""
    import torch
    is_np = not isinstance(rec, torch.Tensor)
    r = torch.as_tensor(np.asarray(rec)) if is_np else rec
    if r.dtype != torch.int64 or r.dim() != 2 or int(r.shape[1]) != QUALITY_REC:
        raise ValueError("rec must be int64 [K,%d]" % QUALITY_REC)
    d = r.to(torch.float64)
    n_pix, s_y, s_yy, n_lap, s_l, s_ll, dark, bright = d.unbind(1)
    nl = n_lap.clamp(min=1.0)
    mu_l = s_l / nl
    sharp = ((s_ll / nl - mu_l * mu_l) / 256.0).clamp(min=0.0) * (n_lap > 0)
    mean = s_y / n_pix
    std = (s_yy / n_pix - mean * mean).clamp(min=0.0).sqrt()
    out = torch.stack([sharp, mean / 16.0, std / 16.0, (n_pix - dark - bright) / n_pix], dim=1)
    return out.numpy() if is_np else out


def _track_best_update(faces, rec, lm, best_q_in, best_q_out, gallery, best_frame, frame_id, status, reset, weights, factor,
                       m, opts, best_m, best_lm, best_rec, rows=False, slot=None,
                       names=("K", "status", "reset", "best_q_in", "best_q_out")):
    """The one statement of `track_best_update_device` and, with rows=True, of `track_best_update_rows_device`.  The
    dense form: the gallery has the faces' full shape and best_q_in, best_q_out are two buffers of the faces' length.
    The rows form: gallery, best_q_out and the three optional outputs have n_slots entries and are written at `slot`.
    names: what the caller names the number of faces, status, reset and the two quality buffers."""
    import torch
    k_what, status_what, reset_what, q_in_what, q_out_what = names
    if opts is None:
        opts = BestShot()
    elif not isinstance(opts, BestShot):
        raise ValueError("opts must be None or a BestShot (got %r)" % (opts,))
    frame_id = _frame_id(frame_id)
    if not isinstance(faces, torch.Tensor) or faces.dim() < 1 or not faces.is_cuda or not faces.is_contiguous():
        raise ValueError("faces must be a contiguous CUDA tensor of %s faces" % k_what)
    n = n_slots = int(faces.shape[0])
    if rows:
        if (not isinstance(gallery, torch.Tensor) or gallery.dtype != faces.dtype or gallery.dim() != faces.dim()
                or gallery.shape[1:] != faces.shape[1:] or not gallery.is_cuda or not gallery.is_contiguous()):
            raise ValueError("gallery must be a contiguous CUDA tensor of the dtype and face shape of faces")
        n_slots = int(gallery.shape[0])
        if not 1 <= n_slots <= 65535 or n > 65535:
            raise ValueError("at most 65535 slots and 65535 rows, at least one slot (got %d slots, %d rows)" % (n_slots, n))
        _check_out(slot, torch.int32, (n,), "slot")
    elif (not isinstance(gallery, torch.Tensor) or gallery.dtype != faces.dtype or gallery.shape != faces.shape
            or not gallery.is_cuda or not gallery.is_contiguous()):
        raise ValueError("gallery must be a contiguous CUDA tensor of the dtype and shape of faces")
    _check_out(rec, torch.int64, (n, QUALITY_REC), "rec")
    lm, ls = _strided_points(lm)
    c = int(lm.shape[1])
    if int(lm.shape[0]) != n:
        raise ValueError("lm must be a CUDA float64 [%d,C,2] tensor" % n)
    weights, wst = _weights_arg(weights, n, c)
    for t, dtype, name in ((status, torch.int32, status_what), (reset, torch.int32, reset_what),
                           (factor, torch.float64, "factor")):
        if t is not None:
            _check_out(t, dtype, (n,), name)
    if m is not None:
        _check_matrices(m, n)
    _check_out(best_q_in, torch.float64, (n,), q_in_what)
    _check_out(best_q_out, torch.float64, (n_slots,), q_out_what)
    _check_overlap(best_q_in, best_q_out, "%s and %s" % (q_in_what, q_out_what))
    if rows:
        _check_overlap(faces, gallery, "faces and gallery")
    _check_out(best_frame, torch.int64, (n_slots,), "best_frame")
    if best_m is not None:
        if m is None:
            raise ValueError("best_m needs m")
        _check_matrices(best_m, n_slots, "best_m")
    if best_lm is not None:
        _check_out(best_lm, torch.float64, (n_slots, c, 2), "best_lm")
    if best_rec is not None:
        _check_out(best_rec, torch.int64, (n_slots, QUALITY_REC), "best_rec")
    if n and c:
        co = opts.struct()
        head = (_lib.stream_ptr(), _lib.ptr(faces), faces.numel() // n * faces.element_size(), n, _lib.ptr(rec), _ptr(status),
                _ptr(reset), _lib.ptr(lm), ls, _ptr(weights), wst, c, _ptr(factor), _ptr(m), frame_id, _lib.C.byref(co))
        tail = (_lib.ptr(best_q_in), _lib.ptr(best_q_out), _lib.ptr(gallery), _lib.ptr(best_frame), _ptr(best_m),
                _ptr(best_lm), _ptr(best_rec))
        if rows:
            _lib.check(_lib.load().flm_track_best_update_rows(*head, _lib.ptr(slot), n_slots, *tail),
                       "flm_track_best_update_rows")
        else:
            _lib.check(_lib.load().flm_track_best_update(*head, *tail), "flm_track_best_update")
    return best_q_out


def track_best_update_device(faces, rec, lm, best_q_in, best_q_out, gallery, best_frame, frame_id, status=None,
                             reset=None, weights=None, factor=None, m=None, opts=None, best_m=None, best_lm=None,
                             best_rec=None):
    """Per slot, keep the face if it beats the slot's best, in one launch (flm_track_best_update; include/flm.h states it
    line by line).

    faces: contiguous CUDA tensor of K faces (any format: copied as bytes) and `gallery` a tensor of its dtype and
    shape; rec CUDA int64 [K,8] from `face_quality_device`; lm CUDA float64 [K,C,2] and `weights` None or CUDA float64
    [K,C] (both may be views of a landmark record tensor, read in place); status, reset: None or CUDA int32 [K]; factor:
    None or CUDA float64 [K]; m: None or CUDA float32 [K,2,3]; frame_id: a host integer; opts: None or a `BestShot`.
    best_q_in, best_q_out CUDA float64 [K], two different buffers (-1: the slot holds no best); best_frame CUDA int64 [K];
    best_m, best_lm, best_rec: None or CUDA float32 [K,2,3], float64 [K,C,2], int64 [K,8].  A slot that is eligible and
    strictly better has its face, quality, frame id, matrix, landmarks and record written; any other keeps every bit
    and best_q_out = its previous best.  Returns best_q_out."""
    return _track_best_update(faces, rec, lm, best_q_in, best_q_out, gallery, best_frame, frame_id, status, reset, weights,
                              factor, m, opts, best_m, best_lm, best_rec)


# ---- rows: stepping the streams that delivered a frame, each on its own clock (include/flm.h, "rows") -----------------

def track_gather_streams_device(active, m_crop, boxes, slots_per_stream, frame_index=None, dt=None, best_q=None,
                                reset=None, out=None):
    """The snapshot a step of some streams starts from, in one launch (flm_track_gather_streams; include/flm.h states it).

    active: contiguous CUDA int32 [A] stream ids (distinct; an id outside [0, S) gives K inert rows); m_crop CUDA float32
    [S*K,2,3] and boxes CUDA int32 [S*K,4]: the tracker's state, K = slots_per_stream; frame_index: None (ring slot 0) or
    CUDA int32 [S]; dt: None or CUDA float64 [S]; best_q: None or CUDA float64 [S*K]; reset: None or CUDA int32 [S*K], read
    and then cleared for the named streams (the pending reset moves into the snapshot).  Returns a dict of compact CUDA
    tensors over the A*K rows: slot int32 [A*K] (-1: inert), m float32 [A*K,2,3], boxes int32 [A*K,4], frame_index int32
    [A*K], and dt float64, best_q float64, reset int32 [A*K], each present when its input is.  out: None or a dict that
    names where to write (any of those keys); only what it does not name is allocated."""
    import torch
    k = int(slots_per_stream)
    if (not isinstance(active, torch.Tensor) or active.dtype != torch.int32 or active.dim() != 1 or not active.is_cuda
            or not active.is_contiguous() or int(active.shape[0]) < 1):
        raise ValueError("active must be a contiguous CUDA int32 [A] tensor with A >= 1")
    a = int(active.shape[0])
    _check_matrices(m_crop, None, "m_crop")
    n = int(m_crop.shape[0])
    if k < 1 or n < 1 or n % k:
        raise ValueError("m_crop holds %d slots: slots_per_stream=%d must be >= 1 and divide it" % (n, k))
    s = n // k
    if n > 65535 or a * k > 65535:
        raise ValueError("at most 65535 slots and 65535 rows (got %d slots, %d rows)" % (n, a * k))
    _check_boxes(boxes, n)
    if frame_index is not None:
        _check_out(frame_index, torch.int32, (s,), "frame_index")
    if dt is not None:
        _check_out(dt, torch.float64, (s,), "dt")
    if best_q is not None:
        _check_out(best_q, torch.float64, (n,), "best_q")
    if reset is not None:
        _check_out(reset, torch.int32, (n,), "reset")
    out = dict(out or {})
    rows, dev = a * k, m_crop.device
    spec = (("slot", torch.int32, (rows,), True), ("m", torch.float32, (rows, 2, 3), True),
            ("boxes", torch.int32, (rows, 4), True), ("frame_index", torch.int32, (rows,), True),
            ("dt", torch.float64, (rows,), dt is not None), ("best_q", torch.float64, (rows,), best_q is not None),
            ("reset", torch.int32, (rows,), reset is not None))
    if set(out) - {name for name, *_ in spec}:
        raise ValueError("out names %r, which the gather does not write" % sorted(set(out) - {n_ for n_, *_ in spec}))
    for name, dtype, shape, wanted in spec:
        if not wanted:
            if out.get(name) is not None:
                raise ValueError("out[%r] needs its input" % name)
            out.pop(name, None)
        elif out.get(name) is None:
            out[name] = torch.empty(shape, dtype=dtype, device=dev)
        else:
            _check_out(out[name], dtype, shape, "out[%r]" % name)
    _check_overlap(out["m"], m_crop, "out['m'] and m_crop")
    _check_overlap(out["boxes"], boxes, "out['boxes'] and boxes")
    _check_overlap(out.get("best_q"), best_q, "out['best_q'] and best_q")
    _check_overlap(out.get("reset"), reset, "out['reset'] and reset")
    p = _ptr
    _lib.check(_lib.load().flm_track_gather_streams(
        _lib.stream_ptr(), _lib.ptr(active), a, s, k, p(frame_index), p(dt), _lib.ptr(m_crop), _lib.ptr(boxes), p(best_q),
        p(reset), _lib.ptr(out["slot"]), _lib.ptr(out["m"]), _lib.ptr(out["boxes"]), _lib.ptr(out["frame_index"]),
        p(out.get("dt")), p(out.get("best_q")), p(out.get("reset"))), "flm_track_gather_streams")
    return out


def _track_gather_live(m_crop, boxes, slots_per_stream, frame_hw, budget, stream_on, frame_index, dt, best_q, reset, age,
                       cursor, out, flow_frame=None, flow_ready=None):
    """The one statement of `track_gather_live_device` and, with flow_frame and flow_ready, of `track_gather_flow_device`:
    the flow form adds the two state tensors, the "prev_frame_index" column and two more counts."""
    import torch
    k, n_rows = int(slots_per_stream), int(budget)
    fh, fw = [int(v) for v in frame_hw]
    _check_matrices(m_crop, None, "m_crop")
    n = int(m_crop.shape[0])
    if k < 1 or n < 1 or n % k:
        raise ValueError("m_crop holds %d slots: slots_per_stream=%d must be >= 1 and divide it" % (n, k))
    s = n // k
    if n > 65535 or not 1 <= n_rows <= 65535:
        raise ValueError("at most 65535 slots and a budget in [1, 65535] (got %d slots, budget %d)" % (n, n_rows))
    _check_boxes(boxes, n)
    dt_dev, dt_host = None, 0.0
    if age is None:
        if dt is not None:
            raise ValueError("dt goes with age")
    elif isinstance(dt, torch.Tensor):
        dt_dev = dt
    elif dt is None or isinstance(dt, bool) or not (float(dt) > 0.0 and float(dt) < float("inf")):
        raise ValueError("with age, dt must be a finite number > 0 or a CUDA float64 [%d] tensor (got %r)" % (s, dt))
    else:
        dt_host = float(dt)
    flow = flow_ready is not None
    for x, dtype, shape, what in ((stream_on, torch.int32, (s,), "stream_on"), (frame_index, torch.int32, (s,), "frame_index"),
                                  (flow_frame, torch.int32, (n,), "flow_frame"), (flow_ready, torch.int32, (n,), "flow_ready"),
                                  (dt_dev, torch.float64, (s,), "dt"), (best_q, torch.float64, (n,), "best_q"),
                                  (reset, torch.int32, (n,), "reset"), (age, torch.float64, (n,), "age"),
                                  (cursor, torch.int32, (1,), "cursor")):
        if x is not None:
            _check_out(x, dtype, shape, what)
    out = dict(out or {})
    dev = m_crop.device
    spec = (("slot", torch.int32, (n_rows,), True), ("m", torch.float32, (n_rows, 2, 3), True),
            ("boxes", torch.int32, (n_rows, 4), True), ("frame_index", torch.int32, (n_rows,), True),
            ("dt", torch.float64, (n_rows,), age is not None), ("best_q", torch.float64, (n_rows,), best_q is not None),
            ("reset", torch.int32, (n_rows,), reset is not None), ("counts", torch.int32, (6 if flow else 4,), True),
            ("prev_frame_index", torch.int32, (n_rows,), flow))
    if set(out) - {name for name, *_ in spec}:
        raise ValueError("out names %r, which the gather does not write" % sorted(set(out) - {n_ for n_, *_ in spec}))
    for name, dtype, shape, wanted in spec:
        if not wanted:
            if out.get(name) is not None:
                raise ValueError("out[%r] needs its input" % name)
            out.pop(name, None)
        elif out.get(name) is None:
            out[name] = torch.empty(shape, dtype=dtype, device=dev)
        else:
            _check_out(out[name], dtype, shape, "out[%r]" % name)
    _check_overlap(out["m"], m_crop, "out['m'] and m_crop")
    _check_overlap(out["boxes"], boxes, "out['boxes'] and boxes")
    _check_overlap(out.get("best_q"), best_q, "out['best_q'] and best_q")
    _check_overlap(out.get("reset"), reset, "out['reset'] and reset")
    _check_overlap(out.get("dt"), age, "out['dt'] and age")
    p = _ptr
    if flow:
        _lib.check(_lib.load().flm_track_gather_flow(
            _lib.stream_ptr(), p(stream_on), s, k, fh, fw, n_rows, p(frame_index), p(dt_dev), dt_host, _lib.ptr(m_crop),
            _lib.ptr(boxes), p(best_q), p(reset), p(age), p(cursor), _lib.ptr(flow_frame), _lib.ptr(flow_ready),
            _lib.ptr(out["slot"]), _lib.ptr(out["m"]), _lib.ptr(out["boxes"]), _lib.ptr(out["frame_index"]),
            _lib.ptr(out["prev_frame_index"]), p(out.get("dt")), p(out.get("best_q")), p(out.get("reset")),
            _lib.ptr(out["counts"])), "flm_track_gather_flow")
        return out
    _lib.check(_lib.load().flm_track_gather_live(
        _lib.stream_ptr(), p(stream_on), s, k, fh, fw, n_rows, p(frame_index), p(dt_dev), dt_host, _lib.ptr(m_crop),
        _lib.ptr(boxes), p(best_q), p(reset), p(age), p(cursor), _lib.ptr(out["slot"]), _lib.ptr(out["m"]),
        _lib.ptr(out["boxes"]), _lib.ptr(out["frame_index"]), p(out.get("dt")), p(out.get("best_q")), p(out.get("reset")),
        _lib.ptr(out["counts"])), "flm_track_gather_live")
    return out


def track_gather_live_device(m_crop, boxes, slots_per_stream, frame_hw, budget, stream_on=None, frame_index=None,
                             dt=None, best_q=None, reset=None, age=None, cursor=None, out=None):
    """The snapshot a step of the LIVE slots starts from, in one launch (flm_track_gather_live; include/flm.h states it):
    `track_gather_streams_device` with the row map made on the device from the slots' boxes.

    m_crop CUDA float32 [S*K,2,3] and boxes CUDA int32 [S*K,4]: the tracker's state, K = slots_per_stream; frame_hw:
    (H, W) of the frames, what a box is clipped to; budget: a host integer, the number of rows.  stream_on: None (every
    stream) or CUDA int32 [S], non-zero for the streams whose slots may be served; frame_index: None (ring slot 0) or
    CUDA int32 [S]; best_q: None or CUDA float64 [S*K]; reset: None or CUDA int32 [S*K], read and then cleared for the
    slots that are served.  age: None or CUDA float64 [S*K], the seconds every slot has waited unserved, read and
    written; with it `dt` is required, a host number or a CUDA float64 [S] tensor -- the time step of every stream -- and
    a served row's dt is its stream's plus its slot's age.  cursor: None or CUDA int32 [1], the slot the order starts
    from, read and written: live slots beyond the budget are served first by the next call.  Returns a dict of compact
    CUDA tensors over the `budget` rows, as `track_gather_streams_device` returns them -- slot int32 (-1: inert), m,
    boxes, frame_index, and dt (with age), best_q, reset, each present when its input is -- plus counts int32 [4]:
    (eligible slots, rows served, eligible slots left out, the next cursor).  out: None or a dict that names where to
    write (any of those keys); only what it does not name is allocated."""
    return _track_gather_live(m_crop, boxes, slots_per_stream, frame_hw, budget, stream_on, frame_index, dt, best_q, reset,
                              age, cursor, out)


def track_gather_flow_device(m_crop, boxes, flow_frame, flow_ready, slots_per_stream, frame_hw, budget, stream_on=None,
                             frame_index=None, dt=None, best_q=None, reset=None, age=None, cursor=None, out=None):
    """The snapshot a FLOW tick of the live slots starts from, in one launch (flm_track_gather_flow; include/flm.h states
    it): `track_gather_live_device` over the live slots that have a usable history.

    flow_frame CUDA int32 [S*K], the ring slot every slot's history was found in, and flow_ready CUDA int32 [S*K], 1 where
    the history is usable -- read, and then cleared for every slot of a stream that is on (`track_flow_history_device`
    sets it again for the rows the tick serves alive).  The other arguments as `track_gather_live_device` takes them;
    cursor is a cursor of the flow ticks' own.  Returns its dict plus prev_frame_index int32 [budget], the ring slot of
    every row's previous frame, and with counts int32 [6]: (live slots, eligible slots: live with a history, rows served,
    eligible slots left out, live slots without a history, the next cursor)."""
    import torch
    for x, what in ((flow_frame, "flow_frame"), (flow_ready, "flow_ready")):
        if not isinstance(x, torch.Tensor):
            raise ValueError("%s must be a contiguous CUDA int32 [S*K] tensor" % what)
    return _track_gather_live(m_crop, boxes, slots_per_stream, frame_hw, budget, stream_on, frame_index, dt, best_q, reset,
                              age, cursor, out, flow_frame=flow_frame, flow_ready=flow_ready)


def track_step_rows_device(lm, m_crop_c, boxes_c, slot, grid_hw, in_hw, frame_hw, tmpl_crop, m_next, boxes_next, status,
                           tmpl_align=None, weights=None, min_points=2, min_score=0.0, min_side=0.0,
                           max_side=float("inf"), lm_frame=None, m_align=None, status_rows=None, filter=None, dt=None,
                           state=None, lm_raw=None):
    """`track_step_device` on the rows of a compacted batch, in one launch (flm_track_step_rows; include/flm.h).

    lm, weights, m_crop_c CUDA float32 [N,2,3] and boxes_c CUDA int32 [N,4] are read at the row; slot: contiguous CUDA
    int32 [N], the global slot of every row (outside [0, n_slots): the row is inert).  m_next CUDA float32 [n_slots,2,3],
    boxes_next CUDA int32 [n_slots,4], status CUDA int32 [n_slots] and, with `filter`, state CUDA float64 [n_slots,C,6]
    are the tracker's own tensors, written at the slot; slots no row names keep their bits.  m_next and boxes_next may be
    the tensors m_crop_c and boxes_c were gathered from, but not m_crop_c and boxes_c themselves.  dt: None (1/filter.fps),
    a host number, or a CUDA float64 [N] tensor of one time step per row (a row whose dt is not > 0 and finite loses its
    history and nothing else).  Returns (lm_frame float64 [N,C,2], m_align float32 [N,2,3] or None, status_rows int32
    [N]); lm_frame, m_align, status_rows and lm_raw name where to write."""
    lm_frame, m_align, _, _, _, status_rows = _track_step(
        lm, m_crop_c, boxes_c, grid_hw, in_hw, frame_hw, tmpl_crop, tmpl_align, weights, min_points, min_score, min_side,
        max_side, lm_frame, m_align, m_next, boxes_next, status, filter, dt, state, lm_raw, rows=True, slot=slot,
        status_rows=status_rows, m_what="m_crop_c", k_what="n_slots")
    return lm_frame, m_align, status_rows


def track_best_update_rows_device(faces, rec, lm, slot, best_q_c, best_q, gallery, best_frame, frame_id, status_rows=None,
                                  reset_c=None, weights=None, factor=None, m=None, opts=None, best_m=None, best_lm=None,
                                  best_rec=None):
    """`track_best_update_device` on the rows of a compacted batch, in one launch (flm_track_best_update_rows).

    faces (N faces), rec int64 [N,8], lm, weights, status_rows, reset_c int32 [N], factor float64 [N], m float32 [N,2,3]
    and best_q_c float64 [N] -- the snapshot of the slots' best quality, from `track_gather_streams_device` -- are read
    at the row; slot: contiguous CUDA int32 [N].  best_q float64 [n_slots], gallery [n_slots,...] of the faces' dtype and
    face shape, best_frame int64 [n_slots] and best_m, best_lm, best_rec (each or None) are the tracker's own, written in
    place at the slot of a row that is taken; an inert row and a slot no row names write nothing.  best_q_c and best_q
    must be two buffers.  Returns best_q."""
    return _track_best_update(faces, rec, lm, best_q_c, best_q, gallery, best_frame, frame_id, status_rows, reset_c, weights,
                              factor, m, opts, best_m, best_lm, best_rec, rows=True, slot=slot,
                              names=("N", "status_rows", "reset_c", "best_q_c", "best_q"))


# ---- head pose: where a face looks, from its landmarks (include/flm.h, "head pose") -----------------------------------
POSE_REC = _lib.POSE_REC


class HeadModel:
    """A rigid 3-D model of a face for flm_head_pose: `indices`, P distinct landmark numbers, and `points` float64 [P,3],
    their coordinates in the model frame -- X to the image's right, Y down, Z away from the camera, any unit -- with
    4 <= P <= 256.  The points must not be coplanar (the fit reports a coplanar set as not ok).  The two tensors are
    uploaded once per device and cached."""

    def __init__(self, indices, points):
        idx = np.asarray(indices)
        xyz = np.asarray(points, np.float64)
        if idx.ndim != 1 or idx.dtype.kind not in "iu" or xyz.shape != (idx.shape[0], 3):
            raise ValueError("a head model is P integer landmark indices and float64 [P,3] points")
        if not 4 <= idx.shape[0] <= 256:
            raise ValueError("a head model has 4 to 256 points (got %d)" % idx.shape[0])
        if idx.size and (idx.min() < 0 or idx.max() >= 2 ** 31):
            raise ValueError("a landmark index must be in [0, 2^31)")
        if len(set(int(v) for v in idx)) != idx.shape[0]:
            raise ValueError("the landmark indices of a head model must be distinct")
        if not np.isfinite(xyz).all():
            raise ValueError("the points of a head model must be finite")
        self.indices = np.ascontiguousarray(idx, np.int32)
        self.points = np.ascontiguousarray(xyz)
        self._dev = {}

    @classmethod
    def default(cls, n_landmarks):
        """The six-point model of the 68-landmark layout: nose tip, chin, the outer eye corners, the mouth corners."""
        if int(n_landmarks) != 68:
            raise ValueError("the default head model is defined for 68 landmarks; pass an alignment.HeadModel for %d"
                             % int(n_landmarks))
        return cls([30, 8, 36, 45, 48, 54],
                   [[0.0, 0.0, 0.0], [0.0, 330.0, 65.0], [-225.0, -170.0, 135.0], [225.0, -170.0, 135.0],
                    [-150.0, 150.0, 125.0], [150.0, 150.0, 125.0]])

    def __len__(self):
        return int(self.indices.shape[0])

    def tensors(self, device):
        """(indices int32 [P], points float64 [P,3]) on `device`."""
        import torch
        key = str(device)
        if key not in self._dev:
            self._dev[key] = (torch.from_numpy(self.indices).to(device), torch.from_numpy(self.points).to(device))
        return self._dev[key]

    def __repr__(self):
        return "HeadModel(%d points)" % len(self)


class HeadPose:
    """The options of flm_head_pose (include/flm.h): `model`, a HeadModel (None: HeadModel.default of the landmark count
    at hand); min_volume: the least normalised volume of the participating model points at which a fit counts (0 for
    coplanar points, at most 1); min_frontal in [0, 1]: a face whose R[2][2] -- the cosine between its normal and the
    optical axis -- lies below it gets a best-shot factor of 0."""

    def __init__(self, model=None, min_volume=1e-6, min_frontal=0.0):
        if model is not None and not isinstance(model, HeadModel):
            raise ValueError("model must be None or an alignment.HeadModel (got %r)" % (model,))
        min_volume, min_frontal = float(min_volume), float(min_frontal)
        if not min_volume >= 0.0:
            raise ValueError("min_volume must be >= 0 (got %r)" % min_volume)
        if not 0.0 <= min_frontal <= 1.0:
            raise ValueError("min_frontal must be in [0, 1] (got %r)" % min_frontal)
        self.model, self.min_volume, self.min_frontal = model, min_volume, min_frontal

    def model_for(self, n_landmarks):
        return self.model if self.model is not None else HeadModel.default(n_landmarks)

    def struct(self):
        return _lib.PoseOpts.make(self.min_volume, self.min_frontal)

    def __repr__(self):
        return "HeadPose(model=%r, min_volume=%r, min_frontal=%r)" % (self.model, self.min_volume, self.min_frontal)


def _check_span_overlap(a, b, what):
    """`_check_overlap` for views: the bytes from a view's first element to its last count, gaps included."""
    def span(t):
        last = sum((int(n) - 1) * int(st) for n, st in zip(t.shape, t.stride()))
        return t.data_ptr(), t.data_ptr() + (last + 1) * t.element_size()
    if a is None or b is None or not a.numel() or not b.numel():
        return
    (a0, a1), (b0, b1) = span(a), span(b)
    if a0 < b1 and b0 < a1:
        raise ValueError("%s must be two buffers that do not overlap" % what)


def head_pose_device(lm, model, weights=None, opts=None, slot=None, out=None, factor_out=None):
    """The head pose of N faces from their landmarks, in one launch (flm_head_pose; include/flm.h states it line by line).

    lm: CUDA float64 [N,C,2] and `weights` None or CUDA float64 [N,C] (both may be views of a landmark record tensor, read
    in place); model: a `HeadModel`; opts: None or a `HeadPose` (its own model is not read here).  slot: None -- `out` is
    float64 [N,18] and row r writes record r -- or CUDA int32 [N]: `out`, required, is float64 [n_slots,18], a row
    writes at its slot, an inert row (slot outside [0, n_slots)) writes nothing and a slot no row names keeps its bits.
    factor_out: None or CUDA float64 [N], written by row: R[2][2] of a fit that is ok and at least min_frontal, else 0.
    Returns `out`: {R row by row, s, mx, my, rms, count, ok, yaw, pitch, roll} per face."""
    import torch
    if not isinstance(model, HeadModel):
        raise ValueError("model must be an alignment.HeadModel (got %r)" % (model,))
    if opts is None:
        opts = HeadPose()
    elif not isinstance(opts, HeadPose):
        raise ValueError("opts must be None or a HeadPose (got %r)" % (opts,))
    lm, ls = _strided_points(lm)
    n, c = int(lm.shape[0]), int(lm.shape[1])
    weights, wst = _weights_arg(weights, n, c)
    if slot is None:
        out = _out(out, torch.float64, (n, POSE_REC), "out", lm.device)
        n_slots = 0
    else:
        _check_out(slot, torch.int32, (n,), "slot")
        if (not isinstance(out, torch.Tensor) or out.dtype != torch.float64 or out.dim() != 2 or int(out.shape[1]) != POSE_REC
                or not out.is_cuda or not out.is_contiguous() or not 1 <= int(out.shape[0]) <= 65535):
            raise ValueError("with slot, out must be a contiguous CUDA float64 [n_slots,%d] tensor of 1 to 65535 slots"
                             % POSE_REC)
        n_slots = int(out.shape[0])
    if factor_out is not None:
        _check_out(factor_out, torch.float64, (n,), "factor_out")
    for a, what in ((lm, "lm"), (weights, "weights"), (slot, "slot")):
        _check_span_overlap(a, out, "%s and out" % what)
        _check_span_overlap(a, factor_out, "%s and factor_out" % what)
    _check_span_overlap(out, factor_out, "out and factor_out")
    if n and c:
        idx, xyz = model.tensors(lm.device)
        co = opts.struct()
        _lib.check(_lib.load().flm_head_pose(_lib.stream_ptr(), _lib.ptr(lm), ls, _ptr(weights), wst, n, c, _lib.ptr(idx),
                                             _lib.ptr(xyz), len(model), _lib.C.byref(co), _ptr(slot), n_slots,
                                             _lib.ptr(out), _ptr(factor_out)), "flm_head_pose")
    return out


# ---- face parts: eye and mouth patches, openness and blink state (include/flm.h, "face parts", "openness") -------------
OPEN_REC, OPEN_STATE = _lib.OPEN_REC, _lib.OPEN_STATE
PART_FILL = 0.8   # FaceParts.default: the share of the patch's width that the part's width fills (an unmeasured guess)


class FaceParts:
    """A set of face parts for flm_part_affines / flm_warp_parts_frames: R parts, 1 <= R <= 8, each `indices[r]`, 2 to 32
    landmark numbers, and `templates[r]`, float64 [len(indices[r]),2], where those landmarks belong in PATCH pixels
    (x, y); `size` = (patch_h, patch_w), 1 to 256 each, one size for all parts.  A part is fitted over its points in the
    order given; an index may repeat.  The device tensors are uploaded once per device and cached."""

    def __init__(self, indices, templates, size):
        idx = [np.asarray(v) for v in indices]
        tm = [np.asarray(t, np.float64) for t in templates]
        if not 1 <= len(idx) <= _lib.PARTS_MAX or len(tm) != len(idx):
            raise ValueError("a set of parts has 1 to %d parts, one template per part" % _lib.PARTS_MAX)
        for v, t in zip(idx, tm):
            if v.ndim != 1 or v.dtype.kind not in "iu" or not 2 <= v.shape[0] <= _lib.PART_MAX_POINTS:
                raise ValueError("a part is 2 to %d integer landmark indices" % _lib.PART_MAX_POINTS)
            if v.min() < 0 or v.max() >= 2 ** 31:
                raise ValueError("a landmark index must be in [0, 2^31)")
            if t.shape != (v.shape[0], 2) or not np.isfinite(t).all():
                raise ValueError("the template of a part is finite float64 [points,2]")
        ph, pw = _sizes(size, "the patch size")
        if ph > _lib.PART_MAX_SIDE or pw > _lib.PART_MAX_SIDE:
            raise ValueError("a patch is at most %d x %d (got %dx%d)" % (_lib.PART_MAX_SIDE, _lib.PART_MAX_SIDE, ph, pw))
        r = len(idx)
        self.size = (ph, pw)
        self.counts = np.array([v.shape[0] for v in idx], np.int32)
        self.indices = np.full((r, _lib.PART_MAX_POINTS), -1, np.int32)
        self.templates = np.zeros((r, _lib.PART_MAX_POINTS, 2), np.float64)
        for i, (v, t) in enumerate(zip(idx, tm)):
            self.indices[i, :v.shape[0]] = v
            self.templates[i, :v.shape[0]] = t
        for a in (self.counts, self.indices, self.templates):
            a.setflags(write=False)
        self._dev, self._counts_arg = {}, None

    @classmethod
    def default(cls, n_landmarks, size=(32, 48)):
        """The right eye (36-41), the left eye (42-47) and the mouth (48-67) of the 68-landmark layout.  Each part's
        template is the part's points of `canonical_template`, scaled by one factor and centred in the patch so that the
        part's WIDTH fills PART_FILL = 0.8 of the patch's width; the factor, like the default size, is an unmeasured guess."""
        if int(n_landmarks) != 68:
            raise ValueError("the default face parts are defined for 68 landmarks; pass an alignment.FaceParts for %d"
                             % int(n_landmarks))
        ph, pw = _sizes(size, "the patch size")
        base = canonical_template(68, 2, 2)   # the unit square
        idx, tm = [], []
        for lo, hi in ((36, 42), (42, 48), (48, 68)):
            p = base[lo:hi]
            mn, mx = p.min(axis=0), p.max(axis=0)
            s = PART_FILL * (pw - 1) / (mx[0] - mn[0])
            tm.append((p - (mn + mx) / 2) * s + np.array([(pw - 1) / 2, (ph - 1) / 2]))
            idx.append(np.arange(lo, hi))
        return cls(idx, tm, (ph, pw))

    def __len__(self):
        return int(self.counts.shape[0])

    def part(self, r):
        """(indices int32 [n], template float64 [n,2]) of part r, as given."""
        n = int(self.counts[r])
        return self.indices[r, :n].copy(), self.templates[r, :n].copy()

    def tensors(self, device):
        """(indices int32 [R,32], templates float64 [R,32,2]) on `device`."""
        import torch
        key = str(device)
        if key not in self._dev:
            self._dev[key] = (torch.from_numpy(self.indices.copy()).to(device), torch.from_numpy(self.templates.copy()).to(device))
        return self._dev[key]

    def counts_arg(self):
        """The host array `part_n` of the C calls, made once: the calls only read it."""
        if self._counts_arg is None:
            self._counts_arg = (_lib.C.c_int32 * len(self))(*[int(v) for v in self.counts])
        return self._counts_arg

    def __repr__(self):
        return "FaceParts(%d parts of %s points, %dx%d)" % (len(self), list(self.counts), self.size[0], self.size[1])


def _check_parts(parts):
    if not isinstance(parts, FaceParts):
        raise ValueError("parts must be an alignment.FaceParts (got %r)" % (parts,))


def part_affines_device(lm, parts, weights=None, out=None, ok_out=None):
    """lm: CUDA float64 [K,C,2] frame-space landmarks and `weights` None or CUDA float64 [K,C] (both may be views of a
    landmark record tensor, read in place); parts: a `FaceParts` -> (CUDA float32 [K,R,2,3], the similarity frame px ->
    patch px of every part of every face, fitted to the part's own landmarks; CUDA int32 [K,R], 1 where the fit had two
    participating points or more and a positive variance -- elsewhere the matrix is the identity) (flm_part_affines)."""
    import torch
    _check_parts(parts)
    lm, ls = _strided_points(lm)
    k, c, r = int(lm.shape[0]), int(lm.shape[1]), len(parts)
    weights, wst = _weights_arg(weights, k, c)
    if out is None:
        out = torch.empty((k, r, 2, 3), dtype=torch.float32, device=lm.device)
    else:
        _check_out(out, torch.float32, (k, r, 2, 3), "out")
    ok_out = _out(ok_out, torch.int32, (k, r), "ok_out", lm.device)
    if k and c:
        idx, tm = parts.tensors(lm.device)
        _lib.check(_lib.load().flm_part_affines(_lib.stream_ptr(), _lib.ptr(lm), ls, _ptr(weights), wst, k, c, _lib.ptr(idx),
                                                _lib.ptr(tm), parts.counts_arg(), r, _lib.ptr(out), _lib.ptr(ok_out)),
                   "flm_part_affines")
    return out, ok_out


def warp_parts_frames_device(frames, lm, parts, weights=None, frame_index_dev=None, boxes_dev=None, samples=1, fmt=None,
                             src=None, out=None, affines_out=None, ok_out=None):
    """The patches of every part of every face in one launch (flm_warp_parts_frames): each part is cut from the frame
    under the similarity that takes the part's own landmarks onto its template.  frames, frame_index_dev, boxes_dev,
    samples, fmt, src: as warp_frames_device takes them (and with its result for a ring slot outside the ring and an empty
    box: a zero face); lm, weights, parts: as part_affines_device takes them.  Returns CUDA [K,R,ph,pw,3] float32, or
    [K,R] faces in `fmt`; `out`, when given, has that shape.  affines_out: None or contiguous CUDA float32 [K,R,2,3];
    ok_out: None or contiguous CUDA int32 [K,R]: they receive what part_affines_device returns.  A part whose fit is not
    ok gives a zero face.  Patch (f, r) has the bits warp_frames_device gives with m = affines[:, r] at the patch size."""
    import torch
    _check_parts(parts)
    if fmt is not None:
        _check_format(fmt)
    if src is not None:
        _check_frame_format(src)
        ring = src.ring(frames)
    elif (not isinstance(frames, torch.Tensor) or frames.dim() != 4 or frames.shape[3] != 3 or frames.dtype != torch.uint8
            or not frames.is_cuda or not frames.is_contiguous()):
        raise ValueError("frames must be a contiguous CUDA uint8 [F,H,W,3] tensor")
    lm, ls = _strided_points(lm)
    k, c, r = int(lm.shape[0]), int(lm.shape[1]), len(parts)
    weights, wst = _weights_arg(weights, k, c)
    if lm.device != frames.device:
        raise ValueError("lm must be on the device of frames (%s, got %s)" % (frames.device, lm.device))
    if samples not in (1, 2, 4):
        raise ValueError("samples must be 1, 2 or 4")
    ph, pw = parts.size
    if src is not None:
        nf, fh, fw, stride = ring
    else:
        nf, fh, fw = [int(v) for v in frames.shape[:3]]
        stride = fh * fw * 3
    if frame_index_dev is not None:
        _check_out(frame_index_dev, torch.int32, (k,), "frame_index_dev")
    if boxes_dev is not None:
        _check_boxes(boxes_dev, k)
    ofmt = fmt if fmt is not None else AlignedFormat()
    shape = (k, r) + tuple(ofmt.shape(1, ph, pw)[1:])
    if out is None:
        out = torch.empty(shape, dtype=ofmt.torch_dtype, device=frames.device)
    elif (not isinstance(out, torch.Tensor) or out.dtype != ofmt.torch_dtype or tuple(out.shape) != shape or not out.is_cuda
          or not out.is_contiguous()):
        raise ValueError("out must be a contiguous CUDA %s tensor of shape %s" % (ofmt.dtype, list(shape)))
    if affines_out is not None:
        _check_out(affines_out, torch.float32, (k, r, 2, 3), "affines_out")
    if ok_out is not None:
        _check_out(ok_out, torch.int32, (k, r), "ok_out")
    if not k or not c:
        return out
    idx, tm = parts.tensors(frames.device)
    cf = None if fmt is None else fmt.struct()
    cs = None if src is None else src.struct(frames)
    _lib.check(_lib.load().flm_warp_parts_frames(
        _lib.stream_ptr(), _lib.ptr(frames), stride, nf, fh, fw, _ptr(frame_index_dev), _ptr(boxes_dev), _lib.ptr(lm), ls,
        _ptr(weights), wst, c, _lib.ptr(idx), _lib.ptr(tm), parts.counts_arg(), r, k, _lib.ptr(out), ph, pw, int(samples),
        None if cf is None else _lib.C.byref(cf), None if cs is None else _lib.C.byref(cs), _ptr(affines_out),
        _ptr(ok_out)), "flm_warp_parts_frames")
    return out


class Openness:
    """The measures and thresholds of flm_face_openness (include/flm.h).  measures: a sequence of 1 to 8 entries
    ((a, b), ((u, l), ...)) -- the width pair of landmarks and 1 to 4 pairs across the opening -- or None for
    `Openness.default(68)`'s; close_below < open_above: the hysteresis of the closed state; min_closed <= max_closed:
    the closures that count as an event, in the unit of dt; min_width: the least width in frame px at which a measure is
    read; dt: the time step a FaceTracker without `smooth` gives every tick (one with `smooth` uses the step's own).
    THE FIVE DEFAULT NUMBERS ARE UNMEASURED GUESSES: no trained checkpoint and no labelled blink data stand behind them."""

    DEFAULT_MEASURES = (((36, 39), ((37, 41), (38, 40))), ((42, 45), ((43, 47), (44, 46))),
                        ((60, 64), ((61, 67), (62, 66), (63, 65))))

    def __init__(self, measures=None, close_below=0.18, open_above=0.22, min_closed=0.03, max_closed=0.5, min_width=4.0,
                 dt=1.0 / 30.0):
        import math
        if measures is None:
            measures = self.DEFAULT_MEASURES
        try:
            ms = tuple(((int(a), int(b)), tuple((int(u), int(l)) for u, l in pairs)) for (a, b), pairs in measures)
        except (TypeError, ValueError):
            raise ValueError("a measure is ((a, b), ((u, l), ...)): a width pair and 1 to 4 pairs of landmark indices") from None
        if not 1 <= len(ms) <= _lib.OPEN_MAX_MEASURES or any(not 1 <= len(p) <= _lib.OPEN_MAX_PAIRS for _, p in ms):
            raise ValueError("openness takes 1 to %d measures of 1 to %d pairs each" % (_lib.OPEN_MAX_MEASURES, _lib.OPEN_MAX_PAIRS))
        if any(not -2 ** 31 <= v < 2 ** 31 for (a, b), p in ms for v in (a, b) + tuple(x for q in p for x in q)):
            raise ValueError("a landmark index must fit int32")
        close_below, open_above, min_closed, max_closed, min_width, dt = [
            float(v) for v in (close_below, open_above, min_closed, max_closed, min_width, dt)]
        if not close_below < open_above:
            raise ValueError("close_below must be below open_above (got %r, %r)" % (close_below, open_above))
        if not (min_closed >= 0.0 and max_closed >= 0.0 and min_width >= 0.0):
            raise ValueError("min_closed, max_closed and min_width must be >= 0")
        if max_closed < min_closed:
            raise ValueError("max_closed must not be below min_closed")
        if not (dt > 0.0 and math.isfinite(dt)):
            raise ValueError("dt must be finite and > 0 (got %r)" % dt)
        self.measures = ms
        self.close_below, self.open_above, self.min_closed, self.max_closed = close_below, open_above, min_closed, max_closed
        self.min_width, self.dt = min_width, dt
        self._struct = None

    @classmethod
    def default(cls, n_landmarks, **kw):
        """Both eyes and the inner mouth of the 68-landmark layout: right eye, width (36,39), pairs (37,41) (38,40); left
        eye, width (42,45), pairs (43,47) (44,46); inner mouth, width (60,64), pairs (61,67) (62,66) (63,65)."""
        if int(n_landmarks) != 68:
            raise ValueError("the default openness measures are defined for 68 landmarks; pass an alignment.Openness for %d"
                             % int(n_landmarks))
        return cls(cls.DEFAULT_MEASURES, **kw)

    def __len__(self):
        return len(self.measures)

    def struct(self):
        """The flm_open_opts of these options, made once: the calls only read it."""
        if self._struct is None:
            self._struct = _lib.OpenOpts.make(self.measures, close_below=self.close_below, open_above=self.open_above,
                                              min_closed=self.min_closed, max_closed=self.max_closed,
                                              min_width=self.min_width)
        return self._struct

    def __repr__(self):
        return ("Openness(%d measures, close_below=%r, open_above=%r, min_closed=%r, max_closed=%r, min_width=%r)"
                % (len(self), self.close_below, self.open_above, self.min_closed, self.max_closed, self.min_width))


OPEN_STATE_EMPTY = (0.0, 0.0, 0.0, -1.0, 0.0, 0.0, -1.0, 0.0)   # the state of a measure after a reset


def face_openness_device(lm, opts=None, weights=None, slot=None, out=None, state=None, reset=None, dt=None,
                         status_rows=None, frame_id=0):
    """How open the eyes and the mouth of N faces are, and their closure counts, in one launch (flm_face_openness;
    include/flm.h states it line by line).

    lm: CUDA float64 [N,C,2] and `weights` None or CUDA float64 [N,C] (views of a landmark record tensor are read in
    place); opts: None (`Openness()`) or an `Openness` of G measures.  slot: None -- `out` is float64 [N,G,4] and row r
    writes record r -- or CUDA int32 [N]: `out`, required, is float64 [n_slots,G,4], a row writes at its slot, an inert
    row writes nothing and a slot no row names keeps its bits.  state: None, or contiguous CUDA float64 [N or n_slots,G,8],
    updated in place, with `reset` CUDA int32 [N or n_slots] (a non-zero flag empties the slot's state first and is
    cleared by the call), dt: a host number or a CUDA float64 [N] tensor by row (None: the Openness's dt), status_rows:
    None or CUDA int32 [N] (a row whose status is not 0 leaves its state alone) and frame_id.  Returns `out`:
    {openness or -1, width, ok, sum} per face and measure."""
    import torch
    if opts is None:
        opts = Openness()
    elif not isinstance(opts, Openness):
        raise ValueError("opts must be None or an alignment.Openness (got %r)" % (opts,))
    lm, ls = _strided_points(lm)
    n, c, g = int(lm.shape[0]), int(lm.shape[1]), len(opts)
    weights, wst = _weights_arg(weights, n, c)
    if slot is None:
        out = _out(out, torch.float64, (n, g, OPEN_REC), "out", lm.device)
        rows, n_slots = n, 0
    else:
        _check_out(slot, torch.int32, (n,), "slot")
        if (not isinstance(out, torch.Tensor) or out.dtype != torch.float64 or out.dim() != 3
                or tuple(out.shape[1:]) != (g, OPEN_REC) or not out.is_cuda or not out.is_contiguous()
                or not 1 <= int(out.shape[0]) <= 65535):
            raise ValueError("with slot, out must be a contiguous CUDA float64 [n_slots,%d,%d] tensor of 1 to 65535 slots"
                             % (g, OPEN_REC))
        rows = n_slots = int(out.shape[0])
    dt_dev, dt_host = None, opts.dt
    if state is not None:
        _check_out(state, torch.float64, (rows, g, OPEN_STATE), "state")
        if reset is None:
            raise ValueError("state goes with reset, a CUDA int32 [%d] tensor" % rows)
        _check_out(reset, torch.int32, (rows,), "reset")
        if isinstance(dt, torch.Tensor):
            _check_out(dt, torch.float64, (n,), "dt")
            dt_dev = dt
        elif dt is not None:
            dt_host = float(dt)
            if not (dt_host > 0.0 and dt_host < float("inf")):
                raise ValueError("dt must be finite and > 0 (got %r)" % (dt,))
        if status_rows is not None:
            _check_out(status_rows, torch.int32, (n,), "status_rows")
    elif reset is not None or dt is not None or status_rows is not None:
        raise ValueError("reset, dt and status_rows go with state")
    frame_id = _frame_id(frame_id)
    outs = [(out, "out"), (state, "state"), (reset, "reset")]
    for a, what in ((lm, "lm"), (weights, "weights"), (slot, "slot"), (dt_dev, "dt"), (status_rows, "status_rows")):
        for b, name in outs:
            _check_span_overlap(a, b, "%s and %s" % (what, name))
    for i, (a, what) in enumerate(outs):
        for b, name in outs[i + 1:]:
            _check_span_overlap(a, b, "%s and %s" % (what, name))
    if n and c:
        co = opts.struct()
        _lib.check(_lib.load().flm_face_openness(
            _lib.stream_ptr(), _lib.ptr(lm), ls, _ptr(weights), wst, n, c, _lib.C.byref(co), _ptr(slot), n_slots,
            _lib.ptr(out), _ptr(state), _ptr(reset), _ptr(dt_dev), dt_host, _ptr(status_rows), frame_id), "flm_face_openness")
    return out


# ---- finished tracks: track ids and the exit queue of best shots (include/flm.h, flm_track_retire) ---------------------
EXIT_META = 8   # FLM_EXIT_META: track_id, slot, born_frame, frame_id of the end, best_frame, end, seq, 0


class TrackExits:
    """The exit queue of a tracker (flm_track_retire; include/flm.h): a ring of `capacity` rows, 1 to 65535, one per
    finished track, holding its best shot; min_q >= 0: a track whose best quality lies below it -- or that never had a
    best shot -- is discarded and only counted."""

    def __init__(self, capacity=256, min_q=0.0):
        if isinstance(capacity, bool) or int(capacity) != capacity or not 1 <= int(capacity) <= 65535:
            raise ValueError("capacity must be an integer in [1, 65535] (got %r)" % (capacity,))
        min_q = float(min_q)
        if not min_q >= 0.0:
            raise ValueError("min_q must be >= 0 and not NaN (got %r)" % min_q)
        self.capacity, self.min_q = int(capacity), min_q

    def struct(self):
        return _lib.ExitOpts.make(self.min_q)

    def __repr__(self):
        return "TrackExits(capacity=%r, min_q=%r)" % (self.capacity, self.min_q)


def track_retire_device(boxes, status, frame_hw, best_q, gallery, best_frame, born, track_id, born_frame, head, x_faces,
                        x_meta, x_q, exit_row, frame_id, flush=False, opts=None, best_m=None, best_lm=None, best_rec=None,
                        x_m=None, x_lm=None, x_rec=None):
    """Retire the tracks that have ended and name the ones that have begun, in two launches (flm_track_retire;
    include/flm.h states it line by line).

    Read: boxes CUDA int32 [K,4], status CUDA int32 [K], frame_hw; best_q CUDA float64 [K], gallery a contiguous CUDA
    tensor of K faces (any format: copied as bytes), best_frame CUDA int64 [K]; best_m, best_lm, best_rec: None or CUDA
    float32 [K,2,3], float64 [K,C,2], int64 [K,8], each together with x_m, x_lm, x_rec over the Q ring rows.  In/out:
    born CUDA int32 [K] (non-zero: a track was started in the slot since the last call; cleared), track_id CUDA int64 [K]
    (-1: no track), born_frame CUDA int64 [K], head CUDA int64 [4] = (seq, next_id, discarded, overrun).  Out: the ring
    x_faces (Q faces of the gallery's dtype and face shape), x_meta CUDA int64 [Q,8], x_q CUDA float64 [Q]; exit_row CUDA
    int32 [K]: -1 nothing ended, -2 discarded, -3 overrun, else the ring row.  frame_id: a host integer; flush: end every
    held track; opts: None or a `TrackExits` (its capacity must be Q).  No two tensors may overlap.  Returns exit_row."""
    import torch
    if opts is None:
        opts = TrackExits(capacity=int(x_meta.shape[0]) if isinstance(x_meta, torch.Tensor) and x_meta.dim() else 256)
    elif not isinstance(opts, TrackExits):
        raise ValueError("opts must be None or a TrackExits (got %r)" % (opts,))
    frame_id = _frame_id(frame_id)
    fh, fw = _sizes(frame_hw, "frame_hw")
    if not isinstance(boxes, torch.Tensor) or boxes.dim() != 2 or not 1 <= int(boxes.shape[0]) <= 65535:
        raise ValueError("boxes must be a contiguous CUDA int32 [K,4] tensor of 1 to 65535 slots")
    k = int(boxes.shape[0])
    _check_boxes(boxes, k)
    if (not isinstance(gallery, torch.Tensor) or gallery.dim() < 1 or int(gallery.shape[0]) != k or not gallery.is_cuda
            or not gallery.is_contiguous() or gallery.numel() < k):
        raise ValueError("gallery must be a contiguous CUDA tensor of %d faces" % k)
    if (not isinstance(x_faces, torch.Tensor) or x_faces.dtype != gallery.dtype or x_faces.dim() != gallery.dim()
            or x_faces.shape[1:] != gallery.shape[1:] or not x_faces.is_cuda or not x_faces.is_contiguous()):
        raise ValueError("x_faces must be a contiguous CUDA tensor of the dtype and face shape of gallery")
    q = int(x_faces.shape[0])
    if not 1 <= q <= 65535 or q != opts.capacity:
        raise ValueError("the ring must have the %d rows of opts, 1 to 65535 (x_faces has %d)" % (opts.capacity, q))
    _check_out(status, torch.int32, (k,), "status")
    _check_out(best_q, torch.float64, (k,), "best_q")
    _check_out(best_frame, torch.int64, (k,), "best_frame")
    _check_out(born, torch.int32, (k,), "born")
    _check_out(track_id, torch.int64, (k,), "track_id")
    _check_out(born_frame, torch.int64, (k,), "born_frame")
    _check_out(head, torch.int64, (4,), "head")
    _check_out(x_meta, torch.int64, (q, EXIT_META), "x_meta")
    _check_out(x_q, torch.float64, (q,), "x_q")
    _check_out(exit_row, torch.int32, (k,), "exit_row")
    for a, b, what in ((best_m, x_m, "best_m and x_m"), (best_lm, x_lm, "best_lm and x_lm"), (best_rec, x_rec, "best_rec and x_rec")):
        if (a is None) != (b is None):
            raise ValueError("%s go together: both or neither" % what)
    c = 1
    if best_m is not None:
        _check_matrices(best_m, k, "best_m")
        _check_matrices(x_m, q, "x_m")
    if best_lm is not None:
        if not isinstance(best_lm, torch.Tensor) or best_lm.dim() != 3 or not 1 <= int(best_lm.shape[1]) <= 1024:
            raise ValueError("best_lm must be a contiguous CUDA float64 [%d,C,2] tensor, 1 <= C <= 1024" % k)
        c = int(best_lm.shape[1])
        _check_out(best_lm, torch.float64, (k, c, 2), "best_lm")
        _check_out(x_lm, torch.float64, (q, c, 2), "x_lm")
    if best_rec is not None:
        _check_out(best_rec, torch.int64, (k, QUALITY_REC), "best_rec")
        _check_out(x_rec, torch.int64, (q, QUALITY_REC), "x_rec")
    named = [(boxes, "boxes"), (status, "status"), (best_q, "best_q"), (gallery, "gallery"), (best_frame, "best_frame"),
             (best_m, "best_m"), (best_lm, "best_lm"), (best_rec, "best_rec"), (born, "born"), (track_id, "track_id"),
             (born_frame, "born_frame"), (head, "head"), (x_faces, "x_faces"), (x_meta, "x_meta"), (x_q, "x_q"), (x_m, "x_m"),
             (x_lm, "x_lm"), (x_rec, "x_rec"), (exit_row, "exit_row")]
    spans = sorted((t.data_ptr(), t.data_ptr() + t.numel() * t.element_size(), name) for t, name in named if t is not None)
    for (_, end, an), (start, _, bn) in zip(spans, spans[1:]):         # sorted by address: neighbours are enough
        if start < end:
            raise ValueError("%s and %s must be two buffers that do not overlap" % (an, bn))
    co = opts.struct()
    _lib.check(_lib.load().flm_track_retire(
        _lib.stream_ptr(), _lib.ptr(boxes), _lib.ptr(status), k, fh, fw, _lib.ptr(best_q), _lib.ptr(gallery),
        gallery.numel() // k * gallery.element_size(), _lib.ptr(best_frame), _ptr(best_m), _ptr(best_lm), c, _ptr(best_rec),
        frame_id, 1 if flush else 0, _lib.C.byref(co), _lib.ptr(born), _lib.ptr(track_id), _lib.ptr(born_frame),
        _lib.ptr(head), q, _lib.ptr(x_faces), _lib.ptr(x_meta), _lib.ptr(x_q), _ptr(x_m), _ptr(x_lm), _ptr(x_rec),
        _lib.ptr(exit_row)), "flm_track_retire")
    return exit_row


def exit_rows(seq, cursor, capacity):
    """The consumer's side of the exit ring, on the host: `seq` is head[0] as the consumer downloaded it, `cursor` the
    sequence number it has read up to (0 at the start; afterwards the `seq` of its previous look), `capacity` the ring's
    rows.  Returns (rows, lost): the ring rows of the exits that are new and still in the ring, oldest first, as an int64
    array, and how many new exits were overwritten before they were read (wrap-around).  The exit of sequence number s
    lies in row s % capacity; the ring keeps the last `capacity` of them."""
    for v, what in ((seq, "seq"), (cursor, "cursor"), (capacity, "capacity")):
        if isinstance(v, bool) or int(v) != v:
            raise ValueError("%s must be an integer (got %r)" % (what, v))
    seq, cursor, capacity = int(seq), int(cursor), int(capacity)
    if not 1 <= capacity <= 65535:
        raise ValueError("capacity must be in [1, 65535] (got %d)" % capacity)
    if not 0 <= cursor <= seq:
        raise ValueError("0 <= cursor <= seq is needed (got cursor %d, seq %d)" % (cursor, seq))
    lost = max(seq - cursor - capacity, 0)
    return np.arange(cursor + lost, seq, dtype=np.int64) % capacity, lost


# ---- pose-binned best shots: one best face per view of every track (include/flm.h, flm_track_views_update) -------------
VIEWS_MAX_EDGES = _lib.VIEWS_MAX_EDGES


class PoseViews:
    """The pose bins of a tracker's multi-view gallery (flm_track_views_update; include/flm.h): `yaw` and `pitch`, each a
    strictly ascending sequence of at most 7 edges in DEGREES inside (-90, 90), cut the faces of a track into
    (len(yaw)+1) x (len(pitch)+1) bins, and the tracker keeps the best face of every bin.  The default, yaw=(-20, 20) and
    no pitch edge, gives three views: bin 0 a face turned to the image's right (yaw < -20), bin 1 frontal, bin 2 turned to
    the image's left.  An edge d becomes math.sin(math.radians(d)), in float64 on the host, and is compared on the device
    with u = -R[2][0] = cos(pitch)*sin(yaw) (yaw edges) or v = R[2][1] = sin(pitch) (pitch edges) of the head-pose record:
    a pitch edge is exact, a yaw edge is exact at pitch 0 and lies at a slightly larger yaw on a face that also looks up
    or down.  u >= edge falls into the upper bin; bin = iv*(len(yaw)+1) + iu.  sharp_ref, min_exposed: as `BestShot`; the
    quality of a view is min(sharpness/sharp_ref, 1) x the exposed share x the mean landmark score, WITHOUT the
    frontality factor of the best shot -- the bin accounts for pose.  `from_edges` takes raw u and v edges."""

    def __init__(self, yaw=(-20.0, 20.0), pitch=(), sharp_ref=100.0, min_exposed=0.5):
        edges = []
        for name, deg in (("yaw", yaw), ("pitch", pitch)):
            try:
                deg = [float(d) for d in deg]
            except (TypeError, ValueError):
                raise ValueError("%s must be a sequence of edges in degrees (got %r)" % (name, deg)) from None
            if any(not -90.0 < d < 90.0 for d in deg):
                raise ValueError("%s edges must lie inside (-90, 90) degrees (got %r)" % (name, deg))
            edges.append([math.sin(math.radians(d)) for d in deg])
        self._set(edges[0], edges[1], sharp_ref, min_exposed)

    @classmethod
    def from_edges(cls, u_edges, v_edges=(), sharp_ref=100.0, min_exposed=0.5):
        """Raw edges: u_edges on u = -R[2][0], v_edges on v = R[2][1], each strictly ascending inside (-1, 1)."""
        o = cls.__new__(cls)
        o._set(u_edges, v_edges, sharp_ref, min_exposed)
        return o

    def _set(self, u_edges, v_edges, sharp_ref, min_exposed):
        out = []
        for name, e in (("u", u_edges), ("v", v_edges)):
            try:
                e = [float(x) for x in e]
            except (TypeError, ValueError):
                raise ValueError("%s edges must be a sequence of numbers (got %r)" % (name, e)) from None
            if len(e) > VIEWS_MAX_EDGES:
                raise ValueError("at most %d %s edges (got %d)" % (VIEWS_MAX_EDGES, name, len(e)))
            if any(not -1.0 < x < 1.0 for x in e):
                raise ValueError("%s edges must be finite and inside (-1, 1) (got %r)" % (name, e))
            if any(not b > a for a, b in zip(e, e[1:])):
                raise ValueError("%s edges must be strictly ascending (got %r)" % (name, e))
            out.append(tuple(e))
        sharp_ref, min_exposed = float(sharp_ref), float(min_exposed)
        if not sharp_ref > 0.0:
            raise ValueError("sharp_ref must be > 0 (got %r)" % sharp_ref)
        if min_exposed != min_exposed:
            raise ValueError("min_exposed must not be NaN")
        self.u_edges, self.v_edges = out
        self.sharp_ref, self.min_exposed = sharp_ref, min_exposed

    @property
    def bins(self):
        return (len(self.u_edges) + 1) * (len(self.v_edges) + 1)

    def struct(self):
        return _lib.ViewsOpts.make(self.u_edges, self.v_edges, self.sharp_ref, self.min_exposed)

    def __repr__(self):
        return "PoseViews.from_edges(%r, %r, sharp_ref=%r, min_exposed=%r)" % (self.u_edges, self.v_edges, self.sharp_ref,
                                                                               self.min_exposed)


def _check_no_overlap(named):
    """No two of the (tensor or None, name) pairs may share a byte."""
    spans = sorted((t.data_ptr(), t.data_ptr() + t.numel() * t.element_size(), name) for t, name in named
                   if t is not None and t.numel())
    for (_, end, an), (start, _, bn) in zip(spans, spans[1:]):         # sorted by address: neighbours are enough
        if start < end:
            raise ValueError("%s and %s must be two buffers that do not overlap" % (an, bn))


def _check_view_faces(t, lead, like, what):
    """`t` is a contiguous CUDA tensor [*lead, face...] of the dtype and face shape of `like` ([N, face...])."""
    import torch
    nl = len(lead)
    if (not isinstance(t, torch.Tensor) or t.dtype != like.dtype or t.dim() != like.dim() - 1 + nl
            or tuple(t.shape[:nl]) != tuple(lead) or t.shape[nl:] != like.shape[1:] or not t.is_cuda or not t.is_contiguous()):
        raise ValueError("%s must be a contiguous CUDA tensor [%s,...] of the dtype and face shape of the faces"
                         % (what, ",".join(str(v) for v in lead)))


def track_views_update_device(faces, rec, lm, pose, view_q, view_frame, view_gallery, take, frame_id, status=None,
                              reset=None, weights=None, m=None, opts=None, slot=None, view_m=None, view_lm=None,
                              view_pose=None):
    """Per row, keep the face if it beats what its slot holds in the face's POSE BIN, in two launches
    (flm_track_views_update; include/flm.h states it line by line).

    faces: contiguous CUDA tensor of N faces (any format: copied as bytes); rec CUDA int64 [N,8] from
    `face_quality_device`; lm CUDA float64 [N,C,2] and `weights` None or CUDA float64 [N,C] (both may be views of a
    landmark record tensor, read in place); status, reset: None or CUDA int32 [N]; m: None or CUDA float32 [N,2,3];
    frame_id: a host integer; opts: None or a `PoseViews`, B = opts.bins.  slot: None -- row r is slot r and
    n_slots = N -- or contiguous CUDA int32 [N]: a row writes at its slot, an inert row (slot outside [0, n_slots)) and a
    slot no row names write nothing.  pose: CUDA float64 [n_slots,18], the records `head_pose_device` wrote, read at
    the slot.  In/out: view_q CUDA float64 [n_slots,B] (-1: the bin holds nothing), view_frame CUDA int64 [n_slots,B],
    view_gallery [n_slots,B,...] of the faces' dtype and face shape, and view_m float32 [n_slots,B,2,3], view_lm float64
    [n_slots,B,C,2], view_pose float64 [n_slots,B,18], each or None.  Out: take CUDA int32 [N]: the bin a row's face was
    taken into, or -1.  A non-zero reset empties the slot's bins first; a face is taken when it is eligible, its pose is
    ok, and its quality -- the best shot's without the pose factor -- is strictly above its bin's.  No output may
    overlap an input or another output.  Returns take."""
    import torch
    if opts is None:
        opts = PoseViews()
    elif not isinstance(opts, PoseViews):
        raise ValueError("opts must be None or a PoseViews (got %r)" % (opts,))
    frame_id = _frame_id(frame_id)
    b = opts.bins
    if not isinstance(faces, torch.Tensor) or faces.dim() < 1 or not faces.is_cuda or not faces.is_contiguous():
        raise ValueError("faces must be a contiguous CUDA tensor of N faces")
    n = int(faces.shape[0])
    if not 1 <= n <= 65535:
        raise ValueError("1 to 65535 rows (got %d)" % n)
    if (not isinstance(pose, torch.Tensor) or pose.dtype != torch.float64 or pose.dim() != 2 or int(pose.shape[1]) != POSE_REC
            or not pose.is_cuda or not pose.is_contiguous() or not 1 <= int(pose.shape[0]) <= 65535):
        raise ValueError("pose must be a contiguous CUDA float64 [n_slots,%d] tensor of 1 to 65535 slots" % POSE_REC)
    n_slots = int(pose.shape[0])
    if slot is None:
        if n_slots != n:
            raise ValueError("without slot, pose must have one record per face ([%d,%d], got %d)" % (n, POSE_REC, n_slots))
    else:
        _check_out(slot, torch.int32, (n,), "slot")
    _check_out(rec, torch.int64, (n, QUALITY_REC), "rec")
    lm, ls = _strided_points(lm)
    c = int(lm.shape[1])
    if int(lm.shape[0]) != n or not 1 <= c <= 1024:
        raise ValueError("lm must be a CUDA float64 [%d,C,2] tensor, 1 <= C <= 1024" % n)
    weights, wst = _weights_arg(weights, n, c)
    for t, name in ((status, "status"), (reset, "reset")):
        if t is not None:
            _check_out(t, torch.int32, (n,), name)
    if m is not None:
        _check_matrices(m, n)
    _check_out(view_q, torch.float64, (n_slots, b), "view_q")
    _check_out(view_frame, torch.int64, (n_slots, b), "view_frame")
    _check_view_faces(view_gallery, (n_slots, b), faces, "view_gallery")
    _check_out(take, torch.int32, (n,), "take")
    if view_m is not None:
        if m is None:
            raise ValueError("view_m needs m")
        _check_out(view_m, torch.float32, (n_slots, b, 2, 3), "view_m")
    if view_lm is not None:
        _check_out(view_lm, torch.float64, (n_slots, b, c, 2), "view_lm")
    if view_pose is not None:
        _check_out(view_pose, torch.float64, (n_slots, b, POSE_REC), "view_pose")
    outs = [(view_q, "view_q"), (view_frame, "view_frame"), (view_gallery, "view_gallery"), (view_m, "view_m"),
            (view_lm, "view_lm"), (view_pose, "view_pose"), (take, "take")]
    _check_no_overlap(outs)
    for a, an in ((faces, "faces"), (rec, "rec"), (lm, "lm"), (weights, "weights"), (status, "status"), (reset, "reset"),
                  (m, "m"), (slot, "slot"), (pose, "pose")):
        for o, on in outs:
            _check_span_overlap(a, o, "%s and %s" % (an, on))
    co = opts.struct()
    _lib.check(_lib.load().flm_track_views_update(
        _lib.stream_ptr(), _lib.ptr(faces), faces.numel() // n * faces.element_size(), n, _lib.ptr(rec), _ptr(status),
        _ptr(reset), _lib.ptr(lm), ls, _ptr(weights), wst, c, _ptr(m), frame_id, _lib.C.byref(co), _ptr(slot), n_slots,
        _lib.ptr(pose), _lib.ptr(view_q), _lib.ptr(view_frame), _lib.ptr(view_gallery), _ptr(view_m), _ptr(view_lm),
        _ptr(view_pose), _lib.ptr(take)), "flm_track_views_update")
    return take


def track_exit_views_device(exit_row, view_q, view_frame, view_gallery, x_view_q, x_view_frame, x_view_gallery, view_m=None,
                            view_lm=None, view_pose=None, x_view_m=None, x_view_lm=None, x_view_pose=None):
    """The views of the tracks `track_retire_device` has just written, into the exit ring, in one launch
    (flm_track_exit_views; include/flm.h).

    exit_row: CUDA int32 [K], what that retire call returned.  view_q CUDA float64 [K,B], view_frame CUDA int64 [K,B],
    view_gallery a contiguous CUDA tensor [K,B,...] (any format: copied as bytes): the views as
    `track_views_update_device` keeps them; view_m float32 [K,B,2,3], view_lm float64 [K,B,C,2], view_pose float64
    [K,B,18]: each None or given together with its ring counterpart.  The ring of Q rows: x_view_q [Q,B], x_view_frame
    [Q,B], x_view_gallery [Q,B,...] of the gallery's dtype and face shape, x_view_m, x_view_lm, x_view_pose.  Ring row
    exit_row[t] >= 0 receives slot t's B qualities and frame ids and, for every bin whose quality is >= 0, the bin's
    face, matrix, landmarks and pose; an empty bin leaves its ring bytes as they were, and so does every slot whose
    exit_row is negative.  No two tensors may overlap.  Returns x_view_q."""
    import torch
    if (not isinstance(view_q, torch.Tensor) or view_q.dim() != 2 or not 1 <= int(view_q.shape[0]) <= 65535
            or not 1 <= int(view_q.shape[1]) <= 64):
        raise ValueError("view_q must be a contiguous CUDA float64 [K,B] tensor, 1 <= K <= 65535, 1 <= B <= 64")
    k, b = int(view_q.shape[0]), int(view_q.shape[1])
    _check_out(view_q, torch.float64, (k, b), "view_q")
    _check_out(exit_row, torch.int32, (k,), "exit_row")
    _check_out(view_frame, torch.int64, (k, b), "view_frame")
    if (not isinstance(x_view_q, torch.Tensor) or x_view_q.dim() != 2 or not 1 <= int(x_view_q.shape[0]) <= 65535):
        raise ValueError("x_view_q must be a contiguous CUDA float64 [Q,%d] tensor, 1 <= Q <= 65535" % b)
    q = int(x_view_q.shape[0])
    _check_out(x_view_q, torch.float64, (q, b), "x_view_q")
    _check_out(x_view_frame, torch.int64, (q, b), "x_view_frame")
    if (not isinstance(view_gallery, torch.Tensor) or view_gallery.dim() < 2 or tuple(view_gallery.shape[:2]) != (k, b)
            or not view_gallery.is_cuda or not view_gallery.is_contiguous() or view_gallery.numel() < k * b):
        raise ValueError("view_gallery must be a contiguous CUDA tensor of [%d,%d] faces" % (k, b))
    _check_view_faces(x_view_gallery, (q, b), view_gallery[:, 0], "x_view_gallery")
    for s, x, what in ((view_m, x_view_m, "view_m and x_view_m"), (view_lm, x_view_lm, "view_lm and x_view_lm"),
                       (view_pose, x_view_pose, "view_pose and x_view_pose")):
        if (s is None) != (x is None):
            raise ValueError("%s go together: both or neither" % what)
    c = 1
    if view_m is not None:
        _check_out(view_m, torch.float32, (k, b, 2, 3), "view_m")
        _check_out(x_view_m, torch.float32, (q, b, 2, 3), "x_view_m")
    if view_lm is not None:
        if not isinstance(view_lm, torch.Tensor) or view_lm.dim() != 4 or not 1 <= int(view_lm.shape[2]) <= 1024:
            raise ValueError("view_lm must be a contiguous CUDA float64 [%d,%d,C,2] tensor, 1 <= C <= 1024" % (k, b))
        c = int(view_lm.shape[2])
        _check_out(view_lm, torch.float64, (k, b, c, 2), "view_lm")
        _check_out(x_view_lm, torch.float64, (q, b, c, 2), "x_view_lm")
    if view_pose is not None:
        _check_out(view_pose, torch.float64, (k, b, POSE_REC), "view_pose")
        _check_out(x_view_pose, torch.float64, (q, b, POSE_REC), "x_view_pose")
    _check_no_overlap([(exit_row, "exit_row"), (view_q, "view_q"), (view_frame, "view_frame"), (view_gallery, "view_gallery"),
                       (view_m, "view_m"), (view_lm, "view_lm"), (view_pose, "view_pose"), (x_view_q, "x_view_q"),
                       (x_view_frame, "x_view_frame"), (x_view_gallery, "x_view_gallery"), (x_view_m, "x_view_m"),
                       (x_view_lm, "x_view_lm"), (x_view_pose, "x_view_pose")])
    _lib.check(_lib.load().flm_track_exit_views(
        _lib.stream_ptr(), _lib.ptr(exit_row), k, q, b, view_gallery.numel() // (k * b) * view_gallery.element_size(), c,
        _lib.ptr(view_q), _lib.ptr(view_frame), _lib.ptr(view_gallery), _ptr(view_m), _ptr(view_lm), _ptr(view_pose),
        _lib.ptr(x_view_q), _lib.ptr(x_view_frame), _lib.ptr(x_view_gallery), _ptr(x_view_m), _ptr(x_view_lm),
        _ptr(x_view_pose)), "flm_track_exit_views")
    return x_view_q


# ---- frame annotation: marks, boxes and mosaics written into the ring (include/flm.h, flm_frames_annotate) ------------------
class FrameAnnotation:
    """What `annotate_frames_device` writes into the ring for every face (flm_annotate_opts; include/flm.h states each
    layer): marks: the 21-pixel disc of `utils.plots.draw_marks` at every accepted landmark; box: the thickness in
    pixels of an outline of the face's region (0: none, at most 16); redact: the cell size in pixels of a mosaic over
    the region (0: none, else even and 2..64); margin (left, top, right, bottom): how far the region reaches beyond the
    box of the accepted landmarks, as fractions of that box's longer side, each in [0, 4]; mark_color, box_color: (B,G,R)
    bytes.  The default margins (0.1, 0.35, 0.1, 0.1) are guesses at "the face, forehead included" on the 68-point
    layout, whose topmost points are the eyebrows: nobody has measured them.  A caller who must not leak a face sets
    them generously."""

    def __init__(self, marks=True, box=0, redact=0, margin=(0.1, 0.35, 0.1, 0.1), mark_color=(0, 255, 0),
                 box_color=(0, 255, 0)):
        if not isinstance(marks, (bool, np.bool_)):
            raise ValueError("marks must be True or False (got %r)" % (marks,))
        for name, v in (("box", box), ("redact", redact)):
            if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
                raise ValueError("%s must be an integer (got %r)" % (name, v))
        if not 0 <= box <= 16:
            raise ValueError("box must be in [0, 16] (got %r)" % (box,))
        if redact != 0 and (redact < 2 or redact > 64 or redact % 2):
            raise ValueError("redact must be 0, or even and in [2, 64] (got %r)" % (redact,))
        try:
            margin = tuple(float(v) for v in margin)
        except (TypeError, ValueError):
            raise ValueError("margin must be four numbers (left, top, right, bottom) (got %r)" % (margin,)) from None
        if len(margin) != 4 or any(not 0.0 <= v <= 4.0 for v in margin):
            raise ValueError("margin must be four numbers in [0, 4] (got %r)" % (margin,))
        colors = []
        for name, col in (("mark_color", mark_color), ("box_color", box_color)):
            try:
                col = tuple(col)
            except TypeError:
                raise ValueError("%s must be three bytes (B, G, R) (got %r)" % (name, col)) from None
            if len(col) != 3 or any(isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer))
                                    or not 0 <= v <= 255 for v in col):
                raise ValueError("%s must be three bytes (B, G, R) (got %r)" % (name, col))
            colors.append(tuple(int(v) for v in col))
        self.marks, self.box, self.redact, self.margin = bool(marks), int(box), int(redact), margin
        self.mark_color, self.box_color = colors

    def struct(self):
        return _lib.AnnotateOpts.make(int(self.marks), self.box, self.redact, self.margin, self.mark_color, self.box_color)

    def __repr__(self):
        return "FrameAnnotation(marks=%r, box=%r, redact=%r, margin=%r, mark_color=%r, box_color=%r)" % (
            self.marks, self.box, self.redact, self.margin, self.mark_color, self.box_color)


def annotate_frames_device(frames, lm, frame_index_dev=None, opts=None, src=None, regions_out=None):
    """Marks, outlines and mosaics of K faces written INTO the ring (flm_frames_annotate; include/flm.h states every
    layer and the order they are applied in).

    frames: the ring, as `src` (a FrameFormat; None: FrameFormat.bgr()) holds it -- a contiguous CUDA uint8 [F,H,W,3]
    tensor, or the decoder's [F,rows,pitch] NV12 ring; lm: CUDA float64 [K,C,2] landmarks in FRAME pixels (a view of a
    landmark record tensor is read in place), rejected points (-1,-1) are skipped; frame_index_dev: None (every face lies
    in slot 0) or a contiguous CUDA int32 [K] tensor, a face whose index lies outside the ring is left out; opts: None or
    a `FrameAnnotation`; regions_out: None or a contiguous CUDA int32 [K,4] tensor.  Neither the landmarks nor
    regions_out may overlap the ring.  The slots are changed for every later reader: annotate a frame after the calls
    that still need its pixels.  No download, no synchronisation.  Returns the regions int32 [K,4] (x0,y0,x1,y1), unclipped."""
    import torch
    if opts is None:
        opts = FrameAnnotation()
    elif not isinstance(opts, FrameAnnotation):
        raise ValueError("opts must be None or a FrameAnnotation (got %r)" % (opts,))
    if src is None:
        src = FrameFormat.bgr()
    _check_frame_format(src)
    nf, fh, fw, stride = src.ring(frames)
    if src.pixel == "bgr" and (fw < 2 or fh < 1 or fh * fw * 3 >= 2 ** 31):
        raise ValueError("frames of %dx%d are outside the kernels' reach (width >= 2, H*W*3 < 2^31)" % (fh, fw))
    lm, ls = _strided_points(lm)
    k, c = int(lm.shape[0]), int(lm.shape[1])
    if k > 65535 or (opts.redact and k > 4096):
        raise ValueError("at most 65535 faces per call, 4096 with redact (got %d)" % k)
    if c > 1024:
        raise ValueError("at most 1024 landmarks per face (got %d)" % c)
    if frame_index_dev is not None:
        _check_out(frame_index_dev, torch.int32, (k,), "frame_index_dev")
    regions = _out(regions_out, torch.int32, (k, 4), "regions_out", frames.device)
    _check_span_overlap(lm, frames, "lm and the ring")
    _check_overlap(regions, frames, "regions_out and the ring")
    _check_span_overlap(lm, regions, "lm and regions_out")
    _check_overlap(frame_index_dev, frames, "frame_index_dev and the ring")
    _check_overlap(frame_index_dev, regions, "frame_index_dev and regions_out")
    if k and c:
        co, cs = opts.struct(), src.struct(frames)
        _lib.check(_lib.load().flm_frames_annotate(_lib.stream_ptr(), _lib.ptr(frames), stride, nf, fh, fw, _lib.C.byref(cs),
                                                   _ptr(frame_index_dev), _lib.ptr(lm), ls, k, c, _lib.C.byref(co),
                                                   _lib.ptr(regions)), "flm_frames_annotate")
    elif k:
        regions.zero_()
    return regions


# ---- landmark flow: the landmarks carried between two forwards (include/flm.h, "landmark flow") -------------------------
FLOW_NO_HISTORY, FLOW_LOW_TEXTURE, FLOW_RESIDUAL = _lib.FLOW_NO_HISTORY, _lib.FLOW_LOW_TEXTURE, _lib.FLOW_RESIDUAL
FLOW_OUTSIDE, FLOW_MOVED, FLOW_NOT_FINITE = _lib.FLOW_OUTSIDE, _lib.FLOW_MOVED, _lib.FLOW_NOT_FINITE
FLOW_FB = _lib.FLOW_FB


class LandmarkFlow:
    """flm_flow_opts: the pyramid, the window and the gates of flm_landmark_flow (include/flm.h).  levels: pyramid levels,
    1..6 (the crop's sides are multiples of 2^(levels-1)); radius: the window is (2*radius+1)^2 pixels, 1..7; max_iter:
    iterations per level, 1..64; eps: a level stops when its update is shorter than this, in px; min_eig: the least
    eigenvalue per pixel (grey levels squared) at which a level is solved; max_err: the largest mean absolute residual
    (grey levels) and max_move: the longest move (crop px) of an accepted point -- both defaults are guesses that no
    measurement on real faces backs.  levels=4 rests on a synthetic prototype (three levels lost 14 px shifts in a 256 px
    crop); radius, max_iter, eps and min_eig are the customary values of such trackers, unmeasured here.  max_fb: None (the
    default: off) or the largest round trip, in crop px, of the forward-backward check of flm_landmark_flow_rows: an
    accepted point is flowed back from where it arrived, and rejected with FLOW_FB unless it returns to within max_fb of
    where it started.  It costs a second walk.  The value one would start from, 1.0 as in median-flow trackers, is a GUESS
    too: like max_err and max_move it has not been measured on real faces."""

    def __init__(self, levels=4, radius=7, max_iter=10, eps=0.03, min_eig=0.5, max_err=12.0, max_move=64.0, max_fb=None):
        for name, v, lo, hi in (("levels", levels, 1, 6), ("radius", radius, 1, 7), ("max_iter", max_iter, 1, 64)):
            if isinstance(v, bool) or int(v) != v or not lo <= int(v) <= hi:
                raise ValueError("%s must be an integer in [%d, %d], got %r" % (name, lo, hi, v))
        eps, min_eig, max_err, max_move = float(eps), float(min_eig), float(max_err), float(max_move)
        if not eps > 0.0:
            raise ValueError("eps must be > 0, got %r" % eps)
        if not min_eig >= 0.0:
            raise ValueError("min_eig must be >= 0, got %r" % min_eig)
        if not max_err >= 0.0:
            raise ValueError("max_err must be >= 0, got %r" % max_err)
        if not max_move > 0.0:
            raise ValueError("max_move must be > 0, got %r" % max_move)
        self.levels, self.radius, self.max_iter = int(levels), int(radius), int(max_iter)
        self.eps, self.min_eig, self.max_err, self.max_move = eps, min_eig, max_err, max_move
        if max_fb is not None:
            max_fb = float(max_fb)
            if not (max_fb > 0.0 and max_fb < float("inf")):
                raise ValueError("max_fb must be None (no forward-backward check) or a finite number > 0, got %r" % max_fb)
        self.max_fb = max_fb

    def check_crop(self, h, w):
        """ValueError unless crops of h x w have a pyramid of `levels` levels."""
        t = 1 << (self.levels - 1)
        if h % t or w % t or (h >> (self.levels - 1)) < 2 or (w >> (self.levels - 1)) < 2 or h > 32768 or w > 32768:
            raise ValueError("crops of %dx%d have no pyramid of %d levels: the sides must be multiples of %d, at least %d "
                             "and at most 32768" % (h, w, self.levels, t, 2 * t))

    def pyramid_bytes(self, h, w):
        return sum((h >> l) * (w >> l) for l in range(self.levels))

    def struct(self):
        return _lib.FlowOpts.make(self.levels, self.radius, self.max_iter, self.eps, self.min_eig, self.max_err, self.max_move)

    def __repr__(self):
        return ("LandmarkFlow(levels=%r, radius=%r, max_iter=%r, eps=%r, min_eig=%r, max_err=%r, max_move=%r%s)"
                % (self.levels, self.radius, self.max_iter, self.eps, self.min_eig, self.max_err, self.max_move,
                   "" if self.max_fb is None else ", max_fb=%r" % self.max_fb))


def _check_flow(flow):
    if not isinstance(flow, LandmarkFlow):
        raise ValueError("flow must be an alignment.LandmarkFlow (got %r)" % (flow,))


def flow_pyramid_device(crops, levels, out=None):
    """The luma pyramids of N crops in one launch (flm_flow_pyramid).  crops: a contiguous CUDA uint8 [N,H,W,3] (B,G,R) or
    [N,H,W] (luma) tensor; levels: 1..6, H and W multiples of 2^(levels-1) and at least twice that -> CUDA uint8
    [N, bytes]: per crop its levels 0 .. levels-1 one after the other, level l of (H >> l) x (W >> l) bytes."""
    import torch
    if (not isinstance(crops, torch.Tensor) or crops.dtype != torch.uint8 or crops.dim() not in (3, 4)
            or (crops.dim() == 4 and int(crops.shape[3]) != 3) or not crops.is_contiguous()):
        raise ValueError("crops must be a contiguous CUDA uint8 [N,H,W,3] or [N,H,W] tensor")
    if isinstance(levels, bool) or int(levels) != levels or not 1 <= int(levels) <= 6:
        raise ValueError("levels must be an integer in [1, 6], got %r" % (levels,))
    flow = LandmarkFlow(levels=int(levels))
    n, h, w = [int(v) for v in crops.shape[:3]]
    flow.check_crop(h, w)
    if n > 131070:
        raise ValueError("at most 131070 crops per call (got %d)" % n)
    if not crops.is_cuda:
        raise ValueError("crops must be a contiguous CUDA uint8 [N,H,W,3] or [N,H,W] tensor")
    out = _out(out, torch.uint8, (n, flow.pyramid_bytes(h, w)), "out", crops.device)
    _check_overlap(crops, out, "crops and out")
    if n:
        _lib.check(_lib.load().flm_flow_pyramid(_lib.stream_ptr(), _lib.ptr(crops), n, h, w, 1 if crops.dim() == 3 else 3,
                                                int(levels), _lib.ptr(out)), "flm_flow_pyramid")
    return out


def _landmark_flow_args(pyr_prev, pyr_cur, slot, lm_prev, m, hw, flow, weights, out):
    """The checks of `landmark_flow_device` (slot None: row r reads slot r, K rows) and of `landmark_flow_rows_device`,
    stated once.  Returns (h, w, rows, n_slots, c, the outputs: (lm, w, err, flags), with fb before flags for rows)."""
    import torch
    _check_flow(flow)
    h, w = _sizes(hw, "hw")
    flow.check_crop(h, w)
    if not isinstance(lm_prev, torch.Tensor) or lm_prev.dim() != 3 or int(lm_prev.shape[2]) != 2:
        raise ValueError("lm_prev must be a contiguous CUDA float64 [%s,C,2] tensor"
                         % ("K" if slot is None else "n_slots"))
    n_slots, c = int(lm_prev.shape[0]), int(lm_prev.shape[1])
    _check_out(lm_prev, torch.float64, (n_slots, c, 2), "lm_prev")
    if slot is None:
        n = n_slots
        if n > 65535 or c > 1024:
            raise ValueError("at most 65535 faces of 1024 landmarks per call (got %d of %d)" % (n, c))
    else:
        if not isinstance(slot, torch.Tensor) or slot.dim() != 1:
            raise ValueError("slot must be a contiguous CUDA int32 [N] tensor")
        n = int(slot.shape[0])
        _check_out(slot, torch.int32, (n,), "slot")
        if not 1 <= n_slots <= 65535 or n > 65535 or c > 1024:
            raise ValueError("at most 65535 slots and 65535 rows of 1024 landmarks, at least one slot (got %d slots, "
                             "%d rows of %d)" % (n_slots, n, c))
    nb = flow.pyramid_bytes(h, w)
    _check_out(pyr_prev, torch.uint8, (n, nb), "pyr_prev")
    _check_out(pyr_cur, torch.uint8, (n, nb), "pyr_cur")
    _check_matrices(m, n)
    if weights is not None:
        _check_out(weights, torch.float64, (n_slots, c), "weights")
    kinds = [(torch.float64, (n, c, 2), "lm"), (torch.float64, (n, c), "w"), (torch.int32, (n, c), "err"),
             (torch.float64, (n, c), "fb"), (torch.int32, (n, c), "flags")]
    if slot is None:
        del kinds[3]
    given = (None,) * len(kinds) if out is None else tuple(out)
    if len(given) != len(kinds):
        raise ValueError("out must be None or a tuple (%s) of tensors, any of them None"
                         % ", ".join(k[2] for k in kinds))
    outs = tuple(_out(t, dtype, shape, "out " + what, lm_prev.device) for t, (dtype, shape, what) in zip(given, kinds))
    for a, t in enumerate(outs):
        for src in (pyr_prev, pyr_cur, slot, lm_prev, m, weights):
            _check_overlap(t, src, "an output and an input")
        for u in outs[a + 1:]:
            _check_overlap(t, u, "two outputs")
    return h, w, n, n_slots, c, outs


def landmark_flow_device(pyr_prev, pyr_cur, lm_prev, m, hw, flow, weights=None, out=None):
    """The landmarks of K faces carried from the previous crops to the current ones in one launch (flm_landmark_flow;
    include/flm.h states it line by line).

    pyr_prev, pyr_cur: CUDA uint8 [K, bytes] as `flow_pyramid_device` makes them with flow.levels, of crops of hw = (H, W)
    cut from the two frames with the SAME matrices m (CUDA float32 [K,2,3] frame px -> crop px); lm_prev: contiguous CUDA
    float64 [K,C,2] in FRAME px, a negative or non-finite point has no history; weights: None or contiguous CUDA float64
    [K,C]; out: None or a tuple (lm, w, err, flags) of tensors to write, any of them None.
    Returns (lm float64 [K,C,2] in CROP px, (-1,-1) for a rejected point; w float64 [K,C], the point's weight (1.0
    without weights), 0 for a rejected point; err int32 [K,C], the window's sum of absolute differences, -1 where it was
    not reached; flags int32 [K,C], 0 or the FLOW_* bits that rejected the point).  The landmarks are what
    `track_step_device` takes with grid_hw = in_hw = hw."""
    h, w, k, _, c, outs = _landmark_flow_args(pyr_prev, pyr_cur, None, lm_prev, m, hw, flow, weights, out)
    if k and c:
        fo = flow.struct()
        _lib.check(_lib.load().flm_landmark_flow(_lib.stream_ptr(), _lib.ptr(pyr_prev), _lib.ptr(pyr_cur), k, h, w,
                                                 _lib.ptr(lm_prev), _ptr(weights), _lib.ptr(m), c, _lib.C.byref(fo),
                                                 *[_lib.ptr(t) for t in outs]), "flm_landmark_flow")
    return outs


def landmark_flow_rows_device(pyr_prev, pyr_cur, slot, lm_prev, m, hw, flow, weights=None, out=None):
    """`landmark_flow_device` on the rows of a compacted batch, with the forward-backward check of `flow.max_fb`, in one
    launch (flm_landmark_flow_rows; include/flm.h states it).

    pyr_prev, pyr_cur CUDA uint8 [N, bytes] and m CUDA float32 [N,2,3] are read at the row; slot: contiguous CUDA int32
    [N], the global slot of every row (outside [0, n_slots): the row is inert); lm_prev contiguous CUDA float64
    [n_slots,C,2] in frame px and weights None or CUDA float64 [n_slots,C] -- the history store itself -- are read at the
    slot.  out: None or a tuple (lm, w, err, fb, flags) of tensors to write, any of them None.
    Returns (lm float64 [N,C,2] crop px, w float64 [N,C], err int32 [N,C], fb float64 [N,C], flags int32 [N,C]) over
    the rows, as `landmark_flow_device` returns them; fb is the squared round trip of the forward-backward check in crop
    px squared, -1.0 where it did not run or did not finish, and flags may carry FLOW_FB.  An inert row is (-1,-1),
    weight 0, err -1, fb -1.0, FLOW_NO_HISTORY.  With flow.max_fb None, slot = arange(N) and N = n_slots the first three
    and the flags are the bits of `landmark_flow_device`."""
    h, w, n, n_slots, c, outs = _landmark_flow_args(pyr_prev, pyr_cur, slot, lm_prev, m, hw, flow, weights, out)
    if n and c:
        fo = flow.struct()
        _lib.check(_lib.load().flm_landmark_flow_rows(
            _lib.stream_ptr(), _lib.ptr(pyr_prev), _lib.ptr(pyr_cur), n, h, w, _lib.ptr(slot), n_slots, _lib.ptr(lm_prev),
            _ptr(weights), _lib.ptr(m), c, _lib.C.byref(fo), 0.0 if flow.max_fb is None else flow.max_fb,
            *[_lib.ptr(t) for t in outs]), "flm_landmark_flow_rows")
    return outs


def track_flow_history_device(slot, status_rows, frame_index_c, flow_frame, flow_ready, lm_rows=None, hist_lm=None,
                              w_rows=None, hist_w=None):
    """The rows of a tick moved to the history of their slots, in one launch (flm_track_flow_history_put; include/flm.h
    states it and the history rule).

    slot, status_rows, frame_index_c: contiguous CUDA int32 [N], the global slot, the status and the ring slot of every
    row; flow_frame, flow_ready: CUDA int32 [n_slots], the tracker's own.  A row served with status 0 sets flow_frame to
    its ring slot and flow_ready to 1 at its slot, any other row of a slot clears flow_ready there; an inert row writes
    nothing and a slot no row names keeps every bit.  lm_rows CUDA float64 [N,C,2] with hist_lm [n_slots,C,2], and w_rows
    [N,C] with hist_w [n_slots,C]: the raw landmarks (and weights) of the rows served with status 0 are copied to their
    slots; without them only flow_frame and flow_ready are written.  Returns flow_ready."""
    import torch
    if not isinstance(slot, torch.Tensor) or slot.dim() != 1:
        raise ValueError("slot must be a contiguous CUDA int32 [N] tensor")
    n = int(slot.shape[0])
    for x, what in ((slot, "slot"), (status_rows, "status_rows"), (frame_index_c, "frame_index_c")):
        _check_out(x, torch.int32, (n,), what)
    if not isinstance(flow_ready, torch.Tensor) or flow_ready.dim() != 1:
        raise ValueError("flow_ready must be a contiguous CUDA int32 [n_slots] tensor")
    n_slots = int(flow_ready.shape[0])
    _check_out(flow_ready, torch.int32, (n_slots,), "flow_ready")
    _check_out(flow_frame, torch.int32, (n_slots,), "flow_frame")
    if not 1 <= n_slots <= 65535 or n > 65535:
        raise ValueError("at most 65535 slots and 65535 rows, at least one slot (got %d slots, %d rows)" % (n_slots, n))
    if (lm_rows is None) != (hist_lm is None) or (w_rows is None) != (hist_w is None) or (w_rows is not None and lm_rows is None):
        raise ValueError("lm_rows goes with hist_lm, w_rows with hist_w, and weights with landmarks")
    c = 1
    if lm_rows is not None:
        if not isinstance(lm_rows, torch.Tensor) or lm_rows.dim() != 3:
            raise ValueError("lm_rows must be a contiguous CUDA float64 [N,C,2] tensor")
        c = int(lm_rows.shape[1])
        _check_out(lm_rows, torch.float64, (n, c, 2), "lm_rows")
        _check_out(hist_lm, torch.float64, (n_slots, c, 2), "hist_lm")
        _check_overlap(lm_rows, hist_lm, "lm_rows and hist_lm")
        if w_rows is not None:
            _check_out(w_rows, torch.float64, (n, c), "w_rows")
            _check_out(hist_w, torch.float64, (n_slots, c), "hist_w")
            _check_overlap(w_rows, hist_w, "w_rows and hist_w")
    for t in (flow_frame, flow_ready):
        for src in (slot, status_rows, frame_index_c):
            _check_overlap(t, src, "an output and an input")
    if n and 1 <= c <= 1024:
        _lib.check(_lib.load().flm_track_flow_history_put(
            _lib.stream_ptr(), _lib.ptr(slot), _lib.ptr(status_rows), _lib.ptr(frame_index_c), _ptr(lm_rows), _ptr(w_rows), n,
            n_slots, c, _ptr(hist_lm), _ptr(hist_w), _lib.ptr(flow_frame), _lib.ptr(flow_ready)),
            "flm_track_flow_history_put")
    elif n:
        raise ValueError("at most 1024 landmarks (got %d)" % c)
    return flow_ready
