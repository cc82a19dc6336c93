"""numpy restatement of the aligned-face epilogue (include/flm.h, flm_image_format): what flm_warp_affine_fmt and
flm_warp_affine_frames_fmt store, given the float32 NHWC BGR faces flm_warp_affine / flm_warp_affine_frames write.

    convert(aligned_f32_nhwc, fmt) -> numpy array of the format's shape

float32, float16 and uint8 come back as those numpy types; bfloat16 comes back as its uint16 BITS (numpy has no such
type).  `bits(x)` gives the raw integer view every comparison of 8- and 16-bit results uses.  No device, no library.
"""
import numpy as np

f32 = np.float32


def _as_format(fmt):
    """(layout, dtype, reverse, scale[3] float32, bias[3] float32) of an alignment.AlignedFormat or of a plain tuple
    (layout, dtype, channels, scale, bias).  Scale and bias are rounded to float32 here exactly as ctypes rounds them
    into the C struct."""
    if isinstance(fmt, tuple):
        layout, dtype, channels, scale, bias = fmt
    else:
        layout, dtype, channels, scale, bias = fmt.layout, fmt.dtype, fmt.channels, fmt.scale, fmt.bias
    assert layout in ("nhwc", "nchw") and dtype in ("float32", "float16", "bfloat16", "uint8") and channels in ("bgr", "rgb")
    return layout, dtype, channels == "rgb", np.asarray(scale, np.float64).astype(f32), np.asarray(bias, np.float64).astype(f32)


def bf16_bits(u):
    """float32 -> bfloat16 bits, round to nearest, ties to even, on the float32 bits (no NaN in the tests' data)."""
    b = np.ascontiguousarray(u, f32).view(np.uint32).astype(np.uint64)
    return ((b + 0x7fff + ((b >> 16) & 1)) >> 16).astype(np.uint16)


def convert(aligned, fmt):
    layout, dtype, reverse, scale, bias = _as_format(fmt)
    v = np.asarray(aligned)
    assert v.dtype == f32 and v.ndim == 4 and v.shape[3] == 3
    if reverse:
        v = v[..., ::-1]                       # output channel c reads source channel 2-c
    with np.errstate(over="ignore"):
        t = (v * scale).astype(f32)            # float32 multiply, rounded
        u = (t + bias).astype(f32)             # float32 add, rounded: never fused
        if dtype == "float32":
            out = u
        elif dtype == "float16":
            out = u.astype(np.float16)         # nearest even, gradual subnormals, overflow to inf
        elif dtype == "bfloat16":
            out = bf16_bits(u)
        else:
            out = np.clip(np.rint(u), 0, 255).astype(np.uint8)   # rint: ties to even
    if layout == "nchw":
        out = out.transpose(0, 3, 1, 2)
    return np.ascontiguousarray(out)


def bits(x):
    """The raw bits of a result: float16 -> uint16, float32 -> uint32, integer types as they are."""
    x = np.ascontiguousarray(x)
    if x.dtype == np.float16:
        return x.view(np.uint16)
    if x.dtype == np.float32:
        return x.view(np.uint32)
    return x
