"""numpy restatement of the NV12 -> BGR conversion of include/flm.h (the frame the NV12 calls compute on), and a float
forward transform BGR -> NV12 that only makes test frames."""
import numpy as np

# (CY, CUB, CUG, CVG, CVR), x 2^20
COEF = {
    "bt601": (1220542, 2116026, -409993, -852492, 1673527),
    "bt709": (1220945, 2215014, -223607, -558796, 1879825),
}
# (Kr, Kb) of the forward transform
_K = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}


def yuv_to_bgr(y, u, v, matrix):
    """The conversion on integer arrays of equal shape: int32 arithmetic (held in int64, the bounds of include/flm.h say
    nothing overflows int32), arithmetic shift, clamp."""
    cy, cub, cug, cvg, cvr = COEF[matrix]
    y, u, v = [np.asarray(a).astype(np.int64) for a in (y, u, v)]
    yy = np.maximum(y - 16, 0) * cy
    u = u - 128
    v = v - 128
    acc = np.stack([yy + cub * u, yy + cvg * v + cug * u, yy + cvr * v], -1) + (1 << 19)
    assert np.abs(acc).max() < 2 ** 31
    return np.clip(acc >> 20, 0, 255).astype(np.uint8)


def nv12_to_bgr_ref(slot_bytes, fh, fw, y_pitch, uv_offset, uv_pitch, matrix):
    """slot_bytes: flat uint8 array of one slot -> uint8 BGR [fh,fw,3].  Pixel (x, y): Y = s[y*y_pitch + x],
    U = s[uv_offset + (y>>1)*uv_pitch + (x & ~1)], V the byte after U (chroma replicated over its 2x2 block)."""
    s = np.asarray(slot_bytes, np.uint8).reshape(-1)
    yy, xx = np.mgrid[0:fh, 0:fw]
    y = s[yy * y_pitch + xx]
    uo = uv_offset + (yy >> 1) * uv_pitch + (xx & ~1)
    return yuv_to_bgr(y, s[uo], s[uo + 1], matrix)


def slot_bytes_needed(fh, fw, y_pitch, uv_offset, uv_pitch):
    """flm_frame_format_bytes restated: the last U,V row ends after its fw bytes."""
    return uv_offset + (fh // 2 - 1) * uv_pitch + fw


def bgr_to_nv12(bgr, matrix):
    """Float forward transform, limited range, chroma as the mean of its 2x2 block: (Y [fh,fw], UV [fh/2,fw]) uint8.
    Only a source of plausible test frames; nothing is compared against it."""
    kr, kb = _K[matrix]
    kg = 1.0 - kr - kb
    b, g, r = [bgr[..., c].astype(np.float64) for c in range(3)]
    yf = kr * r + kg * g + kb * b
    cb = (b - yf) / (2.0 * (1.0 - kb))
    cr = (r - yf) / (2.0 * (1.0 - kr))
    fh, fw = yf.shape
    y = np.clip(np.rint(16.0 + 219.0 * yf / 255.0), 0, 255).astype(np.uint8)
    mean = lambda a: a.reshape(fh // 2, 2, fw // 2, 2).mean((1, 3))
    u = np.clip(np.rint(128.0 + 224.0 * mean(cb) / 255.0), 0, 255).astype(np.uint8)
    v = np.clip(np.rint(128.0 + 224.0 * mean(cr) / 255.0), 0, 255).astype(np.uint8)
    return y, np.stack([u, v], -1).reshape(fh // 2, fw)


def pack_slot(y, uv, y_pitch, uv_row, rows, rng=None):
    """One [rows, y_pitch] slot (both planes at the same pitch, U,V rows from `uv_row`): padding is random junk when a
    generator is given, else zero."""
    fh, fw = y.shape
    slot = (rng.integers(0, 256, (rows, y_pitch), dtype=np.uint8) if rng is not None
            else np.zeros((rows, y_pitch), np.uint8))
    slot[:fh, :fw] = y
    slot[uv_row:uv_row + fh // 2, :fw] = uv
    return slot
