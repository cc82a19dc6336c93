// The per-sample arithmetic of the alignment warps, stated once for the kernels of flm_warp_fmt.hip.  It restates,
// operation for operation, what warp_kernel / warp_u8_kernel / warp_u8_rows_kernel (flm_misc.hip) and warp_frames_kernel
// (flm_frames.hip) compute -- those kernels keep their own copies until an A/B on the bench's warp says that folding
// them onto this header costs nothing -- so a sample taken here has the bits of a sample taken there
// (tests/test_gpu_aligned_format.py compares them exactly).  The build's -ffp-contract=off keeps every multiply and add
// below apart unless it is written as fmaf.
#pragma once

#include "flm_common.h"

namespace flm {

// M^-1 of a face: det = fma(m00, m11, -(m01*m10)), idet = 1/det, the four products by idet, and the two translation
// terms as negated fmas -- the specification above warp_kernel.
struct WarpInverse {
  float i00, i01, i02, i10, i11, i12;
};
__device__ __forceinline__ WarpInverse warp_inverse(const float* __restrict__ mm) {
  const float m00 = mm[0], m01 = mm[1], m02 = mm[2], m10 = mm[3], m11 = mm[4], m12 = mm[5];
  const float det = fmaf(m00, m11, -(m01 * m10));
  const float idet = 1.0f / det;
  WarpInverse w;
  w.i00 = m11 * idet; w.i01 = -m01 * idet; w.i10 = -m10 * idet; w.i11 = m00 * idet;
  w.i02 = -fmaf(w.i00, m02, w.i01 * m12);
  w.i12 = -fmaf(w.i10, m02, w.i11 * m12);
  return w;
}

// Source position of destination (xd, yd): the two fmaf chains, the edge clamp, floor.  xmax = Ws-1, ymax = Hs-1.
struct WarpPos {
  float fx, fy;  // xs - floor(xs), ys - floor(ys)
  int x0, y0;
};
__device__ __forceinline__ WarpPos warp_position(const WarpInverse& w, float xd, float yd, float xmax, float ymax) {
  float xs = fmaf(w.i00, xd, fmaf(w.i01, yd, w.i02));
  float ys = fmaf(w.i10, xd, fmaf(w.i11, yd, w.i12));
  xs = fminf(fmaxf(xs, 0.f), xmax);
  ys = fminf(fmaxf(ys, 0.f), ymax);
  const float xf = floorf(xs), yf = floorf(ys);
  WarpPos p;
  p.fx = xs - xf;
  p.fy = ys - yf;
  p.x0 = (int)xf;
  p.y0 = (int)yf;
  return p;
}

// Destination coordinates of sub-sample q of an S x S grid around pixel (x, y): q = i*S + j, i the row;
// xd = x + (2j+1-S)/(2S), yd = y + (2i+1-S)/(2S) (the offsets are exact in float32 for S = 2, 4).  S = 1: (x, y).
template <int S>
__device__ __forceinline__ void warp_subsample(float x, float y, int q, float& xd, float& yd) {
  xd = S == 1 ? x : x + (float)(2 * (q % S) + 1 - S) / (float)(2 * S);
  yd = S == 1 ? y : y + (float)(2 * (q / S) + 1 - S) / (float)(2 * S);
}

// uint8 BGR source of w >= 2 columns: the two pixels of a source row are six contiguous bytes, read as two unaligned
// dwords (bytes 0..3 and 2..5 of the pair).  The pair starts at xl = min(x0, w-2), so it ends inside its row; x0 = w-1
// (only for xs = w-1 exactly) goes through the weight: fx = 1 and fmaf(1, t1-t0, t0) = t1 exactly on small integers.
// The bottom row is y0+1 while that is inside the image, else y0 again.  Byte offsets are 32-bit: h*w*3 < 2^31.
// Gather and blend are separate calls so that a kernel can issue every gather of a thread before it consumes the first.
struct WarpTapsU8 {
  unsigned ta, tb, ba, bb;
  float fx, fy;
};
__device__ __forceinline__ void warp_gather_u8(const uint8_t* __restrict__ s8, int h, int w, const WarpInverse& inv,
                                               float xd, float yd, WarpTapsU8& t) {
  const WarpPos p = warp_position(inv, xd, yd, (float)(w - 1), (float)(h - 1));
  const int xl = min(p.x0, w - 2);
  t.fx = p.x0 != xl ? 1.0f : p.fx;
  t.fy = p.fy;
  const unsigned ot = ((unsigned)p.y0 * (unsigned)w + (unsigned)xl) * 3u;
  const unsigned ob = ot + (p.y0 + 1 < h ? (unsigned)w * 3u : 0u);
  __builtin_memcpy(&t.ta, s8 + ot, 4);
  __builtin_memcpy(&t.tb, s8 + ot + 2, 4);
  __builtin_memcpy(&t.ba, s8 + ob, 4);
  __builtin_memcpy(&t.bb, s8 + ob + 2, 4);
}
// top = fma(fx, p01-p00, p00); bot = fma(fx, p11-p10, p10); out = fma(fy, bot-top, top), per channel
__device__ __forceinline__ void warp_blend_u8(const WarpTapsU8& t, float out[3]) {
  const unsigned a = t.ta, b = t.tb, c2 = t.ba, d = t.bb;
  // pixel 0 = bytes 0,1,2 of the first dword; pixel 1 = byte 3 of the first, bytes 2,3 of the second
  const float t0[3] = {(float)(a & 0xffu), (float)((a >> 8) & 0xffu), (float)((a >> 16) & 0xffu)};
  const float t1[3] = {(float)(a >> 24), (float)((b >> 16) & 0xffu), (float)(b >> 24)};
  const float b0[3] = {(float)(c2 & 0xffu), (float)((c2 >> 8) & 0xffu), (float)((c2 >> 16) & 0xffu)};
  const float b1[3] = {(float)(c2 >> 24), (float)((d >> 16) & 0xffu), (float)(d >> 24)};
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float top = fmaf(t.fx, t1[c] - t0[c], t0[c]);
    const float bot = fmaf(t.fx, b1[c] - b0[c], b0[c]);
    out[c] = fmaf(t.fy, bot - top, top);
  }
}

// Any other source (float32, or uint8 of a single column): the four taps at (x0|x1, y0|y1) with x1 = min(x0+1, w-1),
// y1 = min(y0+1, h-1), loaded channel by channel as warp_kernel loads them.
template <bool U8>
__device__ __forceinline__ void warp_sample_any(const void* __restrict__ src, int h, int w, const WarpInverse& inv,
                                                float xd, float yd, float out[3]) {
  const WarpPos p = warp_position(inv, xd, yd, (float)(w - 1), (float)(h - 1));
  const int x1 = min(p.x0 + 1, w - 1), y1 = min(p.y0 + 1, h - 1);
  const int o00 = (p.y0 * w + p.x0) * 3, o01 = (p.y0 * w + x1) * 3;
  const int o10 = (y1 * w + p.x0) * 3, o11 = (y1 * w + x1) * 3;
  const uint8_t* s8 = static_cast<const uint8_t*>(src);
  const float* sf = static_cast<const float*>(src);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float p00, p01, p10, p11;
    if (U8) {
      p00 = (float)s8[o00 + c]; p01 = (float)s8[o01 + c]; p10 = (float)s8[o10 + c]; p11 = (float)s8[o11 + c];
    } else {
      p00 = sf[o00 + c]; p01 = sf[o01 + c]; p10 = sf[o10 + c]; p11 = sf[o11 + c];
    }
    const float top = fmaf(p.fx, p01 - p00, p00);
    const float bot = fmaf(p.fx, p11 - p10, p10);
    out[c] = fmaf(p.fy, bot - top, top);
  }
}

}  // namespace flm
