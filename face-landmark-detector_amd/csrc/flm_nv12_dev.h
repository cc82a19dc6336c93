// NV12 frame slots as a pixel source: where the bytes of a tap lie and how they become integer B,G,R.  Stated once, as
// __host__ __device__ code, for the kernels of flm_frames_nv12.hip and for the host sweep of
// tests/native/nv12_taps_host.cpp, which runs these same functions over every source position of small frames inside a
// heap buffer of exactly the slot's bytes.  include/flm.h states the contract; this header is its arithmetic.
//
// A slot at byte address s holds fh x fw pixels (both even): luma rows y_pitch bytes apart from s, and fh/2 rows of
// interleaved U,V byte pairs uv_pitch bytes apart from s + uv_off.  Pixel (x, y):
//   Y = s[y*y_pitch + x];   U = s[uv_off + (y>>1)*uv_pitch + (x & ~1)];   V = the byte after U
// (chroma replicated over its 2x2 block).  All offsets are 32-bit: the launchers check slot bytes < 2^31.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "flm.h"

namespace flm {

// ---- the conversion ------------------------------------------------------------------------------------
// int32 throughout, >> arithmetic:
//   yy = max(Y-16, 0)*CY;  u = U-128;  v = V-128
//   B = clamp((yy + CUB*u + 2^19) >> 20);  G = clamp((yy + CVG*v + CUG*u + 2^19) >> 20);  R = clamp((yy + CVR*v + 2^19) >> 20)
// |accumulator| <= 573,636,921 for both coefficient sets over all (Y,U,V).
struct Nv12Coef {
  int cy, cub, cug, cvg, cvr;
};
__host__ __device__ inline Nv12Coef nv12_coef(int matrix) {
  // FLM_YUV_BT601_LIMITED: 1.164 / 2.018 / -0.391 / -0.813 / 1.596 x 2^20, the published fixed-point form of OpenCV's
  // COLOR_YUV2BGR_NV12; FLM_YUV_BT709_LIMITED: round(exact coefficient x 2^20) with Kr = 0.2126, Kb = 0.0722
  return matrix == FLM_YUV_BT709_LIMITED ? Nv12Coef{1220945, 2215014, -223607, -558796, 1879825}
                                         : Nv12Coef{1220542, 2116026, -409993, -852492, 1673527};
}

// The chroma part of the three accumulators, rounding term included: one per U,V pair, shared by the pixels under it.
// Integer sums are exact in any order, so splitting the accumulator this way changes no bit.
__host__ __device__ __forceinline__ void nv12_chroma(int U, int V, const Nv12Coef& k, int c[3]) {
  const int u = U - 128, v = V - 128;
  c[0] = k.cub * u + (1 << 19);
  c[1] = k.cvg * v + k.cug * u + (1 << 19);
  c[2] = k.cvr * v + (1 << 19);
}
__host__ __device__ __forceinline__ int nv12_clamp8(int a) { return a < 0 ? 0 : a > 255 ? 255 : a; }
__host__ __device__ __forceinline__ void nv12_pixel(int Y, const int c[3], const Nv12Coef& k, int bgr[3]) {
  const int y16 = Y - 16;
  const int yy = (y16 < 0 ? 0 : y16) * k.cy;
  bgr[0] = nv12_clamp8((yy + c[0]) >> 20);
  bgr[1] = nv12_clamp8((yy + c[1]) >> 20);
  bgr[2] = nv12_clamp8((yy + c[2]) >> 20);
}
__host__ __device__ __forceinline__ void nv12_to_bgr(int Y, int U, int V, const Nv12Coef& k, int bgr[3]) {
  int c[3];
  nv12_chroma(U, V, k, c);
  nv12_pixel(Y, c, k, bgr);
}

// ---- slot geometry, defaults resolved ----------------------------------------------------------------------
struct Nv12Geom {
  int fh, fw;
  unsigned y_pitch, uv_pitch, uv_off;
};
// Bytes of a slot that a kernel may read: the last chroma row ends after its fw bytes, not after its pitch.
__host__ __device__ inline unsigned long long nv12_slot_bytes(const Nv12Geom& g) {
  return (unsigned long long)g.uv_off + (unsigned long long)(g.fh / 2 - 1) * g.uv_pitch + (unsigned long long)g.fw;
}

// ---- one tap, any position: the crop / resize and the plain converter's ragged edge -----------------------------
__host__ __device__ __forceinline__ void nv12_tap_bgr(const uint8_t* __restrict__ s, const Nv12Geom& g, const Nv12Coef& k,
                                                      int x, int y, int bgr[3]) {
  const int Y = s[(unsigned)y * g.y_pitch + (unsigned)x];
  const uint8_t* c = s + (g.uv_off + (unsigned)(y >> 1) * g.uv_pitch + (unsigned)(x & ~1));
  nv12_to_bgr(Y, c[0], c[1], k, bgr);
}

// ---- the four taps of a bilinear warp sample ---------------------------------------------------------------
// (x0, y0, fx, fy) are warp_position's.  As in warp_gather_u8 the pixel pair starts at xl = min(x0, fw-2), x0 = fw-1
// goes through the weight (fx = 1), and the bottom row is y0+1 while that is inside the frame, else y0 again.  Per row:
// the luma pair is one 2-byte load at column xl; the chroma under it is one 4-byte load of two U,V pairs starting at
// column xl & ~1 -- for odd xl the low half belongs to pixel xl and the high half to pixel xl+1, for even xl both
// pixels take the low half.  At the last column pair (xl == fw-2) that dword would run 2 bytes past the row, and on the
// last chroma row past the slot: there it starts one pair earlier (inside the row, or for fw == 2 in the bytes before
// it, which the slot holds because uv_off >= y_pitch*fh >= 4) and both pixels take the high half.  No load leaves
// [s, s + nv12_slot_bytes).
// Which half each pixel takes travels in the sign bits of the two weights, which are never negative themselves
// (sign of fx: pixel xl+1 takes the high half; sign of fy: pixel xl does too): a register per sample less to keep
// alive while the gathers of the 4 x 4 grid are in flight.
struct Nv12Taps {
  unsigned ya, yb;  // luma pairs of the top / bottom row, low byte = pixel xl
  unsigned ca, cb;  // chroma dwords of the top / bottom row
  float fx, fy;     // the weights, with the two flags in their signs
};
__host__ __device__ __forceinline__ void nv12_gather(const uint8_t* __restrict__ s, const Nv12Geom& g, int x0, int y0,
                                                     float fx, float fy, Nv12Taps& t) {
  const int xl = x0 < g.fw - 2 ? x0 : g.fw - 2;
  const float wx = x0 != xl ? 1.0f : fx;
  const int y1 = y0 + 1 < g.fh ? y0 + 1 : y0;
  const int xe = xl & ~1;
  const bool last = xe + 4 > g.fw;
  const bool hi1 = last || (xl & 1);
  const unsigned cx = (unsigned)(last ? xe - 2 : xe);  // (-2 for fw == 2: the sums below wrap back into the slot)
  const unsigned oya = (unsigned)y0 * g.y_pitch + (unsigned)xl, oyb = (unsigned)y1 * g.y_pitch + (unsigned)xl;
  const unsigned oca = g.uv_off + (unsigned)(y0 >> 1) * g.uv_pitch + cx;
  const unsigned ocb = g.uv_off + (unsigned)(y1 >> 1) * g.uv_pitch + cx;
  unsigned short la, lb;
  __builtin_memcpy(&la, s + oya, 2);
  __builtin_memcpy(&lb, s + oyb, 2);
  __builtin_memcpy(&t.ca, s + oca, 4);
  __builtin_memcpy(&t.cb, s + ocb, 4);
  t.ya = la;
  t.yb = lb;
  t.fx = hi1 ? -wx : wx;
  t.fy = last ? -fy : fy;
}
__host__ __device__ __forceinline__ bool nv12_sign(float f) {
  unsigned b;
  __builtin_memcpy(&b, &f, 4);
  return (b >> 31) != 0;
}
// The four taps as integer B,G,R (section "the conversion"), then warp_blend_u8's three fmafs per channel:
//   top = fma(fx, p01-p00, p00); bot = fma(fx, p11-p10, p10); out = fma(fy, bot-top, top)
__host__ __device__ __forceinline__ void nv12_blend(const Nv12Taps& t, const Nv12Coef& k, float out[3]) {
  const bool hi1 = nv12_sign(t.fx), hi0 = nv12_sign(t.fy);
  const float fx = fabsf(t.fx), fy = fabsf(t.fy);
  const unsigned a0 = hi0 ? t.ca >> 16 : t.ca & 0xffffu, a1 = hi1 ? t.ca >> 16 : t.ca & 0xffffu;
  const unsigned b0 = hi0 ? t.cb >> 16 : t.cb & 0xffffu, b1 = hi1 ? t.cb >> 16 : t.cb & 0xffffu;
  int c[3], p00[3], p01[3], p10[3], p11[3];
  nv12_chroma((int)(a0 & 0xffu), (int)(a0 >> 8), k, c);
  nv12_pixel((int)(t.ya & 0xffu), c, k, p00);
  nv12_chroma((int)(a1 & 0xffu), (int)(a1 >> 8), k, c);
  nv12_pixel((int)(t.ya >> 8), c, k, p01);
  nv12_chroma((int)(b0 & 0xffu), (int)(b0 >> 8), k, c);
  nv12_pixel((int)(t.yb & 0xffu), c, k, p10);
  nv12_chroma((int)(b1 & 0xffu), (int)(b1 >> 8), k, c);
  nv12_pixel((int)(t.yb >> 8), c, k, p11);
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const float t0 = (float)p00[ch], t1 = (float)p01[ch], u0 = (float)p10[ch], u1 = (float)p11[ch];
    const float top = fmaf(fx, t1 - t0, t0);
    const float bot = fmaf(fx, u1 - u0, u0);
    out[ch] = fmaf(fy, bot - top, top);
  }
}

}  // namespace flm
