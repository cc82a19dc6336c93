// The store side of the alignment warps that write a consumer's format (flm_warp_fmt.hip, flm_frames_nv12.hip): the
// pixel types, the epilogue that takes a float32 BGR value to its element, and the host-side dispatch on (layout, type).
// flm_warp_fmt.hip describes the store shapes; include/flm.h states the contract.
#pragma once

#include "flm_common.h"

namespace flm {

struct FmtArgs {
  float scale[3], bias[3];  // by OUTPUT channel
  int reverse;              // output channel c reads source channel 2-c
};

// ---- pixel types: u (float32) -> the stored element ---------------------------------------------------
template <int TYPE> struct Pix;
template <> struct Pix<FLM_PIX_F32> {
  typedef float T;
  static __device__ __forceinline__ T cvt(float u) { return u; }
};
template <> struct Pix<FLM_PIX_F16> {  // binary16, nearest even, gradual subnormals, overflow to inf: v_cvt_f16_f32
  typedef _Float16 T;
  static __device__ __forceinline__ T cvt(float u) { return (_Float16)u; }
};
template <> struct Pix<FLM_PIX_BF16> {  // bfloat16, nearest even, on the float32 bits; a NaN stays a (quiet) NaN
  typedef uint16_t T;
  static __device__ __forceinline__ T cvt(float u) {
    const unsigned b = __float_as_uint(u);
    const unsigned r = (b + 0x7fffu + ((b >> 16) & 1u)) >> 16;
    return (uint16_t)(u != u ? (b >> 16) | 0x40u : r);
  }
};
template <> struct Pix<FLM_PIX_U8> {  // rint (ties to even), clamp to [0,255]; fmaxf(NaN, 0) = 0: a NaN stores 0
  typedef uint8_t T;
  static __device__ __forceinline__ T cvt(float u) { return (uint8_t)fminf(fmaxf(rintf(u), 0.f), 255.f); }
};

typedef unsigned u4v __attribute__((ext_vector_type(4)));
__device__ __forceinline__ bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// ---- epilogue: one pixel per lane, 64 consecutive pixels per wave ---------------------------------------
// v: the float32 BGR value of pixel p of face f (p = pbase + lane).  When all 64 pixels of the wave are inside the
// face (`whole`) the wave stores them together; otherwise the lanes with `live` (p < npix) store their own elements.  `line`: the wave's LDS line,
// 192 * sizeof(T) bytes, 16-byte aligned.
template <int LAYOUT, int TYPE>
__device__ __forceinline__ void store_pixel(typename Pix<TYPE>::T* __restrict__ dst, int f, int npix, int pbase_lane,
                                            int lane, bool live, const float v[3], const FmtArgs& a,
                                            unsigned char* line) {
  typedef typename Pix<TYPE>::T T;
  constexpr int ES = (int)sizeof(T);
  // the wave's first pixel is the same in every lane: said to the compiler, the run's address and the tests on it
  // stay scalar
  const int pbase = __builtin_amdgcn_readfirstlane(pbase_lane);
  const bool whole = pbase + 64 <= npix;
  const float s[3] = {a.reverse ? v[2] : v[0], v[1], a.reverse ? v[0] : v[2]};
  T e[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float t = s[c] * a.scale[c];
    const float u = t + a.bias[c];
    e[c] = Pix<TYPE>::cvt(u);
  }
  unsigned char* aline = static_cast<unsigned char*>(__builtin_assume_aligned(line, 16));
  if (LAYOUT == FLM_LAYOUT_NHWC) {
    T* run = dst + ((size_t)f * npix + pbase) * 3;  // the wave's 192 elements
    if (whole && aligned16(run)) {
#pragma unroll
      for (int c = 0; c < 3; ++c) __builtin_memcpy(aline + (3 * lane + c) * ES, &e[c], ES);
      __builtin_amdgcn_wave_barrier();
      if (lane < 12 * ES) {
        u4v q;
        __builtin_memcpy(&q, aline + 16 * lane, 16);
        __builtin_nontemporal_store(q, reinterpret_cast<u4v*>(reinterpret_cast<unsigned char*>(run) + 16 * lane));
      }
      __builtin_amdgcn_wave_barrier();
    } else if (whole || live) {
      T* d = run + 3 * lane;
      d[0] = e[0]; d[1] = e[1]; d[2] = e[2];
    }
  } else {
    T* run = dst + (size_t)f * 3 * npix + pbase;  // 64 elements here, and in the two planes npix and 2*npix further
    if (whole) {
      constexpr int LPP = 4 * ES;                 // lanes per plane: 64 * ES / 16
      const bool al[3] = {aligned16(run), aligned16(run + npix), aligned16(run + 2 * (size_t)npix)};  // (wave-uniform)
      if (al[0] || al[1] || al[2]) {
#pragma unroll
        for (int c = 0; c < 3; ++c) __builtin_memcpy(aline + (c * 64 + lane) * ES, &e[c], ES);
        __builtin_amdgcn_wave_barrier();
        const int c = lane / LPP, j = lane - c * LPP;
        if (lane < 3 * LPP && (c == 0 ? al[0] : c == 1 ? al[1] : al[2])) {
          u4v q;
          __builtin_memcpy(&q, aline + 16 * lane, 16);  // plane c starts at byte c*64*ES = 16*c*LPP of the line
          __builtin_nontemporal_store(
              q, reinterpret_cast<u4v*>(reinterpret_cast<unsigned char*>(run + (size_t)c * npix) + 16 * j));
        }
        __builtin_amdgcn_wave_barrier();
      }
#pragma unroll
      for (int c = 0; c < 3; ++c)
        if (!al[c]) run[(size_t)c * npix + lane] = e[c];
    } else if (live) {
#pragma unroll
      for (int c = 0; c < 3; ++c) run[(size_t)c * npix + lane] = e[c];
    }
  }
}

// A face the float32 calls fill with zeros: v = 0 through the same epilogue.
template <int LAYOUT, int TYPE>
__device__ __forceinline__ void store_zero_face(typename Pix<TYPE>::T* __restrict__ dst, int f, int npix, const FmtArgs& a,
                                                unsigned char* line) {
  const int lane = threadIdx.x & 63;
  const int pend = (npix + 63) & ~63;
  const float z[3] = {0.f, 0.f, 0.f};
  for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < pend; p += gridDim.x * blockDim.x)
    store_pixel<LAYOUT, TYPE>(dst, f, npix, p - lane, lane, p < npix, z, a, line);
}

static inline FmtArgs fmt_args(const flm_image_format* fmt) {
  FmtArgs a;
  for (int c = 0; c < 3; ++c) {
    a.scale[c] = fmt->scale[c];
    a.bias[c] = fmt->bias[c];
  }
  a.reverse = fmt->reverse_channels;
  return a;
}

// FMT_DISPATCH(CALL): CALL(LAYOUT, TYPE) for the format's pair (check_image_format has passed: both are in range)
#define FMT_DISPATCH_TYPE(CALL, L)                      \
  switch (fmt->type) {                                  \
    case FLM_PIX_F32: CALL(L, FLM_PIX_F32); break;      \
    case FLM_PIX_F16: CALL(L, FLM_PIX_F16); break;      \
    case FLM_PIX_BF16: CALL(L, FLM_PIX_BF16); break;    \
    default: CALL(L, FLM_PIX_U8); break;                \
  }
#define FMT_DISPATCH(CALL)                                          \
  do {                                                              \
    if (fmt->layout == FLM_LAYOUT_NHWC) {                           \
      FMT_DISPATCH_TYPE(CALL, FLM_LAYOUT_NHWC)                      \
    } else {                                                        \
      FMT_DISPATCH_TYPE(CALL, FLM_LAYOUT_NCHW)                      \
    }                                                               \
  } while (0)

}  // namespace flm
