// The per-pixel pieces of flm_face_quality: a stored element back to float32, the de-normalise and quantise step, and
// the integer luma.  Stated once, as __host__ __device__ code, for face_quality_kernel (flm_quality.hip) and for the host
// sweep of tests/native/quality_host.cpp, which runs these same functions over every uint8 triple and every 16-bit
// pattern under the host's sanitizers.  include/flm.h states the contract; this header is its arithmetic.
//
// Ranges: a quantised value p lies in [0, 4080] (sixteenths of an 8-bit level), so the luma sum is at most
// 16384 * 4080 + 8192 < 2^27 and Y lies in [0, 4080]; a Laplacian lies in [-16320, 16320] and its square below 2^28.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "flm.h"

namespace flm {

constexpr int kQualityMaxP = 4080;  // 255 * 16

// ---- the stored element as float32: every conversion is exact --------------------------------------------
template <int TYPE> struct QPix;
template <> struct QPix<FLM_PIX_F32> {
  typedef float T;
  static __host__ __device__ __forceinline__ float load(T x) { return x; }
};
template <> struct QPix<FLM_PIX_F16> {  // the bits of an IEEE binary16
  typedef uint16_t T;
  static __host__ __device__ __forceinline__ float load(T x) {
    _Float16 h;
    __builtin_memcpy(&h, &x, 2);
    return (float)h;
  }
};
template <> struct QPix<FLM_PIX_BF16> {  // the upper half of a float32
  typedef uint16_t T;
  static __host__ __device__ __forceinline__ float load(T x) {
    const uint32_t b = (uint32_t)x << 16;
    float f;
    __builtin_memcpy(&f, &b, 4);
    return f;
  }
};
template <> struct QPix<FLM_PIX_U8> {
  typedef uint8_t T;
  static __host__ __device__ __forceinline__ float load(T x) { return (float)x; }
};

// xf -> p: undo the format's bias and scale (two float32 operations, two roundings), then sixteenths of an 8-bit level,
// to nearest (ties to even), a NaN giving 0 (fmaxf(NaN, 0) = 0), clamped to [0, 4080].
__host__ __device__ __forceinline__ int quality_quant(float xf, float bias, float inv) {
  const float t = xf - bias;
  const float v = t * inv;
  const float r = rintf(v * 16.0f);
  return (int)fminf(fmaxf(r, 0.0f), (float)kQualityMaxP);
}

// BT.601 luma, weights times 2^14 (they sum to 16384), rounded to nearest: [0,4080]^3 -> [0,4080]
__host__ __device__ __forceinline__ int quality_luma(int b, int g, int r) {
  return (1868 * b + 9617 * g + 4899 * r + 8192) >> 14;
}

}  // namespace flm
