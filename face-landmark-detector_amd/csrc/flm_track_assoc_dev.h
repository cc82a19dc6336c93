// The integer pieces of flm_track_associate: the detector's box maths, the clip, the area, the intersection, the
// threshold test and the order of pairs.  Stated once, as __host__ __device__ code, for track_assoc_kernel
// (flm_track_assoc.hip) and for the host sweep of tests/native/track_assoc_host.cpp, which runs these same functions
// over boxes at the extremes of the contract under the host's sanitizers.  include/flm.h states the contract; this
// header is its arithmetic.
//
// Ranges the callers guarantee, and what follows from them: detection coordinates lie in [-2^28, 2^28] before the box
// maths (assoc_in_range), so every difference and sum below stays inside int32 (|y1-y0| <= 2^29, |diff| <= 2^30, the
// moved and grown coordinates within +-(2^28 + 2^29 + 2^26)); track boxes are any int32, and are only ever clipped.
// Clipped boxes lie in [0,fw] x [0,fh] with fh*fw <= 2^30, so area and inter are at most 2^30, uni at most 2^31 and
// every product of the pair order below 2^61.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "flm.h"

namespace flm {

constexpr int kAssocCoordLimit = 1 << 28;
constexpr int kAssocMaxItems = 1024;             // slots and detections per call

struct AssocBox {
  int x0, y0, x1, y1;
};

__host__ __device__ __forceinline__ bool assoc_in_range(const AssocBox& b) {
  const int L = kAssocCoordLimit;
  return b.x0 >= -L && b.x0 <= L && b.y0 >= -L && b.y0 <= L && b.x1 >= -L && b.x1 <= L && b.y1 >= -L && b.y1 <= L;
}

// The box maths of prediction.face_boxes: the box moved down by a tenth of its height, then grown to a square about its
// centre, the odd pixel going to the right / the bottom.  Needs assoc_in_range(b).
__host__ __device__ __forceinline__ AssocBox assoc_square(AssocBox b) {
  const int off = (int)fabs((double)(b.y1 - b.y0) * 0.1);
  b.y0 += off;
  b.y1 += off;
  const int diff = (b.y1 - b.y0) - (b.x1 - b.x0);
  const int ad = diff < 0 ? -diff : diff;
  const int delta = ad >> 1, odd = ad & 1;
  if (diff > 0) {
    b.x0 -= delta;
    b.x1 += delta + odd;
  } else if (diff < 0) {
    b.y0 -= delta;
    b.y1 += delta + odd;
  }
  return b;
}

// The clip of flm_landmarks_to_frame; empty: cx1-cx0 <= 0 or cy1-cy0 <= 0.
__host__ __device__ __forceinline__ int assoc_clamp(int v, int hi) { return v < 0 ? 0 : v > hi ? hi : v; }
__host__ __device__ __forceinline__ AssocBox assoc_clip(const AssocBox& b, int fh, int fw) {
  return AssocBox{assoc_clamp(b.x0, fw), assoc_clamp(b.y0, fh), assoc_clamp(b.x1, fw), assoc_clamp(b.y1, fh)};
}
__host__ __device__ __forceinline__ bool assoc_empty(const AssocBox& c) { return c.x1 - c.x0 <= 0 || c.y1 - c.y0 <= 0; }

// Area of a clipped box that is not empty, and the intersection of two such boxes (0: none).
__host__ __device__ __forceinline__ int64_t assoc_area(const AssocBox& c) {
  return (int64_t)(c.x1 - c.x0) * (int64_t)(c.y1 - c.y0);
}
__host__ __device__ __forceinline__ int64_t assoc_inter(const AssocBox& a, const AssocBox& b) {
  const int w = (a.x1 < b.x1 ? a.x1 : b.x1) - (a.x0 > b.x0 ? a.x0 : b.x0);
  const int h = (a.y1 < b.y1 ? a.y1 : b.y1) - (a.y0 > b.y0 ? a.y0 : b.y0);
  return (w <= 0 || h <= 0) ? 0 : (int64_t)w * (int64_t)h;
}
__host__ __device__ __forceinline__ int64_t assoc_union(int64_t area_a, int64_t area_b, int64_t inter) {
  return area_a + area_b - inter;
}

// inter and uni of clipped boxes fit 32 bits (see the ranges above), which is what the two functions below take from
// their int64 arguments: the conversions to double and the products are then single 32-bit instructions on the device,
// and their values are those of the int64 expressions the header states.

// "IoU >= t": one float64 multiplication.
__host__ __device__ __forceinline__ bool assoc_iou_ge(int64_t inter, int64_t uni, double t) {
  return inter > 0 && (double)(uint32_t)inter >= t * (double)(uint32_t)uni;
}

// The strict order of pairs: p = (slot sp, detection dp) comes before q when its IoU is larger, exactly; on a tie the
// lower slot, then the lower detection.
__host__ __device__ __forceinline__ bool assoc_before(int64_t inter_p, int64_t uni_p, int sp, int dp, int64_t inter_q,
                                                      int64_t uni_q, int sq, int dq) {
  const uint64_t l = (uint64_t)(uint32_t)inter_p * (uint64_t)(uint32_t)uni_q;  // (< 2^61)
  const uint64_t r = (uint64_t)(uint32_t)inter_q * (uint64_t)(uint32_t)uni_p;
  if (l != r) return l > r;
  if (sp != sq) return sp < sq;
  return dp < dq;
}

}  // namespace flm
