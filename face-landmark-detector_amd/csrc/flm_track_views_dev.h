// The bin of a face and the per-row decision of flm_track_views_update (include/flm.h, "pose-binned best shots", states
// the contract), as __host__ __device__ functions: track_views_decide_kernel (flm_track_views.hip) is built from them,
// and tests/native/track_views_host.cpp runs the same functions on the host against a serial restatement.
//
// The bin is read off the pose record flm_head_pose wrote, by comparisons of doubles alone -- the platform's atan2 and
// asin play no part, so a face falls into the same bin on every machine:
//   u = -R[2][0] = cos(pitch) * sin(yaw)        v = R[2][1] = sin(pitch)
// WHICH WAY: in the model frame of flm_head_pose (X to the image's right, Y down, Z away from the camera) the face's
// outward normal is -Z, which R takes to -(R[0][2], R[1][2], R[2][2]); for R = Ry(yaw) that is (-sin(yaw), 0, -cos(yaw)).
// So u > 0 is a face turned to the image's LEFT (its nose lies left of the midpoint of its eyes in the image), u < 0 one
// turned to the image's right.  For R = Rx(pitch) the normal is (0, sin(pitch), -cos(pitch)), and Y points down: v > 0
// is a face that looks DOWN in the image (its nose lies below where a frontal face has it), v < 0 one that looks up.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "flm.h"

namespace flm {

struct ViewsBins {
  int n_u, n_v;  // edges in use, 0 .. FLM_VIEWS_MAX_EDGES
  double u_edge[FLM_VIEWS_MAX_EDGES], v_edge[FLM_VIEWS_MAX_EDGES];
};

// The number of the first n edges e with x >= e (every edge index is a constant: the struct stays in registers).
__host__ __device__ __forceinline__ int views_edges_below(double x, const double* edge, int n) {
  int k = 0;
#pragma unroll
  for (int i = 0; i < FLM_VIEWS_MAX_EDGES; ++i) k += (i < n && x >= edge[i]) ? 1 : 0;
  return k;
}

__host__ __device__ __forceinline__ int views_bins(const ViewsBins& b) { return (b.n_u + 1) * (b.n_v + 1); }

// The bin of the face whose pose record is `pose` (FLM_POSE_REC doubles), or -1 for a face that is not binned: a fit
// that is not ok, or a NaN u or v.
__host__ __device__ __forceinline__ int views_bin(const double* pose, const ViewsBins& b) {
  const bool ok = pose[14] == 1.0;
  const double u = -pose[6], v = pose[7];
  if (!ok || u != u || v != v) return -1;
  const int iu = views_edges_below(u, b.u_edge, b.n_u), iv = views_edges_below(v, b.v_edge, b.n_v);
  return iv * (b.n_u + 1) + iu;
}

// ELIGIBLE but for the bin: the test of flm_track_best_update on q = (s * e) * wbar.
__host__ __device__ __forceinline__ bool views_eligible(bool status_ok, int64_t n_lap, double e, double min_exposed,
                                                        double q) {
  return status_ok && n_lap > 0 && e >= min_exposed && q >= 0.0;  // (q >= 0: no NaN)
}

// The decision of one row on its slot's view_q[0 .. n_bins), in place: a reset empties every bin first; the face is
// TAKEN when it is eligible, binned and strictly better than what its bin holds.  Returns take: the bin, or -1.
__host__ __device__ __forceinline__ int views_decide(bool reset, bool eligible, double q, int bin, double* view_q,
                                                     int n_bins) {
  if (reset)
    for (int b = 0; b < n_bins; ++b) view_q[b] = -1.0;
  if (!eligible || bin < 0) return -1;
  if (!(q > view_q[bin])) return -1;
  view_q[bin] = q;
  return bin;
}

}  // namespace flm
