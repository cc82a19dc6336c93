// flm_head_pose (include/flm.h states every operation; flm_pose_dev.h holds them; the comments here only say how the work is
// laid out).  One launch, a workgroup of one wave per row, as track_step_kernel:
//   (1) the lanes stage the model's points -- the 3-D point, the landmark it names, its weight, 0.0 for a point that does
//       not take part -- into LDS, point p by lane p % 64;
//   (2) the six sums of the first pass run on lanes 0..5, one sum per lane, sequentially over p in LDS; the means go
//       through LDS;
//   (3) the twelve sums of the second pass run on lanes 0..11 the same way;
//   (4) lane 0 solves, sums the residual, and writes the record and the factor.
// Every sum is one lane's sequential loop in model order: the result does not depend on the launch shape.
#include "flm_common.h"
#include "flm_pose_dev.h"

namespace flm {

constexpr int kPoseMaxPoints = 256;

struct PoseArgs {
  const double* lm;
  size_t lm_stride;
  const double* wt;      // or null
  size_t w_stride;
  int c, p;
  const int32_t* idx;    // [P]
  const double* xyz;     // [P,3]
  double min_volume, min_frontal;
  const int32_t* slot;   // [N] or null
  int n_slots;
  double* pose;          // [N or n_slots, 18]
  double* factor;        // [N] or null
};

__global__ __launch_bounds__(64) void head_pose_kernel(const PoseArgs g) {
  __shared__ double pt[kPoseMaxPoints * kPosePt];
  __shared__ double sums[kPoseSums1 + kPoseSums2];
  __shared__ double mean[5];
  __shared__ int s_cnt;
  const int r = blockIdx.x, lane = threadIdx.x;
  size_t gs = (size_t)r;
  if (g.slot) {
    const int v = g.slot[r];
    if (v < 0 || v >= g.n_slots) {  // an inert row: the whole wave leaves before any barrier
      if (g.factor && lane == 0) g.factor[r] = 0.0;
      return;
    }
    gs = (size_t)v;
  }
  for (int i = lane; i < g.p; i += 64) {
    const int id = g.idx[i];
    const bool in_range = id >= 0 && id < g.c;
    double x = -1.0, y = -1.0, w = 0.0;
    if (in_range) {
      const size_t e = (size_t)r * g.c + id;
      const double* q = g.lm + e * g.lm_stride;
      x = q[0];
      y = q[1];
      w = g.wt ? g.wt[e * g.w_stride] : 1.0;
    }
    pose_stage(pt + kPosePt * i, g.xyz + 3 * (size_t)i, in_range, x, y, w);
  }
  __syncthreads();
  if (lane < kPoseSums1) {
    int cnt = 0;
    sums[lane] = pose_sum1(lane, pt, g.p, &cnt);
    if (lane == 0) s_cnt = cnt;
  }
  __syncthreads();
  if (lane < 5) mean[lane] = sums[lane + 1] / sums[0];
  __syncthreads();
  if (lane < kPoseSums2) sums[kPoseSums1 + lane] = pose_sum2(lane, pt, g.p, mean);
  __syncthreads();
  if (lane != 0) return;
  double rec[FLM_POSE_REC];
  const bool ok = pose_solve(sums, sums + kPoseSums1, s_cnt, pt, g.p, g.min_volume, rec, nullptr);
  double* o = g.pose + gs * FLM_POSE_REC;
#pragma unroll
  for (int i = 0; i < FLM_POSE_REC; ++i) o[i] = rec[i];
  if (g.factor) g.factor[r] = pose_factor(ok, rec, g.min_frontal);
}

// Pointers, options, strides and overlaps are checked by the caller in flm_api.hip.
int launch_head_pose(hipStream_t s, const double* lm, size_t lm_stride, const double* wt, size_t w_stride, int n, int c,
                     const int32_t* idx, const double* xyz, int p, const flm_pose_opts* opts, const int32_t* slot,
                     int n_slots, double* pose, double* factor) {
  PoseArgs g;
  g.lm = lm; g.lm_stride = lm_stride; g.wt = wt; g.w_stride = w_stride; g.c = c; g.p = p;
  g.idx = idx; g.xyz = xyz;
  g.min_volume = opts->min_volume; g.min_frontal = opts->min_frontal;
  g.slot = slot; g.n_slots = n_slots; g.pose = pose; g.factor = factor;
  head_pose_kernel<<<n, 64, 0, s>>>(g);
  FLM_LAUNCH_CHECK("head_pose_kernel");
  return FLM_OK;
}

}  // namespace flm
