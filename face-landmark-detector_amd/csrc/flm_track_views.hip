// flm_track_views_update and flm_track_exit_views (include/flm.h states the contract; flm_track_views_dev.h holds the bin
// and the per-row decision, flm_best_dev.h the quality arithmetic shared with flm_track_best_update, flm_copy_dev.h the
// row copy shared with the best-shot and exit kernels; the comments here only say how the work is laid out).
//
// flm_track_views_update, two launches:
//   track_views_decide_kernel  one THREAD per row.  The thread derives q, the bin and the decision of its row and is the
//       only reader and writer of its slot's [B] qualities, so view_q is updated in place: no snapshot, no second buffer,
//       and nothing another thread of the launch reads is written.  It writes take, and for a taken row the bin's frame
//       id, matrix, landmarks and pose record -- a few hundred bytes, not worth a workgroup.
//   track_views_copy_kernel    grid (chunk, row): reads take (and the row's slot); the workgroups of a row that is not
//       taken leave at once, the others move the face into the bin's gallery row.
// flm_track_exit_views, one launch:
//   track_exit_views_kernel    grid (chunk x bin, slot): the workgroups of a slot whose exit_row is negative leave at
//       once.  Chunk 0 of (slot, bin) writes the bin's quality and frame id into the ring row, and, for a bin that holds a
//       face, its matrix, landmarks and pose; every chunk of such a bin moves its share of the face.  Nothing the launch
//       reads is written by it.
#include "flm_best_dev.h"
#include "flm_common.h"
#include "flm_copy_dev.h"
#include "flm_track_views_dev.h"

namespace flm {

constexpr int kViewsThreads = 64;                                            // rows per workgroup of the decision
constexpr int kViewsCopyThreads = 256, kViewsCopyChunk = kViewsCopyThreads * 16 * 4;  // bytes a workgroup is dealt

__global__ __launch_bounds__(kViewsThreads) void track_views_decide_kernel(const TrackViewsArgs g) {
  const int r = blockIdx.x * kViewsThreads + threadIdx.x;
  if (r >= g.n) return;
  int gs = r;
  if (g.slot) {
    gs = g.slot[r];
    if (gs < 0 || gs >= g.n_slots) {  // an inert row
      g.take[r] = -1;
      return;
    }
  }
  const size_t sg = (size_t)gs, sr = (size_t)r;
  const double* lm = g.lm + sr * g.c * g.lm_stride;
  const BestTerms t = best_terms(g.rec + sr * FLM_QUALITY_REC, lm, g.lm_stride,
                                 g.wt ? g.wt + sr * g.c * g.w_stride : nullptr, g.w_stride, g.c, g.sharp_ref);
  const double q = t.sew;
  const bool eligible = views_eligible(!g.status || g.status[r] == 0, t.n_lap, t.e, g.min_exposed, q);
  ViewsBins b;
  b.n_u = g.n_u;
  b.n_v = g.n_v;
#pragma unroll
  for (int i = 0; i < FLM_VIEWS_MAX_EDGES; ++i) {
    b.u_edge[i] = g.u_edge[i];
    b.v_edge[i] = g.v_edge[i];
  }
  const double* pose = g.pose + sg * FLM_POSE_REC;
  const int bin = views_bin(pose, b);
  const int take = views_decide(g.reset && g.reset[r] != 0, eligible, q, bin, g.view_q + sg * g.bins, g.bins);
  g.take[r] = take;
  if (take < 0) return;
  const size_t o = sg * g.bins + (size_t)take;
  g.view_frame[o] = g.frame_id;
  if (g.view_m) {
    const float* mi = g.m + sr * 6;
    float* mo = g.view_m + o * 6;
    mo[0] = mi[0]; mo[1] = mi[1]; mo[2] = mi[2]; mo[3] = mi[3]; mo[4] = mi[4]; mo[5] = mi[5];
  }
  if (g.view_pose) {
    double* po = g.view_pose + o * FLM_POSE_REC;
#pragma unroll
    for (int i = 0; i < FLM_POSE_REC; ++i) po[i] = pose[i];
  }
  if (g.view_lm) {
    double* lo = g.view_lm + o * g.c * 2;
    for (int i = 0; i < g.c; ++i) {
      lo[2 * i] = lm[(size_t)i * g.lm_stride];
      lo[2 * i + 1] = lm[(size_t)i * g.lm_stride + 1];
    }
  }
}

__global__ __launch_bounds__(kViewsCopyThreads) void track_views_copy_kernel(const TrackViewsArgs g) {
  const int r = blockIdx.y;
  const int take = g.take[r];
  if (take < 0) return;  // not taken: the whole workgroup leaves
  const int gs = g.slot ? g.slot[r] : r;
  // The decision wrote take < bins for rows with a valid slot alone; the two tests below cannot fire on its output.  They
  // keep the copy inside the gallery if a caller's stream lets something else write take_dev or slot_dev in between.
  if (take >= g.bins || gs < 0 || gs >= g.n_slots) return;
  copy_row_bytes(g.faces + (size_t)r * g.face_bytes,
                 g.view_gallery + ((size_t)gs * g.bins + (size_t)take) * g.face_bytes, g.face_bytes,
                 (size_t)blockIdx.x * kViewsCopyThreads + threadIdx.x, (size_t)gridDim.x * kViewsCopyThreads);
}

__global__ __launch_bounds__(kViewsCopyThreads) void track_exit_views_kernel(const TrackExitViewsArgs g) {
  const int t = blockIdx.y, tid = threadIdx.x;
  const int row = g.exit_row[t];
  if (row < 0 || row >= g.q) return;  // nothing of this slot was written: the whole workgroup leaves
  const int chunk = blockIdx.x / g.bins, b = blockIdx.x - chunk * g.bins, n_chunks = gridDim.x / g.bins;
  const size_t si = (size_t)t * g.bins + b, di = (size_t)row * g.bins + b;
  const double qv = g.view_q[si];
  if (chunk == 0 && tid == 0) {
    g.x_view_q[di] = qv;
    g.x_view_frame[di] = g.view_frame[si];
  }
  if (!(qv >= 0.0)) return;  // an empty bin: its ring bytes stay
  if (chunk == 0) {
    if (g.x_view_m && tid < 6) g.x_view_m[di * 6 + tid] = g.view_m[si * 6 + tid];
    if (g.x_view_pose && tid >= 64 && tid < 64 + FLM_POSE_REC)
      g.x_view_pose[di * FLM_POSE_REC + (tid - 64)] = g.view_pose[si * FLM_POSE_REC + (tid - 64)];
    if (g.x_view_lm) {
      const double* li = g.view_lm + si * g.c * 2;
      double* lo = g.x_view_lm + di * g.c * 2;
      for (int i = tid; i < 2 * g.c; i += kViewsCopyThreads) lo[i] = li[i];
    }
  }
  copy_row_bytes(g.view_gallery + si * g.face_bytes, g.x_view_gallery + di * g.face_bytes, g.face_bytes,
                 (size_t)chunk * kViewsCopyThreads + tid, (size_t)n_chunks * kViewsCopyThreads);
}

static unsigned views_copy_chunks(size_t face_bytes) {
  size_t chunks = (face_bytes + 15 + kViewsCopyChunk - 1) / kViewsCopyChunk;  // (+15: the lead-in of an unaligned face)
  return (unsigned)(chunks > 1024 ? 1024 : chunks);
}

int launch_track_views_update(hipStream_t s, const TrackViewsArgs& g) {
  track_views_decide_kernel<<<cdiv(g.n, kViewsThreads), kViewsThreads, 0, s>>>(g);
  FLM_LAUNCH_CHECK("track_views_decide_kernel");
  track_views_copy_kernel<<<dim3(views_copy_chunks(g.face_bytes), g.n), kViewsCopyThreads, 0, s>>>(g);
  FLM_LAUNCH_CHECK("track_views_copy_kernel");
  return FLM_OK;
}

int launch_track_exit_views(hipStream_t s, const TrackExitViewsArgs& g) {
  // (chunks <= 1024 and bins <= 64: the grid's x stays at or below 65536)
  track_exit_views_kernel<<<dim3(views_copy_chunks(g.face_bytes) * (unsigned)g.bins, g.k), kViewsCopyThreads, 0, s>>>(g);
  FLM_LAUNCH_CHECK("track_exit_views_kernel");
  return FLM_OK;
}

}  // namespace flm
