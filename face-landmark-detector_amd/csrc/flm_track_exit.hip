// flm_track_retire (include/flm.h states the contract; flm_track_exit_dev.h holds the per-slot decision and the row
// arithmetic; the comments here only say how the work is laid out).  Two launches:
//   track_exit_decide_kernel  ONE workgroup walks the K slots a chunk of blockDim.x at a time, twice.  The first walk
//       only counts the emitted tracks: E decides which of them are written and which are overrun.  The second walk
//       ranks the emitted tracks and the births side by side, as track_gather_live_kernel ranks its live slots: a
//       ballot and mbcnt give the prefix inside the wave, the waves' totals meet in LDS, and a carry every thread keeps
//       for itself runs from chunk to chunk.  No atomics: every rank is a function of the inputs.  A thread owns its
//       slot: it writes exit_row, the slot's id, birth frame and flag, and, for a written track, the ring row's meta
//       words, quality, matrix and record.  Nothing is written during the first walk, so the second reads the inputs the
//       first read.  head is read by every thread before the first barrier and written by thread 0 after the last.
//   track_exit_copy_kernel    grid (chunk, slot): the workgroups of a slot whose exit_row is negative leave at once; the
//       others move the slot's gallery bytes -- and, workgroup 0 of the slot, its landmarks -- into the ring row.  It
//       reads exit_row and buffers no launch writes meanwhile.
#include "flm_common.h"
#include "flm_copy_dev.h"
#include "flm_track_exit_dev.h"

namespace flm {

constexpr int kExitCopyThreads = 256, kExitCopyChunk = kExitCopyThreads * 16 * 4;  // bytes a workgroup is dealt

__device__ __forceinline__ ExitDecision exit_decide_slot(const TrackExitArgs& g, int t) {
  const int32_t* bx = g.boxes + (size_t)t * 4;
  const bool live = exit_box_live(bx[0], bx[1], bx[2], bx[3], g.fh, g.fw);
  return exit_decide(g.track_id[t], g.born[t], live, g.flush, g.best_q[t], g.min_q, g.status[t]);
}

__global__ __launch_bounds__(1024) void track_exit_decide_kernel(const TrackExitArgs g) {
  __shared__ int wave_cnt[3][16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n_waves = blockDim.x >> 6;
  const int64_t seq0 = g.head[0], next_id = g.head[1], disc0 = g.head[2], over0 = g.head[3];

  // ---- the first walk: E
  int wave_e = 0;   // the same number in every lane of a wave
  for (int base = 0; base < g.k; base += blockDim.x) {
    const int t = base + tid;
    const bool em = t < g.k && exit_decide_slot(g, t).emitted;
    wave_e += __popcll(__ballot(em));
  }
  if (lane == 0) wave_cnt[0][wave] = wave_e;
  __syncthreads();
  int e_total = 0;
  for (int w = 0; w < n_waves; ++w) e_total += wave_cnt[0][w];
  __syncthreads();   // wave_cnt is rewritten below

  // ---- the second walk: ranks, rows, ids
  int carry_e = 0, carry_b = 0, carry_d = 0;   // emitted, born, discarded in the chunks before this one
  for (int base = 0; base < g.k; base += blockDim.x) {
    const int t = base + tid;
    const bool in = t < g.k;
    ExitDecision d;
    d.ends = d.emitted = d.birth = d.clears = false;
    d.end = 0;
    if (in) d = exit_decide_slot(g, t);
    const unsigned long long m_e = __ballot(d.emitted), m_b = __ballot(d.birth), m_d = __ballot(d.ends && !d.emitted);
    const int below_e = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m_e >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m_e, 0u));
    const int below_b = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m_b >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m_b, 0u));
    if (lane == 0) {
      wave_cnt[0][wave] = __popcll(m_e);
      wave_cnt[1][wave] = __popcll(m_b);
      wave_cnt[2][wave] = __popcll(m_d);
    }
    __syncthreads();
    int before_e = 0, before_b = 0, tot_e = 0, tot_b = 0, tot_d = 0;
    for (int w = 0; w < n_waves; ++w) {
      const int ce = wave_cnt[0][w], cb = wave_cnt[1][w];
      before_e += w < wave ? ce : 0;
      before_b += w < wave ? cb : 0;
      tot_e += ce;
      tot_b += cb;
      tot_d += wave_cnt[2][w];
    }
    if (in) {
      const int r = carry_e + before_e + below_e, b = carry_b + before_b + below_b;
      const int32_t row = exit_row_of(d, r, e_total, g.q, seq0);
      const int64_t id = g.track_id[t];
      if (row >= 0) {   // a written track: the ring row's small records (row < q by exit_ring_row)
        exit_meta_store(g.x_meta + (size_t)row * FLM_EXIT_META, id, t, g.born_frame[t], g.frame_id, g.best_frame[t], d.end,
                        seq0 + r);
        g.x_q[row] = g.best_q[t];
        if (g.x_m) {
          const float* mi = g.best_m + (size_t)t * 6;
          float* mo = g.x_m + (size_t)row * 6;
          mo[0] = mi[0]; mo[1] = mi[1]; mo[2] = mi[2]; mo[3] = mi[3]; mo[4] = mi[4]; mo[5] = mi[5];
        }
        if (g.x_rec) {
          const int64_t* ri = g.best_rec + (size_t)t * FLM_QUALITY_REC;
          int64_t* ro = g.x_rec + (size_t)row * FLM_QUALITY_REC;
#pragma unroll
          for (int i = 0; i < FLM_QUALITY_REC; ++i) ro[i] = ri[i];
        }
      }
      g.exit_row[t] = row;
      if (d.birth || d.clears) g.track_id[t] = exit_next_track_id(d, id, b, next_id);
      if (d.birth) g.born_frame[t] = g.frame_id;
      g.born[t] = 0;
    }
    carry_e += tot_e;
    carry_b += tot_b;
    carry_d += tot_d;
    __syncthreads();   // wave_cnt is rewritten by the next chunk
  }
  if (tid == 0) exit_head_store(g.head, seq0, next_id, disc0, over0, carry_e, carry_b, carry_d, g.q);
}

// The face of every written track, and its landmarks: pieces of 16 bytes at the 16-byte lines of the SOURCE address, as
// track_best_body copies them (flm_copy_dev.h); element accesses where the two addresses are not congruent and at the
// row's two ends.
__global__ __launch_bounds__(kExitCopyThreads) void track_exit_copy_kernel(const TrackExitArgs g) {
  const int t = blockIdx.y, tid = threadIdx.x;
  const int row = g.exit_row[t];
  if (row < 0 || row >= g.q) return;   // nothing of this slot was written: the whole workgroup leaves
  if (g.x_lm && blockIdx.x == 0) {
    const double* li = g.best_lm + (size_t)t * g.c * 2;
    double* lo = g.x_lm + (size_t)row * g.c * 2;
    for (int i = tid; i < 2 * g.c; i += kExitCopyThreads) lo[i] = li[i];
  }
  copy_row_bytes(g.gallery + (size_t)t * g.face_bytes, g.x_gallery + (size_t)row * g.face_bytes, g.face_bytes,
                 (size_t)blockIdx.x * kExitCopyThreads + tid, (size_t)gridDim.x * kExitCopyThreads);
}

int launch_track_retire(hipStream_t s, const TrackExitArgs& g) {
  const int waves = cdiv(g.k, 64);   // whole waves, 16 at the most: the kernel walks the rest in chunks
  const int threads = 64 * (waves < 16 ? waves : 16);
  track_exit_decide_kernel<<<1, threads, 0, s>>>(g);
  FLM_LAUNCH_CHECK("track_exit_decide_kernel");
  size_t chunks = (g.face_bytes + 15 + kExitCopyChunk - 1) / kExitCopyChunk;   // (+15: the lead-in of an unaligned face)
  if (chunks > 1024) chunks = 1024;
  track_exit_copy_kernel<<<dim3((unsigned)chunks, g.k), kExitCopyThreads, 0, s>>>(g);
  FLM_LAUNCH_CHECK("track_exit_copy_kernel");
  return FLM_OK;
}

}  // namespace flm
