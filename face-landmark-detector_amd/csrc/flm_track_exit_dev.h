// The per-slot decision and the row arithmetic of flm_track_retire (include/flm.h states the contract), as
// __host__ __device__ functions: track_exit_decide_kernel (flm_track_exit.hip) is built from them, and
// tests/native/track_exit_host.cpp runs the same functions on the host against a serial restatement.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "flm.h"

namespace flm {

// Step 1: the clip of the tracking section; live = the clipped box is not empty.
__host__ __device__ __forceinline__ bool exit_box_live(int x0, int y0, int x1, int y1, int fh, int fw) {
  const int cx0 = x0 < 0 ? 0 : (x0 > fw ? fw : x0), cx1 = x1 < 0 ? 0 : (x1 > fw ? fw : x1);
  const int cy0 = y0 < 0 ? 0 : (y0 > fh ? fh : y0), cy1 = y1 < 0 ? 0 : (y1 > fh ? fh : y1);
  return cx1 - cx0 > 0 && cy1 - cy0 > 0;
}

struct ExitDecision {
  bool ends;      // step 2
  bool emitted;   // step 3: ends and best_q >= min_q
  bool birth;     // step 6: born and live
  bool clears;    // the slot's id becomes -1: it ended or was born, and is no birth
  int64_t end;    // step 5: status, -1 (restarted before its end was seen) or -2 (flush); read only when ends
};

__host__ __device__ __forceinline__ ExitDecision exit_decide(int64_t track_id, int32_t born_flag, bool live, int flush,
                                                             double best_q, double min_q, int32_t status) {
  ExitDecision d;
  const bool born = born_flag != 0, held = track_id >= 0;
  d.ends = held && (born || !live || flush != 0);
  d.emitted = d.ends && best_q >= min_q;   // (false for a NaN, and for the -1 of "no best": min_q >= 0)
  d.birth = born && live;
  d.clears = (d.ends || born) && !d.birth;
  d.end = born ? (int64_t)-1 : !live ? (int64_t)status : (int64_t)-2;
  return d;
}

// Step 4: the ring row of sequence number seq, the non-negative remainder (seq is a count, never negative, in a head the
// call itself has kept; a junk head still names a row inside the ring).
__host__ __device__ __forceinline__ int exit_ring_row(int64_t seq, int q) {
  const int64_t m = seq % (int64_t)q;
  return (int)(m < 0 ? m + q : m);
}

// exit_row of a slot: -1 nothing ended, -2 discarded, -3 overrun, else the ring row.  r: the rank among the e emitted
// tracks of the call.
__host__ __device__ __forceinline__ int32_t exit_row_of(const ExitDecision& d, int r, int e, int q, int64_t seq0) {
  if (!d.ends) return -1;
  if (!d.emitted) return -2;
  if (r < e - q) return -3;
  return (int32_t)exit_ring_row(seq0 + r, q);
}

// Step 5: the FLM_EXIT_META words of a written row.
__host__ __device__ __forceinline__ void exit_meta_store(int64_t* o, int64_t track_id, int slot, int64_t born_frame,
                                                         int64_t frame_id, int64_t best_frame, int64_t end, int64_t seq) {
  o[0] = track_id; o[1] = (int64_t)slot; o[2] = born_frame; o[3] = frame_id;
  o[4] = best_frame; o[5] = end; o[6] = seq; o[7] = 0;
}

// Step 6: the id a slot holds after the call; b: the rank among the births.
__host__ __device__ __forceinline__ int64_t exit_next_track_id(const ExitDecision& d, int64_t track_id, int b, int64_t next_id) {
  return d.birth ? next_id + b : d.clears ? (int64_t)-1 : track_id;
}

// Step 4 and 6: head = {seq, next_id, discarded, overrun} after a call with e emitted, b born and n_disc discarded tracks.
__host__ __device__ __forceinline__ void exit_head_store(int64_t* head, int64_t seq0, int64_t next_id, int64_t disc0,
                                                         int64_t over0, int e, int b, int n_disc, int q) {
  head[0] = seq0 + e;
  head[1] = next_id + b;
  head[2] = disc0 + n_disc;
  head[3] = over0 + (e > q ? e - q : 0);
}

}  // namespace flm
