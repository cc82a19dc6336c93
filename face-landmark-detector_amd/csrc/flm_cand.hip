// Candidate path of the landmark mode (flm_convt.hip): the per-class thresholds of a sampling launch and
// the exact top-n selection from the candidate keys the last transposed conv emitted.  The key lists are the decode's
// (flm_topn_dev.h), so ties resolve as they do when a materialised map is decoded (flm_decode.hip).
#include "flm_common.h"
#include "flm_topn_dev.h"

namespace flm {

// Exact top n of a face's candidate keys (flm_convt.hip, epilogue 3): key = order_bits(p) << 32 | class << 17 |
// pixel, in the order the workgroups of the candidate launch flushed them.  grid = (G, faces): workgroup g owns the
// classes g*cpg .. g*cpg + cpg - 1, wave w of its NW the classes g*cpg + w + NW*k.  The keys are first BUCKETED by class in
// LDS (counting sort: histogram, prefix, scatter; kMergeKeys per pass, a longer list takes several passes with the
// lists kept in registers), then every wave feeds only the ~cnt/68 keys of each of its classes to the same descending
// (value, pixel) lists as the decode of a materialised map, so ties resolve identically -- the keys are distinct and
// the lists order-independent, so the bucket order does not matter.  (Round 1 had every wave scan ALL keys of the face
// once per class it owned: 0.16 ms per 512 faces, a serial chain of cnt/64 steps x 5 classes per wave.)
struct CandMergeArgs {
  const unsigned long long* cand;
  unsigned* cand_cnt;  // [n] fill counts, [n] = fallback flag
  unsigned* cand_redo; // [n] or null: the fallback flag per face
  int n, w, l, n_points, cap;
  float thresh;
  double* out;  // [n][l][2], or landmark records [n][l][FLM_LANDMARK_REC] for the stats kernel
  int cpg;  // classes per workgroup
};

constexpr int kMergeKeys = 6144;     // 48 KiB of keys per pass: three workgroups per CU
constexpr int kCandFineBatch = 128;  // below: four workgroups per face (the chip would sit empty with one)

// STATS: the lists are finished as landmark records (finish_topn_stats); the selection is the same code, and the
// STATS = false instantiations are the kernels FLM_OUT_LANDMARKS ran before the flag.
template <int CPW, int NW, bool STATS>  // NW waves, CPW = ceil(cpg / NW) classes per wave
__global__ __launch_bounds__(NW * 64) void cand_merge_kernel(CandMergeArgs a) {
  __shared__ unsigned long long keys[kMergeKeys];
  __shared__ int hist[NW * CPW + 1], off[NW * CPW + 1];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int face = blockIdx.y;
  const int cfirst = a.cpg * blockIdx.x, cend = min(cfirst + a.cpg, a.l);
  const int nc = cend - cfirst;
  const unsigned cnt = min(a.cand_cnt[face], (unsigned)a.cap);
  const unsigned long long* src = a.cand + (size_t)face * a.cap;
  unsigned long long list[CPW], tau[CPW];
#pragma unroll
  for (int k = 0; k < CPW; ++k) { list[k] = 0ull; tau[k] = 0ull; }
  constexpr int KPT = kMergeKeys / (NW * 64);  // keys per thread and pass, all loads in flight at once
  for (unsigned base = 0; base < cnt; base += kMergeKeys) {
    unsigned long long kreg[KPT];
#pragma unroll
    for (int j = 0; j < KPT; ++j) {
      const unsigned i = base + tid + NW * 64 * j;
      kreg[j] = i < cnt ? src[i] : 0ull;
    }
    if (tid <= NW * CPW) hist[tid] = 0;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < KPT; ++j) {
      const int rel = (int)((kreg[j] >> 17) & 127u) - cfirst;
      if (kreg[j] != 0ull && (unsigned)rel < (unsigned)nc) atomicAdd(&hist[rel], 1);
      else kreg[j] = 0ull;
    }
    __syncthreads();
    if (wave == 0) {  // exclusive prefix over the classes; hist becomes the write cursor
      const int v = lane < nc ? hist[lane] : 0;
      int incl = v;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(incl, d);
        if (lane >= d) incl += t;
      }
      if (lane < nc) {
        off[lane] = incl - v;
        hist[lane] = incl - v;
      }
      if (lane == 63 && nc >= 64) {
        int run = incl;
        for (int c = 64; c < nc; ++c) {
          off[c] = run;
          const int h = hist[c];
          hist[c] = run;
          run += h;
        }
        off[nc] = run;
      }
      if (nc < 64 && lane == nc) off[nc] = incl;  // (incl of lane nc = the total: its own v is 0)
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < KPT; ++j) {
      if (kreg[j] != 0ull) {
        const int rel = (int)((kreg[j] >> 17) & 127u) - cfirst;
        keys[atomicAdd(&hist[rel], 1)] = (kreg[j] & 0xffffffff00000000ull) | (kreg[j] & 0x1ffffull);
      }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < CPW; ++k) {
      const int rel = wave + NW * k;
      if (rel < nc) {  // wave-uniform
        const int lo = off[rel], hi = off[rel + 1];
        for (int i0 = lo; i0 < hi; i0 += 64) {
          const unsigned long long cand = (i0 + lane < hi) ? keys[i0 + lane] : 0ull;
          if (__any(cand > tau[k])) insert_candidates(list[k], tau[k], cand, a.n_points, lane);
        }
      }
    }
    __syncthreads();  // the next pass overwrites the buckets
  }
#pragma unroll
  for (int k = 0; k < CPW; ++k) {
    const int c = cfirst + wave + NW * k;
    if (c < cend) {
      // fewer than n keys: the threshold did not have n pixels above it (or the class has fewer than n non-zero
      // pixels), so the list may not hold the whole top n -> let the materialising path redo the batch
      if (readlane64(list[k], a.n_points - 1) == 0ull && lane == 0) {
        atomicOr(&a.cand_cnt[a.n], 1u);
        if (a.cand_redo) a.cand_redo[face] = 1u;
      }
      if constexpr (STATS) finish_topn_stats(list[k], a.n_points, a.w, a.thresh, lane, a.out + ((size_t)face * a.l + c) * FLM_LANDMARK_REC);
      else finish_topn(list[k], a.n_points, a.w, a.thresh, lane, a.out + ((size_t)face * a.l + c) * 2);
    }
  }
}

// tau[face][class] = n-th largest of the face's wave maxima (flm_convt.hip, epilogue 4); 0 when fewer than n are
// non-zero (the consumer clamps to FLT_MIN and cand_merge_kernel checks that n keys arrived).
__global__ __launch_bounds__(256) void cand_tau_kernel(const unsigned* __restrict__ wave_max, int slots, int ld, int l,
                                                       int n_points, float* __restrict__ tau) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int face = blockIdx.x;
  const unsigned* src = wave_max + (size_t)face * slots * ld;
  for (int c = blockIdx.y * 4 + wave; c < l; c += 4 * gridDim.y) {  // one class per wave and round
    unsigned long long list = 0ull, t = 0ull;
    for (int s0 = 0; s0 < slots; s0 += 64) {
      const int sl = s0 + lane;
      const unsigned v = sl < slots ? src[(size_t)sl * ld + c] : 0u;
      const unsigned long long key = v ? (((unsigned long long)v << 32) | (unsigned)sl) : 0ull;
      if (__any(key > t)) insert_candidates(list, t, key, n_points, lane);
    }
    const unsigned long long k = readlane64(list, n_points - 1);
    if (lane == 0) tau[(size_t)face * l + c] = __uint_as_float((unsigned)(k >> 32));
  }
}

// The same threshold for n <= 8 with the reads coalesced: lanes run along the classes (the ld values of a slot are
// contiguous), three groups of threads share the slots, every thread keeps its n largest maxima in registers (a sorted
// insertion, values with multiplicity, zeros never enter), and one thread per class merges the three short lists.  The
// wave-per-class kernel above reads a slot column with a stride of ld words: 64 cache lines per load (bf16 batch 512:
// 45 -> 23 us).
template <int NMAX>
__global__ __launch_bounds__(256) void cand_tau_small_kernel(const unsigned* __restrict__ wave_max, int slots, int ld, int l,
                                                             int n_points, float* __restrict__ tau) {
  __shared__ unsigned part[3][NMAX][96];
  const int face = blockIdx.x, tid = threadIdx.x;
  const int g = tid / ld, c = tid - g * ld;   // ld <= 85: three groups fit 256 threads
  const unsigned* src = wave_max + (size_t)face * slots * ld;
  unsigned top[NMAX];
#pragma unroll
  for (int k = 0; k < NMAX; ++k) top[k] = 0u;
  if (g < 3) {
#pragma unroll 8
    for (int sl = g; sl < slots; sl += 3) {
      unsigned v = src[(size_t)sl * ld + c];
      if (v > top[NMAX - 1]) {
#pragma unroll
        for (int k = 0; k < NMAX; ++k) {  // descending; v sinks to its place, the smallest falls out
          const unsigned hi = v > top[k] ? v : top[k], lo = v > top[k] ? top[k] : v;
          top[k] = hi;
          v = lo;
        }
      }
    }
#pragma unroll
    for (int k = 0; k < NMAX; ++k) part[g][k][c] = top[k];
  }
  __syncthreads();
  if (g == 0 && c < l) {
#pragma unroll
    for (int gg = 1; gg < 3; ++gg)
#pragma unroll
      for (int j = 0; j < NMAX; ++j) {
        unsigned v = part[gg][j][c];
        if (v > top[NMAX - 1]) {
#pragma unroll
          for (int k = 0; k < NMAX; ++k) {
            const unsigned hi = v > top[k] ? v : top[k], lo = v > top[k] ? top[k] : v;
            top[k] = hi;
            v = lo;
          }
        }
      }
    unsigned t = 0u;
#pragma unroll
    for (int k = 0; k < NMAX; ++k)
      if (k == n_points - 1) t = top[k];
    tau[(size_t)face * l + c] = __uint_as_float(t);
  }
}

int launch_cand_tau(hipStream_t s, const unsigned* wave_max, int n, int slots, int ld, int l, int n_points, float* tau) {
  if (n_points < 1 || n_points > 64 || slots < 1) {
    set_error("cand_tau: unsupported n_points=%d slots=%d", n_points, slots);
    return FLM_ERR_UNSUPPORTED;
  }
  // (one workgroup per face: below ~200 faces it leaves the chip empty and the wave-per-class kernel, 24 waves per
  // face, is faster -- 64 faces: 18 us against 32)
  if (n >= 192 && n_points <= 8 && ld <= 85 && l <= ld) {
    // NMAX = n_points would do; two instantiations keep the code small (lists longer than n only cost compares)
    if (n_points <= 4) cand_tau_small_kernel<4><<<n, 256, 0, s>>>(wave_max, slots, ld, l, n_points, tau);
    else cand_tau_small_kernel<8><<<n, 256, 0, s>>>(wave_max, slots, ld, l, n_points, tau);
    FLM_LAUNCH_CHECK("cand_tau_small_kernel");
    return FLM_OK;
  }
  cand_tau_kernel<<<dim3(n, 6), 256, 0, s>>>(wave_max, slots, ld, l, n_points, tau);
  FLM_LAUNCH_CHECK("cand_tau_kernel");
  return FLM_OK;
}

int launch_cand_merge(hipStream_t s, const unsigned long long* cand, unsigned* cand_cnt, int n, int w, int l,
                      int n_points, float thresh, int cap, double* out, int stats, unsigned* cand_redo) {
  if (l > 68 || n_points < 1 || n_points > 64) {
    set_error("cand_merge: unsupported l=%d n_points=%d", l, n_points);
    return FLM_ERR_UNSUPPORTED;
  }
  CandMergeArgs a;
  a.cand = cand; a.cand_cnt = cand_cnt; a.cand_redo = cand_redo; a.n = n; a.w = w; a.l = l; a.n_points = n_points; a.cap = cap;
  a.thresh = thresh; a.out = out;
  if (n < kCandFineBatch) {
    a.cpg = 17;
    if (stats) cand_merge_kernel<5, 4, true><<<dim3(cdiv(l, 17), n), 256, 0, s>>>(a);
    else cand_merge_kernel<5, 4, false><<<dim3(cdiv(l, 17), n), 256, 0, s>>>(a);
  } else {
    a.cpg = 68;
    if (stats) cand_merge_kernel<9, 8, true><<<dim3(1, n), 512, 0, s>>>(a);
    else cand_merge_kernel<9, 8, false><<<dim3(1, n), 512, 0, s>>>(a);
  }
  FLM_LAUNCH_CHECK("cand_merge_kernel");
  return FLM_OK;
}

// ---- per-face fallback: the faces that raised, compacted into the row budget -------------------------------------------
// ONE workgroup of 256 walks cand_redo[0..n) a chunk of 256 faces at a time, as track_gather_live_kernel (flm_track.hip)
// walks its slots: a ballot and mbcnt give a raised face's rank within its wave, the waves' totals meet in LDS, and a
// carry every thread keeps for itself runs from chunk to chunk -- so the exclusive prefix count IS the row, no atomics, and
// the order (ascending faces) is a function of the input.  R is known after the last chunk: the rows from R on, the counts
// and the two gate words are written then.
__global__ __launch_bounds__(256) void fallback_plan_kernel(const unsigned* __restrict__ cand_redo, int n, int budget,
                                                            int* __restrict__ rows, unsigned* __restrict__ counts) {
  __shared__ int wave_total[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int carry = 0;  // raised faces before this chunk
  for (int base = 0; base < n; base += 256) {
    const int face = base + tid;
    const bool raised = face < n && cand_redo[face] != 0u;
    const unsigned long long mask = __ballot(raised);
    const int below = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
    if (lane == 0) wave_total[wave] = __popcll(mask);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const int t = wave_total[w];
      before += w < wave ? t : 0;
      total += t;
    }
    const int rank = carry + before + below;
    carry += total;
    if (raised && rank < budget) rows[rank] = face;
    __syncthreads();  // wave_total is rewritten by the next chunk
  }
  const int R = carry;
  for (int r = R + tid; r < budget; r += 256) rows[r] = -1;
  if (tid == 0) {
    const bool batch = R > budget;
    counts[0] = (unsigned)R;
    counts[1] = batch ? 0u : (unsigned)R;
    counts[2] = batch ? 1u : 0u;
    counts[3] = (unsigned)budget;
    counts[4] = (R > 0 && !batch) ? 1u : 0u;  // rows_gate
    counts[5] = batch ? 1u : 0u;              // batch_gate
  }
}

int launch_fallback_plan(hipStream_t s, const unsigned* cand_redo, int n, int budget, int* rows, unsigned* counts) {
  if (!cand_redo || !rows || !counts || n < 1 || budget < 1 || budget > n) {
    set_error("fallback_plan: bad argument (n=%d budget=%d)", n, budget);
    return FLM_ERR_ARG;
  }
  fallback_plan_kernel<<<1, 256, 0, s>>>(cand_redo, n, budget, rows, counts);
  FLM_LAUNCH_CHECK("fallback_plan_kernel");
  return FLM_OK;
}

}  // namespace flm
