// Heatmap -> landmark coordinates ("soft-argmax"), HBM-bound single pass over the heatmaps.
//
// Restates get_average_xy / transfer_xy_coord / transfer_target (reference utils/metrics.py:46-109):
//   n_points < 1 : full-map weighted centroid                                  (:58-64)
//   n_points >= 1: weighted centroid of the n largest pixels                   (:66-77)
//   reject -> (-1,-1) when  hsum / n_points <= thresh                          (:78-79)
// Numeric types follow the reference's numpy behaviour: in the top-n branch `hsum` is a sequential
// float32 sum in ascending value order and the index-weighted sums are float64; the coordinates are
// float64.  Ties at the n-th place: pixels are ordered by (value, flat index), the n largest kept.
//
// Pass 1 (decode_partial*): grid = (chunks, faces).  A workgroup streams its pixel range in tiles of
// 64 pixels x L channels: coalesced 16-byte loads -> LDS (row stride odd, so a wave reading one
// channel of 64 pixels is bank-conflict-free) -> each wave owns L/4 channels with lane = pixel.
// The stream is stated once (TileStream, and DmaRing for 68-landmark maps) and feeds two kernel families:
//   top-n (flm_decode top-n and flm_decode_sweep, which is the same launch with several modes):
//         per channel a descending list of the n best (value,index) keys spread over the wave's
//         lanes (lane i = i-th best; flm_topn_dev.h); a 64-pixel batch is tested against the list's n-th key with
//         one compare + ballot, insertions (rare after warm-up) are a ballot/popcount + one lane shift.
//   all-pixel (flm_decode mode 0, *_all_kernel): per-lane float64 partial sums in registers, one wave
//         reduction at the end.
// Pass 2 (decode_merge*): one wave per (face, landmark) merges the chunk partials and finishes the
// arithmetic in the reference's order.
#include "flm_decode_dev.h"

#include <algorithm>
#include <type_traits>

namespace flm {

// ---- top-n selection ---------------------------------------------------------------------------------------------------
// Offer pixel `pix` (one per lane; !pvalid: none) with value hv to a channel's list of the n best; true when the list
// changed.  WIDE: 64 < n <= 128, ranks 64..127 in list_hi.
template <bool WIDE>
__device__ __forceinline__ bool topn_offer(float hv, int pix, bool pvalid, int n, int lane, unsigned long long& list,
                                           unsigned long long& list_hi, unsigned long long& tau) {
  const unsigned long long key = pvalid ? (((unsigned long long)order_bits(hv) << 32) | (unsigned)pix) : 0ull;
  if (!__any(key > tau)) return false;
  if constexpr (WIDE) insert_candidates_wide(list, list_hi, tau, key, n, lane);
  else insert_candidates(list, tau, key, n, lane);
  return true;
}

// a chunk's list of channel c -> keys[face][chunk][c][0..n)
template <bool WIDE>
__device__ __forceinline__ void store_list(unsigned long long* part, int c, int n, int lane, unsigned long long list,
                                           unsigned long long list_hi) {
  if (lane < n) part[(size_t)c * n + lane] = list;
  if (WIDE && lane + 64 < n) part[(size_t)c * n + 64 + lane] = list_hi;
}

// ---- all-pixel centroid ------------------------------------------------------------------------------------------------
// the chunk sums of (face, c) added in chunk order and finished as utils/metrics.py:58-64,78-79 do: hsum is float32
// (np.sum of a float32 map), n_points = H*W
__device__ __forceinline__ void all_pixel_finish(const DecodeArgs& a, int face, int c, double& x, double& y) {
  const int L = a.l;
  const double* part = a.sums + (size_t)face * a.chunks * L * 3;
  double v0 = 0.0, v1 = 0.0, v2 = 0.0;
  for (int s = 0; s < a.chunks; ++s) {
    v0 += part[((size_t)s * L + c) * 3 + 0];
    v1 += part[((size_t)s * L + c) * 3 + 1];
    v2 += part[((size_t)s * L + c) * 3 + 2];
  }
  const float hsum = (float)v0;
  x = v1 / (double)hsum;
  y = v2 / (double)hsum;
  if (hsum / (float)(a.h * a.w) <= a.thresh) { x = -1.0; y = -1.0; }
}

// The sweep's all-pixel sums ride beside the key lists: thread t of a workgroup owns channel t % L and every G-th pixel
// of a tile (G = 256 / L groups), three float64 accumulators per thread instead of three per channel and lane, so that
// the sums fit beside the lists without spilling.  The groups are reduced through LDS in a fixed order at the end of the
// chunk; the order of the float64 additions differs from the lane sums' above, hence flm_decode_sweep's mode 0 agrees
// with flm_decode(0) within 1e-9 px rather than bit for bit -- and flm_decode(0) keeps its own kernels.
// This thread's share of a tile: pixels g, g + G, ... of the tile (row stride `rs` floats), channel c
__device__ __forceinline__ void group_sums_tile(const float* tile, int rs, int c, int g, int G, int p0, int npx, int w,
                                                double& s0, double& sx, double& sy) {
  if (g >= G) return;
  int pix = p0 + g;
  int y = pix / w, x = pix - y * w;
  for (int p = g; p < npx; p += G) {
    const double hv = (double)tile[p * rs + c];
    s0 += hv;
    sx = fma(hv, (double)x, sx);
    sy = fma(hv, (double)y, sy);
    x += G;
    while (x >= w) { x -= w; ++y; }
  }
}

// end of chunk: the G groups' sums of every channel, added in group order, to sums[face][chunk][c][0..2].
// `red` is LDS of at least 256 x 3 doubles that no wave reads any more.
__device__ __forceinline__ void group_sums_flush(const DecodeArgs& a, double* red, int tid, int g, int G, double s0,
                                                 double sx, double sy) {
  __syncthreads();
  if (g < G) {
    red[tid * 3 + 0] = s0;
    red[tid * 3 + 1] = sx;
    red[tid * 3 + 2] = sy;
  }
  __syncthreads();
  if (tid < a.l) {
    double v0 = 0.0, v1 = 0.0, v2 = 0.0;
    for (int k = 0; k < G; ++k) {
      const int t = k * a.l + tid;
      v0 += red[t * 3 + 0];
      v1 += red[t * 3 + 1];
      v2 += red[t * 3 + 2];
    }
    double* dst = a.sums + (((size_t)blockIdx.y * a.chunks + blockIdx.x) * a.l + tid) * 3;
    dst[0] = v0;
    dst[1] = v1;
    dst[2] = v2;
  }
}

// ---- pass 1, top-n family (flm_decode top-n, flm_decode_sweep) -----------------------------------------------------------
// Register-prefetch form.  Per chunk the descending (value, index) list of the n_max best keys of every channel (CPW
// channels per wave; WIDE: two list registers) and, when ALL, the group sums.  Dynamic LDS: the tile, and at least
// 256 x 3 doubles when ALL.
template <int CPW, bool WIDE, bool ALL>
__global__ __launch_bounds__(256) void decode_partial_kernel(DecodeArgs a) {
  if (decode_row_off(a, blockIdx.y)) return;
  extern __shared__ __attribute__((aligned(16))) float tile[];  // [PT][LS]
  const int L = a.l, LS = L | 1;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const Chunk k = chunk_of(a);
  const int c_first = wave * CPW;
  const int n_max = a.n_max;
  const int G = 256 / L, ag = tid / L, ac = tid - ag * L;  // group sums: group, channel

  double s0 = 0.0, sx = 0.0, sy = 0.0;
  unsigned long long list[CPW], tau[CPW];
  unsigned long long list_hi[WIDE ? CPW : 1];  // ranks 64..127
#pragma unroll
  for (int i = 0; i < CPW; ++i) {
    list[i] = 0ull; tau[i] = 0ull;
    if (WIDE) list_hi[i] = 0ull;
  }

  TileStream ts(tile, a.hm + (size_t)k.face * (a.h * a.w) * L, L, k.p_begin, k.p_end, a.vec, tid);
  for (int p0 = k.p_begin; p0 < k.p_end; p0 += PT) {
    const int npx = ts.stage(p0);
    if (ALL) group_sums_tile(tile, LS, ac, ag, G, p0, npx, a.w, s0, sx, sy);
    if (n_max > 0) {  // (uniform)
      const int pix = p0 + lane;
      const bool pvalid = lane < npx;
#pragma unroll
      for (int i = 0; i < CPW; ++i) {
        const int c = c_first + i;
        if (c < L)  // wave-uniform
          topn_offer<WIDE>(tile[lane * LS + c], pix, pvalid, n_max, lane, list[i], list_hi[WIDE ? i : 0], tau[i]);
      }
    }
  }

  if (n_max > 0) {
    unsigned long long* part = a.keys + ((size_t)k.face * a.chunks + k.chunk) * L * n_max;
#pragma unroll
    for (int i = 0; i < CPW; ++i) {
      const int c = c_first + i;
      if (c < L) store_list<WIDE>(part, c, n_max, lane, list[i], list_hi[WIDE ? i : 0]);
    }
  }
  if (ALL) group_sums_flush(a, reinterpret_cast<double*>(tile), tid, ag, G, s0, sx, sy);
}

// LDS-DMA form (68 landmarks, 16-byte-aligned faces, n_max <= 64); the group sums read the same ring slot, row stride 68.
template <bool ALL>
__global__ __launch_bounds__(256) void decode_partial_dma_kernel(DecodeArgs a) {
  if (decode_row_off(a, blockIdx.y)) return;
  extern __shared__ __attribute__((aligned(16))) char ring[];  // [D_RING][PT][DL] floats
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const Chunk k = chunk_of(a);
  if (k.p_begin >= k.p_end) return;  // (uniform)
  const int n_max = a.n_max;
  constexpr int G = 256 / DL;
  const int ag = tid / DL, ac = tid - ag * DL;

  double s0 = 0.0, sx = 0.0, sy = 0.0;
  unsigned long long list[D_CPW], tau[D_CPW], none = 0ull;
  float tauf[D_CPW];  // the value of the list's n-th key (NaN while the list is not full)
#pragma unroll
  for (int i = 0; i < D_CPW; ++i) {
    list[i] = 0ull; tau[i] = 0ull;
    tauf[i] = from_order_bits(0u);
  }

  const DmaRing dr(ring, a.hm + (size_t)k.face * (a.h * a.w) * DL, k.p_begin, k.p_end, lane, wave);
  for (int t = 0; t < dr.ntiles; ++t) {
    const char* slot = dr.stage(t);
    const int p0 = k.p_begin + t * PT;
    if (ALL) group_sums_tile(reinterpret_cast<const float*>(slot), DL, ac, ag, G, p0, min(PT, k.p_end - p0), a.w, s0, sx, sy);
    if (n_max > 0) {  // (uniform)
      float v[D_CPW];
      dma_read_pixel(slot, lane, wave, v);
      const int pix = p0 + lane;
      const bool pvalid = pix < k.p_end;
      // The per-value test is ONE float compare against the list's n-th VALUE (a scalar): "not less than" lets every true
      // candidate through -- an equal value may still win on the pixel index, a NaN orders above everything as its order
      // bits do, and while the list is not full its n-th value reads as NaN, which nothing is less than -- and the 64-bit
      // key is only built for a class that has a candidate.  The sweep over n said that this test, not the insertions,
      // is what separates top-4 from the all-pixel mode's streaming rate (0.283 -> 0.26 ms at batch 64).
#pragma unroll
      for (int i = 0; i < D_CPW; ++i) {
        if (__any(!(v[i] < tauf[i])) && topn_offer<false>(v[i], pix, pvalid, n_max, lane, list[i], none, tau[i]))
          tauf[i] = from_order_bits((unsigned)(tau[i] >> 32));
      }
    }
  }

  if (n_max > 0) {
    unsigned long long* part = a.keys + ((size_t)k.face * a.chunks + k.chunk) * DL * n_max;
#pragma unroll
    for (int i = 0; i < D_CPW; ++i) store_list<false>(part, dma_channel(i, wave), n_max, lane, list[i], none);
  }
  if (ALL) group_sums_flush(a, reinterpret_cast<double*>(ring), tid, ag, G, s0, sx, sy);
}

// ---- pass 2, top-n family: one wave per (face, landmark) merges the chunk lists to the face's top n_max once, then ----
// finishes every mode from it.  Two thin kernels over the same functions: flm_decode has one mode and no all-pixel sums,
// and the mode loop costs its merge 4 %, so it keeps the loop-free form.
template <bool WIDE>
__global__ __launch_bounds__(64) void decode_merge_kernel(DecodeArgs a) {
  if (decode_row_off(a, blockIdx.y)) return;
  const int lane = threadIdx.x;
  const int c = blockIdx.x, face = blockIdx.y;
  const int oface = decode_out_face(a, face);
  if (oface < 0) return;
  unsigned long long list = 0ull, list_hi = 0ull, tau = 0ull;
  merge_chunk_lists<WIDE>(a, face, c, lane, list, list_hi, tau);
  finish_topn(list, a.n_max, a.w, a.thresh, lane, a.out + ((size_t)oface * a.l + c) * 2, list_hi);
}

template <bool WIDE>
__global__ __launch_bounds__(64) void decode_merge_modes_kernel(DecodeArgs a) {
  const int lane = threadIdx.x;
  const int c = blockIdx.x, face = blockIdx.y;
  unsigned long long list = 0ull, list_hi = 0ull, tau = 0ull;
  if (a.n_max > 0) merge_chunk_lists<WIDE>(a, face, c, lane, list, list_hi, tau);
  double ax = 0.0, ay = 0.0;
  if (a.has_all) all_pixel_finish(a, face, c, ax, ay);
  for (int m = 0; m < a.n_modes; ++m) {
    const int np = a.modes[m];
    double* out = a.out + (((size_t)m * a.n + face) * a.l + c) * 2;
    if (np == 0) {
      if (lane == 0) {
        out[0] = ax;
        out[1] = ay;
      }
    } else {
      finish_topn(list, np, a.w, a.thresh, lane, out, list_hi);
    }
  }
}

// ---- flm_decode's all-pixel mode: lane sums over the same two tile streams ------------------------------------------------
template <int CPW>
__global__ __launch_bounds__(256) void decode_partial_all_kernel(DecodeArgs a) {
  if (a.gate && *a.gate == 0) return;
  extern __shared__ __attribute__((aligned(16))) float tile[];  // [PT][LS]
  const int L = a.l, LS = L | 1;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const Chunk k = chunk_of(a);
  const int c_first = wave * CPW;
  double s0[CPW], sx[CPW], sy[CPW];
#pragma unroll
  for (int i = 0; i < CPW; ++i) { s0[i] = 0.0; sx[i] = 0.0; sy[i] = 0.0; }

  TileStream ts(tile, a.hm + (size_t)k.face * (a.h * a.w) * L, L, k.p_begin, k.p_end, a.vec, tid);
  for (int p0 = k.p_begin; p0 < k.p_end; p0 += PT) {
    const int npx = ts.stage(p0);
    const int pix = p0 + lane;
    const bool pvalid = lane < npx;
    const double dx = (double)(pix % a.w), dy = (double)(pix / a.w);
#pragma unroll
    for (int i = 0; i < CPW; ++i) {
      const int c = c_first + i;
      if (c < L) lane_sums_add(pvalid ? (double)tile[lane * LS + c] : 0.0, dx, dy, s0[i], sx[i], sy[i]);
    }
  }

  double* part = a.sums + ((size_t)k.face * a.chunks + k.chunk) * L * 3;
#pragma unroll
  for (int i = 0; i < CPW; ++i) {
    const int c = c_first + i;
    if (c < L) lane_sums_write(part + c * 3, lane, s0[i], sx[i], sy[i]);
  }
}

__global__ __launch_bounds__(256) void decode_partial_all_dma_kernel(DecodeArgs a) {
  if (a.gate && *a.gate == 0) return;
  extern __shared__ __attribute__((aligned(16))) char ring[];  // [D_RING][PT][DL] floats
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const Chunk k = chunk_of(a);
  if (k.p_begin >= k.p_end) return;  // (uniform)
  double s0[D_CPW], sx[D_CPW], sy[D_CPW];
#pragma unroll
  for (int i = 0; i < D_CPW; ++i) { s0[i] = 0.0; sx[i] = 0.0; sy[i] = 0.0; }

  const DmaRing dr(ring, a.hm + (size_t)k.face * (a.h * a.w) * DL, k.p_begin, k.p_end, lane, wave);
  for (int t = 0; t < dr.ntiles; ++t) {
    const char* slot = dr.stage(t);
    const int p0 = k.p_begin + t * PT;
    float v[D_CPW];
    dma_read_pixel(slot, lane, wave, v);
    const int pix = p0 + lane;
    const bool pvalid = pix < k.p_end;
    const double dx = (double)(pix % a.w), dy = (double)(pix / a.w);
#pragma unroll
    for (int i = 0; i < D_CPW; ++i) lane_sums_add(pvalid ? (double)v[i] : 0.0, dx, dy, s0[i], sx[i], sy[i]);
  }

  double* part = a.sums + ((size_t)k.face * a.chunks + k.chunk) * DL * 3;
#pragma unroll
  for (int i = 0; i < D_CPW; ++i) lane_sums_write(part + dma_channel(i, wave) * 3, lane, s0[i], sx[i], sy[i]);
}

__global__ __launch_bounds__(64) void decode_merge_all_kernel(DecodeArgs a) {
  if (a.gate && *a.gate == 0) return;
  if (threadIdx.x != 0) return;
  const int c = blockIdx.x, face = blockIdx.y;
  double x, y;
  all_pixel_finish(a, face, c, x, y);
  double* out = a.out + ((size_t)face * a.l + c) * 2;
  out[0] = x;
  out[1] = y;
}


// Chunks per face.  The kernel holds 155 registers: three workgroups per CU, 768 on the chip at a time.  What counts is
// that the launch is whole rounds of those 768 -- 1024 or 1152 workgroups run a second, mostly empty round (batch 512:
// 4.4-4.7 TB/s instead of 5.6) -- and, among whole rounds, as few chunks per face as possible: every chunk starts with
// empty lists (~30 serial inserts per class until its threshold has risen) and adds n entries per class to the merge
// (batch 64: 12 chunks per face = one round, 3.8 TB/s; 24 = two rounds, 3.3; 48: 2.9; tools/bench_hbm.py).
static void decode_plan(int n, int h, int w, int* chunks, int* chunk_px) {
  const int HW = h * w, faces = n > 0 ? n : 1;
  constexpr int kResident = 768, kMaxChunks = 32;
  int best_s = 1;
  double best_u = 0.0;
  for (int s = 1; s <= kMaxChunks; ++s) {
    const long long wgs = (long long)faces * s;
    const long long rounds = (wgs + kResident - 1) / kResident;
    const double u = (double)wgs / (double)(rounds * kResident);  // how full the rounds are
    if (u > best_u * 1.05) {  // (ties and near-ties go to the fewer chunks)
      best_u = u;
      best_s = s;
    }
  }
  const int s = best_s;
  int px = (HW + s - 1) / s;
  px = (px + PT - 1) / PT * PT;
  *chunk_px = px;
  *chunks = (HW + px - 1) / px;
}

// workspace: the key lists, then the all-pixel sums (`stats`: six per (chunk, landmark) instead of three)
static void decode_layout(int n, int h, int w, int l, int n_max, int has_all, size_t* keys_bytes, size_t* sums_bytes,
                          int stats = 0) {
  int chunks, chunk_px;
  decode_plan(n, h, w, &chunks, &chunk_px);
  *keys_bytes = align_up((size_t)n * chunks * l * n_max * sizeof(unsigned long long), 256);
  *sums_bytes = has_all ? align_up((size_t)n * chunks * l * (stats ? FLM_LANDMARK_REC : 3) * sizeof(double), 256) : 0;
}

size_t decode_ws_bytes(int n, int h, int w, int l, int mode, int n_points, int stats) {
  size_t kb, sb;
  if (mode == FLM_DECODE_ALL) decode_layout(n, h, w, l, 0, 1, &kb, &sb, stats);
  else decode_layout(n, h, w, l, n_points > 0 ? n_points : 1, 0, &kb, &sb);
  return kb + sb;
}

// `who`: "decode" or "decode_sweep", the prefix of the entry point's error texts
static int decode_check_shape(const char* who, int n, int h, int w, int l) {
  if (n <= 0 || h <= 0 || w <= 0 || l <= 0 || l > kMaxClasses) {
    set_error("%s: unsupported shape n=%d h=%d w=%d l=%d (max %d landmarks)", who, n, h, w, l, kMaxClasses);
    return FLM_ERR_SHAPE;
  }
  if ((long long)h * w >= (1ll << 31)) {
    set_error("%s: map too large", who);
    return FLM_ERR_SHAPE;
  }
  return FLM_OK;
}

static int sweep_check_modes(const int* modes, int n_modes, int* n_max, int* has_all) {
  if (!modes || n_modes < 1 || n_modes > FLM_SWEEP_MAX_MODES) {
    set_error("decode_sweep: 1 <= n_modes <= %d mode entries required (got %d%s)", FLM_SWEEP_MAX_MODES, n_modes,
              modes ? "" : ", null list");
    return FLM_ERR_ARG;
  }
  *n_max = 0;
  *has_all = 0;
  for (int i = 0; i < n_modes; ++i) {
    if (modes[i] < 0 || modes[i] > 128) {
      set_error("decode_sweep: mode %d is %d; each mode is 0 (all pixels) or 1 <= n_points <= 128", i, modes[i]);
      return FLM_ERR_UNSUPPORTED;
    }
    if (modes[i] == 0) *has_all = 1;
    *n_max = std::max(*n_max, modes[i]);
  }
  return FLM_OK;
}

// 68-landmark maps, 16-byte-aligned faces, one list register: the LDS-DMA form (a chunk stays below the 2 GiB buffer range)
// (knob "decode_lds_dma": same results either way)
static bool use_dma(int l, int vec, bool wide, int chunk_px) {
  return tuning(KNOB_DECODE_LDS_DMA) && l == DL && vec && !wide && (long long)chunk_px * DL * 4 < (1ll << 31);
}

constexpr size_t kRingLds = (size_t)D_RING * D_TILE_B;
static_assert(kRingLds >= 256 * 3 * sizeof(double), "the ring holds the group sums' reduction");

template <bool ALL>
static int launch_partial_dma(hipStream_t s, dim3 grid, const DecodeArgs& a) {
  static FuncAttrOnce attr;
  FLM_FUNC_ATTR_ONCE(attr, (&decode_partial_dma_kernel<ALL>), kRingLds);
  decode_partial_dma_kernel<ALL><<<grid, 256, kRingLds, s>>>(a);
  return FLM_OK;
}

// f(std::bool_constant<b>): a run-time flag as a template argument
template <class F>
static void with_bool(bool b, F f) {
  if (b) f(std::true_type{});
  else f(std::false_type{});
}

// The two passes over maps whose shape and modes have been checked: flm_decode's all-pixel mode (no mode list) on its own
// kernels, flm_decode's top-n mode (one mode) and the sweep on the top-n family.  `stats` (flm_decode_stats; not the
// sweep): `out` takes landmark records and the launches that differ are flm_decode_stats.hip's -- in top-n mode the
// merge alone, pass 1 being the same launch; in all-pixel mode both passes, with six sums per (chunk, landmark).
enum DecodeKind { kDecodeAll, kDecodeTopN, kDecodeSweep };
static int decode_run(const char* who, hipStream_t s, const float* hm, int n, int h, int w, int l, const int* modes,
                      int n_modes, int n_max, int has_all, DecodeKind kind, float thresh, double* out, void* ws,
                      size_t ws_bytes, const unsigned* gate, bool stats = false, const int* rows = nullptr,
                      const unsigned* rows_cnt = nullptr) {
  if (reinterpret_cast<uintptr_t>(hm) & 15) {
    set_error("%s: heatmap pointer must be 16-byte aligned", who);
    return FLM_ERR_ARG;
  }
  size_t kb, sb;
  decode_layout(n, h, w, l, n_max, has_all, &kb, &sb, stats);
  if (ws_bytes < kb + sb) {
    set_error("%s: workspace too small", who);
    return FLM_ERR_WORKSPACE;
  }
  DecodeArgs a;
  a.hm = hm; a.n = n; a.h = h; a.w = w; a.l = l;
  decode_plan(n, h, w, &a.chunks, &a.chunk_px);
  a.vec = (((long long)h * w * l) & 3) == 0;
  a.n_max = n_max; a.has_all = has_all; a.thresh = thresh;
  a.keys = static_cast<unsigned long long*>(ws);
  a.sums = reinterpret_cast<double*>(static_cast<char*>(ws) + kb);
  a.out = out;
  a.gate = gate;
  a.rows = rows; a.rows_cnt = rows_cnt;
  a.n_modes = n_modes;
  for (int i = 0; i < FLM_SWEEP_MAX_MODES; ++i) a.modes[i] = i < n_modes ? modes[i] : 0;

  const dim3 grid(a.chunks, n), mgrid(l, n);
  const bool wide = n_max > 64;  // two list registers per lane (the reference's sweep reaches n = 81)
  const bool big = l > 68;       // 24 channels per wave instead of 17
  const size_t tile_lds = sizeof(float) * PT * (l | 1);
  const bool dma = use_dma(l, a.vec, wide, a.chunk_px);
  if (kind == kDecodeAll && stats) return launch_decode_all_stats(s, grid, mgrid, a, dma, big, tile_lds, kRingLds);
  if (kind == kDecodeAll) {
    if (dma) {
      static FuncAttrOnce attr;
      FLM_FUNC_ATTR_ONCE(attr, (&decode_partial_all_dma_kernel), kRingLds);
      decode_partial_all_dma_kernel<<<grid, 256, kRingLds, s>>>(a);
    } else if (big) {
      decode_partial_all_kernel<24><<<grid, 256, tile_lds, s>>>(a);
    } else {
      decode_partial_all_kernel<17><<<grid, 256, tile_lds, s>>>(a);
    }
    FLM_LAUNCH_CHECK("decode_partial_all_kernel");
    decode_merge_all_kernel<<<mgrid, 64, 0, s>>>(a);
    FLM_LAUNCH_CHECK("decode_merge_all_kernel");
    return FLM_OK;
  }
  if (dma) {
    const int rc = has_all ? launch_partial_dma<true>(s, grid, a) : launch_partial_dma<false>(s, grid, a);
    if (rc != FLM_OK) return rc;
    FLM_LAUNCH_CHECK("decode_partial_dma_kernel");
  } else {
    const size_t lds = has_all ? std::max(tile_lds, 256 * 3 * sizeof(double)) : tile_lds;
    with_bool(big, [&](auto b) {
      with_bool(wide, [&](auto wd) {
        with_bool(has_all, [&](auto all) {
          decode_partial_kernel<decltype(b)::value ? 24 : 17, decltype(wd)::value, decltype(all)::value><<<grid, 256, lds, s>>>(a);
        });
      });
    });
    FLM_LAUNCH_CHECK("decode_partial_kernel");
  }
  if (stats) return launch_decode_merge_stats(s, mgrid, a, wide);
  with_bool(wide, [&](auto wd) {
    if (kind == kDecodeSweep) decode_merge_modes_kernel<decltype(wd)::value><<<mgrid, 64, 0, s>>>(a);
    else decode_merge_kernel<decltype(wd)::value><<<mgrid, 64, 0, s>>>(a);
  });
  FLM_LAUNCH_CHECK("decode_merge_kernel");
  return FLM_OK;
}

int launch_decode(hipStream_t s, const float* hm, int n, int h, int w, int l, int mode, int n_points, float thresh,
                  double* out, void* ws, size_t ws_bytes, const unsigned* gate, int stats, const int* rows,
                  const unsigned* rows_cnt) {
  const int rc = decode_check_shape("decode", n, h, w, l);
  if (rc != FLM_OK) return rc;
  if ((rows || rows_cnt) && (!rows || !rows_cnt || mode != FLM_DECODE_TOPN)) {
    set_error("decode: a row map needs the top-n mode, the map and its count");
    return FLM_ERR_UNSUPPORTED;
  }
  if (mode == FLM_DECODE_TOPN && (n_points < 1 || n_points > 128)) {
    set_error("decode: top-n mode supports 1 <= n_points <= 128 (got %d)", n_points);
    return FLM_ERR_UNSUPPORTED;
  }
  if (mode != FLM_DECODE_ALL && mode != FLM_DECODE_TOPN) {
    set_error("decode: unknown mode %d", mode);
    return FLM_ERR_ARG;
  }
  if (mode == FLM_DECODE_ALL)
    return decode_run("decode", s, hm, n, h, w, l, nullptr, 0, 0, 1, kDecodeAll, thresh, out, ws, ws_bytes, gate, stats != 0);
  return decode_run("decode", s, hm, n, h, w, l, &n_points, 1, n_points, 0, kDecodeTopN, thresh, out, ws, ws_bytes, gate,
                    stats != 0, rows, rows_cnt);
}

// ---- one-pass multi-n decode (flm_decode_sweep) ------------------------------------------------------------------------
// The reference's n_points experiment (utils/metrics.py:118-154) decodes the same maps at n = k*k, k = 1..9, and at the
// all-pixel centroid.  Here one read of the maps serves every mode: the partial pass keeps, per chunk, the descending
// (value, index) list of n_max = max(top-n modes) keys and, when some mode is 0, the float64 all-pixel sums; the merge
// builds the face's top n_max list once and finishes every mode from it.  Under the total (value, index) order the top n
// set is the first n keys of the top n_max list, so a top-n slice selects exactly what a decode at that n alone selects,
// ties included; each n then redoes its own float32 hsum chain in the reference's order (rank n-1 down to rank 0: a
// prefix sum of the n_max chain rounds differently), its own float64 index sums and its own reject test -- finish_topn.
size_t decode_sweep_ws_bytes(int n, int h, int w, int l, const int* modes, int n_modes) {
  int n_max, has_all;
  if (decode_check_shape("decode_sweep", n, h, w, l) != FLM_OK || sweep_check_modes(modes, n_modes, &n_max, &has_all) != FLM_OK)
    return 0;
  size_t kb, sb;
  decode_layout(n, h, w, l, n_max, has_all, &kb, &sb);
  return kb + sb;
}

int launch_decode_sweep(hipStream_t s, const float* hm, int n, int h, int w, int l, const int* modes, int n_modes,
                        float thresh, double* out, void* ws, size_t ws_bytes) {
  int n_max, has_all;
  int rc = decode_check_shape("decode_sweep", n, h, w, l);
  if (rc == FLM_OK) rc = sweep_check_modes(modes, n_modes, &n_max, &has_all);
  if (rc != FLM_OK) return rc;
  return decode_run("decode_sweep", s, hm, n, h, w, l, modes, n_modes, n_max, has_all, kDecodeSweep, thresh, out, ws, ws_bytes, nullptr);
}

// ---- Gaussian target maps (flm_gaussian_heatmaps) ----------------------------------------------------------------------
// generate_hm / gaussian_k (data/generator.py:274-296) on the device: float64 keypoints [N,L,2] (x,y) in grid pixels ->
// float32 [N,H,W,L], hm[r,c,i] = float32(exp(-((c - x0)**2 + (r - y0)**2) / (2 * sigma**2))) in float64, in that
// operation order (-ffp-contract=off: nothing fuses); a keypoint equal to (-1,-1) gives an all-zero map (:292).
// `two_sigma_sq` is the host's `2 * sigma**2`.  Far from the centre the value rounds to +0.0f: where
// d2 > 106 * two_sigma_sq the exponent -d2 / two_sigma_sq is below -105 even after the rounding of that product, so
// exp() < 2.6e-46 < 2^-150 (half the smallest float32 subnormal) and the float32 value is +0.0f -- the skipped exp()
// cannot change a bit.  NaN / infinite inputs fail the test and take the formula.  The kernel is bound by its writes:
// four consecutive floats of the channel-last output per thread, one 16-byte store.
__global__ __launch_bounds__(256) void gaussian_hm_kernel(const double* __restrict__ kp, int n, int l, int h, int w,
                                                          double two_sigma_sq, float* __restrict__ out, long long total) {
  const long long e0 = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (e0 >= total) return;
  const double cut = 106.0 * two_sigma_sq;
  const long long hw = (long long)h * w;
  const long long q = e0 / l;  // (face, pixel) of the first element; the next three follow by increments
  int c = (int)(e0 - q * l);
  long long face = q / hw;
  const int pix = (int)(q - face * hw);
  int row = pix / w, col = pix - row * w;
  float v[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float r = 0.f;
    if (e0 + j < total) {
      const double x0 = kp[(face * l + c) * 2 + 0], y0 = kp[(face * l + c) * 2 + 1];
      if (!(x0 == -1.0 && y0 == -1.0)) {
        const double dx = (double)col - x0, dy = (double)row - y0;
        const double d2 = dx * dx + dy * dy;
        if (!(d2 > cut)) r = (float)exp(-d2 / two_sigma_sq);
      }
    }
    v[j] = r;
    if (++c == l) {
      c = 0;
      if (++col == w) {
        col = 0;
        if (++row == h) { row = 0; ++face; }
      }
    }
  }
  if (e0 + 3 < total) {
    *reinterpret_cast<float4*>(out + e0) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
    for (int j = 0; j < 4 && e0 + j < total; ++j) out[e0 + j] = v[j];
  }
}

int launch_gaussian_heatmaps(hipStream_t s, const double* kp, int n, int l, int h, int w, double two_sigma_sq,
                             float* out) {
  if (n <= 0 || l <= 0 || h <= 0 || w <= 0 || (long long)h * w >= (1ll << 31)) {
    set_error("gaussian_heatmaps: unsupported shape n=%d l=%d h=%d w=%d", n, l, h, w);
    return FLM_ERR_SHAPE;
  }
  if (reinterpret_cast<uintptr_t>(out) & 15) {
    set_error("gaussian_heatmaps: output pointer must be 16-byte aligned");
    return FLM_ERR_ARG;
  }
  const long long total = (long long)n * h * w * l;
  const long long blocks = (total + 1023) / 1024;
  if (blocks >= (1ll << 31)) {
    set_error("gaussian_heatmaps: output too large");
    return FLM_ERR_SHAPE;
  }
  gaussian_hm_kernel<<<dim3((unsigned)blocks), 256, 0, s>>>(kp, n, l, h, w, two_sigma_sq, out, total);
  FLM_LAUNCH_CHECK("gaussian_hm_kernel");
  return FLM_OK;
}

}  // namespace flm
