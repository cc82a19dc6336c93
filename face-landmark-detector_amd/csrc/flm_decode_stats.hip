// The heatmap decode as landmark records (flm_decode_stats, FLM_OUT_LANDMARKS_STATS): x, y, score, var_x, var_y, cov_xy
// per landmark; include/flm.h states the arithmetic operation by operation.  These are the launches that differ from
// flm_decode's (flm_decode.hip plans them, decode_run):
//   top-n      pass 1 is flm_decode's own launch; the merge below finishes the face's list with finish_topn_stats
//              (flm_topn_dev.h) -- the selected pixels already sit in the wave's list registers, so the record costs a
//              second walk over at most 128 keys and nothing in the HBM-bound pass.
//   all-pixel  the lane sums of flm_decode's kernels (same three chains, so x and y keep its bits) with the raw second
//              moments beside them: six partial sums per (chunk, landmark) instead of three, twice the float64 fmas on
//              a stream that stays HBM-bound.
#include "flm_decode_dev.h"

namespace flm {

template <bool WIDE>
__global__ __launch_bounds__(64) void decode_merge_stats_kernel(DecodeArgs a) {
  if (decode_row_off(a, blockIdx.y)) return;
  const int lane = threadIdx.x;
  const int c = blockIdx.x, face = blockIdx.y;
  const int oface = decode_out_face(a, face);
  if (oface < 0) return;
  unsigned long long list = 0ull, list_hi = 0ull, tau = 0ull;
  merge_chunk_lists<WIDE>(a, face, c, lane, list, list_hi, tau);
  finish_topn_stats(list, a.n_max, a.w, a.thresh, lane, a.out + ((size_t)oface * a.l + c) * FLM_LANDMARK_REC, list_hi);
}

int launch_decode_merge_stats(hipStream_t s, dim3 mgrid, const DecodeArgs& a, bool wide) {
  if (wide) decode_merge_stats_kernel<true><<<mgrid, 64, 0, s>>>(a);
  else decode_merge_stats_kernel<false><<<mgrid, 64, 0, s>>>(a);
  FLM_LAUNCH_CHECK("decode_merge_stats_kernel");
  return FLM_OK;
}

// ---- all-pixel mode ----------------------------------------------------------------------------------------------------
constexpr int NS = FLM_LANDMARK_REC;  // sums per (chunk, landmark): S0, Sx, Sy, Sxx, Syy, Sxy

__device__ __forceinline__ void lane_moments_add(double hv, double dx, double dy, double& sxx, double& syy, double& sxy) {
  sxx = fma(hv, dx * dx, sxx);
  syy = fma(hv, dy * dy, syy);
  sxy = fma(hv, dx * dy, sxy);
}

// decode_partial_all_kernel (flm_decode.hip) with six lane sums per channel
template <int CPW>
__global__ __launch_bounds__(256) void decode_partial_all_stats_kernel(DecodeArgs a) {
  if (a.gate && *a.gate == 0) return;
  extern __shared__ __attribute__((aligned(16))) float tile[];  // [PT][LS]
  const int L = a.l, LS = L | 1;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const Chunk k = chunk_of(a);
  const int c_first = wave * CPW;
  double s0[CPW], sx[CPW], sy[CPW], sxx[CPW], syy[CPW], sxy[CPW];
#pragma unroll
  for (int i = 0; i < CPW; ++i) { s0[i] = 0.0; sx[i] = 0.0; sy[i] = 0.0; sxx[i] = 0.0; syy[i] = 0.0; sxy[i] = 0.0; }

  TileStream ts(tile, a.hm + (size_t)k.face * (a.h * a.w) * L, L, k.p_begin, k.p_end, a.vec, tid);
  for (int p0 = k.p_begin; p0 < k.p_end; p0 += PT) {
    const int npx = ts.stage(p0);
    const int pix = p0 + lane;
    const bool pvalid = lane < npx;
    const double dx = (double)(pix % a.w), dy = (double)(pix / a.w);
#pragma unroll
    for (int i = 0; i < CPW; ++i) {
      const int c = c_first + i;
      if (c < L) {
        const double hv = pvalid ? (double)tile[lane * LS + c] : 0.0;
        lane_sums_add(hv, dx, dy, s0[i], sx[i], sy[i]);
        lane_moments_add(hv, dx, dy, sxx[i], syy[i], sxy[i]);
      }
    }
  }

  double* part = a.sums + ((size_t)k.face * a.chunks + k.chunk) * L * NS;
#pragma unroll
  for (int i = 0; i < CPW; ++i) {
    const int c = c_first + i;
    if (c < L) {
      lane_sums_write(part + c * NS, lane, s0[i], sx[i], sy[i]);
      lane_sums_write(part + c * NS + 3, lane, sxx[i], syy[i], sxy[i]);
    }
  }
}

// decode_partial_all_dma_kernel (flm_decode.hip) with six lane sums per channel
__global__ __launch_bounds__(256) void decode_partial_all_dma_stats_kernel(DecodeArgs a) {
  if (a.gate && *a.gate == 0) return;
  extern __shared__ __attribute__((aligned(16))) char ring[];  // [D_RING][PT][DL] floats
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const Chunk k = chunk_of(a);
  if (k.p_begin >= k.p_end) return;  // (uniform)
  double s0[D_CPW], sx[D_CPW], sy[D_CPW], sxx[D_CPW], syy[D_CPW], sxy[D_CPW];
#pragma unroll
  for (int i = 0; i < D_CPW; ++i) { s0[i] = 0.0; sx[i] = 0.0; sy[i] = 0.0; sxx[i] = 0.0; syy[i] = 0.0; sxy[i] = 0.0; }

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
    for (int i = 0; i < D_CPW; ++i) {
      const double hv = pvalid ? (double)v[i] : 0.0;
      lane_sums_add(hv, dx, dy, s0[i], sx[i], sy[i]);
      lane_moments_add(hv, dx, dy, sxx[i], syy[i], sxy[i]);
    }
  }

  double* part = a.sums + ((size_t)k.face * a.chunks + k.chunk) * DL * NS;
#pragma unroll
  for (int i = 0; i < D_CPW; ++i) {
    double* dst = part + dma_channel(i, wave) * NS;
    lane_sums_write(dst, lane, s0[i], sx[i], sy[i]);
    lane_sums_write(dst + 3, lane, sxx[i], syy[i], sxy[i]);
  }
}

// The chunk sums of (face, c) added in chunk order and finished as a record: the first three are all_pixel_finish's
// chain (flm_decode.hip), so x and y keep flm_decode's bits; a variance that cancels below zero is written as 0.
__global__ __launch_bounds__(64) void decode_merge_all_stats_kernel(DecodeArgs a) {
  if (a.gate && *a.gate == 0) return;
  if (threadIdx.x != 0) return;
  const int c = blockIdx.x, face = blockIdx.y;
  const int L = a.l;
  const double* part = a.sums + (size_t)face * a.chunks * L * NS;
  double v[NS];
#pragma unroll
  for (int j = 0; j < NS; ++j) v[j] = 0.0;
  for (int s = 0; s < a.chunks; ++s) {
#pragma unroll
    for (int j = 0; j < NS; ++j) v[j] += part[((size_t)s * L + c) * NS + j];
  }
  const float hsum = (float)v[0];
  double x = v[1] / (double)hsum, y = v[2] / (double)hsum;
  const float mean = hsum / (float)(a.h * a.w);
  double var_x = -1.0, var_y = -1.0, cov_xy = 0.0;
  if (mean <= a.thresh) {
    x = -1.0; y = -1.0;
  } else {
    var_x = v[3] / (double)hsum - x * x;
    var_y = v[4] / (double)hsum - y * y;
    cov_xy = v[5] / (double)hsum - x * y;
    if (var_x < 0.0) var_x = 0.0;
    if (var_y < 0.0) var_y = 0.0;
  }
  double* rec = a.out + ((size_t)face * L + c) * NS;
  rec[0] = x;
  rec[1] = y;
  rec[2] = (double)mean;
  rec[3] = var_x;
  rec[4] = var_y;
  rec[5] = cov_xy;
}

int launch_decode_all_stats(hipStream_t s, dim3 grid, dim3 mgrid, const DecodeArgs& a, bool dma, bool big, size_t tile_lds,
                            size_t ring_lds) {
  if (dma) {
    static FuncAttrOnce attr;
    FLM_FUNC_ATTR_ONCE(attr, (&decode_partial_all_dma_stats_kernel), ring_lds);
    decode_partial_all_dma_stats_kernel<<<grid, 256, ring_lds, s>>>(a);
  } else if (big) {
    decode_partial_all_stats_kernel<24><<<grid, 256, tile_lds, s>>>(a);
  } else {
    decode_partial_all_stats_kernel<17><<<grid, 256, tile_lds, s>>>(a);
  }
  FLM_LAUNCH_CHECK("decode_partial_all_stats_kernel");
  decode_merge_all_stats_kernel<<<mgrid, 64, 0, s>>>(a);
  FLM_LAUNCH_CHECK("decode_merge_all_stats_kernel");
  return FLM_OK;
}

}  // namespace flm
