// Descending (value, index) key lists spread over the lanes of a wave: the selection primitive shared by the heatmap
// decode (flm_decode.hip) and the candidate path of the landmark mode (flm_cand.hip).  A key is
// order_bits(value) << 32 | index, 0 = empty slot; lane i of a list register holds the i-th best key.
#pragma once
#include "flm_common.h"

namespace flm {

__device__ __forceinline__ unsigned order_bits(float v) {
  const unsigned u = __float_as_uint(v);
  return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ __forceinline__ float from_order_bits(unsigned o) {
  const unsigned u = (o & 0x80000000u) ? (o ^ 0x80000000u) : ~o;
  return __uint_as_float(u);
}
__device__ __forceinline__ unsigned long long readlane64(unsigned long long v, int srclane) {
  const unsigned lo = __builtin_amdgcn_readlane((unsigned)v, srclane);
  const unsigned hi = __builtin_amdgcn_readlane((unsigned)(v >> 32), srclane);
  return ((unsigned long long)hi << 32) | lo;
}
// lane i <- lane i-1 across the whole wave, lane 0 <- 0: the gfx9 DPP wave shift (wave_shr:1, one VALU move per half)
// instead of __shfl_up's ds_bpermute round trip -- this sits on the serial chain of every list insertion.
__device__ __forceinline__ unsigned long long shfl_up64(unsigned long long v, int lane) {
  const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)v, 0x138, 0xf, 0xf, false);
  const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)(v >> 32), 0x138, 0xf, 0xf, false);
  (void)lane;
  return ((unsigned long long)hi << 32) | lo;
}

// Insert every key of `cand` (one per lane, 0 = none) that beats the list's n-th entry.
// list: descending across lanes 0..n-1 (0 = empty slot); tau = list[n-1].
__device__ __forceinline__ void insert_candidates(unsigned long long& list, unsigned long long& tau,
                                                  unsigned long long cand, int n, int lane) {
  unsigned long long mask = __ballot(cand > tau);
  while (mask) {
    const int src = __builtin_ctzll(mask);
    const unsigned long long k = readlane64(cand, src);
    if (lane == src) cand = 0;
    const int pos = __builtin_popcountll(__ballot(list > k));  // entries that stay ahead of k
    const unsigned long long up = shfl_up64(list, lane);
    list = (lane < pos) ? list : (lane == pos ? k : up);
    if (lane >= n) list = 0;
    tau = readlane64(list, n - 1);
    mask = __ballot(cand > tau);
  }
}

// The same for 64 < n <= 128 (the reference's own sweep decodes n = k*k up to 81, utils/metrics.py:130-133): the list
// takes two registers per lane, ranks 0..63 in `l0` and 64..127 in `l1`; an insertion shifts both, the last entry of
// `l0` carrying into lane 0 of `l1`.  tau = entry n-1 (in `l1`).
__device__ __forceinline__ void insert_candidates_wide(unsigned long long& l0, unsigned long long& l1,
                                                       unsigned long long& tau, unsigned long long cand, int n, int lane) {
  unsigned long long mask = __ballot(cand > tau);
  while (mask) {
    const int src = __builtin_ctzll(mask);
    const unsigned long long k = readlane64(cand, src);
    if (lane == src) cand = 0;
    const int pos = __builtin_popcountll(__ballot(l0 > k)) + __builtin_popcountll(__ballot(l1 > k));
    const unsigned long long carry = readlane64(l0, 63);
    const unsigned long long up0 = shfl_up64(l0, lane), up1 = shfl_up64(l1, lane);
    if (pos < 64) {  // wave-uniform
      l0 = (lane < pos) ? l0 : (lane == pos ? k : up0);
      l1 = lane == 0 ? carry : up1;
    } else {
      const int q = pos - 64;
      l1 = (lane < q) ? l1 : (lane == q ? k : up1);
    }
    if (lane + 64 >= n) l1 = 0;
    tau = readlane64(l1, n - 65);
    mask = __ballot(cand > tau);
  }
}

// utils/metrics.py:69-77 on a finished list: float32 sum in ascending value order (= list lanes n-1 .. 0),
// float64 index-weighted sums, reject when hsum / n_points <= thresh.
__device__ __forceinline__ void finish_topn(unsigned long long list, int n_points, int w, float thresh, int lane,
                                            double* out, unsigned long long list_hi = 0ull) {
  float hsum = 0.f;
  double i0 = 0.0, i1 = 0.0;
  for (int i = n_points - 1; i >= 0; --i) {
    const unsigned long long k = i >= 64 ? readlane64(list_hi, i - 64) : readlane64(list, i);
    if (k == 0ull) continue;
    const float hv = from_order_bits((unsigned)(k >> 32));
    const unsigned idx = (unsigned)k;
    hsum += hv;
    i0 += (double)(idx / (unsigned)w) * (double)hv;
    i1 += (double)(idx % (unsigned)w) * (double)hv;
  }
  double x = i1 / (double)hsum, y = i0 / (double)hsum;
  if (hsum / (float)n_points <= thresh) { x = -1.0; y = -1.0; }
  if (lane == 0) {
    out[0] = x;
    out[1] = y;
  }
}

// The same finish as a landmark record (include/flm.h, FLM_LANDMARK_REC): x, y and the reject test are finish_topn's own
// chain; score is the float32 quotient that test compares; the moments come from a second walk over the keys in the same
// order, centred on (x, y), so every term of var_x / var_y is non-negative and nothing cancels.
__device__ __forceinline__ void finish_topn_stats(unsigned long long list, int n_points, int w, float thresh, int lane,
                                                  double* rec, unsigned long long list_hi = 0ull) {
  float hsum = 0.f;
  double i0 = 0.0, i1 = 0.0;
  for (int i = n_points - 1; i >= 0; --i) {
    const unsigned long long k = i >= 64 ? readlane64(list_hi, i - 64) : readlane64(list, i);
    if (k == 0ull) continue;
    const float hv = from_order_bits((unsigned)(k >> 32));
    const unsigned idx = (unsigned)k;
    hsum += hv;
    i0 += (double)(idx / (unsigned)w) * (double)hv;
    i1 += (double)(idx % (unsigned)w) * (double)hv;
  }
  double x = i1 / (double)hsum, y = i0 / (double)hsum;
  const float mean = hsum / (float)n_points;
  double var_x = -1.0, var_y = -1.0, cov_xy = 0.0;
  if (mean <= thresh) {
    x = -1.0; y = -1.0;
  } else {
    double vxx = 0.0, vyy = 0.0, vxy = 0.0;
    for (int i = n_points - 1; i >= 0; --i) {
      const unsigned long long k = i >= 64 ? readlane64(list_hi, i - 64) : readlane64(list, i);
      if (k == 0ull) continue;
      const float hv = from_order_bits((unsigned)(k >> 32));
      const unsigned idx = (unsigned)k;
      const double dx = (double)(idx % (unsigned)w) - x, dy = (double)(idx / (unsigned)w) - y;
      vxx += (double)hv * (dx * dx);
      vyy += (double)hv * (dy * dy);
      vxy += (double)hv * (dx * dy);
    }
    var_x = vxx / (double)hsum;
    var_y = vyy / (double)hsum;
    cov_xy = vxy / (double)hsum;
  }
  if (lane == 0) {
    rec[0] = x;
    rec[1] = y;
    rec[2] = (double)mean;
    rec[3] = var_x;
    rec[4] = var_y;
    rec[5] = cov_xy;
  }
}

}  // namespace flm
