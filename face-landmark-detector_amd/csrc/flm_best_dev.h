// The quality arithmetic flm_track_best_update and flm_track_views_update share (include/flm.h, "the best shot of a
// track", states every operation), stated once as __host__ __device__ code: s, e and wbar of one face and their product
// (s * e) * wbar.  float64, one IEEE operation per written operator, in the written order; the file must be compiled
// without contraction.  The best shot multiplies the product by the caller's factor; the pose views take it as it is.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "flm.h"

namespace flm {

struct BestTerms {
  double sew;     // (s * e) * wbar
  double e;       // the share of pixels that are neither dark nor bright
  int64_t n_lap;  // the record's number of interior pixels
};

// r: the face's record; lm, wt: the face's first landmark and first weight (wt may be null: wbar = 1).
__host__ __device__ __forceinline__ BestTerms best_terms(const int64_t* r, const double* lm, size_t lm_stride,
                                                         const double* wt, size_t w_stride, int c, double sharp_ref) {
  const int64_t n_pix = r[0], n_lap = r[3], s_l = r[4], s_ll = r[5], n_dark = r[6], n_bright = r[7];
  const double nl = (double)n_lap;
  const double mu = (double)s_l / nl;
  const double m2 = (double)s_ll / nl;
  const double mm = mu * mu;
  const double var = m2 - mm;
  const double sharp = fmax(var / 256.0, 0.0);
  const double sh = fmin(sharp / sharp_ref, 1.0);
  const double e = (double)(n_pix - n_dark - n_bright) / (double)n_pix;
  double wbar = 1.0;
  if (wt) {
    double sum = 0.0;
    int n = 0;
    for (int i = 0; i < c; ++i) {
      const double x = lm[(size_t)i * lm_stride], y = lm[(size_t)i * lm_stride + 1];
      if (x == -1.0 && y == -1.0) continue;
      sum = sum + wt[(size_t)i * w_stride];
      ++n;
    }
    wbar = n ? sum / (double)n : 0.0;
  }
  const double se = sh * e;
  BestTerms t;
  t.sew = se * wbar;
  t.e = e;
  t.n_lap = n_lap;
  return t;
}

}  // namespace flm
