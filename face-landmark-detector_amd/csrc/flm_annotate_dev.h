// Frame annotation (flm_frames_annotate): the integer pieces, stated once as __host__ __device__ code for the kernels of
// flm_annotate.hip, for flm_bgr_to_yuv (host only) and for the host sweep of tests/native/annotate_host.cpp, which runs
// these same functions.  include/flm.h ("frame annotation") states the contract; this header is its arithmetic.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "flm.h"

namespace flm {

// ---- accepted landmarks and the region of a face ----------------------------------------------------------------------
// x >= 0 && y >= 0 && x <= 2^30 && y <= 2^30: the rejected point (-1,-1), NaN and +-inf fail, -0.0 passes.
__host__ __device__ __forceinline__ bool annot_accepted(double x, double y) {
  const double lim = 1073741824.0;  // 2^30
  return x >= 0.0 && y >= 0.0 && x <= lim && y <= lim;
}

struct AnnotBox {
  int x0, y0, x1, y1;  // half open
};

// clamp to +-2^30, then the cast: box_coord of flm_track_step
__host__ __device__ __forceinline__ int annot_coord(double t) {
  const double lim = 1073741824.0;
  const double c = t < -lim ? -lim : (t > lim ? lim : t);
  return (int)c;
}

// The running min / max over the accepted points of a face.  Written as comparisons: the result is one of the inputs, and
// the int32 region below does not depend on which of -0.0 and 0.0 a tie keeps.
struct AnnotExtent {
  double mnx, mny, mxx, mxy;
  int any;
};
__host__ __device__ __forceinline__ AnnotExtent annot_extent_empty() {
  return AnnotExtent{HUGE_VAL, HUGE_VAL, -HUGE_VAL, -HUGE_VAL, 0};
}
__host__ __device__ __forceinline__ void annot_extent_add(AnnotExtent& e, double x, double y) {
  if (!annot_accepted(x, y)) return;
  e.mnx = x < e.mnx ? x : e.mnx;
  e.mny = y < e.mny ? y : e.mny;
  e.mxx = x > e.mxx ? x : e.mxx;
  e.mxy = y > e.mxy ? y : e.mxy;
  e.any = 1;
}
__host__ __device__ __forceinline__ void annot_extent_merge(AnnotExtent& e, const AnnotExtent& o) {
  e.mnx = o.mnx < e.mnx ? o.mnx : e.mnx;
  e.mny = o.mny < e.mny ? o.mny : e.mny;
  e.mxx = o.mxx > e.mxx ? o.mxx : e.mxx;
  e.mxy = o.mxy > e.mxy ? o.mxy : e.mxy;
  e.any |= o.any;
}

// R of the header: float64, one IEEE operation per written operator (the library is built with -ffp-contract=off).
__host__ __device__ __forceinline__ AnnotBox annot_region(const AnnotExtent& e, const double margin[4]) {
  if (!e.any) return AnnotBox{0, 0, 0, 0};
  const double w = e.mxx - e.mnx, h = e.mxy - e.mny;
  const double side = w > h ? w : h;
  AnnotBox r;
  r.x0 = annot_coord(floor(e.mnx - margin[0] * side));
  r.y0 = annot_coord(floor(e.mny - margin[1] * side));
  r.x1 = annot_coord(ceil(e.mxx + margin[2] * side) + 1.0);
  r.y1 = annot_coord(ceil(e.mxy + margin[3] * side) + 1.0);
  return r;
}

// P = R clipped to the frame; empty when x1 <= x0 or y1 <= y0.
__host__ __device__ __forceinline__ AnnotBox annot_clip(const AnnotBox& r, int fw, int fh) {
  AnnotBox p;
  p.x0 = r.x0 < 0 ? 0 : r.x0;
  p.y0 = r.y0 < 0 ? 0 : r.y0;
  p.x1 = r.x1 > fw ? fw : r.x1;
  p.y1 = r.y1 > fh ? fh : r.y1;
  return p;
}
__host__ __device__ __forceinline__ bool annot_empty(const AnnotBox& p) { return p.x1 <= p.x0 || p.y1 <= p.y0; }
// A face takes part when P is not empty and its frame index names a slot of the ring.
__host__ __device__ __forceinline__ bool annot_takes_part(const AnnotBox& p, int fi, int nframes) {
  return !annot_empty(p) && fi >= 0 && fi < nframes;
}

// ---- the mosaic's cells ------------------------------------------------------------------------------------------------
// Cells of s x s pixels on a grid anchored at the frame's origin.  The cells a non-empty P (inside the frame, so every
// coordinate is >= 0) intersects: columns [x0/s, (x1-1)/s + 1), rows likewise.
__host__ __device__ __forceinline__ AnnotBox annot_cells(const AnnotBox& p, int s) {
  return AnnotBox{p.x0 / s, p.y0 / s, (p.x1 - 1) / s + 1, (p.y1 - 1) / s + 1};
}
__host__ __device__ __forceinline__ bool annot_cell_in(const AnnotBox& cells, int cx, int cy) {
  return cx >= cells.x0 && cx < cells.x1 && cy >= cells.y0 && cy < cells.y1;
}
// Ownership: a cell that P of face f intersects is processed by f unless a face j < f of the same frame that takes part
// intersects it too.  annot_competes says whether j can take any cell from f at all (what a workgroup collects once);
// annot_cell_in on j's cells then decides one cell.  r_*: the unclipped regions as the first launch wrote them.
__host__ __device__ __forceinline__ bool annot_competes(const AnnotBox& r_j, int fi_j, const AnnotBox& cells_f, int fi_f,
                                                        int nframes, int fw, int fh, int s, AnnotBox* cells_j) {
  const AnnotBox pj = annot_clip(r_j, fw, fh);
  if (fi_j != fi_f || !annot_takes_part(pj, fi_j, nframes)) return false;
  *cells_j = annot_cells(pj, s);
  return cells_j->x0 < cells_f.x1 && cells_f.x0 < cells_j->x1 && cells_j->y0 < cells_f.y1 && cells_f.y0 < cells_j->y1;
}
// The plain statement of the same predicate, a sequential scan: what the kernel's collected list must agree with.
__host__ __device__ inline bool annot_owns(const int32_t* regions, const int32_t* frame_idx, int nframes, int fw, int fh,
                                           int s, int f, int cx, int cy) {
  const AnnotBox rf{regions[4 * f], regions[4 * f + 1], regions[4 * f + 2], regions[4 * f + 3]};
  const int fi = frame_idx ? frame_idx[f] : 0;
  const AnnotBox pf = annot_clip(rf, fw, fh);
  if (!annot_takes_part(pf, fi, nframes)) return false;
  const AnnotBox cf = annot_cells(pf, s);
  if (!annot_cell_in(cf, cx, cy)) return false;
  for (int j = 0; j < f; ++j) {
    const AnnotBox rj{regions[4 * j], regions[4 * j + 1], regions[4 * j + 2], regions[4 * j + 3]};
    AnnotBox cj;
    if (annot_competes(rj, frame_idx ? frame_idx[j] : 0, cf, fi, nframes, fw, fh, s, &cj) && annot_cell_in(cj, cx, cy))
      return false;
  }
  return true;
}

// ---- the 21-pixel disc of draw_marks -----------------------------------------------------------------------------------
// dx*dx + dy*dy <= 5: rows of 3, 5, 5, 5, 3 pixels.  Offset o in [0, 21), row by row from dy = -2.
constexpr int kAnnotDisc = 21;
__host__ __device__ __forceinline__ void annot_disc_offset(int o, int* dx, int* dy) {
  if (o < 3) { *dy = -2; *dx = o - 1; }
  else if (o < 18) { const int r = (o - 3) / 5; *dy = r - 1; *dx = (o - 3) - 5 * r - 2; }
  else { *dy = 2; *dx = o - 19; }
}

// ---- the colour of a layer on an NV12 ring -----------------------------------------------------------------------------
// int32 throughout, >> arithmetic; coefficients round(exact x 2^16) of the limited-range forward matrix over (B,G,R).
struct AnnotYuvCoef {
  int y[3], u[3], v[3];
};
__host__ __device__ inline AnnotYuvCoef annot_yuv_coef(int matrix) {
  return matrix == FLM_YUV_BT709_LIMITED
             ? AnnotYuvCoef{{4064, 40254, 11966}, {28784, -22189, -6596}, {-2639, -26145, 28784}}
             : AnnotYuvCoef{{6416, 33039, 16829}, {28784, -19071, -9714}, {-4681, -24103, 28784}};
}
__host__ __device__ __forceinline__ int annot_clampi(int a, int lo, int hi) { return a < lo ? lo : (a > hi ? hi : a); }
__host__ __device__ inline void annot_bgr_to_yuv(int matrix, const uint8_t bgr[3], uint8_t yuv[3]) {
  const AnnotYuvCoef k = annot_yuv_coef(matrix);
  const int B = bgr[0], G = bgr[1], R = bgr[2];
  yuv[0] = (uint8_t)annot_clampi(16 + ((k.y[0] * B + k.y[1] * G + k.y[2] * R + (1 << 15)) >> 16), 16, 235);
  yuv[1] = (uint8_t)annot_clampi(128 + ((k.u[0] * B + k.u[1] * G + k.u[2] * R + (1 << 15)) >> 16), 16, 240);
  yuv[2] = (uint8_t)annot_clampi(128 + ((k.v[0] * B + k.v[1] * G + k.v[2] * R + (1 << 15)) >> 16), 16, 240);
}

}  // namespace flm
