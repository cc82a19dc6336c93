// The arithmetic of flm_flow_pyramid and flm_landmark_flow (include/flm.h states the contract), as __host__ __device__
// functions: the pyramid kernel of flm_flow.hip, the flow kernel of flm_flow_rows.hip and a host program
// (tests/native/flow_host.cpp) run this text.  Everything summed
// over a window is an exact integer; every float64 line is one IEEE operation per written operator, in the written order;
// the file must be compiled without contraction.
#ifndef FLM_FLOW_DEV_H_
#define FLM_FLOW_DEV_H_

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FLM_FLOW_HD __host__ __device__ inline
#else
#define FLM_FLOW_HD inline
#endif

namespace flm {

constexpr int kFlowMaxLevels = 6;
constexpr int kFlowMaxRadius = 7;
constexpr int kFlowNoHistory = 1, kFlowLowTexture = 2, kFlowResidual = 4, kFlowOutside = 8, kFlowMoved = 16,
              kFlowNotFinite = 32;
constexpr double kFlowReach = 1048576.0;   // 2^20: a coordinate beyond it is NOT_FINITE

// The options of a call as the kernel takes them (flm_flow_opts without its header fields).
struct FlowParams {
  int levels, radius, max_iter;
  double eps, min_eig, max_err, max_move;
};

FLM_FLOW_HD int flow_luma(int b, int g, int r) { return (1868 * b + 9617 * g + 4899 * r + 8192) >> 14; }
FLM_FLOW_HD int flow_down(int a, int b, int c, int d) { return (a + b + c + d + 2) >> 2; }
FLM_FLOW_HD bool flow_fin(double v) { return v >= -1.79769313486231570815e308 && v <= 1.79769313486231570815e308; }
FLM_FLOW_HD bool flow_in_reach(double x, double y) {   // finite and |.| <= 2^20 (a NaN fails)
  return x >= -kFlowReach && x <= kFlowReach && y >= -kFlowReach && y <= kFlowReach;
}
FLM_FLOW_HD int flow_clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// Bytes of the levels below level l of an h x w image: where level l starts in the pyramid of one image.
FLM_FLOW_HD size_t flow_level_offset(int h, int w, int l) {
  size_t off = 0;
  for (int j = 0; j < l; ++j) off += (size_t)(h >> j) * (size_t)(w >> j);
  return off;
}

// S(I, x, y) on a level of hl x wl bytes, for |x|, |y| < 2^30 (a guess in reach doubles at most five times): in
// [0, 255*1024].
FLM_FLOW_HD int32_t flow_sample(const uint8_t* I, int hl, int wl, double x, double y) {
  const double fx = floor(x), fy = floor(y);
  const int ix = (int)fx, iy = (int)fy;
  const int ax = (int)((x - fx) * 32.0), ay = (int)((y - fy) * 32.0);
  const int x0 = flow_clampi(ix, wl - 1), x1 = flow_clampi(ix + 1, wl - 1);
  const int y0 = flow_clampi(iy, hl - 1), y1 = flow_clampi(iy + 1, hl - 1);
  const int p00 = I[(size_t)y0 * wl + x0], p01 = I[(size_t)y0 * wl + x1];
  const int p10 = I[(size_t)y1 * wl + x0], p11 = I[(size_t)y1 * wl + x1];
  return (32 - ax) * (32 - ay) * p00 + ax * (32 - ay) * p01 + (32 - ax) * ay * p10 + ax * ay * p11;
}

// The start of a point: NO_HISTORY, NOT_FINITE or 0, and p0 in crop px.
FLM_FLOW_HD int flow_start(const float* m, double x, double y, double* p0x, double* p0y) {
  *p0x = -1.0;
  *p0y = -1.0;
  if (!(x >= 0.0 && y >= 0.0 && flow_fin(x) && flow_fin(y))) return kFlowNoHistory;
  const double m00 = (double)m[0], m01 = (double)m[1], m02 = (double)m[2];
  const double m10 = (double)m[3], m11 = (double)m[4], m12 = (double)m[5];
  *p0x = (m00 * x + m01 * y) + m02;
  *p0y = (m10 * x + m11 * y) + m12;
  return flow_in_reach(*p0x, *p0y) ? 0 : kFlowNotFinite;
}

FLM_FLOW_HD double flow_level_coord(double p0, int l) { return (p0 + 0.5) / (double)(1 << l) - 0.5; }

// The smaller eigenvalue of the window's structure tensor per pixel, in grey levels squared.
FLM_FLOW_HD double flow_min_eig(double A, double B, double C, int n) {
  return (((A + C) - sqrt((A - C) * (A - C) + 4.0 * B * B)) / 2.0) / ((double)n * 4194304.0);
}

FLM_FLOW_HD void flow_solve(double A, double B, double C, double det, double bx, double by, double* dx, double* dy) {
  *dx = 2.0 * (C * bx - B * by) / det;
  *dy = 2.0 * (A * by - B * bx) / det;
}

// One update of the guess: returns 0 to go on, 1 converged, 2 NOT_FINITE.
FLM_FLOW_HD int flow_update(double dx, double dy, double eps, double* qx, double* qy) {
  *qx = *qx + dx;
  *qy = *qy + dy;
  if (!flow_in_reach(*qx, *qy)) return 2;
  return (dx * dx + dy * dy < eps * eps) ? 1 : 0;
}

// The three gates of the end.
FLM_FLOW_HD int flow_gates(int32_t err, int n, double qx, double qy, double p0x, double p0y, int h, int w,
                           double max_err, double max_move) {
  int f = 0;
  if (!((double)err / ((double)n * 1024.0) <= max_err)) f |= kFlowResidual;
  if (!(0.0 <= qx && qx <= (double)(w - 1) && 0.0 <= qy && qy <= (double)(h - 1))) f |= kFlowOutside;
  const double mx = qx - p0x, my = qy - p0y;
  if (!(mx * mx + my * my <= max_move * max_move)) f |= kFlowMoved;
  return f;
}

// The pyramid walk of one point, serially: flow_point calls it once, flow_rows_point (flm_flow_rows_dev.h) once more
// for its backward pass.
// From p0 in crop px, the window of image `a` is looked for in image `b`, as "for l = levels-1 down to 0" of
// flm_landmark_flow states it.  Returns LOW_TEXTURE, NOT_FINITE or both bits; *qx, *qy: the guess where the walk stopped;
// *sad: the residual sum of the end, or -1 after NOT_FINITE.
FLM_FLOW_HD int flow_walk(const uint8_t* a, const uint8_t* b, int h, int w, double p0x, double p0y, const FlowParams& o,
                          double* qx_out, double* qy_out, int32_t* sad_out) {
  const int r = o.radius;
  int flags = 0;
  double qx = 0.0, qy = 0.0, px = 0.0, py = 0.0;
  *sad_out = -1;
  for (int l = o.levels - 1; l >= 0; --l) {
    const int hl = h >> l, wl = w >> l;
    const uint8_t* P = a + flow_level_offset(h, w, l);
    const uint8_t* Q = b + flow_level_offset(h, w, l);
    px = flow_level_coord(p0x, l);
    py = flow_level_coord(p0y, l);
    if (l == o.levels - 1) {
      qx = px;
      qy = py;
    }
    int64_t sa = 0, sb = 0, sc = 0;
    for (int j = -r; j <= r; ++j)
      for (int i = -r; i <= r; ++i) {
        const int64_t gx = flow_sample(P, hl, wl, px + (double)(i + 1), py + (double)j) -
                           flow_sample(P, hl, wl, px + (double)(i - 1), py + (double)j);
        const int64_t gy = flow_sample(P, hl, wl, px + (double)i, py + (double)(j + 1)) -
                           flow_sample(P, hl, wl, px + (double)i, py + (double)(j - 1));
        sa += gx * gx;
        sb += gx * gy;
        sc += gy * gy;
      }
    const double A = (double)sa, B = (double)sb, C = (double)sc;
    const double det = A * C - B * B;
    const double e = flow_min_eig(A, B, C, (2 * r + 1) * (2 * r + 1));
    if (!(e >= o.min_eig)) {
      if (l == 0) flags |= kFlowLowTexture;
    } else {
      for (int it = 0; it < o.max_iter; ++it) {
        int64_t sx = 0, sy = 0;
        for (int j = -r; j <= r; ++j)
          for (int i = -r; i <= r; ++i) {
            const int64_t t = flow_sample(P, hl, wl, px + (double)i, py + (double)j);
            const int64_t gx = flow_sample(P, hl, wl, px + (double)(i + 1), py + (double)j) -
                               flow_sample(P, hl, wl, px + (double)(i - 1), py + (double)j);
            const int64_t gy = flow_sample(P, hl, wl, px + (double)i, py + (double)(j + 1)) -
                               flow_sample(P, hl, wl, px + (double)i, py + (double)(j - 1));
            const int64_t d = t - flow_sample(Q, hl, wl, qx + (double)i, qy + (double)j);
            sx += d * gx;
            sy += d * gy;
          }
        double dx, dy;
        flow_solve(A, B, C, det, (double)sx, (double)sy, &dx, &dy);
        const int st = flow_update(dx, dy, o.eps, &qx, &qy);
        if (st == 2) {
          *qx_out = qx;
          *qy_out = qy;
          return flags | kFlowNotFinite;
        }
        if (st == 1) break;
      }
    }
    if (l > 0) {
      qx = 2.0 * qx + 0.5;
      qy = 2.0 * qy + 0.5;
    }
  }
  int64_t sad = 0;
  for (int j = -r; j <= r; ++j)
    for (int i = -r; i <= r; ++i) {
      const int64_t d = (int64_t)flow_sample(a, h, w, px + (double)i, py + (double)j) -
                        flow_sample(b, h, w, qx + (double)i, qy + (double)j);
      sad += d < 0 ? -d : d;
    }
  *sad_out = (int32_t)sad;
  *qx_out = qx;
  *qy_out = qy;
  return flags;
}

// The whole flow of one point, serially: what a host program calls.  The kernel runs the same functions with the window
// spread over the lanes of a wave.  Returns the flags; *qx, *qy: the guess where it stopped (p0, or -1, where no level
// ran); *err: the SAD or -1.
FLM_FLOW_HD int flow_point(const uint8_t* prev, const uint8_t* cur, int h, int w, const float* m, double x, double y,
                           const FlowParams& o, double* qx_out, double* qy_out, int32_t* err_out) {
  double p0x, p0y;
  int flags = flow_start(m, x, y, &p0x, &p0y);
  *qx_out = p0x;
  *qy_out = p0y;
  *err_out = -1;
  if (flags) return flags;
  flags = flow_walk(prev, cur, h, w, p0x, p0y, o, qx_out, qy_out, err_out);
  if (flags & kFlowNotFinite) return flags;
  const int side = 2 * o.radius + 1;
  return flags | flow_gates(*err_out, side * side, *qx_out, *qy_out, p0x, p0y, h, w, o.max_err, o.max_move);
}

}  // namespace flm
#endif  // FLM_FLOW_DEV_H_
