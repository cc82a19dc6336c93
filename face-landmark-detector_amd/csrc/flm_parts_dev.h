// The arithmetic of flm_part_affines / flm_warp_parts_frames (the fit of one part) and of flm_face_openness (the record
// of one measure, the step of its blink state), as __host__ __device__ functions: the kernels of flm_parts.hip and a host
// program (tests/native/parts_host.cpp) run this text.  include/flm.h states the contract.  Every line is one IEEE float64
// operation per written operator; the file must be compiled without contraction.
#ifndef FLM_PARTS_DEV_H_
#define FLM_PARTS_DEV_H_

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FLM_PARTS_HD __host__ __device__ inline
#else
#define FLM_PARTS_HD inline
#endif

#ifndef FLM_PART_MAX_POINTS
#define FLM_PART_MAX_POINTS 32
#endif
#ifndef FLM_OPEN_REC
#define FLM_OPEN_REC 4
#endif
#ifndef FLM_OPEN_STATE
#define FLM_OPEN_STATE 8
#endif

namespace flm {

constexpr int kPartPt = 5;  // doubles per staged point: x, y, w, template x, template y

// Stage entry i of a part: landmark `id` of face f, read at the element strides of
// flm_similarity_from_landmarks_weighted; an index outside [0,c) is staged as (-1,-1) with weight 0.
FLM_PARTS_HD void part_stage(double* pt, const double* lm, size_t lm_stride, const double* wt, size_t w_stride, size_t f,
                             int c, int id, const double* tmpl) {
  double x = -1.0, y = -1.0, w = 0.0;
  if (id >= 0 && id < c) {
    const size_t e = f * (size_t)c + (size_t)id;
    x = lm[e * lm_stride];
    y = lm[e * lm_stride + 1];
    w = wt ? wt[e * w_stride] : 1.0;
  }
  pt[0] = x; pt[1] = y; pt[2] = w; pt[3] = tmpl[0]; pt[4] = tmpl[1];
}

// similarity_weighted_kernel (flm_misc.hip) with sx = sy = 1 over the n staged points, in their order.  Writes the
// matrix (the identity when not ok) and returns ok: two participating points or more and var > 0.
FLM_PARTS_HD bool part_fit(const double* pt, int n, float* m) {
  double mpx = 0, mpy = 0, mqx = 0, mqy = 0, wsum = 0;
  int cnt = 0;
  for (int i = 0; i < n; ++i) {
    const double* q = pt + kPartPt * i;
    if (!(q[0] >= 0.0 && q[1] >= 0.0 && q[2] > 0.0)) continue;
    mpx += q[2] * q[0]; mpy += q[2] * q[1];
    mqx += q[2] * q[3]; mqy += q[2] * q[4];
    wsum += q[2];
    ++cnt;
  }
  double a = 1.0, b = 0.0, tx = 0.0, ty = 0.0;
  bool ok = false;
  if (cnt >= 2) {
    mpx /= wsum; mpy /= wsum; mqx /= wsum; mqy /= wsum;
    double sa = 0, sb = 0, var = 0;
    for (int i = 0; i < n; ++i) {
      const double* q = pt + kPartPt * i;
      if (!(q[0] >= 0.0 && q[1] >= 0.0 && q[2] > 0.0)) continue;
      const double px = q[0] - mpx, py = q[1] - mpy;
      const double qx = q[3] - mqx, qy = q[4] - mqy;
      sa += q[2] * (px * qx + py * qy);
      sb += q[2] * (px * qy - py * qx);
      var += q[2] * (px * px + py * py);
    }
    if (var > 0.0) {
      a = sa / var;
      b = sb / var;
      tx = mqx - (a * mpx - b * mpy);
      ty = mqy - (b * mpx + a * mpy);
      ok = true;
    }
  }
  m[0] = (float)a; m[1] = (float)(-b); m[2] = (float)tx;
  m[3] = (float)b; m[4] = (float)a;    m[5] = (float)ty;
  return ok;
}

// ---- openness ----------------------------------------------------------------------------------------------------------
// A landmark of row r as the measures read it: takes part as in flm_head_pose.
struct OpenPoint {
  double x, y;
  bool part;
};
FLM_PARTS_HD OpenPoint open_point(const double* lm, size_t lm_stride, const double* wt, size_t w_stride, size_t r, int c,
                                  int id) {
  OpenPoint p;
  p.x = -1.0; p.y = -1.0; p.part = false;
  if (id >= 0 && id < c) {
    const size_t e = r * (size_t)c + (size_t)id;
    p.x = lm[e * lm_stride];
    p.y = lm[e * lm_stride + 1];
    const double w = wt ? wt[e * w_stride] : 1.0;
    p.part = p.x >= 0.0 && p.y >= 0.0 && w > 0.0;
  }
  return p;
}
FLM_PARTS_HD double open_dist(const OpenPoint& a, const OpenPoint& b) {
  const double dx = a.x - b.x, dy = a.y - b.y;
  return sqrt(dx * dx + dy * dy);
}
FLM_PARTS_HD bool open_fin(double v) { return v >= -1.79769313486231570815e308 && v <= 1.79769313486231570815e308; }

// The record of one measure: width pair (wa, wb), v pairs (up[i], lo[i]).  Returns ok.
FLM_PARTS_HD bool open_record(const double* lm, size_t lm_stride, const double* wt, size_t w_stride, size_t r, int c, int wa,
                              int wb, int v, const int32_t* up, const int32_t* lo, double min_width, double* rec) {
  const OpenPoint a = open_point(lm, lm_stride, wt, w_stride, r, c, wa), b = open_point(lm, lm_stride, wt, w_stride, r, c, wb);
  bool all = a.part && b.part;
  double sum = 0.0;
  for (int i = 0; i < v; ++i) {
    const OpenPoint u = open_point(lm, lm_stride, wt, w_stride, r, c, up[i]), l = open_point(lm, lm_stride, wt, w_stride, r, c, lo[i]);
    all = all && u.part && l.part;
    sum = sum + open_dist(u, l);
  }
  if (!all) {  // a named landmark that does not take part: nothing was measured
    rec[0] = -1.0; rec[1] = -1.0; rec[2] = 0.0; rec[3] = -1.0;
    return false;
  }
  const double dw = open_dist(a, b);
  const double o = (sum / (double)v) / dw;
  const bool ok = dw >= min_width && open_fin(o);
  rec[0] = ok ? o : -1.0; rec[1] = dw; rec[2] = ok ? 1.0 : 0.0; rec[3] = sum;
  return ok;
}

struct OpenThresholds {
  double close_below, open_above, min_closed, max_closed;
};

FLM_PARTS_HD void open_state_reset(double* st) {
  st[0] = 0.0; st[1] = 0.0; st[2] = 0.0; st[3] = -1.0; st[4] = 0.0; st[5] = 0.0; st[6] = -1.0; st[7] = 0.0;
}

// One tick of one measure's state {closed, run, events, last_closed, closed_total, seen_total, last_event_frame, 0}.
// The caller has applied a pending reset.  Nothing is written unless the measure is ok, status == 0 and dt is finite
// and > 0.
FLM_PARTS_HD void open_state_step(double* st, bool ok, double o, int status, double dt, const OpenThresholds& t,
                                  int64_t frame_id) {
  if (!ok || status != 0 || !(dt > 0.0 && open_fin(dt))) return;
  st[5] = st[5] + dt;
  if (st[0] == 0.0) {
    if (o < t.close_below) {
      st[0] = 1.0;
      st[1] = 0.0;
      st[4] = st[4] + dt;
    } else {
      st[1] = st[1] + dt;
    }
  } else if (o > t.open_above) {
    const double d = st[1] + dt;
    st[3] = d;
    if (t.min_closed <= d && d <= t.max_closed) {
      st[2] = st[2] + 1.0;
      st[6] = (double)frame_id;
    }
    st[0] = 0.0;
    st[1] = 0.0;
  } else {
    st[1] = st[1] + dt;
    st[4] = st[4] + dt;
  }
}

}  // namespace flm
#endif  // FLM_PARTS_DEV_H_
