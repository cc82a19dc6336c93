// The arithmetic of flm_head_pose (include/flm.h states the contract), as __host__ __device__ functions: the kernel of
// flm_pose.hip and a host program (tests/native/head_pose_host.cpp) run this text.  Every line is one IEEE float64
// operation per written operator; the file must be compiled without contraction.
//
// The points of one face are STAGED as six doubles each, pt[6*p + {0,1,2,3,4,5}] = {X0, X1, X2, x, y, w}, in model order;
// a point that does not take part is staged with w = 0.0, and every sum skips the points whose w is not > 0.
#ifndef FLM_POSE_DEV_H_
#define FLM_POSE_DEV_H_

#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FLM_POSE_HD __host__ __device__ inline
#else
#define FLM_POSE_HD inline
#endif

#ifndef FLM_POSE_REC
#define FLM_POSE_REC 18
#endif

namespace flm {

constexpr int kPosePt = 6;       // doubles per staged point
constexpr int kPoseSums1 = 6;    // W, sum w*X0, w*X1, w*X2, w*x, w*y
constexpr int kPoseSums2 = 12;   // a00 a01 a02 a11 a12 a22, bx0 bx1 bx2, by0 by1 by2

// Stage point p: takes part when 0 <= idx < c, both coordinates >= 0 and w > 0 (a NaN fails the test).
FLM_POSE_HD void pose_stage(double* pt, const double* xyz, bool in_range, double x, double y, double w) {
  const bool part = in_range && x >= 0.0 && y >= 0.0 && w > 0.0;
  pt[0] = xyz[0]; pt[1] = xyz[1]; pt[2] = xyz[2];
  pt[3] = part ? x : -1.0;
  pt[4] = part ? y : -1.0;
  pt[5] = part ? w : 0.0;
}

// Sum k of the first pass, sequentially from 0.0 in model order: k = 0: sum w; k = 1..5: sum w*{X0, X1, X2, x, y}.
// *cnt (may be null) receives the number of participating points.
FLM_POSE_HD double pose_sum1(int k, const double* pt, int p, int* cnt) {
  double s = 0.0;
  int n = 0;
  for (int i = 0; i < p; ++i) {
    const double* q = pt + kPosePt * i;
    const double w = q[5];
    if (!(w > 0.0)) continue;
    const double t = k == 0 ? w : w * q[k - 1];
    s = s + t;
    ++n;
  }
  if (cnt) *cnt = n;
  return s;
}

// Sum k of the second pass: w * (d[u] * d[v]) with d = (X', x', y') = pt[0..4] - mean[0..4];
// (u, v) of k = 0..11: (0,0) (0,1) (0,2) (1,1) (1,2) (2,2) | (0,3) (1,3) (2,3) | (0,4) (1,4) (2,4).
FLM_POSE_HD double pose_sum2(int k, const double* pt, int p, const double* mean) {
  const int u = (int)((0x210210211000ull >> (4 * k)) & 15u), v = (int)((0x444333221210ull >> (4 * k)) & 15u);
  const double mu = mean[u], mv = mean[v];
  double s = 0.0;
  for (int i = 0; i < p; ++i) {
    const double* q = pt + kPosePt * i;
    const double w = q[5];
    if (!(w > 0.0)) continue;
    const double du = q[u] - mu, dv = q[v] - mv;
    const double t = du * dv;
    s = s + w * t;
  }
  return s;
}

FLM_POSE_HD double pose_norm3(const double* a) { return sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]); }
FLM_POSE_HD bool pose_pos(double v) { return v > 0.0 && v <= 1.79769313486231570815e308; }  // finite and > 0
FLM_POSE_HD bool pose_fin(double v) { return v >= -1.79769313486231570815e308 && v <= 1.79769313486231570815e308; }

FLM_POSE_HD void pose_not_ok(double* rec, int cnt) {
  for (int i = 0; i < 9; ++i) rec[i] = (i == 0 || i == 4 || i == 8) ? 1.0 : 0.0;
  rec[9] = 0.0; rec[10] = -1.0; rec[11] = -1.0; rec[12] = 0.0;
  rec[13] = (double)cnt; rec[14] = 0.0; rec[15] = 0.0; rec[16] = 0.0; rec[17] = 0.0;
}

// Everything after the sums: s1[6], s2[12] as pose_sum1 / pose_sum2 return them (s2 computed with mean[j] = s1[j+1] / s1[0]),
// cnt from pose_sum1.  Writes the record; returns ok.  *vol_out (may be null): vol, NaN where it was not reached.
FLM_POSE_HD bool pose_solve(const double* s1, const double* s2, int cnt, const double* pt, int p, double min_volume,
                            double* rec, double* vol_out) {
  if (vol_out) *vol_out = NAN;
  const double W = s1[0];
  if (cnt < 4 || !pose_pos(W)) {
    pose_not_ok(rec, cnt);
    return false;
  }
  double mean[5];
  for (int j = 0; j < 5; ++j) mean[j] = s1[j + 1] / W;
  const double a00 = s2[0], a01 = s2[1], a02 = s2[2], a11 = s2[3], a12 = s2[4], a22 = s2[5];
  const double* bx = s2 + 6;
  const double* by = s2 + 9;
  const double c00 = a11 * a22 - a12 * a12;
  const double c01 = a02 * a12 - a01 * a22;
  const double c02 = a01 * a12 - a02 * a11;
  const double c11 = a00 * a22 - a02 * a02;
  const double c12 = a01 * a02 - a00 * a12;
  const double c22 = a00 * a11 - a01 * a01;
  const double det = (a00 * c00 + a01 * c01) + a02 * c02;
  const double vol = det / ((a00 * a11) * a22);
  if (vol_out) *vol_out = vol;
  if (!pose_pos(det) || !(vol >= min_volume)) {
    pose_not_ok(rec, cnt);
    return false;
  }
  const double ck[3][3] = {{c00, c01, c02}, {c01, c11, c12}, {c02, c12, c22}};
  double I[3], J[3];
  for (int k = 0; k < 3; ++k) {
    I[k] = ((ck[k][0] * bx[0] + ck[k][1] * bx[1]) + ck[k][2] * bx[2]) / det;
    J[k] = ((ck[k][0] * by[0] + ck[k][1] * by[1]) + ck[k][2] * by[2]) / det;
  }
  const double nI = pose_norm3(I), nJ = pose_norm3(J);
  if (!pose_pos(nI) || !pose_pos(nJ)) {
    pose_not_ok(rec, cnt);
    return false;
  }
  const double s = sqrt(nI * nJ);
  double e[3], f[3];
  for (int k = 0; k < 3; ++k) {
    const double ik = I[k] / nI, jk = J[k] / nJ;
    e[k] = ik + jk;
    f[k] = ik - jk;
  }
  const double ne = pose_norm3(e), nf = pose_norm3(f);
  if (!pose_pos(ne) || !pose_pos(nf)) {
    pose_not_ok(rec, cnt);
    return false;
  }
  const double H = 0.7071067811865476;
  double r1[3], r2[3], r3[3];
  for (int k = 0; k < 3; ++k) {
    const double ek = e[k] / ne, fk = f[k] / nf;
    r1[k] = (ek + fk) * H;
    r2[k] = (ek - fk) * H;
  }
  r3[0] = r1[1] * r2[2] - r1[2] * r2[1];
  r3[1] = r1[2] * r2[0] - r1[0] * r2[2];
  r3[2] = r1[0] * r2[1] - r1[1] * r2[0];
  double se = 0.0;
  for (int i = 0; i < p; ++i) {
    const double* q = pt + kPosePt * i;
    const double w = q[5];
    if (!(w > 0.0)) continue;
    const double X0 = q[0] - mean[0], X1 = q[1] - mean[1], X2 = q[2] - mean[2];
    const double xp = q[3] - mean[3], yp = q[4] - mean[4];
    const double ex = s * ((r1[0] * X0 + r1[1] * X1) + r1[2] * X2) - xp;
    const double ey = s * ((r2[0] * X0 + r2[1] * X1) + r2[2] * X2) - yp;
    se = se + w * (ex * ex + ey * ey);
  }
  const double rms = sqrt(se / W);
  bool fin = pose_fin(s) && pose_fin(rms);
  for (int k = 0; k < 3; ++k) fin = fin && pose_fin(r1[k]) && pose_fin(r2[k]) && pose_fin(r3[k]);
  if (!fin) {
    pose_not_ok(rec, cnt);
    return false;
  }
  for (int k = 0; k < 3; ++k) {
    rec[k] = r1[k];
    rec[3 + k] = r2[k];
    rec[6 + k] = r3[k];
  }
  rec[9] = s; rec[10] = mean[3]; rec[11] = mean[4]; rec[12] = rms;
  rec[13] = (double)cnt; rec[14] = 1.0;
  rec[15] = atan2(-r3[0], r3[2]);
  rec[16] = asin(fmin(fmax(r3[1], -1.0), 1.0));
  rec[17] = atan2(-r1[1], r2[1]);
  return true;
}

// The whole fit of one staged face, serially: what a host program calls.  The kernel runs the same three functions with
// the sums of a pass spread over lanes.
FLM_POSE_HD bool pose_fit(const double* pt, int p, double min_volume, double* rec, double* vol_out) {
  double s1[kPoseSums1], s2[kPoseSums2], mean[5];
  int cnt = 0;
  for (int k = 0; k < kPoseSums1; ++k) s1[k] = pose_sum1(k, pt, p, k == 0 ? &cnt : nullptr);
  for (int j = 0; j < 5; ++j) mean[j] = s1[j + 1] / s1[0];
  for (int k = 0; k < kPoseSums2; ++k) s2[k] = pose_sum2(k, pt, p, mean);
  return pose_solve(s1, s2, cnt, pt, p, min_volume, rec, vol_out);
}

FLM_POSE_HD double pose_factor(bool ok, const double* rec, double min_frontal) {
  return (ok && rec[8] >= min_frontal) ? rec[8] : 0.0;
}

}  // namespace flm
#endif  // FLM_POSE_DEV_H_
