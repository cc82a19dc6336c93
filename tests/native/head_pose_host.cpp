// Host sweep of csrc/flm_pose_dev.h, the arithmetic flm_head_pose's kernel is built from, against a long-double
// restatement of the contract in include/flm.h.
//   1. Seeded poses of the six-point face model, of four non-coplanar points (P = 4) and of a cloud of P = 256 points,
//      with noise on the landmarks, random weights and rejected points.
//   2. The extremes: coordinates at 0 and 2^15, model units of 1e-3 and 1e6, single weights of 1e-300, inf and NaN, all
//      landmarks identical, all model points identical, the coplanar four, three points, none.
// Checks: the ok flags agree wherever the restatement's vol lies a factor of 10 from the threshold on either side; R
// agrees within 1e-9 where both are ok; a record that is not ok is exactly the stated one; an ok record holds nothing
// that is not finite.  Built with the host's address and undefined-behaviour sanitizers.  No GPU call is made.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "flm_pose_dev.h"

static long long failures = 0, checks = 0;
#define CHECK(cond, ...)                                   \
  do {                                                     \
    ++checks;                                              \
    if (!(cond)) {                                         \
      if (++failures <= 20) { std::printf(__VA_ARGS__); std::printf("\n"); } \
    }                                                      \
  } while (0)

typedef long double ld;
static const double kMinVol = 1e-6;

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static double uniform() {  // xorshift64*, in [0, 1)
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return (double)((rng_state * 0x2545f4914f6cdd1dull) >> 11) / 9007199254740992.0;
}
static double uniform(double a, double b) { return a + (b - a) * uniform(); }

struct Face {
  std::vector<double> xyz, x, y, w;  // per model point: the 3-D point, the landmark it names, its weight
  std::vector<char> in_range;
  int p() const { return (int)x.size(); }
  void add(double X, double Y, double Z, double px, double py, double wt, bool in = true) {
    xyz.push_back(X); xyz.push_back(Y); xyz.push_back(Z);
    x.push_back(px); y.push_back(py); w.push_back(wt); in_range.push_back(in);
  }
};

struct RefFit {
  bool ok;
  int cnt;
  ld vol, R[9];
};

static ld norm3(const ld* a) { return sqrtl(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]); }
static bool pos(ld v) { return std::isfinite(v) && v > 0; }

static RefFit reference(const Face& f) {
  RefFit r;
  r.ok = false; r.vol = NAN; r.cnt = 0;
  std::vector<int> part;
  for (int i = 0; i < f.p(); ++i)
    if (f.in_range[i] && f.x[i] >= 0.0 && f.y[i] >= 0.0 && f.w[i] > 0.0) part.push_back(i);
  r.cnt = (int)part.size();
  ld W = 0, m[5] = {0, 0, 0, 0, 0};
  for (int i : part) {
    const ld v[5] = {f.xyz[3 * i], f.xyz[3 * i + 1], f.xyz[3 * i + 2], f.x[i], f.y[i]};
    W += f.w[i];
    for (int j = 0; j < 5; ++j) m[j] += (ld)f.w[i] * v[j];
  }
  for (int j = 0; j < 5; ++j) m[j] /= W;
  ld a[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, b[2][3] = {{0, 0, 0}, {0, 0, 0}};
  for (int i : part) {
    const ld d[5] = {f.xyz[3 * i] - m[0], f.xyz[3 * i + 1] - m[1], f.xyz[3 * i + 2] - m[2], f.x[i] - m[3], f.y[i] - m[4]};
    for (int u = 0; u < 3; ++u) {
      for (int v = 0; v < 3; ++v) a[u][v] += (ld)f.w[i] * d[u] * d[v];
      b[0][u] += (ld)f.w[i] * d[u] * d[3];
      b[1][u] += (ld)f.w[i] * d[u] * d[4];
    }
  }
  ld c[3][3];
  c[0][0] = a[1][1] * a[2][2] - a[1][2] * a[1][2];
  c[0][1] = a[0][2] * a[1][2] - a[0][1] * a[2][2];
  c[0][2] = a[0][1] * a[1][2] - a[0][2] * a[1][1];
  c[1][1] = a[0][0] * a[2][2] - a[0][2] * a[0][2];
  c[1][2] = a[0][1] * a[0][2] - a[0][0] * a[1][2];
  c[2][2] = a[0][0] * a[1][1] - a[0][1] * a[0][1];
  c[1][0] = c[0][1]; c[2][0] = c[0][2]; c[2][1] = c[1][2];
  const ld det = a[0][0] * c[0][0] + a[0][1] * c[0][1] + a[0][2] * c[0][2];
  r.vol = det / (a[0][0] * a[1][1] * a[2][2]);
  ld I[3], J[3];
  for (int k = 0; k < 3; ++k) {
    I[k] = (c[k][0] * b[0][0] + c[k][1] * b[0][1] + c[k][2] * b[0][2]) / det;
    J[k] = (c[k][0] * b[1][0] + c[k][1] * b[1][1] + c[k][2] * b[1][2]) / det;
  }
  const ld nI = norm3(I), nJ = norm3(J);
  ld e[3], g[3];
  for (int k = 0; k < 3; ++k) {
    e[k] = I[k] / nI + J[k] / nJ;
    g[k] = I[k] / nI - J[k] / nJ;
  }
  const ld ne = norm3(e), ng = norm3(g);
  const ld H = 0.7071067811865476;
  for (int k = 0; k < 3; ++k) {
    r.R[k] = (e[k] / ne + g[k] / ng) * H;
    r.R[3 + k] = (e[k] / ne - g[k] / ng) * H;
  }
  r.R[6] = r.R[1] * r.R[5] - r.R[2] * r.R[4];
  r.R[7] = r.R[2] * r.R[3] - r.R[0] * r.R[5];
  r.R[8] = r.R[0] * r.R[4] - r.R[1] * r.R[3];
  bool fin = true;
  for (int k = 0; k < 9; ++k) fin = fin && std::isfinite(r.R[k]);
  // W is judged as the double sum is: a weight of inf makes it inf in either format
  r.ok = r.cnt >= 4 && pos(W) && (double)W <= 1.79769313486231570815e308 && pos(det) && pos(nI) && pos(nJ) && pos(ne) &&
         pos(ng) && r.vol >= (ld)kMinVol && fin;
  return r;
}

static bool bits_equal(double a, double b) { return std::memcmp(&a, &b, 8) == 0; }

// Runs the header on the face and compares; want: -1 = whatever the restatement says, 0 / 1 = this ok flag exactly.
static void run(const char* name, const Face& f, int want) {
  const int p = f.p();
  std::vector<double> pt((size_t)p * flm::kPosePt);
  for (int i = 0; i < p; ++i)
    flm::pose_stage(pt.data() + flm::kPosePt * i, f.xyz.data() + 3 * i, f.in_range[i] != 0, f.x[i], f.y[i], f.w[i]);
  double rec[FLM_POSE_REC], vol = 0;
  const bool ok = flm::pose_fit(pt.data(), p, kMinVol, rec, &vol);
  const RefFit r = reference(f);
  CHECK((int)rec[13] == r.cnt, "%s: cnt %g, restated %d", name, rec[13], r.cnt);
  CHECK(rec[14] == (ok ? 1.0 : 0.0), "%s: the ok entry %g and the return value %d differ", name, rec[14], (int)ok);
  if (want >= 0) CHECK((int)ok == want, "%s: ok = %d, expected %d (vol %g)", name, (int)ok, want, vol);
  const bool decided = std::isfinite(r.vol) && (r.vol >= 10 * (ld)kMinVol || r.vol <= (ld)kMinVol / 10);
  if (decided) CHECK(ok == r.ok, "%s: ok = %d, restated %d (vol %g, restated %Lg)", name, (int)ok, (int)r.ok, vol, r.vol);
  if (!ok) {
    double none[FLM_POSE_REC];
    flm::pose_not_ok(none, r.cnt);
    const double stated[FLM_POSE_REC] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, -1, -1, 0, (double)r.cnt, 0, 0, 0, 0};
    for (int k = 0; k < FLM_POSE_REC; ++k)
      CHECK(bits_equal(rec[k], stated[k]) && bits_equal(none[k], stated[k]), "%s: entry %d of a record that is not ok is %g",
            name, k, rec[k]);
    CHECK(flm::pose_factor(ok, rec, 0.0) == 0.0, "%s: a factor for a fit that is not ok", name);
    return;
  }
  for (int k = 0; k < FLM_POSE_REC; ++k) CHECK(std::isfinite(rec[k]), "%s: entry %d of an ok record is %g", name, k, rec[k]);
  if (r.ok)
    for (int k = 0; k < 9; ++k)
      CHECK(fabsl((ld)rec[k] - r.R[k]) <= 1e-9L, "%s: R[%d] = %.17g, restated %.17Lg (vol %g)", name, k, rec[k], r.R[k], vol);
  // R is orthonormal and right-handed whatever the data
  for (int u = 0; u < 3; ++u)
    for (int v = u; v < 3; ++v) {
      const double d = rec[3 * u] * rec[3 * v] + rec[3 * u + 1] * rec[3 * v + 1] + rec[3 * u + 2] * rec[3 * v + 2];
      CHECK(std::fabs(d - (u == v ? 1.0 : 0.0)) <= 1e-12, "%s: rows %d.%d of R give %.17g", name, u, v, d);
    }
  CHECK(std::fabs(rec[15]) <= 3.1415926535897936 && std::fabs(rec[16]) <= 1.5707963267948968 &&
        std::fabs(rec[17]) <= 3.1415926535897936, "%s: angles %g %g %g", name, rec[15], rec[16], rec[17]);
  CHECK(flm::pose_factor(ok, rec, 0.0) == (rec[8] >= 0.0 ? rec[8] : 0.0), "%s: factor", name);
  CHECK(flm::pose_factor(ok, rec, 1.0) == (rec[8] >= 1.0 ? rec[8] : 0.0), "%s: factor at min_frontal = 1", name);
}

static const double kModel[6][3] = {{0, 0, 0}, {0, 330, 65}, {-225, -170, 135}, {225, -170, 135}, {-150, 150, 125},
                                    {150, 150, 125}};

static void rotation(double yaw, double pitch, double roll, double* R) {
  const double cy = cos(yaw), sy = sin(yaw), cp = cos(pitch), sp = sin(pitch), cr = cos(roll), sr = sin(roll);
  const double m[9] = {cy, 0, sy, sp * sy, cp, -sp * cy, -cp * sy, sp, cp * cy};  // Rx Ry
  for (int k = 0; k < 3; ++k) {
    R[k] = cr * m[k] - sr * m[3 + k];
    R[3 + k] = sr * m[k] + cr * m[3 + k];
    R[6 + k] = m[6 + k];
  }
}

// The model points `pts` under a random pose and scale; the model handed to the fit is `pts` in units of `unit`.
static Face posed(const std::vector<double>& pts, double unit, double noise, double reject, bool weights) {
  double R[9];
  rotation(uniform(-1, 1), uniform(-1, 1), uniform(-3, 3), R);
  const double s = uniform(0.05, 3.0), tx = uniform(3000, 20000), ty = uniform(3000, 20000);
  Face f;
  for (size_t i = 0; i < pts.size() / 3; ++i) {
    const double X = pts[3 * i], Y = pts[3 * i + 1], Z = pts[3 * i + 2];
    double x = s * (R[0] * X + R[1] * Y + R[2] * Z) + tx + uniform(-noise, noise);
    double y = s * (R[3] * X + R[4] * Y + R[5] * Z) + ty + uniform(-noise, noise);
    if (uniform() < reject) x = y = -1.0;
    f.add(X * unit, Y * unit, Z * unit, x, y, weights ? uniform(0.1, 1.0) : 1.0);
  }
  return f;
}

int main() {
  std::vector<double> six(&kModel[0][0], &kModel[0][0] + 18), four(&kModel[0][0], &kModel[0][0] + 12), cloud;
  for (int i = 0; i < 256 * 3; ++i) cloud.push_back(uniform(-300, 300));
  char name[96];
  for (int t = 0; t < 3000; ++t) {
    std::snprintf(name, sizeof name, "six #%d", t);
    run(name, posed(six, 1.0, t % 3 ? 2.0 : 0.0, t % 5 ? 0.0 : 0.15, t % 2), -1);
  }
  for (int t = 0; t < 1000; ++t) {
    std::snprintf(name, sizeof name, "four #%d", t);
    run(name, posed(four, 1.0, t % 3 ? 2.0 : 0.0, 0.0, t % 2), 1);   // nose, chin and the eye corners: not coplanar
  }
  for (int t = 0; t < 200; ++t) {
    std::snprintf(name, sizeof name, "cloud #%d", t);
    run(name, posed(cloud, 1.0, 2.0, 0.3, t % 2), 1);
  }
  // model units
  for (int t = 0; t < 200; ++t) {
    run("unit 1e-3", posed(six, 1e-3, 1.0, 0.0, t % 2), 1);
    run("unit 1e6", posed(six, 1e6, 1.0, 0.0, t % 2), 1);
  }
  // coordinates at 0 and 2^15: the frontal model stretched over the whole range
  {
    Face f;
    for (int i = 0; i < 6; ++i)
      f.add(kModel[i][0], kModel[i][1], kModel[i][2], (kModel[i][0] + 225.0) / 450.0 * 32768.0,
            (kModel[i][1] + 170.0) / 500.0 * 32768.0, 1.0);
    run("0 and 2^15", f, 1);
    CHECK(f.x[2] == 0.0 && f.x[3] == 32768.0 && f.y[2] == 0.0 && f.y[1] == 32768.0, "the extreme coordinates are not exact");
  }
  // single weights of 1e-300, inf and NaN among ordinary ones
  for (int t = 0; t < 50; ++t) {
    Face f = posed(six, 1.0, 1.0, 0.0, true);
    f.w[t % 6] = 1e-300;
    run("one weight of 1e-300", f, 1);
    f.w[t % 6] = NAN;                      // the point is left out; five remain, never the coplanar four alone
    run("one NaN weight", f, 1);
    f.w[t % 6] = INFINITY;                 // W is not finite
    run("one weight of inf", f, 0);
    f.w[t % 6] = -1.0;
    run("one negative weight", f, 1);
  }
  // all landmarks identical, all model points identical: unit weights and whole numbers keep every difference exactly 0
  {
    Face f, g;
    for (int i = 0; i < 6; ++i) {
      f.add(kModel[i][0], kModel[i][1], kModel[i][2], 640.0, 360.0, 1.0);
      g.add(7.0, -3.0, 11.0, 100.0 + 10.0 * i, 200.0 + 7.0 * i * i, 1.0);
    }
    run("identical landmarks", f, 0);
    run("identical model points", g, 0);
  }
  // the coplanar four alone, three points, none, indices out of range
  {
    Face f = posed(six, 1.0, 0.0, 0.0, false), g = f, h = f, k = f, o = f;
    f.x[0] = f.y[0] = f.x[1] = f.y[1] = -1.0;
    run("the coplanar four", f, 0);
    g.x[0] = g.x[2] = -1.0; g.y[4] = -1.0;
    run("three points", g, 0);
    for (int i = 0; i < 6; ++i) h.x[i] = -1.0;
    run("no point", h, 0);
    for (int i = 0; i < 6; ++i) k.w[i] = 0.0;
    run("zero weights", k, 0);
    o.in_range[0] = o.in_range[1] = 0;
    run("indices outside the landmarks", o, 0);
  }
  std::printf("%lld checks, %lld failures\n", checks, failures);
  return failures ? 1 : 0;
}
