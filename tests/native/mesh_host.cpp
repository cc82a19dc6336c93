// Host sweep of csrc/flm_mesh_dev.h, the arithmetic the kernels of csrc/flm_mesh.hip are built from, against a
// long-double restatement of the contract in include/flm.h ("shape-normalised faces").
//   1. The map: seeded meshes (a jittered grid of points under a fan of triangles per cell) over every integer pixel;
//      a pixel exactly on a shared edge and on a shared vertex, where the lowest index must win; a mesh with a hole; a
//      triangle that names a point outside the mesh.
//   2. The affine solve: seeded faces (an affine image of the template plus noise, anchors through M^-1), and the
//      extremes: collapsed, collinear and NaN landmarks (the fallback: the face's M, bit for bit), coordinates at 0 and
//      2^15, a determinant on either side of min_det.
// Checks: the map is EQUAL to the restatement's; every affine element is within 1 ULP of float32 of the restatement's,
// except where the long-double det is within 1e-12 relative of min_det (there either branch is accepted).
// Built without contraction, as the library is, and with the host's address and undefined-behaviour sanitizers.
// No GPU call is made.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "flm_mesh_dev.h"

static long long failures = 0, checks = 0;
#define CHECK(cond, ...)                                   \
  do {                                                     \
    ++checks;                                              \
    if (!(cond)) {                                         \
      if (++failures <= 20) { std::printf(__VA_ARGS__); std::printf("\n"); } \
    }                                                      \
  } while (0)

typedef long double ld;
static const double kMinDet = 1e-6;

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static double uniform() {  // xorshift64*, in [0, 1)
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return (double)((rng_state * 0x2545f4914f6cdd1dull) >> 11) / 9007199254740992.0;
}
static double uniform(double a, double b) { return a + (b - a) * uniform(); }

// ---- the restatement ------------------------------------------------------------------------------------------------
static ld edge_ref(ld ax, ld ay, ld bx, ld by, ld qx, ld qy) { return (bx - ax) * (qy - ay) - (by - ay) * (qx - ax); }

static int locate_ref(const std::vector<double>& pts, const std::vector<int32_t>& tris, ld qx, ld qy) {
  const int p = (int)pts.size() / 2, t = (int)tris.size() / 3;
  for (int i = 0; i < t; ++i) {
    const int a = tris[3 * i], b = tris[3 * i + 1], c = tris[3 * i + 2];
    if (a < 0 || a >= p || b < 0 || b >= p || c < 0 || c >= p) continue;
    if (edge_ref(pts[2 * a], pts[2 * a + 1], pts[2 * b], pts[2 * b + 1], qx, qy) >= 0 &&
        edge_ref(pts[2 * b], pts[2 * b + 1], pts[2 * c], pts[2 * c + 1], qx, qy) >= 0 &&
        edge_ref(pts[2 * c], pts[2 * c + 1], pts[2 * a], pts[2 * a + 1], qx, qy) >= 0)
      return i;
  }
  return 255;
}

struct RefAffine {
  ld det;
  bool fallback;
  ld a[6];
};

static void source_ref(const std::vector<double>& lm, const float* m, const std::vector<double>& pts, int c, int v, ld& sx,
                       ld& sy) {
  if (v < c) {
    sx = lm[2 * v];
    sy = lm[2 * v + 1];
    return;
  }
  const ld m00 = m[0], m01 = m[1], m02 = m[2], m10 = m[3], m11 = m[4], m12 = m[5];
  const ld det = m00 * m11 - m01 * m10;
  const ld tx = (ld)pts[2 * v] - m02, ty = (ld)pts[2 * v + 1] - m12;
  sx = (m11 / det) * tx + (-m01 / det) * ty;
  sy = (-m10 / det) * tx + (m00 / det) * ty;
}

static RefAffine affine_ref(const std::vector<double>& lm, const float* m, const std::vector<double>& pts, int c,
                            const int32_t* tri, double min_det) {
  ld s[3][2], d[3][2];
  for (int j = 0; j < 3; ++j) {
    d[j][0] = pts[2 * tri[j]];
    d[j][1] = pts[2 * tri[j] + 1];
    source_ref(lm, m, pts, c, tri[j], s[j][0], s[j][1]);
  }
  const ld e1x = s[1][0] - s[0][0], e1y = s[1][1] - s[0][1], e2x = s[2][0] - s[0][0], e2y = s[2][1] - s[0][1];
  const ld g1x = d[1][0] - d[0][0], g1y = d[1][1] - d[0][1], g2x = d[2][0] - d[0][0], g2y = d[2][1] - d[0][1];
  RefAffine r;
  r.det = e1x * e2y - e1y * e2x;
  r.fallback = !(fabsl(r.det) >= (ld)min_det);
  if (r.fallback) {
    for (int i = 0; i < 6; ++i) r.a[i] = m[i];
    return r;
  }
  r.a[0] = (g1x * e2y - g2x * e1y) / r.det;
  r.a[1] = (g2x * e1x - g1x * e2x) / r.det;
  r.a[3] = (g1y * e2y - g2y * e1y) / r.det;
  r.a[4] = (g2y * e1x - g1y * e2x) / r.det;
  r.a[2] = d[0][0] - (r.a[0] * s[0][0] + r.a[1] * s[0][1]);
  r.a[5] = d[0][1] - (r.a[3] * s[0][0] + r.a[4] * s[0][1]);
  return r;
}

// |got - want| in units of float32 ULPs on the monotone integer image of the floats; want is rounded to float32 first
static long long ulps(float got, ld want) {
  const float w = (float)want;
  int32_t a, b;
  std::memcpy(&a, &got, 4);
  std::memcpy(&b, &w, 4);
  const long long x = a < 0 ? -(long long)(a & 0x7fffffff) : a, y = b < 0 ? -(long long)(b & 0x7fffffff) : b;
  return x > y ? x - y : y - x;
}

// ---- meshes ---------------------------------------------------------------------------------------------------------
struct Mesh {
  std::vector<double> pts;
  std::vector<int32_t> tris;
  int p() const { return (int)pts.size() / 2; }
  int t() const { return (int)tris.size() / 3; }
  void tri(int a, int b, int c) {  // stored positively oriented
    const double ar = (pts[2 * b] - pts[2 * a]) * (pts[2 * c + 1] - pts[2 * a + 1]) -
                      (pts[2 * b + 1] - pts[2 * a + 1]) * (pts[2 * c] - pts[2 * a]);
    tris.push_back(a);
    tris.push_back(ar >= 0 ? b : c);
    tris.push_back(ar >= 0 ? c : b);
  }
};

// an n x n grid of points over [0,w-1] x [0,h-1], interior points jittered by `jit` of a cell, two triangles per cell
static Mesh grid_mesh(int n, int h, int w, double jit) {
  Mesh m;
  for (int j = 0; j < n; ++j)
    for (int i = 0; i < n; ++i) {
      const bool inner = i > 0 && j > 0 && i < n - 1 && j < n - 1;
      const double cx = (double)(w - 1) / (n - 1), cy = (double)(h - 1) / (n - 1);
      m.pts.push_back(i * cx + (inner ? uniform(-jit, jit) * cx : 0.0));
      m.pts.push_back(j * cy + (inner ? uniform(-jit, jit) * cy : 0.0));
    }
  for (int j = 0; j + 1 < n; ++j)
    for (int i = 0; i + 1 < n; ++i) {
      const int a = j * n + i, b = a + 1, c = a + n, d = c + 1;
      if (uniform() < 0.5) { m.tri(a, b, d); m.tri(a, d, c); }
      else { m.tri(a, b, c); m.tri(b, d, c); }
    }
  return m;
}

static void check_map(const char* what, const Mesh& m, int h, int w, long long* holes = nullptr) {
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x) {
      const int got = flm::mesh_locate(m.pts.data(), m.tris.data(), m.p(), m.t(), (double)x, (double)y);
      const int want = locate_ref(m.pts, m.tris, x, y);
      CHECK(got == want, "%s: map(%d,%d) = %d, restatement %d", what, x, y, got, want);
      if (holes && got == 255) ++*holes;
    }
}

static void map_tests() {
  for (int rep = 0; rep < 24; ++rep) {
    const int n = 3 + rep % 9, h = 16 + (int)(uniform() * 100), w = 16 + (int)(uniform() * 100);
    const Mesh m = grid_mesh(n, h, w, 0.35);
    long long holes = 0;
    check_map("seeded", m, h, w, &holes);
    CHECK(holes == 0, "seeded mesh %d leaves %lld pixels uncovered", rep, holes);
  }
  // exact coordinates: a 3 x 3 grid at 0, 8, 16 -- every pixel on a row, column or diagonal through grid points lies on
  // an edge shared by two triangles, the grid points themselves on a vertex shared by up to eight: the lowest wins
  Mesh g = grid_mesh(3, 17, 17, 0.0);
  check_map("exact", g, 17, 17);
  for (int y = 0; y <= 16; y += 8)
    for (int x = 0; x <= 16; x += 8) {
      int lowest = 255;
      for (int i = g.t() - 1; i >= 0; --i)
        for (int j = 0; j < 3; ++j)
          if (g.tris[3 * i + j] == (y / 8) * 3 + x / 8) lowest = i;
      const int got = flm::mesh_locate(g.pts.data(), g.tris.data(), g.p(), g.t(), x, y);
      CHECK(got == lowest, "shared vertex (%d,%d): %d, lowest triangle with that vertex %d", x, y, got, lowest);
    }
  {  // the edge between the first cell's two triangles: both hold its midpoint, triangle 0 wins; past it, triangle 1
    const int got = flm::mesh_locate(g.pts.data(), g.tris.data(), g.p(), g.t(), 4.0, 4.0);
    const int share0 = flm::mesh_locate(g.pts.data(), g.tris.data() + 3, g.p(), g.t() - 1, 4.0, 4.0);
    CHECK(got == 0 && share0 == 0, "shared edge midpoint: %d with, %d without triangle 0", got, share0);
  }
  // a hole: without triangle 0 its interior has no triangle, its edges still belong to the neighbours
  Mesh hole = g;
  hole.tris.erase(hole.tris.begin(), hole.tris.begin() + 3);
  long long holes = 0;
  check_map("hole", hole, 17, 17, &holes);
  CHECK(holes > 0, "dropping a triangle leaves no hole");
  // an index outside the mesh is skipped, never read
  Mesh bad = g;
  bad.tris[1] = bad.p();
  bad.tris[4] = -1;
  check_map("bad index", bad, 17, 17);
  float o[6];
  const float mm[6] = {1.5f, -0.25f, 3.f, 0.25f, 1.5f, -7.f};
  std::vector<double> lm(2 * bad.p(), 1.0);
  flm::mesh_face_affine(lm.data(), 2, mm, bad.pts.data(), bad.tris.data(), bad.p(), 0, kMinDet, o);
  CHECK(std::memcmp(o, mm, sizeof o) == 0, "a triangle with an index outside the mesh does not take M");
}

// ---- affines --------------------------------------------------------------------------------------------------------
static void check_face(const char* what, const Mesh& mesh, int a, const std::vector<double>& lm, int lm_stride,
                       const float* m, double min_det, int expect_fallback /* -1: whatever the restatement says */) {
  const int c = mesh.p() - a;
  std::vector<double> dense(2 * (size_t)c);
  for (int i = 0; i < c; ++i) {
    dense[2 * i] = lm[(size_t)i * lm_stride];
    dense[2 * i + 1] = lm[(size_t)i * lm_stride + 1];
  }
  for (int t = 0; t < mesh.t(); ++t) {
    float got[6];
    flm::mesh_face_affine(lm.data(), lm_stride, m, mesh.pts.data(), mesh.tris.data() + 3 * t, mesh.p(), a, min_det, got);
    const RefAffine r = affine_ref(dense, m, mesh.pts, c, mesh.tris.data() + 3 * t, min_det);
    const bool is_m = std::memcmp(got, m, sizeof got) == 0;
    if (expect_fallback == 1) CHECK(r.fallback && is_m, "%s: triangle %d does not take the fallback (det %Lg)", what, t, r.det);
    if (fabsl(fabsl(r.det) - (ld)min_det) <= 1e-12L * (ld)min_det) {  // on the threshold: either branch
      ++checks;
      continue;
    }
    if (expect_fallback == 0) CHECK(!r.fallback, "%s: triangle %d falls back (det %Lg)", what, t, r.det);
    if (r.fallback) {
      CHECK(is_m, "%s: triangle %d: det %Lg is below min_det but the matrix is not M", what, t, r.det);
      continue;
    }
    for (int i = 0; i < 6; ++i)
      CHECK(ulps(got[i], r.a[i]) <= 1, "%s: triangle %d element %d: %.9g, restatement %.9Lg (%lld ULP)", what, t, i,
            (double)got[i], r.a[i], ulps(got[i], r.a[i]));
  }
}

static void similarity(double scale, double theta, double cx, double cy, int h, int w, float m[6]) {
  const double ca = scale * std::cos(theta), sa = scale * std::sin(theta);
  m[0] = (float)ca; m[1] = (float)-sa; m[2] = (float)((w - 1) / 2.0 - (ca * cx - sa * cy));
  m[3] = (float)sa; m[4] = (float)ca;  m[5] = (float)((h - 1) / 2.0 - (sa * cx + ca * cy));
}

// landmarks = M^-1 of the template plus `noise` frame pixels, lm_stride elements apart (the gaps hold NaN)
static std::vector<double> face_landmarks(const Mesh& mesh, int a, const float* m, double noise, int lm_stride) {
  const int c = mesh.p() - a;
  std::vector<double> lm((size_t)c * lm_stride + 2, NAN);
  for (int i = 0; i < c; ++i) {
    double sx, sy;
    flm::mesh_anchor_source(m, mesh.pts[2 * i], mesh.pts[2 * i + 1], sx, sy);
    lm[(size_t)i * lm_stride] = sx + uniform(-noise, noise);
    lm[(size_t)i * lm_stride + 1] = sy + uniform(-noise, noise);
  }
  return lm;
}

static void affine_tests() {
  const int h = 112, w = 112;
  for (int rep = 0; rep < 200; ++rep) {
    const int n = 3 + rep % 7;
    const Mesh mesh = grid_mesh(n, h, w, 0.3);
    const int a = rep % 3 == 0 ? 0 : 4 * (n - 1);  // with anchors: the last points (the top row of the grid and more)
    float m[6];
    const double scale = rep % 2 ? uniform(0.05, 0.4) : uniform(0.4, 2.5);
    similarity(scale, uniform(-3.1, 3.1), uniform(100, 1800), uniform(100, 1000), h, w, m);
    const int stride = rep % 4 == 1 ? 6 : 2;
    const std::vector<double> lm = face_landmarks(mesh, a, m, 1.5 / scale * 0.15, stride);
    check_face("seeded", mesh, a, lm, stride, m, kMinDet, 0);
  }
  // extremes, on a tiny mesh: 4 landmarks (a square) + 4 corner anchors
  Mesh tiny;
  const double sq[8][2] = {{30, 30}, {81, 30}, {81, 81}, {30, 81}, {0, 0}, {111, 0}, {111, 111}, {0, 111}};
  for (auto& q : sq) { tiny.pts.push_back(q[0]); tiny.pts.push_back(q[1]); }
  tiny.tri(0, 1, 2); tiny.tri(0, 2, 3); tiny.tri(4, 5, 0); tiny.tri(5, 1, 0); tiny.tri(5, 6, 1); tiny.tri(6, 7, 2);
  Mesh lmonly;  // the two triangles made of landmarks alone
  lmonly.pts = tiny.pts;
  lmonly.tri(0, 1, 2); lmonly.tri(0, 2, 3);
  float m[6];
  similarity(0.25, 0.3, 900, 500, h, w, m);
  std::vector<double> lm = face_landmarks(tiny, 4, m, 0.0, 2);
  check_face("rigid", tiny, 4, lm, 2, m, kMinDet, 0);
  {  // collapsed: all four landmarks one point -> the landmark-only triangles fall back
    std::vector<double> c(8);
    for (int i = 0; i < 4; ++i) { c[2 * i] = 640.25; c[2 * i + 1] = 360.5; }
    check_face("collapsed", lmonly, 4, c, 2, m, kMinDet, 1);
    check_face("collapsed, whole mesh", tiny, 4, c, 2, m, kMinDet, -1);
  }
  {  // collinear, on exactly representable coordinates: det = 0 exactly
    const std::vector<double> c = {100, 200, 150, 250, 200, 300, 250, 350};
    check_face("collinear", lmonly, 4, c, 2, m, kMinDet, 1);
  }
  for (int bad = 0; bad < 8; ++bad) {  // one NaN coordinate: every triangle that reads it falls back, the others do not care
    std::vector<double> c = lm;
    c[bad] = NAN;
    check_face("NaN", tiny, 4, c, 2, m, kMinDet, -1);
    Mesh one;
    one.pts = tiny.pts;
    one.tri(bad / 2, (bad / 2 + 1) % 4, (bad / 2 + 2) % 4);
    check_face("NaN, its triangle", one, 4, c, 2, m, kMinDet, 1);
  }
  {  // coordinates at 0 and 2^15
    const std::vector<double> c = {0, 0, 32768, 0, 32768, 32768, 0, 32768};
    float big[6] = {112.f / 32768.f, 0.f, 0.f, 0.f, 112.f / 32768.f, 0.f};
    check_face("0 and 2^15", lmonly, 4, c, 2, big, kMinDet, 0);
    check_face("0 and 2^15, whole mesh", tiny, 4, c, 2, big, kMinDet, -1);  // the corner anchors meet landmarks
    const std::vector<double> z = {0, 0, 1, 0, 1, 1, 0, 1};
    // (a power-of-two scale: the anchors' M^-1 images are exact, so the elements that are 0 by symmetry are 0 in both
    // computations; with a scale of 51 they are residues of 1e-14 against an exact 0, where a float32 ULP of the element
    // measures nothing)
    float unit[6] = {64.f, 0.f, 30.f, 0.f, 64.f, 30.f};
    check_face("0 and 1", lmonly, 4, z, 2, unit, kMinDet, 0);
    check_face("0 and 1, whole mesh", tiny, 4, z, 2, unit, kMinDet, -1);
  }
  {  // det on either side of min_det and on it: a right triangle of legs e: det = e*e
    for (double det : {0.25e-6, 0.999999e-6, 1e-6, 1.000001e-6, 4e-6}) {
      const double e = std::sqrt(det);
      const std::vector<double> c = {500, 500, 500 + e, 500, 500 + e, 500 + e, 500, 500 + e};
      check_face("threshold", lmonly, 4, c, 2, m, kMinDet, -1);
    }
    const std::vector<double> c = {500, 500, 500.5, 500, 500.5, 500.5, 500, 500.5};
    check_face("min_det = 0", lmonly, 4, c, 2, m, 0.0, 0);
    check_face("min_det = 1", lmonly, 4, c, 2, m, 1.0, 1);
  }
}

int main() {
  map_tests();
  affine_tests();
  std::printf("%lld checks, %lld failures\n", checks, failures);
  return failures ? 1 : 0;
}
