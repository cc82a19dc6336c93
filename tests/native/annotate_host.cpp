// The integer pieces of flm_frames_annotate on the host: csrc/flm_annotate_dev.h -- the header the kernels of
// csrc/flm_annotate.hip and flm_bgr_to_yuv are built from -- against plain restatements of the contract of include/flm.h
// written in this file: the colour conversion over all 2^24 colours and both matrices (and its round trip through
// nv12_to_bgr of csrc/flm_nv12_dev.h), the region of a face at the extremes of the contract, the cell range of a region
// and the ownership predicate over every pair of small boxes on a small grid, and the disc.  Built with the host's
// address and undefined-behaviour sanitizers; nothing here runs on a GPU.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "flm_annotate_dev.h"
#include "flm_nv12_dev.h"

namespace {

int g_failures = 0;
long long g_checks = 0;
#define CHECK(cond, ...)                                 \
  do {                                                   \
    ++g_checks;                                          \
    if (!(cond)) {                                       \
      if (++g_failures <= 20) {                          \
        std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
        std::printf(__VA_ARGS__);                        \
        std::printf("\n");                               \
      }                                                  \
    }                                                    \
  } while (0)

const double kNaN = std::numeric_limits<double>::quiet_NaN();
const double kInf = std::numeric_limits<double>::infinity();
const double kLim = 1073741824.0;

// ---- the colour conversion ------------------------------------------------------------------------------------------------
// round(exact x 2^16) of the limited-range forward matrix from Kr and Kb, in long double; rows Y, U, V over (B, G, R)
void ref_coef(int matrix, long long c[3][3]) {
  const long double kr = matrix == FLM_YUV_BT709_LIMITED ? 0.2126L : 0.299L;
  const long double kb = matrix == FLM_YUV_BT709_LIMITED ? 0.0722L : 0.114L;
  const long double kg = 1.0L - kr - kb, ys = 219.0L / 255.0L * 65536.0L, cs = 224.0L / 255.0L * 65536.0L;
  const long double m[3][3] = {{kb * ys, kg * ys, kr * ys},
                               {0.5L * cs, -kg / (2.0L * (1.0L - kb)) * cs, -kr / (2.0L * (1.0L - kb)) * cs},
                               {-kb / (2.0L * (1.0L - kr)) * cs, -kg / (2.0L * (1.0L - kr)) * cs, 0.5L * cs}};
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) c[i][j] = std::llroundl(m[i][j]);
}

long long floor_shift16(long long a) {  // floor(a / 65536) without shifting a negative number
  return a >= 0 ? a / 65536 : -((-a + 65535) / 65536);
}

void sweep_colours() {
  int worst = 0;
  for (int matrix = 0; matrix < 2; ++matrix) {
    long long c[3][3];
    ref_coef(matrix, c);
    const flm::AnnotYuvCoef k = flm::annot_yuv_coef(matrix);
    for (int j = 0; j < 3; ++j)
      CHECK(k.y[j] == c[0][j] && k.u[j] == c[1][j] && k.v[j] == c[2][j], "matrix %d: coefficient column %d", matrix, j);
    const flm::Nv12Coef back = flm::nv12_coef(matrix);
    for (int v = 0; v < (1 << 24); ++v) {
      const uint8_t bgr[3] = {(uint8_t)(v & 255), (uint8_t)((v >> 8) & 255), (uint8_t)(v >> 16)};
      uint8_t yuv[3];
      flm::annot_bgr_to_yuv(matrix, bgr, yuv);
      long long want[3];
      for (int i = 0; i < 3; ++i) {
        const long long acc = c[i][0] * bgr[0] + c[i][1] * bgr[1] + c[i][2] * bgr[2] + 32768;
        const long long lo = 16, hi = i == 0 ? 235 : 240;
        want[i] = std::min(std::max((i == 0 ? 16 : 128) + floor_shift16(acc), lo), hi);
      }
      CHECK(yuv[0] == want[0] && yuv[1] == want[1] && yuv[2] == want[2], "matrix %d colour %06x: (%d,%d,%d) != (%lld,%lld,%lld)",
            matrix, v, yuv[0], yuv[1], yuv[2], want[0], want[1], want[2]);
      int rt[3];
      flm::nv12_to_bgr(yuv[0], yuv[1], yuv[2], back, rt);
      for (int i = 0; i < 3; ++i) worst = std::max(worst, std::abs(rt[i] - (int)bgr[i]));
    }
  }
  std::printf("round trip through nv12_to_bgr: worst |difference| per channel = %d\n", worst);
  CHECK(worst <= 2, "round trip differs by %d > 2", worst);
}

// ---- regions --------------------------------------------------------------------------------------------------------------
struct Pt {
  double x, y;
};

// the contract, visited in REVERSE order with the library's min / max
void ref_region(const std::vector<Pt>& pts, const double m[4], int out[4]) {
  bool any = false;
  double mnx = 0, mny = 0, mxx = 0, mxy = 0;
  for (size_t i = pts.size(); i-- > 0;) {
    const double x = pts[i].x, y = pts[i].y;
    if (!(x >= 0.0 && y >= 0.0 && x <= kLim && y <= kLim)) continue;
    if (!any) { mnx = mxx = x; mny = mxy = y; any = true; continue; }
    mnx = std::fmin(mnx, x); mny = std::fmin(mny, y); mxx = std::fmax(mxx, x); mxy = std::fmax(mxy, y);
  }
  if (!any) { out[0] = out[1] = out[2] = out[3] = 0; return; }
  const double side = std::fmax(mxx - mnx, mxy - mny);
  volatile double p0 = m[0] * side, p1 = m[1] * side, p2 = m[2] * side, p3 = m[3] * side;  // (one rounding each)
  const double v[4] = {std::floor(mnx - p0), std::floor(mny - p1), std::ceil(mxx + p2) + 1.0, std::ceil(mxy + p3) + 1.0};
  for (int i = 0; i < 4; ++i) out[i] = (int)std::fmin(std::fmax(v[i], -kLim), kLim);
}

// the header's functions as the kernel uses them: 64 partial extents joined by a butterfly
flm::AnnotBox dev_region(const std::vector<Pt>& pts, const double m[4]) {
  flm::AnnotExtent lane[64];
  for (int l = 0; l < 64; ++l) {
    lane[l] = flm::annot_extent_empty();
    for (size_t i = l; i < pts.size(); i += 64) flm::annot_extent_add(lane[l], pts[i].x, pts[i].y);
  }
  for (int o = 32; o; o >>= 1) {
    flm::AnnotExtent next[64];
    for (int l = 0; l < 64; ++l) {
      next[l] = lane[l];
      flm::annot_extent_merge(next[l], lane[l ^ o]);
    }
    std::memcpy(lane, next, sizeof(lane));
  }
  return flm::annot_region(lane[0], m);
}

void check_region(const std::vector<Pt>& pts, const double m[4], const int* want, const char* what) {
  int ref[4];
  ref_region(pts, m, ref);
  const flm::AnnotBox r = dev_region(pts, m);
  CHECK(r.x0 == ref[0] && r.y0 == ref[1] && r.x1 == ref[2] && r.y1 == ref[3], "%s: (%d,%d,%d,%d) != restatement (%d,%d,%d,%d)",
        what, r.x0, r.y0, r.x1, r.y1, ref[0], ref[1], ref[2], ref[3]);
  if (want)
    CHECK(r.x0 == want[0] && r.y0 == want[1] && r.x1 == want[2] && r.y1 == want[3], "%s: (%d,%d,%d,%d) != by hand (%d,%d,%d,%d)",
          what, r.x0, r.y0, r.x1, r.y1, want[0], want[1], want[2], want[3]);
}

void sweep_regions() {
  const double m0[4] = {0, 0, 0, 0}, m4[4] = {4, 4, 4, 4}, md[4] = {0.1, 0.35, 0.1, 0.1};
  const int L = 1 << 30;
  { const int w[4] = {5, 7, 7, 9}; check_region({{5.5, 7.25}}, m0, w, "one point"); check_region({{5.5, 7.25}}, m4, w, "one point, margin 4"); }
  { const int w[4] = {0, 0, 1, 1}; check_region({{0.0, 0.0}}, m4, w, "the origin"); check_region({{-0.0, -0.0}}, md, w, "minus zero"); }
  { const int w[4] = {-L, -L, L, L}; check_region({{0.0, 0.0}, {kLim, kLim}}, m4, w, "the whole range, margin 4"); }
  { const int w[4] = {0, 0, L, L}; check_region({{kLim, kLim}, {0.0, 0.0}}, m0, w, "the whole range, margin 0"); }
  { const int w[4] = {L, L, L, L}; check_region({{kLim, kLim}}, m0, w, "one point at 2^30"); }
  { const int w[4] = {0, 0, 0, 0};
    check_region({}, md, w, "no point");
    check_region({{-1.0, -1.0}, {kNaN, 1.0}, {1.0, kNaN}, {kInf, 1.0}, {1.0, -kInf}, {kLim + 1.0, 3.0}, {3.0, kLim * 2.0},
                  {-1e-300, 4.0}, {kNaN, kNaN}}, md, w, "every point rejected"); }
  { const int w[4] = {3, 4, 4, 5}; check_region({{kNaN, 0.0}, {3.0, 4.0}, {-1.0, -1.0}, {kInf, kInf}}, md, w, "one accepted among rejected"); }
  { const int w[4] = {8, 3, 33, 23}; check_region({{10.0, 10.0}, {30.0, 20.0}, {-1.0, -1.0}}, md, w, "the default margins"); }
  // -0.0 and 0.0 mixed, in both orders: the int32 region does not depend on the zero the minimum keeps
  { const int w[4] = {-1, -2, 7, 4}; check_region({{-0.0, 0.0}, {0.0, -0.0}, {5.0, 2.0}}, md, w, "zeros a"); check_region({{0.0, -0.0}, {5.0, 2.0}, {-0.0, 0.0}}, md, w, "zeros b"); }
  // seeded faces of 1 .. 200 points, a share of them rejected, margins at random in [0, 4]
  uint64_t s = 0x9E3779B97F4A7C15ull;
  auto rnd = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (double)(s >> 11) / 9007199254740992.0; };
  for (int it = 0; it < 20000; ++it) {
    const int c = 1 + (int)(rnd() * 200);
    const double scale = it % 3 == 0 ? kLim : it % 3 == 1 ? 2000.0 : 3.0;
    std::vector<Pt> pts(c);
    for (auto& p : pts) {
      p.x = rnd() * scale; p.y = rnd() * scale;
      const double r = rnd();
      if (r < 0.1) p.x = p.y = -1.0; else if (r < 0.13) p.x = kNaN; else if (r < 0.16) p.y = kInf; else if (r < 0.2) p.x = std::floor(p.x);
    }
    const double m[4] = {rnd() * 4, rnd() * 4, it % 7 ? rnd() * 4 : 0.0, it % 5 ? rnd() : 4.0};
    check_region(pts, m, nullptr, "seeded");
  }
}

// ---- cells and ownership --------------------------------------------------------------------------------------------------
void sweep_ownership() {
  const int fw = 8, fh = 4, s = 2, nframes = 2;
  const int xs[] = {-1, 0, 1, 2, 3, 5, 7, 8, 9}, ys[] = {-1, 0, 1, 2, 3, 4, 5};
  std::vector<flm::AnnotBox> boxes;
  for (int x0 : xs) for (int x1 : xs) for (int y0 : ys) for (int y1 : ys)
    if (x0 <= x1 && y0 <= y1) boxes.push_back(flm::AnnotBox{x0, y0, x1, y1});
  auto inside = [&](const flm::AnnotBox& r, int x, int y) { return x >= r.x0 && x < r.x1 && y >= r.y0 && y < r.y1; };
  auto touches = [&](const flm::AnnotBox& r, int cx, int cy) {  // by pixels: some pixel of the cell, inside the frame, lies in R
    for (int y = cy * s; y < std::min((cy + 1) * s, fh); ++y)
      for (int x = cx * s; x < std::min((cx + 1) * s, fw); ++x)
        if (inside(r, x, y)) return true;
    return false;
  };
  auto takes_part = [&](const flm::AnnotBox& r, int fi) {
    if (fi < 0 || fi >= nframes) return false;
    for (int y = 0; y < fh; ++y)
      for (int x = 0; x < fw; ++x)
        if (inside(r, x, y)) return true;
    return false;
  };
  // the cell range of every box against the pixels
  for (const auto& b : boxes) {
    const flm::AnnotBox p = flm::annot_clip(b, fw, fh);
    CHECK(flm::annot_empty(p) == !takes_part(b, 0), "empty (%d,%d,%d,%d)", b.x0, b.y0, b.x1, b.y1);
    if (flm::annot_empty(p)) continue;
    const flm::AnnotBox c = flm::annot_cells(p, s);
    for (int cy = 0; cy < fh / s; ++cy)
      for (int cx = 0; cx < fw / s; ++cx)
        CHECK(flm::annot_cell_in(c, cx, cy) == touches(b, cx, cy), "cells of (%d,%d,%d,%d) at (%d,%d)", b.x0, b.y0, b.x1, b.y1, cx, cy);
  }
  const int frames_j[] = {0, 1, -1, 2};
  for (size_t a = 0; a < boxes.size(); ++a)
    for (size_t b = 0; b < boxes.size(); ++b)
      for (int fj : frames_j) {
        const int32_t reg[8] = {boxes[a].x0, boxes[a].y0, boxes[a].x1, boxes[a].y1, boxes[b].x0, boxes[b].y0, boxes[b].x1, boxes[b].y1};
        const int32_t idx[2] = {fj, 0};
        for (int cy = 0; cy < fh / s; ++cy)
          for (int cx = 0; cx < fw / s; ++cx) {
            const bool lower = takes_part(boxes[a], fj) && touches(boxes[a], cx, cy);
            const bool own1 = takes_part(boxes[b], 0) && touches(boxes[b], cx, cy) && !(lower && fj == 0);
            CHECK(flm::annot_owns(reg, idx, nframes, fw, fh, s, 1, cx, cy) == own1, "owner of (%d,%d): boxes %zu, %zu, frame %d", cx, cy, a, b, fj);
            if (b == 0) CHECK(flm::annot_owns(reg, idx, nframes, fw, fh, s, 0, cx, cy) == lower, "face 0 at (%d,%d): box %zu, frame %d", cx, cy, a, fj);
          }
      }
  // a NULL frame index is slot 0; three faces: the lowest of those that touch the cell owns it
  const int32_t reg3[12] = {4, 0, 8, 4, 2, 0, 6, 2, 0, 0, 8, 4};
  for (int cy = 0; cy < 2; ++cy)
    for (int cx = 0; cx < 4; ++cx) {
      int owner = -1;
      for (int f = 2; f >= 0; --f)
        if (touches(flm::AnnotBox{reg3[4 * f], reg3[4 * f + 1], reg3[4 * f + 2], reg3[4 * f + 3]}, cx, cy)) owner = f;
      for (int f = 0; f < 3; ++f)
        CHECK(flm::annot_owns(reg3, nullptr, 1, fw, fh, s, f, cx, cy) == (f == owner), "three faces at (%d,%d), face %d", cx, cy, f);
    }
}

void check_disc() {
  bool seen[5][5] = {};
  for (int o = 0; o < flm::kAnnotDisc; ++o) {
    int dx = 9, dy = 9;
    flm::annot_disc_offset(o, &dx, &dy);
    CHECK(dx >= -2 && dx <= 2 && dy >= -2 && dy <= 2 && dx * dx + dy * dy <= 5, "offset %d = (%d,%d)", o, dx, dy);
    if (dx >= -2 && dx <= 2 && dy >= -2 && dy <= 2) {
      CHECK(!seen[dy + 2][dx + 2], "offset %d repeats (%d,%d)", o, dx, dy);
      seen[dy + 2][dx + 2] = true;
    }
  }
  int n = 0;
  for (int dy = -2; dy <= 2; ++dy)
    for (int dx = -2; dx <= 2; ++dx)
      if (dx * dx + dy * dy <= 5) { ++n; CHECK(seen[dy + 2][dx + 2], "(%d,%d) missing", dx, dy); }
  CHECK(n == 21 && flm::kAnnotDisc == 21, "the disc has %d pixels", n);
}

}  // namespace

int main() {
  check_disc();
  sweep_regions();
  sweep_ownership();
  sweep_colours();
  std::printf("annotate_host: %lld checks, %d failures\n", g_checks, g_failures);
  return g_failures ? 1 : 0;
}
