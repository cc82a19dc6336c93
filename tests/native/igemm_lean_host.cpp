// Host checks of the lean set-up's launcher side (csrc/flm_igemm_args.h): the multiply-shift division against `/`, and
// IgemmArgs::all_taps against the tap masks of every tile worked out pixel by pixel.  No GPU call is made.
#include <cstdio>
#include <cstdlib>

#include "flm_igemm_args.h"

using flm::IgemmArgs;

static int failures = 0;
#define CHECK(cond, ...)                                   \
  do {                                                     \
    if (!(cond)) {                                         \
      if (++failures <= 20) { std::printf(__VA_ARGS__); std::printf("\n"); } \
    }                                                      \
  } while (0)

static void check_div(int d) {
  unsigned magic, shift;
  flm::igemm_fastdiv_make(d, magic, shift);
  CHECK(magic < (1u << 31) || d == 1, "magic of %d does not fit 31 bits", d);
  const long long lim = 1ll << 30;
  auto one = [&](long long n) {
    if (n < 0 || n >= lim) return;
    CHECK(flm::igemm_fastdiv((int)n, magic, shift) == (int)(n / d), "%lld / %d: got %d", n, d, flm::igemm_fastdiv((int)n, magic, shift));
  };
  for (long long n = 0; n < 4096; ++n) one(n);
  for (long long k = 1; k * d < lim; k = k * 3 + 1) { one(k * d - 1); one(k * d); one(k * d + 1); }
  const long long kmax = (lim - 1) / d;
  one(kmax * d - 1); one(kmax * d); one(kmax * d + 1); one(lim - 2); one(lim - 1);
  unsigned long long r = 88172645463325252ull + (unsigned)d;
  for (int i = 0; i < 2000; ++i) { r ^= r << 13; r ^= r >> 7; r ^= r << 17; one((long long)(r % (unsigned long long)lim)); }
}

// does some valid pixel of tile t see tap (ky, kx) in bounds?  Pixel orders as in igemm_kernel (MMAP 0 / 1).
static bool tile_sees_every_tap(const IgemmArgs& a, bool quads, int bm, int t) {
  for (int ky = 0; ky < a.kh; ++ky)
    for (int kx = 0; kx < a.kw; ++kx) {
      bool seen = false;
      for (int m = t * bm; m < (t + 1) * bm && m < a.M && !seen; ++m) {
        int py, px;
        if (quads) {
          const int q = m >> 2, d = m & 3, wp = a.w >> 1, hp = a.h >> 1;
          px = 2 * (q % wp) + (d & 1);
          py = 2 * ((q / wp) % hp) + (d >> 1);
        } else {
          px = (m % a.wo) * a.stride;
          py = ((m / a.wo) % a.ho) * a.stride;
        }
        const int iy = py + ky - a.pad, ix = px + kx - a.pad;
        seen = iy >= 0 && iy < a.h && ix >= 0 && ix < a.w;
      }
      if (!seen) return false;
    }
  return true;
}

int main() {
  for (int d = 1; d <= 1100; ++d) check_div(d);
  for (int l = 10; l <= 30; ++l) { check_div((1 << l) - 1); check_div(1 << l); if (l < 30) check_div((1 << l) + 1); }
  for (int d : {12345, 65537, 1000003, 16777259, 715827883, (1 << 30) - 35}) check_div(d);

  int flagged = 0, flagged_rowmajor = 0, cases = 0, missed = 0;
  const int ks[][3] = {{3, 1, 1}, {3, 1, 2}, {3, 0, 1}, {5, 2, 1}, {7, 3, 2}, {7, 3, 1}, {3, 2, 1}, {1, 0, 2}};  // k, pad, stride
  for (int quads = 0; quads < 2; ++quads)
    for (const auto& k : ks)
      for (int bm : {8, 32, 128})
        for (int n = 1; n <= 3; ++n)
          for (int h = 2; h <= 20; h += (h < 8 ? 1 : 3))
            for (int w = 2; w <= 46; w += (w < 8 ? 1 : 5)) {
              IgemmArgs a = {};
              a.kh = a.kw = k[0]; a.pad = k[1]; a.stride = k[2];
              if (quads && (a.stride != 1 || (h & 1) || (w & 1) || 2 * a.pad + 1 != a.kh)) continue;  // pooled layers: 'same', even maps
              a.n = n; a.h = h; a.w = w;
              a.ho = (h + 2 * a.pad - a.kh) / a.stride + 1;
              a.wo = (w + 2 * a.pad - a.kw) / a.stride + 1;
              if (a.ho < 1 || a.wo < 1) continue;
              a.M = n * a.ho * a.wo;
              a.mtiles = (a.M + bm - 1) / bm;
              flm::igemm_fill_lean(a, quads, bm);
              CHECK(a.dx == (quads ? w / 2 : a.wo) && a.dy == (quads ? h / 2 : a.ho), "grid of the row split");
              bool every = true;
              for (int t = 0; t < a.mtiles && every; ++t) every = tile_sees_every_tap(a, quads, bm, t);
              ++cases;
              if (a.all_taps) {
                ++flagged;
                flagged_rowmajor += !quads;
                CHECK(every, "all_taps claimed but a tile misses a tap: quads %d k %d pad %d stride %d bm %d n %d h %d w %d", quads,
                      k[0], k[1], k[2], bm, n, h, w);
              } else if (every) {
                ++missed;  // (allowed: the kernel then finds the full mask itself)
              }
              if (quads && k[0] == 3 && k[1] == 1) CHECK(a.all_taps, "the pooled 3x3 encoder layers must take the flag (h %d w %d)", h, w);
            }
  CHECK(flagged > 100 && flagged_rowmajor > 20, "the flag is hardly ever set (%d, row-major %d of %d)", flagged, flagged_rowmajor, cases);
  std::printf("%d geometries, all_taps set for %d (row-major %d), not set though true for %d; failures %d\n", cases, flagged,
              flagged_rowmajor, missed, failures);
  return failures ? 1 : 0;
}
