// Host checks of the 64-row tile form's launcher side (csrc/flm_igemm_args.h): tile cover, tile tap masks, the position
// search at 64 rows per tile and the list-schedule model that chooses between 64 and 128 rows.  No GPU call is made.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "flm_igemm_args.h"

using flm::IgemmArgs;

// what the library provides to posmajor_fill_perm: the knob "posmajor_order" (set below) and a cache (none here: every
// call searches afresh)
static int g_posmajor_order = 1;
namespace flm {
int tuning(KnobId id) { return id == KNOB_POSMAJOR_ORDER ? g_posmajor_order : 0; }
bool posperm_cache_get(PospermEntry&) { return false; }
void posperm_cache_put(const PospermEntry&) {}
}  // namespace flm

static int failures = 0;
#define CHECK(cond, ...)                                                     \
  do {                                                                       \
    if (!(cond)) {                                                           \
      if (++failures <= 20) { std::printf(__VA_ARGS__); std::printf("\n"); } \
    }                                                                        \
  } while (0)

// fc6's geometry: 7x7 'same' on a d x d map, n faces, 4096 output channels
static IgemmArgs fc6_args(int n, int d) {
  IgemmArgs a = {};
  a.n = n; a.h = a.w = a.ho = a.wo = d; a.stride = 1;
  a.kh = a.kw = 7; a.pad = 3;
  a.M = n * d * d;
  a.ntiles = 32;
  a.ksplit = 1;
  return a;
}

// taps some valid row of tile t sees in bounds, row by row and tap by tap
static unsigned long long tile_mask_by_pixels(const IgemmArgs& a, int bm, int t) {
  unsigned long long mask = 0ull;
  for (int m = t * bm; m < (t + 1) * bm && m < a.M; ++m) {
    const int pos = flm::posmajor_pos(a, m / a.n), y = pos / a.w, x = pos % a.w;
    for (int ky = 0; ky < a.kh; ++ky)
      for (int kx = 0; kx < a.kw; ++kx) {
        const int iy = y + ky - a.pad, ix = x + kx - a.pad;
        if (iy >= 0 && iy < a.h && ix >= 0 && ix < a.w) mask |= 1ull << (ky * a.kw + kx);
      }
  }
  return mask;
}

// sum over the tiles of |tap mask| x rows issued: what the position search lowers
static long long issued(const IgemmArgs& a, int bm) {
  long long s = 0;
  for (int t = 0; t < (a.M + bm - 1) / bm; ++t) s += (long long)__builtin_popcountll(flm::posmajor_tile_mask(a, bm, t)) * bm;
  return s;
}

int main() {
  int cases = 0, searched = 0;
  for (int d : {2, 4, 8})
    for (int n = 1; n <= 130; ++n)
      for (int bm : {64, 128}) {
        IgemmArgs a = fc6_args(n, d);
        a.mtiles = (a.M + bm - 1) / bm;
        g_posmajor_order = 1;
        flm::posmajor_fill_perm(a, bm);
        ++cases;
        searched += a.posperm_on;
        // every output row (face, position) is written by exactly one row of exactly one tile
        std::vector<int> hits((size_t)a.M, 0);
        for (int t = 0; t < a.mtiles; ++t)
          for (int m = t * bm; m < (t + 1) * bm && m < a.M; ++m) {
            const int pos = flm::posmajor_pos(a, m / a.n), face = m % a.n;
            CHECK(pos >= 0 && pos < d * d, "n %d map %d bm %d: row %d maps to position %d", n, d, bm, m, pos);
            if (pos >= 0 && pos < d * d) ++hits[(size_t)face * d * d + pos];
          }
        for (int o = 0; o < a.M; ++o) CHECK(hits[(size_t)o] == 1, "n %d map %d bm %d: output row %d written %d times", n, d, bm, o, hits[(size_t)o]);
        // the tile masks the model (and the kernel's set-up) work out position by position are the pixel-by-pixel masks
        for (int t = 0; t < a.mtiles; ++t)
          CHECK(flm::posmajor_tile_mask(a, bm, t) == tile_mask_by_pixels(a, bm, t), "n %d map %d bm %d: mask of tile %d", n, d, bm, t);
        // the search is never worse than map order
        IgemmArgs b = fc6_args(n, d);
        b.mtiles = a.mtiles;
        g_posmajor_order = 0;
        flm::posmajor_fill_perm(b, bm);
        CHECK(!b.posperm_on, "knob off but a table is on");
        CHECK(issued(a, bm) <= issued(b, bm), "n %d map %d bm %d: search %lld rows x taps, map order %lld", n, d, bm, issued(a, bm), issued(b, bm));
        if (bm == 64 && n == 64) CHECK(!a.posperm_on, "one position per tile: nothing to choose (map %d)", d);
        if (bm == 64 && n == 32 && d == 8) CHECK(a.posperm_on && issued(a, bm) < issued(b, bm), "two positions per 64-row tile: the search must run and gain");
      }
  g_posmajor_order = 1;

  // the schedule model at the headline shape: 64 faces, 8 x 8 map, 64 resident workgroups per XCD (32 CUs x 2), in half
  // tap-units: 128 rows 69 units (heaviest + lightest pair, 49 + 20), 64 rows at most 62 (the CPU model's 61.5)
  const IgemmArgs h = fc6_args(64, 8);
  const long long m128 = flm::posmajor_makespan(h, 128, 64), m64 = flm::posmajor_makespan(h, 64, 64);
  std::printf("64 faces, 8x8: makespan %.1f tap-units with 128 rows, %.1f with 64\n", 0.5 * (double)m128, 0.5 * (double)m64);
  CHECK(m128 == 2 * 69, "128-row makespan %lld half units, expected 138", m128);
  CHECK(m64 <= 2 * 62, "64-row makespan %lld half units, expected at most 124", m64);
  // useful / issued of the two forms there: 0.955 and 1
  IgemmArgs u = h;
  flm::posmajor_fill_perm(u, 128);
  const long long used = issued(h, 64), padded = issued(u, 128);  // one position per tile: exactly the taps in bounds
  CHECK(used * 1000 >= padded * 954 && used * 1000 <= padded * 956, "128-row union padding: %lld issued for %lld used", padded, used);

  // the choice: 64 rows at the headline shape; 128 rows at 128 faces and more, in split-K launches, and without slots
  CHECK(flm::posmajor_pick_rows(h, 64, 64) == 64, "64 faces 8x8 must take 64 rows");
  CHECK(flm::posmajor_pick_rows(h, 64, 96) == 64, "64 faces 8x8 must take 64 rows with three of them per CU too");
  CHECK(flm::posmajor_pick_rows(fc6_args(128, 2), 64, 64) == 128, "128 faces keep 128 rows");
  CHECK(flm::posmajor_pick_rows(fc6_args(512, 8), 64, 64) == 128, "512 faces keep 128 rows");
  IgemmArgs sk = fc6_args(3, 8);
  sk.ksplit = 8;
  CHECK(flm::posmajor_pick_rows(sk, 64, 64) == 128, "split-K launches keep their form");
  CHECK(flm::posmajor_pick_rows(h, 0, 0) == 128, "no slots: 128 rows");
  int picked64 = 0;
  for (int d : {2, 4, 8})
    for (int n = 17; n < 128; ++n) {
      const int rows = flm::posmajor_pick_rows(fc6_args(n, d), 64, 96);
      CHECK(rows == 64 || rows == 128, "rows %d", rows);
      picked64 += rows == 64;
    }
  std::printf("%d geometries (position search on for %d); 64 rows chosen for %d of %d unsplit batches below 128 faces; %d failures\n",
              cases, searched, picked64, 3 * 111, failures);
  return failures ? 1 : 0;
}
