// Host sweep of csrc/flm_track_assoc_dev.h, the integer pieces flm_track_associate's kernel is built from: the box maths,
// the clip, the area, the intersection, the threshold test and the order of pairs, over boxes at the extremes of the
// contract -- coordinates at +-2^28 (any int32 for the clip), frames of 1 x 2^30, 2^30 x 1 and 32768 x 32768, empty,
// inverted and one-pixel boxes -- each result against a restatement in __int128 / long double.  Built with the host's
// undefined-behaviour sanitizer, so a signed overflow inside the header ends the program: this is where one is caught.
// No GPU call is made.
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "flm_track_assoc_dev.h"

typedef __int128 i128;
using flm::AssocBox;

static long long failures = 0, checks = 0;
#define CHECK(cond, ...)                                   \
  do {                                                     \
    ++checks;                                              \
    if (!(cond)) {                                         \
      if (++failures <= 20) { std::printf(__VA_ARGS__); std::printf("\n"); } \
    }                                                      \
  } while (0)

static i128 mn(i128 a, i128 b) { return a < b ? a : b; }
static i128 mx(i128 a, i128 b) { return a > b ? a : b; }
static i128 ab(i128 a) { return a < 0 ? -a : a; }

struct Box128 {
  i128 x0, y0, x1, y1;
};
static Box128 wide(const AssocBox& b) { return Box128{b.x0, b.y0, b.x1, b.y1}; }
static bool same(const AssocBox& a, const Box128& b) { return a.x0 == b.x0 && a.y0 == b.y0 && a.x1 == b.x1 && a.y1 == b.y1; }

// include/flm.h, "association", item 2: |h| * 0.1 truncated is |h| / 10 for every |h| <= 2^29 (the double 0.1 exceeds
// a tenth by 5.6e-18 of it and the product's rounding by 2^-53 of it: 1e-8 at most, against a distance of 0.1 to the
// next integer wherever the quotient is not one itself)
static Box128 square_ref(Box128 b) {
  const i128 off = ab(b.y1 - b.y0) / 10;
  b.y0 += off;
  b.y1 += off;
  const i128 diff = (b.y1 - b.y0) - (b.x1 - b.x0), delta = ab(diff) / 2, odd = ab(diff) % 2;
  if (diff > 0) { b.x0 -= delta; b.x1 += delta + odd; }
  if (diff < 0) { b.y0 -= delta; b.y1 += delta + odd; }
  return b;
}
static Box128 clip_ref(const Box128& b, int fh, int fw) {
  return Box128{mn(mx(b.x0, 0), fw), mn(mx(b.y0, 0), fh), mn(mx(b.x1, 0), fw), mn(mx(b.y1, 0), fh)};
}
static bool empty_ref(const Box128& c) { return c.x1 - c.x0 <= 0 || c.y1 - c.y0 <= 0; }
static i128 area_ref(const Box128& c) { return (c.x1 - c.x0) * (c.y1 - c.y0); }
static i128 inter_ref(const Box128& a, const Box128& b) {
  const i128 w = mn(a.x1, b.x1) - mx(a.x0, b.x0), h = mn(a.y1, b.y1) - mx(a.y0, b.y0);
  return (w <= 0 || h <= 0) ? 0 : w * h;
}

static std::vector<int> coords(int hi, bool any_int32) {
  const int L = flm::kAssocCoordLimit;
  std::vector<int> v = {-L, -L + 1, -1000, -1, 0, 1, 2, 97, hi / 2, hi - 1, hi, hi + 1, L - 1, L};
  if (any_int32) {
    v.push_back(INT_MIN);
    v.push_back(INT_MIN + 1);
    v.push_back(INT_MAX - 1);
    v.push_back(INT_MAX);
  }
  return v;
}

static void sweep_boxes(int fh, int fw) {
  // every 4-tuple of the extremes: the range test, the box maths, the clip, the area
  for (int pass = 0; pass < 2; ++pass) {
    const std::vector<int> xs = coords(fw, pass == 1), ys = coords(fh, pass == 1);
    for (int x0 : xs) for (int y0 : ys) for (int x1 : xs) for (int y1 : ys) {
      const AssocBox b{x0, y0, x1, y1};
      const i128 L = flm::kAssocCoordLimit;
      const bool in = ab(x0) <= L && ab(y0) <= L && ab(x1) <= L && ab(y1) <= L;
      CHECK(flm::assoc_in_range(b) == in, "in_range %d %d %d %d", x0, y0, x1, y1);
      AssocBox q = b;
      if (in) {
        q = flm::assoc_square(b);
        const Box128 e = square_ref(wide(b));
        CHECK(same(q, e), "square %d %d %d %d -> %d %d %d %d", x0, y0, x1, y1, q.x0, q.y0, q.x1, q.y1);
        CHECK((q.x1 - (i128)q.x0) == (q.y1 - (i128)q.y0), "not square %d %d %d %d", x0, y0, x1, y1);
      }
      for (const AssocBox& s : {b, q}) {   // (the clip takes any int32: a track's box is whatever the caller left there)
        const AssocBox c = flm::assoc_clip(s, fh, fw);
        const Box128 e = clip_ref(wide(s), fh, fw);
        CHECK(same(c, e), "clip %d %d %d %d", s.x0, s.y0, s.x1, s.y1);
        CHECK(flm::assoc_empty(c) == empty_ref(e), "empty %d %d %d %d", s.x0, s.y0, s.x1, s.y1);
        if (!empty_ref(e)) {
          CHECK((i128)flm::assoc_area(c) == area_ref(e), "area %d %d %d %d", s.x0, s.y0, s.x1, s.y1);
          CHECK(area_ref(e) <= ((i128)1 << 30), "area bound");
        }
      }
    }
  }
}

struct Pair {
  int64_t in, un;
};

static void sweep_pairs(int fh, int fw) {
  // clipped, non-empty boxes from a shorter list of extremes; every pair of them, and every pair of pairs for the order
  const std::vector<int> xs = {-flm::kAssocCoordLimit, -1, 0, 1, fw / 3, fw / 2, fw - 1, fw, flm::kAssocCoordLimit};
  const std::vector<int> ys = {-flm::kAssocCoordLimit, -1, 0, 1, fh / 3, fh / 2, fh - 1, fh, flm::kAssocCoordLimit};
  std::vector<AssocBox> boxes;
  for (int x0 : xs) for (int y0 : ys) for (int x1 : xs) for (int y1 : ys) {
    const AssocBox c = flm::assoc_clip(AssocBox{x0, y0, x1, y1}, fh, fw);
    if (flm::assoc_empty(c)) continue;
    bool seen = false;
    for (const AssocBox& o : boxes) seen = seen || (o.x0 == c.x0 && o.y0 == c.y0 && o.x1 == c.x1 && o.y1 == c.y1);
    if (!seen) boxes.push_back(c);
  }
  const double ts[] = {0.0, 0.25, 0.5, 0.75, 1.0, 2.0, 0.3, 0.7, -1.0, HUGE_VAL, -HUGE_VAL};
  std::vector<Pair> pairs;
  for (const AssocBox& a : boxes) for (const AssocBox& b : boxes) {
    const int64_t in = flm::assoc_inter(a, b);
    const i128 ein = inter_ref(wide(a), wide(b));
    CHECK((i128)in == ein, "inter");
    const int64_t un = flm::assoc_union(flm::assoc_area(a), flm::assoc_area(b), in);
    const i128 eun = area_ref(wide(a)) + area_ref(wide(b)) - ein;
    CHECK((i128)un == eun && eun >= ein && eun <= ((i128)1 << 31), "union");
    for (double t : ts) {
      const bool got = flm::assoc_iou_ge(in, un, t);
      if (t == 0.0 || t == 0.25 || t == 0.5 || t == 0.75 || t == 1.0 || t == 2.0 || t == -1.0) {
        const i128 t4 = (i128)(t * 4.0);   // a dyadic threshold: t * uni is exact, the test is an integer comparison
        CHECK(got == (ein > 0 && ein * 4 >= t4 * eun), "iou_ge %lld %lld %g", (long long)in, (long long)un, t);
      } else if (std::isinf(t)) {
        CHECK(got == (ein > 0 && t < 0), "iou_ge inf");
      } else {                             // 0.3, 0.7: one rounding; away from the tie both sides must agree
        const long double lt = (long double)t * (long double)eun, li = (long double)ein;
        if (fabsl(li - lt) > 1e-9L * lt) CHECK(got == (ein > 0 && li >= lt), "iou_ge %lld %lld %g", (long long)in, (long long)un, t);
      }
    }
    if (in > 0 && (pairs.size() < 600 || un > (1ll << 29))) pairs.push_back(Pair{in, un});
  }
  if (pairs.size() > 1500) pairs.resize(1500);
  for (size_t p = 0; p < pairs.size(); ++p) for (size_t q = 0; q < pairs.size(); ++q) {
    const i128 l = (i128)pairs[p].in * pairs[q].un, r = (i128)pairs[q].in * pairs[p].un;
    CHECK(l < ((i128)1 << 61) && r < ((i128)1 << 61), "product bound");
    const int sp = (int)(p % 3), dp = (int)(p % 5), sq = (int)(q % 3), dq = (int)(q % 5);
    const bool e = l != r ? l > r : sp != sq ? sp < sq : dp < dq;
    CHECK(flm::assoc_before(pairs[p].in, pairs[p].un, sp, dp, pairs[q].in, pairs[q].un, sq, dq) == e, "before %zu %zu", p, q);
  }
  std::printf("frame %dx%d: %zu boxes, %zu overlapping pairs ordered\n", fh, fw, boxes.size(), pairs.size());
}

int main() {
  const int frames[][2] = {{270, 480}, {1, 1 << 30}, {1 << 30, 1}, {32768, 32768}, {1, 1}};
  for (const auto& f : frames) {
    sweep_boxes(f[0], f[1]);
    sweep_pairs(f[0], f[1]);
  }
  // the largest values the order can meet: inter = 2^30 against uni = 2^31
  CHECK(flm::assoc_before(1ll << 30, 1ll << 30, 5, 5, (1ll << 30) - 1, 1ll << 31, 0, 0), "largest products");
  CHECK(!flm::assoc_before((1ll << 30) - 1, 1ll << 31, 0, 0, 1ll << 30, 1ll << 30, 5, 5), "largest products, reversed");
  CHECK(flm::assoc_before(1ll << 30, 1ll << 31, 2, 9, 1ll << 29, 1ll << 30, 3, 0), "tie: the lower slot");
  CHECK(flm::assoc_before(7, 9, 2, 3, 14, 18, 2, 4) && !flm::assoc_before(14, 18, 2, 4, 7, 9, 2, 3), "tie: the lower detection");
  std::printf("%lld checks, %lld failures\n", checks, failures);
  return failures ? 1 : 0;
}
