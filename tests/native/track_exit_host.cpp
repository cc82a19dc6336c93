// The per-slot decision and the row arithmetic of flm_track_retire on the host: csrc/flm_track_exit_dev.h -- the header
// the kernels of csrc/flm_track_exit.hip are built from -- composed the way the decision kernel composes it (count the
// emitted tracks, then rank them and the births by an exclusive prefix over the slots), against a plain serial
// restatement of the contract of include/flm.h written in this file.  Built with the host's address and
// undefined-behaviour sanitizers; nothing here runs on a GPU.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "flm_track_exit_dev.h"

namespace {

int g_failures = 0, g_checks = 0;
#define CHECK(cond, ...)                      \
  do {                                        \
    ++g_checks;                               \
    if (!(cond)) {                            \
      if (++g_failures <= 20) {               \
        std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
        std::printf(__VA_ARGS__);             \
        std::printf("\n");                    \
      }                                       \
    }                                         \
  } while (0)

struct State {
  int k = 0, q = 0, fh = 270, fw = 480;
  std::vector<int32_t> boxes, status, born, exit_row;
  std::vector<double> best_q, x_q;
  std::vector<int64_t> track_id, born_frame, best_frame, x_meta;
  int64_t head[4] = {0, 0, 0, 0};
  State(int k_, int q_) : k(k_), q(q_), boxes(4 * k_, 0), status(k_, 1), born(k_, 0), exit_row(k_, -9), best_q(k_, -1.0),
                          x_q(q_, -7.5), track_id(k_, -1), born_frame(k_, -1), best_frame(k_, -1),
                          x_meta((size_t)q_ * FLM_EXIT_META, -77) {}
};

bool same(const State& a, const State& b) {
  auto eqd = [](const std::vector<double>& x, const std::vector<double>& y) {
    return x.size() == y.size() && (x.empty() || std::memcmp(x.data(), y.data(), x.size() * sizeof(double)) == 0);
  };
  return a.status == b.status && a.born == b.born && a.exit_row == b.exit_row && eqd(a.best_q, b.best_q) && eqd(a.x_q, b.x_q) &&
         a.track_id == b.track_id && a.born_frame == b.born_frame && a.x_meta == b.x_meta &&
         std::memcmp(a.head, b.head, sizeof(a.head)) == 0;
}

// ---- the header's functions, composed as track_exit_decide_kernel composes them --------------------------------------
void retire_dev(State& s, int64_t frame_id, int flush, double min_q) {
  using namespace flm;
  const int64_t seq0 = s.head[0], next_id = s.head[1], disc0 = s.head[2], over0 = s.head[3];
  auto decide = [&](int t) {
    const int32_t* b = &s.boxes[4 * (size_t)t];
    return exit_decide(s.track_id[t], s.born[t], exit_box_live(b[0], b[1], b[2], b[3], s.fh, s.fw), flush, s.best_q[t], min_q,
                       s.status[t]);
  };
  int e_total = 0;
  for (int t = 0; t < s.k; ++t) e_total += decide(t).emitted ? 1 : 0;
  int r = 0, b = 0, n_disc = 0;   // the exclusive prefixes
  for (int t = 0; t < s.k; ++t) {
    const ExitDecision d = decide(t);
    const int32_t row = exit_row_of(d, r, e_total, s.q, seq0);
    const int64_t id = s.track_id[t];
    if (row >= 0) {
      CHECK(row < s.q, "row %d outside the ring of %d", row, s.q);
      exit_meta_store(&s.x_meta[(size_t)row * FLM_EXIT_META], id, t, s.born_frame[t], frame_id, s.best_frame[t], d.end, seq0 + r);
      s.x_q[row] = s.best_q[t];
    }
    s.exit_row[t] = row;
    if (d.birth || d.clears) s.track_id[t] = exit_next_track_id(d, id, b, next_id);
    if (d.birth) s.born_frame[t] = frame_id;
    s.born[t] = 0;
    r += d.emitted ? 1 : 0;
    b += d.birth ? 1 : 0;
    n_disc += (d.ends && !d.emitted) ? 1 : 0;
  }
  exit_head_store(s.head, seq0, next_id, disc0, over0, r, b, n_disc, s.q);
}

// ---- include/flm.h, step by step, with nothing shared ------------------------------------------------------------------
void retire_ref(State& s, int64_t frame_id, int flush, double min_q) {
  const int k = s.k, q = s.q;
  std::vector<char> live(k), born(k), held(k), ends(k), emitted(k);
  for (int t = 0; t < k; ++t) {
    const long long x0 = s.boxes[4 * t], y0 = s.boxes[4 * t + 1], x1 = s.boxes[4 * t + 2], y1 = s.boxes[4 * t + 3];
    auto clip = [](long long v, long long hi) { return v < 0 ? 0 : v > hi ? hi : v; };
    const bool empty = clip(x1, s.fw) - clip(x0, s.fw) <= 0 || clip(y1, s.fh) - clip(y0, s.fh) <= 0;
    live[t] = !empty;                                                          // 1
    born[t] = s.born[t] != 0;
    held[t] = s.track_id[t] >= 0;
    ends[t] = held[t] && (born[t] || !live[t] || flush != 0);                  // 2
    emitted[t] = ends[t] && !std::isnan(s.best_q[t]) && s.best_q[t] >= min_q;  // 3
  }
  const int64_t seq0 = s.head[0], next_id = s.head[1];
  int e = 0;
  for (int t = 0; t < k; ++t) e += emitted[t];
  int r = 0;
  for (int t = 0; t < k; ++t) {                                                // 4, 5
    s.exit_row[t] = -1;
    if (!ends[t]) continue;
    if (!emitted[t]) {
      s.exit_row[t] = -2;
      s.head[2] += 1;
      continue;
    }
    if (r >= e - q) {
      const int row = (int)((seq0 + r) % q);
      s.exit_row[t] = row;
      int64_t* m = &s.x_meta[(size_t)row * 8];
      m[0] = s.track_id[t]; m[1] = t; m[2] = s.born_frame[t]; m[3] = frame_id; m[4] = s.best_frame[t];
      m[5] = born[t] ? -1 : !live[t] ? (int64_t)s.status[t] : -2;
      m[6] = seq0 + r; m[7] = 0;
      s.x_q[row] = s.best_q[t];
    } else {
      s.exit_row[t] = -3;
      s.head[3] += 1;
    }
    ++r;
  }
  s.head[0] = seq0 + e;
  int b = 0;
  for (int t = 0; t < k; ++t) {                                                // 6
    if (born[t] && live[t]) {
      s.track_id[t] = next_id + b++;
      s.born_frame[t] = frame_id;
    } else if (ends[t] || born[t]) {
      s.track_id[t] = -1;
    }
    s.born[t] = 0;
  }
  s.head[1] = next_id + b;
}

const double kNaN = std::numeric_limits<double>::quiet_NaN();

void set_box(State& s, int t, bool live, int variant) {
  static const int32_t dead[6][4] = {{0, 0, 0, 0}, {-40, 10, 0, 60}, {480, 10, 510, 60}, {10, 270, 60, 279}, {50, 50, 50, 90},
                                     {90, 40, 60, 80}};
  static const int32_t alive[4][4] = {{10, 10, 60, 60}, {-5, -5, 1, 1}, {479, 269, 600, 400},
                                      {INT32_MIN, INT32_MIN, INT32_MAX, INT32_MAX}};
  const int32_t* b = live ? alive[variant % 4] : dead[variant % 6];
  for (int i = 0; i < 4; ++i) s.boxes[4 * (size_t)t + i] = b[i];
}

void compare(State& a, const char* what, int64_t frame_id, int flush, double min_q) {
  State b = a;
  retire_dev(a, frame_id, flush, min_q);
  retire_ref(b, frame_id, flush, min_q);
  CHECK(same(a, b), "%s: k=%d q=%d flush=%d min_q=%g differs from the restatement", what, a.k, a.q, flush, min_q);
  for (int t = 0; t < a.k; ++t) CHECK(a.born[t] == 0, "%s: born[%d] not cleared", what, t);
}

// every combination of (held, born, live, flush) x best_q in {-1, below min_q, equal, above, NaN}
void combinations() {
  for (double min_q : {0.0, 0.25, 1.0}) {
    const double qs[5] = {-1.0, min_q > 0 ? min_q * 0.5 : -0.5, min_q, min_q + 0.5, kNaN};
    for (int flush = 0; flush < 2; ++flush) {
      // one slot at a time, with the expectation written out
      for (int held = 0; held < 2; ++held)
        for (int born = 0; born < 2; ++born)
          for (int live = 0; live < 2; ++live)
            for (int qi = 0; qi < 5; ++qi) {
              State s(1, 1);
              s.track_id[0] = held ? 41 : -1;
              s.born[0] = born ? 3 : 0;
              s.best_q[0] = qs[qi];
              s.status[0] = 18;
              s.head[0] = 5; s.head[1] = 9;
              set_box(s, 0, live, qi);
              compare(s, "single", 12, flush, min_q);
              const bool ends = held && (born || !live || flush), emit = ends && (qi == 2 || qi == 3);
              CHECK(s.exit_row[0] == (!ends ? -1 : !emit ? -2 : 0), "single exit_row %d", s.exit_row[0]);
              CHECK(s.head[0] == 5 + (emit ? 1 : 0) && s.head[2] == (ends && !emit ? 1 : 0) && s.head[3] == 0, "single head");
              CHECK(s.track_id[0] == (born && live ? 9 : (ends || born) ? -1 : held ? 41 : -1), "single id %lld",
                    (long long)s.track_id[0]);
              CHECK(s.head[1] == 9 + (born && live ? 1 : 0), "single next_id");
              if (emit) {
                const int64_t end = born ? -1 : !live ? 18 : -2;
                CHECK(s.x_meta[0] == 41 && s.x_meta[1] == 0 && s.x_meta[3] == 12 && s.x_meta[5] == end && s.x_meta[6] == 5 &&
                          s.x_meta[7] == 0, "single meta end=%lld", (long long)s.x_meta[5]);
              } else {
                CHECK(s.x_meta[0] == -77 && s.x_q[0] == -7.5, "single: the ring row must keep its bits");
              }
            }
      // all of them side by side in one call, into rings smaller and larger than E
      for (int q : {1, 3, 7, 64}) {
        State s(40, q);
        int t = 0;
        for (int held = 0; held < 2; ++held)
          for (int born = 0; born < 2; ++born)
            for (int live = 0; live < 2; ++live)
              for (int qi = 0; qi < 5; ++qi, ++t) {
                s.track_id[t] = held ? 100 + t : -1;
                s.born[t] = born;
                s.best_q[t] = qs[qi];
                s.status[t] = 1 + t;
                s.born_frame[t] = 1000 + t;
                s.best_frame[t] = 2000 + t;
                set_box(s, t, live, t);
              }
        s.head[0] = 1234567; s.head[1] = 140; s.head[2] = 3; s.head[3] = 4;
        compare(s, "all", 77, flush, min_q);
        compare(s, "all, again", 78, flush, min_q);   // the births of the first call are held now
      }
    }
  }
}

void seeded() {
  std::mt19937_64 rng(20240607);
  const int ks[] = {1, 2, 63, 64, 65, 200, 1025};
  const int qs[] = {1, 2, 7, 64, 300};
  for (int k : ks)
    for (int q : qs)
      for (int rep = 0; rep < 3; ++rep) {
        State s(k, q);
        s.head[0] = (int64_t)(rng() % 1000);
        s.head[1] = (int64_t)(rng() % 1000);
        const double min_q = rep == 0 ? 0.0 : 0.3;
        const int dead_share = (int)(rng() % 4);   // 0: nearly all live ... 3: most dead
        for (int call = 0; call < 4; ++call) {
          for (int t = 0; t < k; ++t) {
            const unsigned v = (unsigned)rng();
            set_box(s, t, (int)(v % 4) >= dead_share || (v & 64) != 0, (int)(v >> 8));
            s.born[t] = (v & 0x30000) == 0 ? (int32_t)(1 + (v >> 20) % 3) : 0;
            s.status[t] = (int32_t)((v >> 12) % 128);
            const unsigned w = (unsigned)rng();
            s.best_q[t] = (w % 7 == 0) ? -1.0 : (w % 11 == 0) ? kNaN : (double)(w % 1000) / 999.0;
            s.best_frame[t] = (int64_t)(w >> 10);
          }
          compare(s, "seeded", 100 + call, call == 3 ? 1 : 0, min_q);
        }
      }
}

void rows() {
  using flm::exit_ring_row;
  for (int q : {1, 2, 7, 65535})
    for (int64_t seq : {(int64_t)0, (int64_t)1, (int64_t)6, (int64_t)7, (int64_t)65535, (int64_t)1 << 40, INT64_MAX, (int64_t)-1,
                        (int64_t)-7, INT64_MIN}) {
      const int row = exit_ring_row(seq, q);
      CHECK(row >= 0 && row < q, "ring row %d of seq %lld, q %d", row, (long long)seq, q);
      if (seq >= 0) CHECK(row == (int)(seq % q), "ring row %d of seq %lld, q %d", row, (long long)seq, q);
    }
}

}  // namespace

int main() {
  combinations();
  seeded();
  rows();
  std::printf("track_exit_host: %d checks, %d failures\n", g_checks, g_failures);
  return g_failures ? 1 : 0;
}
