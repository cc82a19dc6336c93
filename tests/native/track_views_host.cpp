// The bin of a face and the per-row decision of flm_track_views_update on the host: csrc/flm_track_views_dev.h -- the
// header track_views_decide_kernel of csrc/flm_track_views.hip is built from -- against a plain serial restatement of
// the contract of include/flm.h written in this file.  Built with the host's address and undefined-behaviour
// sanitizers; nothing here runs on a GPU.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "flm_track_views_dev.h"

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

const double kNaN = std::numeric_limits<double>::quiet_NaN();

// ---- the contract, restated serially ------------------------------------------------------------------------------------
int ref_bin(double ok, double r20, double r21, const std::vector<double>& ue, const std::vector<double>& ve) {
  if (!(ok == 1.0)) return -1;
  const double u = -r20, v = r21;
  if (std::isnan(u) || std::isnan(v)) return -1;
  int iu = 0, iv = 0;
  for (double e : ue)
    if (u >= e) ++iu;
  for (double e : ve)
    if (v >= e) ++iv;
  return iv * ((int)ue.size() + 1) + iu;
}

int ref_decide(bool reset, bool status_ok, int64_t n_lap, double e, double min_exposed, double q, int bin,
               std::vector<double>& vq) {
  if (reset)
    for (double& x : vq) x = -1.0;
  const bool eligible = status_ok && n_lap > 0 && e >= min_exposed && !std::isnan(q) && q >= 0.0 && bin >= 0;
  if (!eligible) return -1;
  if (q > vq[(size_t)bin]) {
    vq[(size_t)bin] = q;
    return bin;
  }
  return -1;
}

std::vector<double> edges_of(int n, double lo, double hi) {  // n strictly ascending edges inside (lo, hi)
  std::vector<double> e;
  for (int i = 0; i < n; ++i) e.push_back(lo + (hi - lo) * (i + 1) / (n + 1));
  return e;
}

flm::ViewsBins bins_of(const std::vector<double>& ue, const std::vector<double>& ve) {
  flm::ViewsBins b;
  b.n_u = (int)ue.size();
  b.n_v = (int)ve.size();
  for (int i = 0; i < FLM_VIEWS_MAX_EDGES; ++i) {
    // the edges past the count hold a value every probe passes: they must never be compared
    b.u_edge[i] = i < b.n_u ? ue[(size_t)i] : -2.0;
    b.v_edge[i] = i < b.n_v ? ve[(size_t)i] : -2.0;
  }
  return b;
}

// u or v below, on and above every edge, +-0, +-1 and NaN
std::vector<double> probes_of(const std::vector<double>& e) {
  std::vector<double> p = {0.0, -0.0, 1.0, -1.0, kNaN};
  for (double x : e) {
    p.push_back(std::nextafter(x, -2.0));
    p.push_back(x);
    p.push_back(std::nextafter(x, 2.0));
  }
  return p;
}

void test_bins() {
  for (int nu = 0; nu <= FLM_VIEWS_MAX_EDGES; ++nu)
    for (int nv = 0; nv <= FLM_VIEWS_MAX_EDGES; ++nv) {
      const std::vector<double> ue = edges_of(nu, -0.9, 0.8), ve = edges_of(nv, -0.5, 0.95);
      const flm::ViewsBins b = bins_of(ue, ve);
      CHECK(flm::views_bins(b) == (nu + 1) * (nv + 1), "bins %d %d", nu, nv);
      std::vector<char> seen((size_t)flm::views_bins(b), 0);
      for (double u : probes_of(ue))
        for (double v : probes_of(ve))
          for (double ok : {0.0, 1.0}) {
            double pose[FLM_POSE_REC];
            for (int i = 0; i < FLM_POSE_REC; ++i) pose[i] = 0.25 * i;
            pose[14] = ok;
            pose[6] = -u;   // u = -pose[6]
            pose[7] = v;
            const int want = ref_bin(ok, pose[6], pose[7], ue, ve), got = flm::views_bin(pose, b);
            CHECK(got == want, "nu=%d nv=%d u=%.17g v=%.17g ok=%g: bin %d, want %d", nu, nv, u, v, ok, got, want);
            CHECK(got >= -1 && got < flm::views_bins(b), "bin %d outside [-1, %d)", got, flm::views_bins(b));
            if (got >= 0) seen[(size_t)got] = 1;
          }
      for (size_t i = 0; i < seen.size(); ++i) CHECK(seen[i], "nu=%d nv=%d: no probe fell into bin %zu", nu, nv, i);
    }
  // an ok that is not exactly 1.0 does not count, NaN included
  {
    const flm::ViewsBins b = bins_of({-0.3, 0.3}, {});
    for (double ok : {0.5, 2.0, -1.0, kNaN}) {
      double pose[FLM_POSE_REC] = {0};
      pose[14] = ok;
      CHECK(flm::views_bin(pose, b) == -1, "ok=%g must not be binned", ok);
    }
    double pose[FLM_POSE_REC] = {0};
    pose[14] = 1.0;
    pose[6] = -0.3;   // u = 0.3: ON the upper edge -> the upper bin
    CHECK(flm::views_bin(pose, b) == 2, "on the edge: bin %d", flm::views_bin(pose, b));
    pose[6] = 0.3;    // u = -0.3: on the lower edge -> the middle bin
    CHECK(flm::views_bin(pose, b) == 1, "on the lower edge: bin %d", flm::views_bin(pose, b));
    pose[6] = std::nextafter(0.3, 1.0);
    CHECK(flm::views_bin(pose, b) == 0, "below the lower edge: bin %d", flm::views_bin(pose, b));
  }
}

void test_decisions() {
  const double prev_value = 0.375, min_exposed = 0.5;
  const int n_bins = 3;
  int taken = 0, kept = 0;
  for (int reset = 0; reset <= 1; ++reset)
    for (int status_ok = 0; status_ok <= 1; ++status_ok)
      for (int64_t n_lap : {(int64_t)0, (int64_t)12100})
        for (double e : {0.25, 0.5, 0.75, kNaN})
          for (int bin : {-1, 0, 1, 2})
            for (double prev : {-1.0, prev_value})
              for (double q : {std::nextafter(prev_value, 0.0), prev_value, std::nextafter(prev_value, 1.0), kNaN, 0.0, -0.0,
                               -1e-300, 1.0}) {
                std::vector<double> a = {0.125, 0.125, 0.125}, b;
                if (bin >= 0) a[(size_t)bin] = prev;
                b = a;
                const int want = ref_decide(reset != 0, status_ok != 0, n_lap, e, min_exposed, q, bin, b);
                const bool eligible = flm::views_eligible(status_ok != 0, n_lap, e, min_exposed, q);
                const int got = flm::views_decide(reset != 0, eligible, q, bin, a.data(), n_bins);
                CHECK(got == want, "reset=%d status_ok=%d n_lap=%lld e=%g bin=%d prev=%g q=%.17g: take %d, want %d", reset,
                      status_ok, (long long)n_lap, e, bin, prev, q, got, want);
                CHECK(std::memcmp(a.data(), b.data(), sizeof(double) * a.size()) == 0,
                      "reset=%d status_ok=%d n_lap=%lld e=%g bin=%d prev=%g q=%.17g: view_q differs", reset, status_ok,
                      (long long)n_lap, e, bin, prev, q);
                if (got >= 0) ++taken; else ++kept;
              }
  CHECK(taken > 0 && kept > 0, "the sweep must take and keep (%d, %d)", taken, kept);
  // a tie keeps the earlier face; a reset lets the same quality in again
  std::vector<double> vq = {0.5, -1.0};
  CHECK(flm::views_decide(false, true, 0.5, 0, vq.data(), 2) == -1 && vq[0] == 0.5, "a tie must not be taken");
  CHECK(flm::views_decide(true, true, 0.5, 0, vq.data(), 2) == 0 && vq[0] == 0.5 && vq[1] == -1.0, "reset, then taken");
  CHECK(flm::views_decide(true, false, 0.9, 1, vq.data(), 2) == -1 && vq[0] == -1.0 && vq[1] == -1.0,
        "a reset empties the bins of a row that is not eligible too");
  CHECK(flm::views_decide(false, true, 0.0, 1, vq.data(), 2) == 1 && vq[1] == 0.0, "q = 0 beats an empty bin");
}

}  // namespace

int main() {
  test_bins();
  test_decisions();
  std::printf("track_views_host: %d checks, %d failures\n", g_checks, g_failures);
  return g_failures ? 1 : 0;
}
