// Host side of the reentrancy contract (include/flm.h: "calls on different streams may run concurrently from different
// threads"), built and run under ThreadSanitizer by tests/test_reentrancy_native_host.py.  No GPU is touched.  Eight
// threads leave a barrier together and each runs, cold and then a few hundred times:
//   * flm::posmajor_fill_perm (csrc/flm_igemm_args.h) on the library's own posperm_cache_get / posperm_cache_put: one
//     geometry every thread shares (fc6: 7x7, pad 3, 4x4 map, 32 faces, 128-row tiles), raced cold, and twelve of its own --
//     97 distinct keys, past the cache's cap of 64, so some are searched on every call.  Every table equals the one a
//     single-threaded child process computed before any thread existed, each key on its first sight (the cache is
//     asked first and must not know it: the search alone produced the table);
//   * flm_set_tuning / flm_get_tuning on every key with accepted and rejected values;
//   * failing calls whose message names a value only this thread passes, between succeeding size queries.
// The flm_profile_* calls are declared not thread-safe and stay out.
#include <pthread.h>
#include <sys/wait.h>
#include <unistd.h>

#include <atomic>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

#include "flm_igemm_args.h"

static std::atomic<int> failures{0};
#define CHECK(cond, ...)                                                                   \
  do {                                                                                     \
    if (!(cond)) {                                                                         \
      if (failures.fetch_add(1) < 20) { std::fprintf(stderr, __VA_ARGS__); std::fprintf(stderr, "\n"); } \
    }                                                                                      \
  } while (0)

constexpr int kThreads = 8, kOwn = 12, kIters = 300;

struct Geo {
  int h, w, k, n, bm;
};
struct Table {
  unsigned long long t[8];
  int on;
};
static const Geo kShared = {4, 4, 7, 32, 128};

// 150 distinct (map, filter, positions per tile) keys; thread t owns entries t, t + 8, ...
static std::vector<Geo> all_geos() {
  std::vector<Geo> v;
  for (int k : {3, 5, 7})
    for (int h = 2; h <= 6; ++h)
      for (int w = 2; w <= 6; ++w)
        for (int n : {64, 32}) v.push_back({h, w, k, n, 128});
  return v;
}

static flm::IgemmArgs args_of(const Geo& g) {
  flm::IgemmArgs a = {};
  a.n = g.n; a.h = a.ho = g.h; a.w = a.wo = g.w; a.stride = 1;
  a.kh = a.kw = g.k; a.pad = g.k / 2;
  a.M = g.n * g.h * g.w;
  a.ntiles = 32;
  a.ksplit = 1;
  return a;
}

static Table fill(const Geo& g) {
  flm::IgemmArgs a = args_of(g);
  a.mtiles = (a.M + g.bm - 1) / g.bm;
  flm::posmajor_fill_perm(a, g.bm);
  Table t;
  for (int i = 0; i < 8; ++i) t.t[i] = a.posperm[i];
  t.on = a.posperm_on;
  return t;
}
static bool same(const Table& x, const Table& y) { return x.on == y.on && !std::memcmp(x.t, y.t, sizeof(x.t)); }

// a permutation of the map's positions (or the untouched zero table of a launch the search leaves alone)
static bool is_permutation(const Geo& g, const Table& t) {
  if (!t.on) return true;
  unsigned long long seen = 0ull;
  for (int i = 0; i < g.h * g.w; ++i) seen |= 1ull << ((t.t[i >> 3] >> ((i & 7) * 8)) & 0xffull);
  return seen == (g.h * g.w == 64 ? ~0ull : (1ull << (g.h * g.w)) - 1ull);
}

// The references, from a child process forked while this one is still single-threaded: its cache is empty, it asks the
// cache for every key first (and must be refused), so every table it returns is the search's own.
static bool reference_tables(const std::vector<Geo>& geos, std::vector<Table>& out) {
  int fd[2];
  if (pipe(fd)) return false;
  const pid_t pid = fork();
  if (pid < 0) return false;
  if (pid == 0) {
    close(fd[0]);
    int bad = 0;
    for (const Geo& g : geos) {
      flm::PospermEntry e = {g.h, g.w, g.k, g.k, g.k / 2, g.bm / g.n, 0, {0, 0, 0, 0, 0, 0, 0, 0}};
      bad += flm::posperm_cache_get(e);
      const Table t = fill(g);
      bad += write(fd[1], &t, sizeof(t)) != (ssize_t)sizeof(t);
    }
    _exit(bad ? 1 : 0);
  }
  close(fd[1]);
  out.resize(geos.size());
  bool ok = true;
  for (Table& t : out) {
    size_t got = 0;
    while (got < sizeof(t)) {
      const ssize_t r = read(fd[0], reinterpret_cast<char*>(&t) + got, sizeof(t) - got);
      if (r <= 0) { ok = false; break; }
      got += (size_t)r;
    }
  }
  close(fd[0]);
  int st = 0;
  waitpid(pid, &st, 0);
  return ok && WIFEXITED(st) && WEXITSTATUS(st) == 0;
}

// ---- knobs: the values the threads set (all accepted) and one the validator rejects (0 = the key accepts everything).
// "posmajor_order" stays non-zero: the tables above are read through the real tuning() while the setters run, and any
// non-zero value means "on".  "f32_two_level" is set too: nothing launches here, so no result can change.
struct KnobCase {
  const char* key;
  int def;
  int ok[4];
  int bad;
};
static const KnobCase kKnobs[] = {
    {"bf16_big_tiles", 1, {0, 1, 2, 3}, 0},      {"bf16_lds_dma", 1, {0, 1, 0, 1}, 0},
    {"bf16_mfma16", 1, {0, 1, 0, 1}, 0},         {"bf16_halo_mfma16", 1, {0, 1, 0, 1}, 0},
    {"f32_two_level", 1, {0, 1, 0, 1}, 0},       {"f32_lean_tile", 1, {0, 1, 0, 1}, 0},
    {"bf16_group_n", 0, {0, 1, 8, 32}, 3},       {"bf16_conv3_halo", 1, {0, 1, 2, 1}, 0},
    {"bf16_score1x1", 1, {0, 1, 0, 1}, 0},       {"bf16_fused_tail", 1, {0, 1, 0, 1}, 0},
    {"decode_lds_dma", 1, {0, 1, 0, 1}, 0},      {"posmajor_order", 1, {1, 2, 3, 1}, 0},
    {"warp_rows", 1, {0, 1, 4, 1}, 2},           {"up3_cand8", 1, {0, 1, 5, 7}, 8},
    {"up3_cand8_rows", 0, {0, 1, 4, 8}, 3},      {"up3_wreg", 0, {0, 1, 0, 1}, 2},
    {"f32_fc6_rows", 0, {0, 64, 128, 0}, 96},
};
static bool ever_set(const KnobCase& k, int v) {
  return v == k.def || v == k.ok[0] || v == k.ok[1] || v == k.ok[2] || v == k.ok[3];
}

// ---- size queries whose serial results every thread must see again
struct SizeCase {
  int arch, n, h, w, c, dt, om, dm, np, cap_div;
};
static const SizeCase kSizes[] = {
    {0, 32, 128, 128, 68, 0, 2, 1, 4, 1}, {0, 3, 96, 160, 68, 1, 2, 1, 25, 1}, {0, 20, 64, 64, 68, 0, 2, 1, 4, 4096},
    {1, 1, 32, 32, 21, 1, 0, 0, 0, 1},    {6, 2, 64, 96, 68, 0, 1, 0, 0, 1},   {4, 7, 64, 64, 5, 1, 4, 1, 9, 1},
};
constexpr int kNSizes = sizeof(kSizes) / sizeof(kSizes[0]);
struct Sizes {
  size_t ws, packed, dec;
};
static Sizes sizes_of(const SizeCase& s) {
  flm_forward_opts o;
  flm_forward_opts_init(&o);
  o.candidate_cap_div = s.cap_div;
  return {flm_fcn_workspace_bytes_opts(s.arch, s.n, s.h, s.w, s.c, s.dt, s.om, s.dm, s.np, &o),
          flm_fcn_packed_bytes(s.arch, s.c, s.dt), flm_decode_workspace_bytes(s.n, s.h + 8, s.w + 8, s.c, s.dm, s.np)};
}

static bool says(const char* what) { return std::strstr(flm_last_error(), what) != nullptr; }

// One round of argument errors (those tests/native/abi_sweep.cpp lists), each with a value only thread `t` passes; no
// call reaches a launch.  Between them, queries that succeed.
static void errors_round(int t, int it, const Sizes* serial) {
  char want[96], key[32];
  char dummy[16];
  const SizeCase& sc = kSizes[(t + it) % kNSizes];
  const int arch = 100 + t;
  CHECK(flm_fcn_forward(nullptr, arch, dummy, dummy, 0, 1, 32, 32, 68, 0, 0, 0, 0, 0.f, dummy, dummy, 16) == FLM_ERR_ARG, "bad arch accepted");
  std::snprintf(want, sizeof(want), "unknown architecture %d", arch);
  CHECK(says(want), "thread %d: '%s' after a bad architecture", t, flm_last_error());
  Sizes s = sizes_of(sc);
  CHECK(s.ws == serial[(t + it) % kNSizes].ws && s.packed == serial[(t + it) % kNSizes].packed && s.dec == serial[(t + it) % kNSizes].dec,
        "thread %d: size query differs from the serial one", t);
  CHECK(says(want), "thread %d: a succeeding query changed the message to '%s'", t, flm_last_error());

  const int mode = 9 + t;
  CHECK(flm_fcn8_forward(nullptr, dummy, dummy, 0, 1, 32, 32, 68, 0, mode, 0, 0, 0.f, dummy, dummy, 16) == FLM_ERR_ARG, "bad enum accepted");
  std::snprintf(want, sizeof(want), "unknown output mode %d", mode);
  CHECK(says(want), "thread %d: '%s' after a bad output mode", t, flm_last_error());

  const size_t small = 16 + (size_t)t;
  CHECK(flm_fcn8_forward(nullptr, dummy, dummy, 0, 1, 32, 32, 68, 0, 0, 0, 0, 0.f, dummy, dummy, small) == FLM_ERR_WORKSPACE, "small workspace accepted");
  std::snprintf(want, sizeof(want), "workspace too small (%zu <", small);
  CHECK(says(want), "thread %d: '%s' after a small workspace", t, flm_last_error());

  CHECK(flm_fcn8_forward(nullptr, nullptr, dummy, 0, 1, 32, 32, 68, 0, 0, 0, 0, 0.f, dummy, dummy, 16) == FLM_ERR_ARG, "null accepted");
  CHECK(says("flm_fcn8_forward: null argument"), "thread %d: '%s' after a null pointer", t, flm_last_error());

  const int h = 32 * (it % 7 + 1) + 1 + t;  // never a multiple of 32
  CHECK(flm_fcn8_forward(nullptr, dummy, dummy, 0, 1, h, 32, 68, 0, 0, 0, 0, 0.f, dummy, dummy, 16) == FLM_ERR_SHAPE, "bad shape accepted");
  std::snprintf(want, sizeof(want), "h=%d w=32)", h);
  CHECK(says(want), "thread %d: '%s' after a bad height", t, flm_last_error());

  const int classes = 200 + t;
  CHECK(flm_fcn_packed_bytes(0, classes, 0) == 0, "bad class count sized");
  std::snprintf(want, sizeof(want), "(got %d)", classes);
  CHECK(says(want), "thread %d: '%s' after a bad class count", t, flm_last_error());
  s = sizes_of(sc);
  CHECK(s.ws == serial[(t + it) % kNSizes].ws, "thread %d: size query differs from the serial one", t);

  const int dtype = 20 + t;
  CHECK(flm_fcn_workspace_bytes(0, 1, 32, 32, 68, dtype, 0, 0, 0) == 0, "bad dtype sized");
  std::snprintf(want, sizeof(want), "unknown dtype %d", dtype);
  CHECK(says(want), "thread %d: '%s' after a bad dtype", t, flm_last_error());

  CHECK(flm_decode(nullptr, nullptr, 1, 8, 8, 1, 0, 0, 0.f, nullptr, nullptr, 0) == FLM_ERR_ARG, "null decode accepted");
  CHECK(says("flm_decode: null argument"), "thread %d: '%s' after a null decode", t, flm_last_error());

  std::snprintf(key, sizeof(key), "nope%d", t);
  int v = -77;
  CHECK(flm_get_tuning(key, &v) == FLM_ERR_ARG && v == -77, "unknown key read");
  std::snprintf(want, sizeof(want), "flm_get_tuning: unknown key '%s'", key);
  CHECK(says(want), "thread %d: '%s' after an unknown key", t, flm_last_error());
}

static void knobs_round(int t, int it) {
  for (const KnobCase& k : kKnobs) {
    int v = -77;
    CHECK(flm_set_tuning(k.key, k.ok[(t + it) & 3]) == FLM_OK, "%s: %d refused", k.key, k.ok[(t + it) & 3]);
    CHECK(flm_get_tuning(k.key, &v) == FLM_OK && ever_set(k, v), "%s: read %d, which no thread ever set", k.key, v);
    if (k.bad) {
      CHECK(flm_set_tuning(k.key, k.bad) ==FLM_ERR_ARG, "%s: %d accepted", k.key, k.bad);
      CHECK(says(k.key) && says("must be"), "thread %d: '%s' after a rejected value", t, flm_last_error());
      CHECK(flm_get_tuning(k.key, &v) == FLM_OK && ever_set(k, v) && v != k.bad, "%s: read %d after a rejected %d", k.key, v, k.bad);
    }
  }
  CHECK(flm::tuning(flm::KNOB_POSMAJOR_ORDER) != 0, "posmajor_order read as 0, which no thread set");
}

int main() {
  const std::vector<Geo> pool = all_geos();
  std::vector<Geo> geos = {kShared};
  for (int i = 0; i < kThreads * kOwn; ++i) geos.push_back(pool[(size_t)i]);
  std::vector<Table> ref;
  if (!reference_tables(geos, ref)) {
    std::fprintf(stderr, "reentrancy_host: the reference child failed (a key was in an empty cache, or the pipe broke)\n");
    return 1;
  }
  int searched = 0;
  for (size_t i = 0; i < geos.size(); ++i) {
    CHECK(is_permutation(geos[i], ref[i]), "reference table %zu is no permutation", i);
    searched += ref[i].on;
  }
  CHECK(ref[0].on, "the shared fc6 geometry must reach the search (four positions per tile)");

  // serial facts before any thread exists: defaults, a rejected value leaves the knob exactly as it was, sizes
  for (const KnobCase& k : kKnobs) {
    int v = -1, u = -1;
    CHECK(flm_get_tuning(k.key, &v) == FLM_OK && v == k.def, "%s: default %d, expected %d", k.key, v, k.def);
    if (k.bad) {
      CHECK(flm_set_tuning(k.key, k.ok[1]) == FLM_OK && flm_set_tuning(k.key, k.bad) == FLM_ERR_ARG, "%s: serial set", k.key);
      CHECK(flm_get_tuning(k.key, &u) == FLM_OK && u == k.ok[1], "%s: %d after a rejected value, was %d", k.key, u, k.ok[1]);
      CHECK(flm_set_tuning(k.key, k.def) == FLM_OK, "%s: restore", k.key);
    }
  }
  Sizes serial[kNSizes];
  for (int i = 0; i < kNSizes; ++i) {
    serial[i] = sizes_of(kSizes[i]);
    CHECK(serial[i].ws > 0 && serial[i].packed > 0 && serial[i].dec > 0, "size case %d refused: %s", i, flm_last_error());
  }

  pthread_barrier_t gate;
  pthread_barrier_init(&gate, nullptr, kThreads);
  std::vector<std::thread> threads;
  for (int t = 0; t < kThreads; ++t)
    threads.emplace_back([&, t] {
      CHECK(flm_last_error()[0] == 0, "thread %d starts with a message: '%s'", t, flm_last_error());
      pthread_barrier_wait(&gate);
      CHECK(same(fill(kShared), ref[0]), "thread %d: cold shared table differs from the reference", t);  // all eight, cold, one key
      for (int it = 0; it < kIters; ++it) {
        CHECK(same(fill(kShared), ref[0]), "thread %d round %d: shared table differs", t, it);
        const size_t own = 1 + (size_t)(t + kThreads * (it % kOwn));
        CHECK(same(fill(geos[own]), ref[own]), "thread %d round %d: table of geometry %zu differs", t, it, own);
        knobs_round(t, it);
        errors_round(t, it, serial);
      }
    });
  for (std::thread& th : threads) th.join();
  pthread_barrier_destroy(&gate);

  // with the knob off no launch gets a table, cached or not
  CHECK(flm_set_tuning("posmajor_order", 0) == FLM_OK && !fill(kShared).on && !fill(geos[1]).on, "knob off but a table is on");
  for (const KnobCase& k : kKnobs) CHECK(flm_set_tuning(k.key, k.def) == FLM_OK, "%s: restore", k.key);
  CHECK(flm_last_error()[0] != 0, "the main thread's serial rejections left no message");
  std::printf("reentrancy_host: %d threads x %d rounds, %zu geometries (search on for %d), %d failures\n", kThreads, kIters,
              geos.size(), searched, failures.load());
  return failures.load() ? 1 : 0;
}
