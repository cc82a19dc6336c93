// Host program for csrc/flm_api_checks.h, the vocabulary of argument checks the extern "C" entry points are stated in:
// ranges_overlap at its edges, the two overlap shapes (null entries, which pair is named, the phrasing), the option-struct
// head (NULL, struct_size, reserved) and the integer range.  The header reports through flm::set_error, which this program
// defines itself, so nothing of the library is linked and no GPU call is made.
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>

#include "flm_api_checks.h"

static char g_msg[512];
namespace flm {
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_msg, sizeof(g_msg), fmt, ap);
  va_end(ap);
}
}  // namespace flm

// the _init FLM_OPTS(flm_exit_opts) names; min_q is not the library's default, so a defaulted struct shows it ran
extern "C" void flm_exit_opts_init(flm_exit_opts* o) {
  o->struct_size = (uint32_t)sizeof(flm_exit_opts);
  o->reserved = 0;
  o->min_q = 0.25;
}

static int failures = 0, checks = 0;
#define CHECK(cond)                                                      \
  do {                                                                   \
    ++checks;                                                            \
    if (!(cond)) {                                                       \
      ++failures;                                                        \
      std::printf("line %d: %s  [message: %s]\n", __LINE__, #cond, g_msg); \
    }                                                                    \
  } while (0)
static bool msg_is(const char* expect) { return !std::strcmp(g_msg, expect); }
static void clear() { std::strcpy(g_msg, "untouched"); }

using namespace flm;

static void test_ranges_overlap() {
  static char buf[64];
  const char* a = buf + 16;  // [16, 32)
  const auto both = [&](const char* b, size_t nb) {  // the answer must not depend on the order of the two ranges
    const bool x = ranges_overlap(a, 16, b, nb), y = ranges_overlap(b, nb, a, 16);
    CHECK(x == y);
    return x;
  };
  CHECK(!both(buf + 32, 8));  // adjacent, behind
  CHECK(!both(buf + 8, 8));   // adjacent, in front
  CHECK(both(buf + 31, 8));   // one byte into the end
  CHECK(both(buf + 8, 9));    // one byte into the start
  CHECK(both(buf + 20, 4));   // inside
  CHECK(both(buf, 64));       // around
  CHECK(both(buf + 16, 16));  // the same range
  // a zero-length range: apart at either end, overlapping strictly inside (what the entry points have always answered)
  CHECK(!both(buf + 16, 0));
  CHECK(both(buf + 20, 0));
  CHECK(!both(buf + 32, 0));
  CHECK(!ranges_overlap(buf + 20, 0, buf + 20, 0));
}

static void test_check_apart() {
  static char buf[128];
  const char* two = "%s: %s and %s overlap (no two arguments may)";
  {  // apart, with a null entry whose bytes would cover everything: FLM_OK, no message
    const NamedRange r[] = {{buf, 16, "a"}, {nullptr, 128, "gone"}, {buf + 16, 16, "b"}, {buf + 32, 0, "c"}};
    clear();
    CHECK(check_apart("who", r, two) == FLM_OK && msg_is("untouched"));
  }
  {  // (a,d) and (b,c) overlap: the first pair in array order is (a,d)
    const NamedRange r[] = {{buf, 16, "a"}, {buf + 32, 16, "b"}, {buf + 40, 16, "c"}, {buf + 8, 16, "d"}};
    clear();
    CHECK(check_apart("who", r, two) == FLM_ERR_ARG && msg_is("who: a and d overlap (no two arguments may)"));
  }
  {  // (b,d) and (b,c) overlap: (b,c) comes first; the message is the given phrasing
    const NamedRange r[] = {{buf, 16, "a"}, {buf + 32, 16, "b"}, {buf + 40, 16, "c"}, {buf + 47, 1, "d"}};
    clear();
    CHECK(check_apart("call", r, "%s: %s overlaps %s") == FLM_ERR_ARG && msg_is("call: b overlaps c"));
  }
  {  // an overlap with a null entry is none
    const NamedRange r[] = {{buf, 16, "a"}, {nullptr, 16, "b"}};
    clear();
    CHECK(check_apart("who", r, two) == FLM_OK && msg_is("untouched"));
  }
}

static void test_check_outputs_apart() {
  static char buf[256];
  const char* fi = "%s: %s and %s overlap (no output may overlap an input)";
  const char* fo = "%s: %s and %s overlap (no two outputs may)";
  {  // inputs may overlap each other; null inputs and null outputs are skipped
    const NamedRange in[] = {{buf, 32, "in0"}, {buf + 16, 32, "in1"}, {nullptr, 256, "in2"}};
    const NamedRange out[] = {{buf + 64, 16, "out0"}, {nullptr, 256, "out1"}, {buf + 80, 16, "out2"}};
    clear();
    CHECK(check_outputs_apart("who", in, out, fi, fo) == FLM_OK && msg_is("untouched"));
  }
  {  // out0 overlaps in1 and out1: its inputs come first
    const NamedRange in[] = {{buf, 16, "in0"}, {buf + 16, 16, "in1"}};
    const NamedRange out[] = {{buf + 31, 16, "out0"}, {buf + 40, 16, "out1"}};
    clear();
    CHECK(check_outputs_apart("who", in, out, fi, fo) == FLM_ERR_ARG &&
          msg_is("who: out0 and in1 overlap (no output may overlap an input)"));
  }
  {  // out0 overlaps out2, out1 overlaps in0: outputs in array order, so out0's pair is named
    const NamedRange in[] = {{buf, 16, "in0"}};
    const NamedRange out[] = {{buf + 64, 16, "out0"}, {buf + 8, 16, "out1"}, {buf + 72, 16, "out2"}};
    clear();
    CHECK(check_outputs_apart("who", in, out, fi, fo) == FLM_ERR_ARG &&
          msg_is("who: out0 and out2 overlap (no two outputs may)"));
  }
  {  // the flow family's phrasing, the same for both
    const NamedRange in[] = {{buf, 16, "m_dev"}};
    const NamedRange out[] = {{buf + 64, 16, "lm_out_dev"}, {buf + 15, 4, "w_out_dev"}};
    clear();
    CHECK(check_outputs_apart("flm_landmark_flow", in, out, "%s: %s overlaps %s", "%s: %s overlaps %s") == FLM_ERR_ARG &&
          msg_is("flm_landmark_flow: w_out_dev overlaps m_dev"));
  }
}

static void test_check_opts() {
  char expect[256];
  {  // NULL: the defaults, filled by the struct's _init
    const flm_exit_opts* opts = nullptr;
    flm_exit_opts defaults;
    std::memset(&defaults, 0xff, sizeof(defaults));
    clear();
    CHECK(check_opts<true>("who", FLM_OPTS(flm_exit_opts), &opts, &defaults) == FLM_OK && msg_is("untouched"));
    CHECK(opts == &defaults && defaults.struct_size == sizeof(flm_exit_opts) && defaults.reserved == 0 &&
          defaults.min_q == 0.25);
  }
  {  // given: left alone, the defaults are not touched
    flm_exit_opts mine, defaults;
    flm_exit_opts_init(&mine);
    mine.min_q = 3.0;
    std::memset(&defaults, 0xff, sizeof(defaults));
    const flm_exit_opts* opts = &mine;
    clear();
    CHECK(check_opts<true>("who", FLM_OPTS(flm_exit_opts), &opts, &defaults) == FLM_OK && msg_is("untouched"));
    CHECK(opts == &mine && mine.min_q == 3.0 && defaults.struct_size == 0xffffffffu);
    // struct_size one byte short
    mine.struct_size = (uint32_t)sizeof(flm_exit_opts) - 1;
    std::snprintf(expect, sizeof(expect),
                  "who: flm_exit_opts struct_size %u is smaller than this library's %zu (initialise with flm_exit_opts_init)",
                  (unsigned)sizeof(flm_exit_opts) - 1, sizeof(flm_exit_opts));
    CHECK(check_opts<true>("who", FLM_OPTS(flm_exit_opts), &opts, &defaults) == FLM_ERR_ARG && msg_is(expect));
    // a larger struct_size (a newer caller) passes
    mine.struct_size = (uint32_t)sizeof(flm_exit_opts) + 8;
    clear();
    CHECK(check_opts<true>("who", FLM_OPTS(flm_exit_opts), &opts, &defaults) == FLM_OK && msg_is("untouched"));
    // reserved = 1; struct_size is looked at first
    mine.reserved = 1;
    CHECK(check_opts<true>("who", FLM_OPTS(flm_exit_opts), &opts, &defaults) == FLM_ERR_ARG &&
          msg_is("who: flm_exit_opts reserved=1, must be 0"));
    mine.struct_size = 0;
    CHECK(check_opts<true>("who", FLM_OPTS(flm_exit_opts), &opts, &defaults) == FLM_ERR_ARG &&
          std::strstr(g_msg, "struct_size 0 is smaller"));
    // a call that words its reserved check itself (flm_flow_opts) asks for the size alone
    mine.struct_size = (uint32_t)sizeof(flm_exit_opts);
    clear();
    CHECK(check_opts<false>("who", FLM_OPTS(flm_exit_opts), &opts, &defaults) == FLM_OK && msg_is("untouched"));
  }
  {  // the reserved field prints as its own type does: unsigned (flm_exit_opts) and signed (flm_best_opts)
    flm_exit_opts e;
    flm_exit_opts_init(&e);
    e.reserved = 0xffffffffu;
    CHECK(check_opts_head<true>("who", "flm_exit_opts", &e) == FLM_ERR_ARG &&
          msg_is("who: flm_exit_opts reserved=4294967295, must be 0"));
    flm_best_opts b;
    std::memset(&b, 0, sizeof(b));
    b.struct_size = (uint32_t)sizeof(b);
    b.reserved = -1;
    CHECK(check_opts_head<true>("who", "flm_best_opts", &b) == FLM_ERR_ARG &&
          msg_is("who: flm_best_opts reserved=-1, must be 0"));
  }
}

static void test_check_range() {
  clear();
  CHECK(check_range("who", "k", 1, 1, 65535) == FLM_OK && check_range("who", "k", 65535, 1, 65535) == FLM_OK &&
        msg_is("untouched"));
  CHECK(check_range("who", "k", 0, 1, 65535) == FLM_ERR_SHAPE && msg_is("who: k=0, needs 1 <= k <= 65535"));
  CHECK(check_range("who", "n_slots", 65536, 1, 65535) == FLM_ERR_SHAPE &&
        msg_is("who: n_slots=65536, needs 1 <= n_slots <= 65535"));
  CHECK(check_range("who", "p", -3, 4, 256) == FLM_ERR_SHAPE && msg_is("who: p=-3, needs 4 <= p <= 256"));
  CHECK(null_argument("who") == FLM_ERR_ARG && msg_is("who: null argument"));
}

int main() {
  test_ranges_overlap();
  test_check_apart();
  test_check_outputs_apart();
  test_check_opts();
  test_check_range();
  std::printf("api checks: %d checks, %d failures\n", checks, failures);
  return failures ? 1 : 0;
}
