// Process state of libflm_hip.so and its extern "C" entry points (see include/flm.h): the calling thread's error string,
// the A/B knob table, the profiling hook.  The other entry points are in flm_api_fcn.hip (pack, workspace, forward,
// decodes), flm_api_image.hip (fits, warps, frames, mesh, annotation) and flm_api_track.hip (the tracker's calls); their
// shared argument checks are in flm_api_checks.h.
#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "flm_api_checks.h"
#include "flm_api_prof.h"

namespace flm {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

int hip_fail(hipError_t e, const char* what) {
  set_error("HIP error %d (%s) at %s", (int)e, hipGetErrorString(e), what);
  return FLM_ERR_HIP;
}

// ---- A/B knobs: one row per KnobId, in the enum's order (include/flm.h documents the keys and values) ------------
struct Knob {
  const char* key;
  std::atomic<int> value;  // initialised with the default
  bool (*valid)(int);      // null: every value is accepted
  const char* domain;      // what a rejected value is told ("<key> must be <domain>")
};
static Knob g_knobs[] = {
    {"bf16_big_tiles", {1}, nullptr, nullptr},
    {"bf16_lds_dma", {1}, nullptr, nullptr},
    {"bf16_mfma16", {1}, nullptr, nullptr},
    {"bf16_halo_mfma16", {1}, nullptr, nullptr},
    {"f32_two_level", {1}, nullptr, nullptr},
    {"f32_lean_tile", {1}, nullptr, nullptr},
    {"bf16_group_n", {0}, [](int v) { return v >= 0 && v <= 32 && !(v & (v - 1)); }, "0 or a power of two <= 32"},
    {"bf16_conv3_halo", {1}, nullptr, nullptr},
    {"bf16_score1x1", {1}, nullptr, nullptr},
    {"bf16_fused_tail", {1}, nullptr, nullptr},
    {"decode_lds_dma", {1}, nullptr, nullptr},
    {"posmajor_order", {1}, nullptr, nullptr},
    {"warp_rows", {1}, [](int v) { return v == 0 || v == 1 || v == 4; }, "0, 1 or 4"},
    {"up3_cand8", {1}, [](int v) { return v >= 0 && v <= 7; }, "in [0,7]"},
    {"up3_cand8_rows", {0}, [](int v) { return v >= 0 && v <= 8 && !(v & (v - 1)); }, "0, 1, 2, 4 or 8"},
    {"up3_wreg", {0}, [](int v) { return v == 0 || v == 1; }, "0 or 1"},
    {"f32_fc6_rows", {0}, [](int v) { return v == 0 || v == 64 || v == 128; }, "0, 64 or 128"},
};
static_assert(sizeof(g_knobs) / sizeof(g_knobs[0]) == KNOB_COUNT, "one row per KnobId");
int tuning(KnobId id) { return g_knobs[id].value.load(std::memory_order_relaxed); }
static Knob* find_knob(const char* who, const char* key) {
  for (Knob& k : g_knobs)
    if (!strcmp(k.key, key)) return &k;
  set_error("%s: unknown key '%s'", who, key);
  return nullptr;
}

// ---- optional per-launch timing (bench.py): hipEvent pairs around every launch of the forward --------
// Off by default; when enabled the forward records two events per layer on the caller's stream and
// never synchronises -- flm_profile_read() does, after the caller's own timed region has ended.
static ProfRec* g_prof = nullptr;
static int g_prof_cap = 0, g_prof_n = 0;
static char g_prof_filter[32] = "";  // non-empty: only launches of this layer are bracketed

ProfRec* prof_begin(hipStream_t s, const char* name) {
  if (!name || !g_prof || g_prof_n >= g_prof_cap || (g_prof_filter[0] && strcmp(g_prof_filter, name))) return nullptr;
  ProfRec* r = &g_prof[g_prof_n++];
  r->name = name;
  (void)hipEventRecord(r->a, s);
  return r;
}

}  // namespace flm

using namespace flm;

extern "C" {

int flm_abi_version(void) { return FLM_ABI_VERSION; }

int flm_debug_query(const char* key, int arg) {
  if (key && !strcmp(key, "igemm_occupancy")) return igemm_occupancy((size_t)arg);
  if (key && !strcmp(key, "igemm_posmajor_rows")) return igemm_posmajor_rows_last();
  return -1;
}

int flm_set_tuning(const char* key, int value) {
  if (!key) return FLM_ERR_ARG;
  if (!strcmp(key, "none")) return FLM_OK;
  if (!strcmp(key, "landmark_candidates") || !strcmp(key, "candidate_sub_phases") || !strcmp(key, "candidate_cap_div")) {
    set_error("flm_set_tuning: '%s' changes the workspace layout and is a per-call option now: pass flm_forward_opts to "
              "flm_fcn_workspace_bytes_opts / flm_fcn_forward_opts", key);
    return FLM_ERR_ARG;
  }
  Knob* k = find_knob("flm_set_tuning", key);
  if (!k) return FLM_ERR_ARG;
  if (k->valid && !k->valid(value)) {
    set_error("flm_set_tuning: %s must be %s", key, k->domain);
    return FLM_ERR_ARG;
  }
  k->value.store(value, std::memory_order_relaxed);
  return FLM_OK;
}

int flm_get_tuning(const char* key, int* value) {
  if (!key || !value) return null_argument("flm_get_tuning");
  const Knob* k = find_knob("flm_get_tuning", key);
  if (!k) return FLM_ERR_ARG;
  *value = k->value.load(std::memory_order_relaxed);
  return FLM_OK;
}

int flm_profile_enable(int max_records) {
  if (g_prof) return FLM_OK;
  if (max_records <= 0 || max_records > (1 << 20)) {
    set_error("flm_profile_enable: bad record count");
    return FLM_ERR_ARG;
  }
  g_prof = new ProfRec[max_records];
  for (int i = 0; i < max_records; ++i) {
    FLM_HIP(hipEventCreate(&g_prof[i].a));
    FLM_HIP(hipEventCreate(&g_prof[i].b));
  }
  g_prof_cap = max_records;
  g_prof_n = 0;
  return FLM_OK;
}

int flm_profile_reset(void) {
  g_prof_n = 0;
  return FLM_OK;
}

int flm_profile_read(int index, char* name_out, int name_cap, float* ms_out) {
  if (!g_prof || index < 0 || index >= g_prof_n) return 1;  // past the end
  ProfRec& r = g_prof[index];
  FLM_HIP(hipEventSynchronize(r.b));
  FLM_HIP(hipEventElapsedTime(ms_out, r.a, r.b));
  if (name_out && name_cap > 0) {
    strncpy(name_out, r.name, name_cap - 1);
    name_out[name_cap - 1] = 0;
  }
  return FLM_OK;
}

int flm_profile_disable(void) {
  if (!g_prof) return FLM_OK;
  for (int i = 0; i < g_prof_cap; ++i) {
    (void)hipEventDestroy(g_prof[i].a);
    (void)hipEventDestroy(g_prof[i].b);
  }
  delete[] g_prof;
  g_prof = nullptr;
  g_prof_cap = g_prof_n = 0;
  return FLM_OK;
}
int flm_profile_filter(const char* layer) {
  if (layer && strlen(layer) >= sizeof(g_prof_filter)) {
    set_error("flm_profile_filter: layer name too long");
    return FLM_ERR_ARG;
  }
  strcpy(g_prof_filter, layer ? layer : "");
  return FLM_OK;
}
const char* flm_last_error(void) { return g_err; }

}  // extern "C"
