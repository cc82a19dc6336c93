// extern "C" entry points of libflm_hip.so (see include/flm.h) and the forward's launch sequence.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "flm_annotate_dev.h"
#include "flm_common.h"
#include "flm_flow_rows_dev.h"

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
struct ProfRec {
  const char* name;
  hipEvent_t a, b;
};
static ProfRec* g_prof = nullptr;
static int g_prof_cap = 0, g_prof_n = 0;
static char g_prof_filter[32] = "";  // non-empty: only launches of this layer are bracketed

struct ProfScope {
  hipStream_t s;
  ProfRec* r;
  ProfScope(hipStream_t st, const char* name) : s(st), r(nullptr) {  // (null name: no record)
    if (name && g_prof && g_prof_n < g_prof_cap && (!g_prof_filter[0] || !strcmp(g_prof_filter, name))) {
      r = &g_prof[g_prof_n++];
      r->name = name;
      (void)hipEventRecord(r->a, s);
    }
  }
  ~ProfScope() {
    if (r) (void)hipEventRecord(r->b, s);
  }
};

// Landmark mode without the probability tensor (flm_convt.hip): for the 68-class FCN-8 kernels, top-n decode
// with n <= 32 (the threshold is the n-th of a face's 144..288 sampled maxima; list capacities grow with n), maps
// below 2^17 pixels.  On by default for both types: bf16 batch
// 512 saves the tensor's write + re-read (up3 + decode 6.2 -> 3.5 ms); fp32 batch 64 gains 1.5 % of the step (the
// fp32 up3 is bound by the matrix pipe and writes its map for free; the gain is the decode).  0 = off (tests, A/B).
// These three are per-call options (flm_forward_opts): they change the workspace layout, so they travel with the call
// and with its workspace query instead of living in process state.
struct CandOpts {
  int enable, sub, cap_div;
};
static bool resolve_opts(const flm_forward_opts* o, CandOpts* c) {
  c->enable = 1;
  c->sub = 0;
  c->cap_div = 1;
  if (!o) return true;
  if (o->struct_size < sizeof(flm_forward_opts)) {
    set_error("flm_forward_opts: struct_size %u is smaller than this library's %zu (initialise with flm_forward_opts_init)",
              o->struct_size, sizeof(flm_forward_opts));
    return false;
  }
  if (o->candidate_sub_phases < 0 || o->candidate_sub_phases > 16 || o->candidate_cap_div < 1) {
    set_error("flm_forward_opts: candidate_sub_phases must be in [0,16] and candidate_cap_div >= 1");
    return false;
  }
  c->enable = o->landmark_candidates != 0;
  c->sub = o->candidate_sub_phases;
  c->cap_div = o->candidate_cap_div;
  return true;
}
// flm_fallback_opts: the row budget of the per-face fallback (0 = off; clamped to n by the layout).  false: rejected.
static bool resolve_fallback(const flm_fallback_opts* fb, int* faces) {
  *faces = 0;
  if (!fb) return true;
  if (fb->struct_size < sizeof(flm_fallback_opts)) {
    set_error("flm_fallback_opts: struct_size %u is smaller than this library's %zu (initialise with flm_fallback_opts_init)",
              fb->struct_size, sizeof(flm_fallback_opts));
    return false;
  }
  if (fb->faces < 0) {
    set_error("flm_fallback_opts: faces must be >= 0 (got %d)", fb->faces);
    return false;
  }
  *faces = fb->faces;
  return true;
}
// More sampled phases cost 1/64 of up3 each and tighten the threshold: the key lists shrink about in proportion.  At
// n = 4 the lists are short anyway (4 phases: 8-10 k keys per face); at n >= 16 their merge costs more than the extra
// phases (batch 512 bf16, n = 25: 12.1 ms with 4 phases, 11.5 with 8; tools/ab_sub.py).
// In fp32 a sampled phase costs sixteen times the matrix time it costs in bf16 while a key costs the same: at n <= 8 two
// phases do (batch 64, n = 4: 8.335 / 8.318 / 8.29 ms per step with 4 / 3 / 2 phases, 9.6 k / 13.4 k / 20.2 k keys per face of
// the 69.6 k the lists hold; bf16 batch 512: 7.76-7.93 / 7.84-8.15 / 8.01-8.03).
static int cand_sub_for(const CandOpts& c, int n_points, bool bf16) {
  if (c.sub > 0) return c.sub;
  return n_points <= 8 ? (bf16 ? 4 : 2) : (n_points <= 15 ? 6 : 8);
}
static bool landmark_candidates_enabled(const CandOpts& c, const ConvTGeom& g, int fcn32, int decode_mode, int n_points,
                                        int oh, int ow) {
  return c.enable && !fcn32 && decode_mode == FLM_DECODE_TOPN && n_points >= 1 && n_points <= 32 &&
         convt_candidates_supported(g) && (long long)oh * ow < (1 << 17);
}

struct EncNames {
  char s[kMaxEnc][8];
  EncNames() {
    for (int i = 0; i < kMaxEnc; ++i) snprintf(s[i], sizeof(s[i]), "enc%d", i + 1);
  }
};

static size_t take(size_t& cur, size_t bytes) {
  size_t o = cur;
  cur = align_up(cur + bytes, 256);
  return o;
}

Fcn8Ws fcn8_ws_layout(int n, int h, int w, int C, int dtype, int out_mode, int decode_mode, int n_points,
                      int arch, const flm_forward_opts* opts, const flm_fallback_opts* fb) {
  Fcn8Ws W;
  CandOpts co;
  int fb_faces = 0;
  if (!resolve_opts(opts, &co) || !resolve_fallback(fb, &fb_faces)) {  // callers validate first; an invalid struct sizes nothing
    W = Fcn8Ws();
    W.total = 0;
    return W;
  }
  const ConvTGeom g = convt_geom(C, dtype);
  const ArchSpec A = arch_spec(arch);
  const size_t es = dtype == FLM_BF16 ? 2 : 4;  // encoder activations, fc6, fc7 are stored in the operand type
  size_t cur = 0;
  int hs[kMaxEnc], wsz[kMaxEnc];
  enc_dims(A, h, w, hs, wsz);
  for (int i = 0; i < A.n_enc; ++i) W.act[i] = take(cur, es * (size_t)n * hs[i] * wsz[i] * A.enc[i].cout);
  for (int k = 0; k < 5; ++k) W.f[k] = W.act[A.f_idx[k]];
  const int h5 = h / 32, w5 = w / 32, h4 = h / 16, w4 = w / 16, h3 = h / 8, w3 = w / 8;
  W.fc6 = take(cur, es * (size_t)n * h5 * w5 * kFc);
  W.fc7 = take(cur, es * (size_t)n * h5 * w5 * kFc);
  W.score5 = take(cur, sizeof(float) * (size_t)n * h5 * w5 * g.Cp);
  W.fuse4 = take(cur, sizeof(float) * (size_t)n * h4 * w4 * g.Cp);
  W.seg = take(cur, sizeof(float) * (size_t)n * h3 * w3 * g.Cp);
  // split-K partial sums: the score convs (8 slices of [n*h5*w5][Cp]) and fc6 / fc7 while they have at most 64
  // tiles (8 slices of [<= 256 rows][4096])
  W.splitk_bytes = sizeof(float) * 8 * (size_t)n * h5 * w5 * g.Cp;
  {
    const size_t rows = (size_t)n * h5 * w5 < 256 ? (size_t)n * h5 * w5 : 256;
    const size_t fc_bytes = sizeof(float) * 8 * rows * kFc;
    if (fc_bytes > W.splitk_bytes) W.splitk_bytes = fc_bytes;
  }
  if (n <= 4) {  // a 3x3 layer on the 1/4-resolution grid with 256 outputs (vanilla enc3, fp32) in 4 slices, 4 faces
    const size_t enc3_bytes = sizeof(float) * 4 * (size_t)4 * (h / 4) * (w / 4) * 256;
    if (enc3_bytes > W.splitk_bytes) W.splitk_bytes = enc3_bytes;
  }
  W.splitk = take(cur, W.splitk_bytes);
  W.oh = h + (A.fcn32 ? 32 : 8);  // (h/32 - 1)*32 + 64 (fcn.py:145) vs (h/8 - 1)*8 + 16 (fcn.py:121)
  W.ow = w + (A.fcn32 ? 32 : 8);
  W.probs = SIZE_MAX;
  W.decode = SIZE_MAX;
  W.sub = W.tau = W.cand = W.cand_cnt = SIZE_MAX;
  W.cand_cap = W.cand_sub = 0;
  W.cand_redo = W.fb_rows = W.fb_counts = W.fb_decode = SIZE_MAX;
  W.fb_faces = 0;
  const int stats = out_mode == FLM_OUT_LANDMARKS_STATS;  // (adds only the all-pixel mode's three further partial sums)
  if (out_mode == FLM_OUT_LANDMARKS || stats) {
    W.probs = take(cur, sizeof(float) * (size_t)n * W.oh * W.ow * C);
    W.decode = take(cur, decode_ws_bytes(n, W.oh, W.ow, C, decode_mode, n_points, stats));
    if (landmark_candidates_enabled(co, g, A.fcn32, decode_mode, n_points, W.oh, W.ow)) {
      W.cand_sub = cand_sub_for(co, n_points, g.bf16 != 0);
      W.sub = take(cur, sizeof(unsigned) * (size_t)n * convt_sample_slots(g, h3, w3, W.cand_sub) * 16 * g.MT);  // sampled maxima
      W.tau = take(cur, sizeof(float) * (size_t)n * C);
      // expected keys per class: the n-th of 1/64 of the pixels ranks about 64*n-th overall; x4 head room
      // (never below one 64-key block: a huge cap_div then still takes the documented overflow fallback instead of
      // sizing an empty list, which the candidate launch rejects)
      W.cand_cap = (int)align_up((size_t)C * 64 * n_points * 4 / co.cap_div, 64);
      if (W.cand_cap < 64) W.cand_cap = 64;
      W.cand = take(cur, sizeof(unsigned long long) * (size_t)n * W.cand_cap);
      W.cand_cnt = take(cur, sizeof(unsigned) * ((size_t)n + 1));
      if (fb_faces > 0) {
        // per-face fallback (flm_fallback_opts): after cand_cnt, so no other name moves.  cand_redo follows cand_cnt
        // directly: one memset clears both.  The compact decode plans its chunks for B rows, so it has partials of its own.
        W.fb_faces = fb_faces < n ? fb_faces : n;
        W.cand_redo = take(cur, sizeof(unsigned) * (size_t)n);
        W.fb_rows = take(cur, sizeof(int) * (size_t)W.fb_faces);
        W.fb_counts = take(cur, sizeof(unsigned) * 6);
        W.fb_decode = take(cur, decode_ws_bytes(W.fb_faces, W.oh, W.ow, C, decode_mode, n_points, stats));
      }
    }
  }
  W.total = cur;
  return W;
}

// The operand type and class count every entry point takes; `what` names the entry point in the message.
static int check_dtype_classes(const char* what, int dtype, int C) {
  if (dtype != FLM_F32 && dtype != FLM_BF16) {
    set_error("%s: unknown dtype %d (FLM_F32 = 0, FLM_BF16 = 1)", what, dtype);
    return FLM_ERR_UNSUPPORTED;
  }
  if (C < 1 || C > kMaxClasses) {
    set_error("%s: n_classes must be in [1,%d] (got %d)", what, kMaxClasses, C);
    return FLM_ERR_SHAPE;
  }
  return FLM_OK;
}

static int check_fcn8_shape(int n, int h, int w, int C, int dtype) {
  const int rc = check_dtype_classes("fcn8", dtype, C);
  if (rc) return rc;
  if (n <= 0 || h <= 0 || w <= 0 || (h % 32) || (w % 32)) {
    set_error("fcn8: input must be [N>0, H, W, 3] with H and W multiples of 32 (got n=%d h=%d w=%d)", n, h, w);
    return FLM_ERR_SHAPE;
  }
  // (factors bounded first: the product below then fits 64 bits -- found by the UBSan sweep, tests/test_abi_sanitized.py)
  if (n > (1 << 24) || h > (1 << 15) || w > (1 << 15) || (long long)n * (h + 32) * (w + 32) * C >= (1ll << 40)) {
    set_error("fcn8: batch too large (n=%d h=%d w=%d: at most 2^40 output values per call)", n, h, w);
    return FLM_ERR_SHAPE;
  }
  return FLM_OK;
}

static int conv_layer(hipStream_t s, const char* blob, const ConvPack& c, const void* x, void* y, int n, int h,
                      int w, int relu, int pool, int posmajor, int dtype, int out_f32 = 0,
                      float* splitk_ws = nullptr, size_t splitk_bytes = 0, int stride = 1,
                      const void* res = nullptr) {
  IgemmDesc d;
  d.bf16 = dtype == FLM_BF16;
  d.out_f32 = out_f32;
  d.stride = stride;
  d.res = res;
  d.splitk_ws = splitk_ws;
  d.splitk_ws_bytes = splitk_bytes;
  d.x = x;
  d.wt = blob + c.w;
  d.scale = reinterpret_cast<const float*>(blob + c.scale);
  d.shift = reinterpret_cast<const float*>(blob + c.shift);
  d.y = y;
  d.n = n; d.h = h; d.w = w; d.cin = c.cin;
  d.cout = c.cout; d.coutpad = c.coutpad; d.ldc = c.cout;
  d.kh = c.kh; d.kw = c.kw; d.pad = c.pad;
  d.relu = relu; d.pool = pool; d.posmajor = posmajor;
  return launch_igemm(s, d);
}

// The decoder's transposed convs on an hi x wi input grid (networks/fcn.py).  up5 / up4 (fcn.py:104-119): stride 2, crop
// to 2hi x 2wi and Add in place onto the skip map y holds.  up3 (fcn.py:121; fcn_32's 64x64 stride-32 form, fcn.py:143-146):
// stride s = 8 | 32 to the raw [n, s*hi + s, s*wi + s, C] map; the caller sets another epilogue and its buffers.
static ConvTDesc up_desc(const Fcn8Pack& L, const char* blob, int layer, int n, int hi, int wi, const float* x, void* y) {
  ConvTDesc t;
  t.g = L.g;
  t.n = n; t.hi = hi; t.wi = wi;
  t.x = x; t.y = y;
  t.epilogue = 0;
  t.s = layer != 3 ? 2 : (L.spec.fcn32 ? 32 : 8);
  if (layer == 3) {
    t.wf = blob + L.up3; t.skip = nullptr;
    t.ho = t.s * hi + t.s; t.wo = t.s * wi + t.s; t.ldy = L.g.C;
  } else {
    t.wf = blob + (layer == 5 ? L.up5 : L.up4); t.skip = static_cast<const float*>(y);
    t.ho = 2 * hi; t.wo = 2 * wi; t.ldy = L.g.Cp;
  }
  return t;
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
  if (!key || !value) {
    set_error("flm_get_tuning: null argument");
    return FLM_ERR_ARG;
  }
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

static size_t packed_bytes_impl(int n_classes, int dtype, int arch) {
  if (check_dtype_classes("flm_fcn_packed_bytes", dtype, n_classes) || !arch_spec(arch).valid) return 0;
  return fcn8_pack_layout(n_classes, dtype, arch).total;
}
size_t flm_fcn_packed_bytes(int arch, int n_classes, int dtype) { return packed_bytes_impl(n_classes, dtype, arch); }
size_t flm_fcn8_packed_bytes(int n_classes, int dtype) { return packed_bytes_impl(n_classes, dtype, FLM_ARCH_FCN8); }
size_t flm_fcn32_packed_bytes(int n_classes, int dtype) { return packed_bytes_impl(n_classes, dtype, FLM_ARCH_FCN32); }

static int pack_impl(flm_stream_t stream, const flm_fcn_params* p, int n_classes, int dtype, void* packed_dev,
                     size_t packed_bytes, int arch) {
  if (!arch_spec(arch).valid) {
    set_error("flm_fcn_pack: unknown architecture %d", arch);
    return FLM_ERR_ARG;
  }
  if (!p || !packed_dev) {
    set_error("flm_fcn8_pack: null argument");
    return FLM_ERR_ARG;
  }
  const int rc = check_dtype_classes("flm_fcn8_pack", dtype, n_classes);
  if (rc) return rc;
  const Fcn8Pack L = fcn8_pack_layout(n_classes, dtype, arch);
  if (packed_bytes < L.total) {
    set_error("flm_fcn8_pack: packed buffer too small (%zu < %zu)", packed_bytes, L.total);
    return FLM_ERR_WORKSPACE;
  }
  return launch_pack_fcn(static_cast<hipStream_t>(stream), *p, n_classes, L, static_cast<char*>(packed_dev));
}
static flm_fcn_params from_fcn8(const flm_fcn8_params* p) {
  flm_fcn_params q;
  q.enc = p->enc;
  q.n_enc = 5;
  q.fc6 = p->fc6; q.fc7 = p->fc7; q.score5 = p->score5; q.score4 = p->score4; q.score3 = p->score3;
  q.up5 = p->up5; q.up4 = p->up4; q.up3 = p->up3;
  return q;
}
int flm_fcn_pack(flm_stream_t stream, int arch, const flm_fcn_params* p, int n_classes, int dtype, void* packed_dev,
                 size_t packed_bytes) {
  return pack_impl(stream, p, n_classes, dtype, packed_dev, packed_bytes, arch);
}
int flm_fcn8_pack(flm_stream_t stream, const flm_fcn8_params* p, int n_classes, int dtype, void* packed_dev,
                  size_t packed_bytes) {
  if (!p) {
    set_error("flm_fcn8_pack: null argument");
    return FLM_ERR_ARG;
  }
  const flm_fcn_params q = from_fcn8(p);
  return pack_impl(stream, &q, n_classes, dtype, packed_dev, packed_bytes, FLM_ARCH_FCN8);
}
int flm_fcn32_pack(flm_stream_t stream, const flm_fcn8_params* p, int n_classes, int dtype, void* packed_dev,
                   size_t packed_bytes) {
  if (!p) {
    set_error("flm_fcn32_pack: null argument");
    return FLM_ERR_ARG;
  }
  const flm_fcn_params q = from_fcn8(p);
  return pack_impl(stream, &q, n_classes, dtype, packed_dev, packed_bytes, FLM_ARCH_FCN32);
}

size_t flm_fcn8_workspace_bytes(int n, int h, int w, int n_classes, int dtype, int out_mode, int decode_mode,
                                int n_points) {
  if (check_fcn8_shape(n, h, w, n_classes, dtype)) return 0;
  return fcn8_ws_layout(n, h, w, n_classes, dtype, out_mode, decode_mode, n_points, FLM_ARCH_FCN8).total;
}
size_t flm_fcn32_workspace_bytes(int n, int h, int w, int n_classes, int dtype, int out_mode, int decode_mode,
                                 int n_points) {
  if (check_fcn8_shape(n, h, w, n_classes, dtype)) return 0;
  return fcn8_ws_layout(n, h, w, n_classes, dtype, out_mode, decode_mode, n_points, FLM_ARCH_FCN32).total;
}
size_t flm_fcn_workspace_bytes_fb(int arch, int n, int h, int w, int n_classes, int dtype, int out_mode,
                                  int decode_mode, int n_points, const flm_forward_opts* opts,
                                  const flm_fallback_opts* fb) {
  if (!arch_spec(arch).valid || check_fcn8_shape(n, h, w, n_classes, dtype)) return 0;
  return fcn8_ws_layout(n, h, w, n_classes, dtype, out_mode, decode_mode, n_points, arch, opts, fb).total;
}
size_t flm_fcn_workspace_bytes_opts(int arch, int n, int h, int w, int n_classes, int dtype, int out_mode,
                                    int decode_mode, int n_points, const flm_forward_opts* opts) {
  return flm_fcn_workspace_bytes_fb(arch, n, h, w, n_classes, dtype, out_mode, decode_mode, n_points, opts, nullptr);
}
void flm_fallback_opts_init(flm_fallback_opts* fb) {
  if (!fb) return;
  fb->struct_size = (uint32_t)sizeof(flm_fallback_opts);
  fb->faces = 0;
}
size_t flm_fcn_workspace_bytes(int arch, int n, int h, int w, int n_classes, int dtype, int out_mode, int decode_mode,
                               int n_points) {
  return flm_fcn_workspace_bytes_opts(arch, n, h, w, n_classes, dtype, out_mode, decode_mode, n_points, nullptr);
}
void flm_forward_opts_init(flm_forward_opts* opts) {
  if (!opts) return;
  opts->struct_size = (uint32_t)sizeof(flm_forward_opts);
  opts->landmark_candidates = 1;
  opts->candidate_sub_phases = 0;
  opts->candidate_cap_div = 1;
}

int64_t flm_fcn8_workspace_offset(const char* name, int n, int h, int w, int n_classes, int dtype, int out_mode,
                                  int decode_mode, int n_points) {
  return flm_fcn_workspace_offset_opts(FLM_ARCH_FCN8, name, n, h, w, n_classes, dtype, out_mode, decode_mode, n_points,
                                       nullptr);
}
int64_t flm_fcn8_workspace_offset_opts(const char* name, int n, int h, int w, int n_classes, int dtype, int out_mode,
                                       int decode_mode, int n_points, const flm_forward_opts* opts) {
  return flm_fcn_workspace_offset_opts(FLM_ARCH_FCN8, name, n, h, w, n_classes, dtype, out_mode, decode_mode, n_points,
                                       opts);
}
int64_t flm_fcn_workspace_offset_opts(int arch, const char* name, int n, int h, int w, int n_classes, int dtype,
                                      int out_mode, int decode_mode, int n_points, const flm_forward_opts* opts) {
  return flm_fcn_workspace_offset_fb(arch, name, n, h, w, n_classes, dtype, out_mode, decode_mode, n_points, opts, nullptr);
}
int64_t flm_fcn_workspace_offset_fb(int arch, const char* name, int n, int h, int w, int n_classes, int dtype,
                                    int out_mode, int decode_mode, int n_points, const flm_forward_opts* opts,
                                    const flm_fallback_opts* fb) {
  const ArchSpec A = arch_spec(arch);
  if (!name || !A.valid || check_fcn8_shape(n, h, w, n_classes, dtype)) return -1;
  const Fcn8Ws W = fcn8_ws_layout(n, h, w, n_classes, dtype, out_mode, decode_mode, n_points, arch, opts, fb);
  if (W.total == 0) return -1;
  if (!strcmp(name, "cand_redo")) return W.cand_redo == SIZE_MAX ? -1 : (int64_t)W.cand_redo;
  if (!strcmp(name, "fallback_rows")) return W.fb_rows == SIZE_MAX ? -1 : (int64_t)W.fb_rows;
  if (!strcmp(name, "fallback_counts")) return W.fb_counts == SIZE_MAX ? -1 : (int64_t)W.fb_counts;
  if (name[0] == 'f' && name[1] >= '1' && name[1] <= '5' && name[2] == 0) return (int64_t)W.f[name[1] - '1'];
  if (!strncmp(name, "act", 3) && name[3] >= '0' && name[3] <= '9') {  // "act<i>": encoder layer i of ArchSpec::enc
    int i = 0;
    const char* c = name + 3;
    for (; *c >= '0' && *c <= '9' && i < kMaxEnc; ++c) i = 10 * i + (*c - '0');
    return (*c == 0 && i < A.n_enc && !(name[3] == '0' && name[4] != 0)) ? (int64_t)W.act[i] : -1;
  }
  if (!strcmp(name, "cand_sub")) return W.sub == SIZE_MAX ? -1 : (int64_t)W.sub;
  if (!strcmp(name, "cand_tau")) return W.tau == SIZE_MAX ? -1 : (int64_t)W.tau;
  if (!strcmp(name, "cand_keys")) return W.cand == SIZE_MAX ? -1 : (int64_t)W.cand;
  if (!strcmp(name, "cand_cnt")) return W.cand_cnt == SIZE_MAX ? -1 : (int64_t)W.cand_cnt;
  if (!strcmp(name, "cand_cap")) return W.cand == SIZE_MAX ? -1 : (int64_t)W.cand_cap;
  if (!strcmp(name, "fc6")) return (int64_t)W.fc6;
  if (!strcmp(name, "fc7")) return (int64_t)W.fc7;
  if (!strcmp(name, "score5")) return (int64_t)W.score5;
  if (!strcmp(name, "fuse4")) return A.fcn32 ? -1 : (int64_t)W.fuse4;  // (the fcn_32 graphs have no skip stages)
  if (!strcmp(name, "seg_feats")) return A.fcn32 ? -1 : (int64_t)W.seg;
  if (!strcmp(name, "probs")) return W.probs == SIZE_MAX ? -1 : (int64_t)W.probs;
  return -1;
}

static_assert((int)FLM_ENC_FIRST3 == (int)ENC_FIRST3 && (int)FLM_ENC_CONV3 == (int)ENC_CONV3 &&
                  (int)FLM_ENC_MB_CONV1 == (int)ENC_MB_CONV1 && (int)FLM_ENC_MB_DW == (int)ENC_MB_DW &&
                  (int)FLM_ENC_MB_PW == (int)ENC_MB_PW && (int)FLM_ENC_RN_CONV1 == (int)ENC_RN_CONV1 &&
                  (int)FLM_ENC_MAXPOOL3 == (int)ENC_MAXPOOL3 && (int)FLM_ENC_CONV == (int)ENC_CONV,
              "flm_enc_kind mirrors EncKind");

int flm_fcn_encoder_layers(int arch) {
  const ArchSpec A = arch_spec(arch);
  if (!A.valid) {
    set_error("flm_fcn_encoder_layers: unknown architecture %d", arch);
    return -1;
  }
  return A.n_enc;
}

int flm_fcn_encoder_layer(int arch, int index, int h, int w, flm_enc_layer_info* info) {
  if (!info) {
    set_error("flm_fcn_encoder_layer: null argument");
    return FLM_ERR_ARG;
  }
  const ArchSpec A = arch_spec(arch);
  if (!A.valid) {
    set_error("flm_fcn_encoder_layer: unknown architecture %d", arch);
    return FLM_ERR_ARG;
  }
  if (index < 0 || index >= A.n_enc) {
    set_error("flm_fcn_encoder_layer: architecture %d has layers 0..%d (got %d)", arch, A.n_enc - 1, index);
    return FLM_ERR_ARG;
  }
  if (h <= 0 || w <= 0 || (h % 32) || (w % 32) || h > (1 << 15) || w > (1 << 15)) {
    set_error("flm_fcn_encoder_layer: H and W must be multiples of 32 up to 2^15 (got h=%d w=%d)", h, w);
    return FLM_ERR_SHAPE;
  }
  int hs[kMaxEnc], wsz[kMaxEnc];
  enc_dims(A, h, w, hs, wsz);
  const EncLayer& e = A.enc[index];
  const int src = e.src >= 0 ? e.src : index - 1;
  info->kind = e.kind;
  info->cin = e.cin;
  info->cout = e.cout;
  info->kernel = e.k;
  info->stride = e.stride;
  const bool relu6 = e.kind == ENC_MB_CONV1 || e.kind == ENC_MB_DW || e.kind == ENC_MB_PW;
  info->activation = e.kind == ENC_MAXPOOL3 ? 0 : (relu6 ? 2 : (e.kind == ENC_CONV ? (e.relu ? 1 : 0) : 1));
  info->pool = e.pool;
  info->src = src;
  info->res = e.res;
  info->in_h = src >= 0 ? hs[src] : h;
  info->in_w = src >= 0 ? wsz[src] : w;
  info->out_h = hs[index];
  info->out_w = wsz[index];
  return FLM_OK;
}

static int forward_impl(flm_stream_t stream, const void* packed_dev, const void* x_dev, int in_format, int n, int h,
                        int w, int C, int dtype, int out_mode, int decode_mode, int n_points, float thresh,
                        void* out_dev, void* workspace_dev, size_t workspace_bytes, int arch,
                        const flm_forward_opts* opts = nullptr, const flm_fallback_opts* fb = nullptr) {
  const ArchSpec A = arch_spec(arch);
  CandOpts co;
  int fb_faces = 0;
  if (!resolve_opts(opts, &co) || !resolve_fallback(fb, &fb_faces)) return FLM_ERR_ARG;
  if (!A.valid) {
    set_error("flm_fcn_forward: unknown architecture %d", arch);
    return FLM_ERR_ARG;
  }
  const int fcn32 = A.fcn32;
  if (!packed_dev || !x_dev || !out_dev || !workspace_dev) {
    set_error("flm_fcn8_forward: null argument");
    return FLM_ERR_ARG;
  }
  int rc = check_fcn8_shape(n, h, w, C, dtype);
  if (rc) return rc;
  if (out_mode < FLM_OUT_PROBS || out_mode > FLM_OUT_LANDMARKS_STATS) {
    set_error("flm_fcn8_forward: unknown output mode %d", out_mode);
    return FLM_ERR_ARG;
  }
  const Fcn8Ws W = fcn8_ws_layout(n, h, w, C, dtype, out_mode, decode_mode, n_points, arch, opts, fb);
  if (workspace_bytes < W.total) {
    set_error("flm_fcn8_forward: workspace too small (%zu < %zu)", workspace_bytes, W.total);
    return FLM_ERR_WORKSPACE;
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  const Fcn8Pack L = fcn8_pack_layout(C, dtype, arch);
  const int bf = dtype == FLM_BF16;
  const char* blob = static_cast<const char*>(packed_dev);
  char* ws = static_cast<char*>(workspace_dev);
  void* f[5];
  for (int i = 0; i < 5; ++i) f[i] = ws + W.f[i];
  void* fc6 = ws + W.fc6;
  void* fc7 = ws + W.fc7;
  float* score5 = reinterpret_cast<float*>(ws + W.score5);
  float* fuse4 = reinterpret_cast<float*>(ws + W.fuse4);
  float* seg = reinterpret_cast<float*>(ws + W.seg);

  const int h5 = h / 32, w5 = w / 32, h4 = h / 16, w4 = w / 16, h3 = h / 8, w3 = w / 8;
  // one implicit-GEMM layer of this call under the profile record `name` (null: the caller holds one), with the split-K
  // scratch where `splitk`
  const auto conv = [&](const char* name, const ConvPack& c, const void* x, void* y, int hh, int ww, int relu, int pool,
                        int posmajor, int out_f32, bool splitk) {
    ProfScope ps(s, name);
    return conv_layer(s, blob, c, x, y, n, hh, ww, relu, pool, posmajor, dtype, out_f32,
                      splitk ? reinterpret_cast<float*>(ws + W.splitk) : nullptr, splitk ? W.splitk_bytes : 0);
  };
  // encoder: vanilla (networks/fcn.py:10-51) or VGG16 (networks/vgg16.py:27-72)
  static const EncNames enc_name_table;  // "enc1".."enc64" (profile record labels); built once, thread-safe (C++11 statics)
  const char (*enc_names)[8] = enc_name_table.s;
  int hs[kMaxEnc], wsz[kMaxEnc];
  enc_dims(A, h, w, hs, wsz);
  {
    int h8 = hs[A.f_idx[2]], h16 = hs[A.f_idx[3]], h32 = hs[A.f_idx[4]];
    if (h8 != h / 8 || h16 != h / 16 || h32 != h / 32) {
      set_error("flm_fcn_forward: encoder grid %d/%d/%d does not match the decoder's H/8, H/16, H/32", h8, h16, h32);
      return FLM_ERR_SHAPE;
    }
  }
  for (int i = 0; i < A.n_enc; ++i) {
    const EncLayer& e = A.enc[i];
    const int src = e.src >= 0 ? e.src : i - 1;
    const void* xin = src >= 0 ? static_cast<const void*>(ws + W.act[src]) : x_dev;
    const int hi = src >= 0 ? hs[src] : h, wi = src >= 0 ? wsz[src] : w;
    void* yout = ws + W.act[i];
    const float* w0 = reinterpret_cast<const float*>(blob + (i == 0 ? L.enc1_w : L.enc[i].w));
    const float* sc0 = reinterpret_cast<const float*>(blob + (i == 0 ? L.enc1_scale : L.enc[i].scale));
    const float* sh0 = reinterpret_cast<const float*>(blob + (i == 0 ? L.enc1_shift : L.enc[i].shift));
    ProfScope ps(s, enc_names[i]);
    switch (e.kind) {
      case ENC_FIRST3:
        rc = launch_enc1(s, xin, in_format, n, hi, wi, w0, sc0, sh0, yout, bf, e.pool);
        break;
      case ENC_MB_CONV1:
        rc = launch_mb_conv1(s, xin, in_format, n, hi, wi, w0, sc0, sh0, yout, bf);
        break;
      case ENC_RN_CONV1:
        rc = launch_rn_conv1(s, xin, in_format, n, hi, wi, w0, sc0, sh0, yout, bf);
        break;
      case ENC_MAXPOOL3:
        rc = launch_maxpool3(s, xin, n, hi, wi, e.cin, yout, bf);
        break;
      case ENC_MB_DW:
        rc = launch_mb_depthwise(s, xin, n, hi, wi, e.cin, e.stride, w0, sc0, sh0, yout, bf);
        break;
      case ENC_CONV3:
        rc = conv(nullptr, L.enc[i], xin, yout, hi, wi, /*relu*/ 1, e.pool, 0, 0, true);
        break;
      case ENC_MB_PW:
        if (L.enc[i].cin != e.cin) {
          // pixel-pair form (flm_pack.hip): half as many "pixels", twice the channels.  A 1x1 conv sees a flat list
          // of pixels, so pairs may run across row ends: any even dimension can be the one that is halved
          int pn = n, ph = hi, pw = wi;
          if (!(pw & 1)) pw >>= 1;
          else if (!(ph & 1)) ph >>= 1;
          else if (!(pn & 1)) pn >>= 1;
          else {
            set_error("flm_fcn_forward: the paired pointwise conv needs an even number of pixels per batch");
            rc = FLM_ERR_SHAPE;
            break;
          }
          rc = conv_layer(s, blob, L.enc[i], xin, yout, pn, ph, pw, /*relu6*/ 2, 0, 0, dtype);
        } else {
          rc = conv_layer(s, blob, L.enc[i], xin, yout, n, hi, wi, /*relu6*/ 2, 0, 0, dtype);
        }
        break;
      case ENC_CONV:
        rc = conv_layer(s, blob, L.enc[i], xin, yout, n, hi, wi, e.relu, 0, 0, dtype, 0, nullptr, 0, e.stride,
                        e.res >= 0 ? ws + W.act[e.res] : nullptr);
        break;
      default:
        set_error("flm_fcn_forward: unknown encoder layer kind %d", e.kind);
        rc = FLM_ERR_ARG;
    }
    if (rc) return rc;
  }
  // head (fcn.py:98-103); Dropout is the identity at inference
  if ((rc = conv("fc6", L.fc6, f[4], fc6, h5, w5, 1, 0, /*posmajor*/ 1, 0, true))) return rc;
  if ((rc = conv("fc7", L.fc7, fc6, fc7, h5, w5, 1, 0, 0, 0, true))) return rc;
  if ((rc = conv("score5", L.score5, fc7, score5, h5, w5, 0, 0, 0, /*out_f32*/ 1, true))) return rc;
  if (!fcn32) {
    // skip branches: score4 on f4 -> fuse4 buffer, score3 on f3 -> seg buffer, then the transposed
    // convs add themselves onto those (crop keeps the top-left window, fcn.py:76-84)
    if ((rc = conv("score4", L.score4, f[3], fuse4, h4, w4, 0, 0, 0, 1, false))) return rc;
    const auto score3 = [&] { return conv("score3", L.score3, f[2], seg, h3, w3, 0, 0, 0, 1, false); };
    const auto up5 = [&] {  // up5 (fcn.py:104) + crop + Add (fcn.py:110-112), in place on fuse4
      ProfScope ps(s, "up5");
      return launch_convt(s, up_desc(L, blob, 5, n, h5, w5, score5, fuse4));
    };
    const auto up4 = [&] {  // up4 (fcn.py:114) + crop + Add (fcn.py:118-119), in place on seg ("seg_feats")
      ProfScope ps(s, "up4");
      return launch_convt(s, up_desc(L, blob, 4, n, h4, w4, fuse4, seg));
    };
    // (bf16, 68 classes: score3 and up4 run as ONE launch after up5, flm_tail_bf16.hip -- same bits)
    if (!(bf && L.g.C == 68 && L.score3.cin == 256 && L.score3.kh == 1)) {
      if ((rc = score3()) || (rc = up5()) || (rc = up4())) return rc;
    } else {
      if ((rc = up5())) return rc;
      int fused;
      { ProfScope ps(s, "seg_fused");
        fused = launch_seg_fused_bf16(s, fuse4, blob + L.up4, f[2], blob + L.score3.w,
                                      reinterpret_cast<const float*>(blob + L.score3.scale),
                                      reinterpret_cast<const float*>(blob + L.score3.shift), seg, n, h4, w4, L.g.C, L.g.Cp,
                                      L.g.G, L.score3.cin, L.score3.coutpad); }
      if (fused < 0) return fused;
      // (knob off, or a shape the fused kernel leaves alone: the two-launch form)
      if (!fused && ((rc = score3()) || (rc = up4()))) return rc;
    }
  }
  // last upsampling + softmax (networks/utils.py:30) / argmax (prediction.py:209):
  //   fcn_8 : Conv2DTranspose(16x16, s8) on seg_feats  (fcn.py:121)
  //   fcn_32: Conv2DTranspose(64x64, s32) on the 1x1 classifier output  (fcn.py:143-146)
  ConvTDesc t = fcn32 ? up_desc(L, blob, 3, n, h5, w5, score5, nullptr) : up_desc(L, blob, 3, n, h3, w3, seg, nullptr);
  if (out_mode == FLM_OUT_LOGITS || out_mode == FLM_OUT_PROBS) {
    t.y = out_dev;
    t.epilogue = (out_mode == FLM_OUT_PROBS) ? 1 : 0;
    if (out_mode == FLM_OUT_LOGITS && (C & 3)) {
      set_error("flm_fcn8_forward: FLM_OUT_LOGITS needs n_classes %% 4 == 0");
      return FLM_ERR_UNSUPPORTED;
    }
    ProfScope ps(s, "up3");
    return launch_convt(s, t);
  }
  if (out_mode == FLM_OUT_CLASSMAP) {
    t.y = out_dev;
    t.epilogue = 2;
    ProfScope ps(s, "up3");
    return launch_convt(s, t);
  }
  // landmarks (utils/metrics.py:102-109), as [n][C][2] or as landmark records
  const int stats = out_mode == FLM_OUT_LANDMARKS_STATS;
  float* probs = reinterpret_cast<float*>(ws + W.probs);
  const unsigned* gate = nullptr;
  if (W.cand != SIZE_MAX) {
    // top-n without the probability tensor (flm_convt.hip): thresholds from the phase-(0,0) sub-map, candidate
    // keys from the full launch, exact selection; then the materialising path below runs gated on the overflow flag
    float* sub = reinterpret_cast<float*>(ws + W.sub);
    float* tau = reinterpret_cast<float*>(ws + W.tau);
    unsigned* cnt = reinterpret_cast<unsigned*>(ws + W.cand_cnt);
    unsigned long long* cand = reinterpret_cast<unsigned long long*>(ws + W.cand);
    // per-face fallback (flm_fallback_opts): the flags lie right behind the counts, so the one memset clears both
    const int B = W.fb_faces;
    unsigned* redo = B ? reinterpret_cast<unsigned*>(ws + W.cand_redo) : nullptr;
    FLM_HIP(hipMemsetAsync(cnt, 0, B ? (W.cand_redo - W.cand_cnt) + sizeof(unsigned) * (size_t)n : sizeof(unsigned) * ((size_t)n + 1), s));
    ConvTDesc ts = t;
    ts.y = sub; ts.epilogue = 4; ts.sub = W.cand_sub;
    { ProfScope ps(s, "up3_sub");
    rc = launch_convt(s, ts); }
    if (rc) return rc;
    { ProfScope ps(s, "tau");
    rc = launch_cand_tau(s, reinterpret_cast<const unsigned*>(sub), n, convt_sample_slots(L.g, t.hi, t.wi, W.cand_sub), 16 * L.g.MT, C, n_points, tau); }
    if (rc) return rc;
    ConvTDesc tc = t;
    tc.y = nullptr; tc.epilogue = 3; tc.tau = tau; tc.cand = cand; tc.cand_cnt = cnt; tc.cand_cap = W.cand_cap;
    tc.cand_redo = redo;
    // (the probability region is written only by the gated fallback below, after this launch: its scratch until then)
    tc.scratch = probs; tc.scratch_bytes = sizeof(float) * (size_t)n * W.oh * W.ow * C;
    { ProfScope ps(s, "up3");
    rc = launch_convt(s, tc); }
    if (rc) return rc;
    { ProfScope ps(s, "decode");
    rc = launch_cand_merge(s, cand, cnt, n, W.ow, C, n_points, thresh, W.cand_cap, static_cast<double*>(out_dev), stats, redo); }
    if (rc) return rc;
    gate = cnt + n;  // overflow flag: non-zero -> redo this batch through the probability tensor
    if (B) {
      // only the faces that raised, as a compact batch of at most B rows (the first B rows of `probs`); more than B of
      // them: the whole-batch redo below, gated on the plan's batch_gate instead of the flag
      int* rows = reinterpret_cast<int*>(ws + W.fb_rows);
      unsigned* counts = reinterpret_cast<unsigned*>(ws + W.fb_counts);
      { ProfScope ps(s, "fallback_plan");
      rc = launch_fallback_plan(s, redo, n, B, rows, counts); }
      if (rc) return rc;
      ConvTDesc tr = t;
      tr.n = B; tr.y = probs; tr.epilogue = 1; tr.gate = counts + 4; tr.rows = rows; tr.rows_cnt = counts;
      { ProfScope ps(s, "up3_rows");
      rc = launch_convt(s, tr); }
      if (rc) return rc;
      { ProfScope ps(s, "decode_rows");
      rc = launch_decode(s, probs, B, W.oh, W.ow, C, decode_mode, n_points, thresh, static_cast<double*>(out_dev),
                         ws + W.fb_decode, decode_ws_bytes(B, W.oh, W.ow, C, decode_mode, n_points, stats), counts + 4, stats,
                         rows, counts); }
      if (rc) return rc;
      gate = counts + 5;
    }
    t.gate = gate;
  }
  t.y = probs;
  t.epilogue = 1;
  { ProfScope ps(s, gate ? "up3_fallback" : "up3");
  rc = launch_convt(s, t); }
  if (rc) return rc;
  ProfScope ps(s, gate ? "decode_fallback" : "decode");
  return launch_decode(s, probs, n, W.oh, W.ow, C, decode_mode, n_points, thresh,
                       static_cast<double*>(out_dev), ws + W.decode,
                       decode_ws_bytes(n, W.oh, W.ow, C, decode_mode, n_points, stats), gate, stats);
}

int flm_fcn8_run_layer(flm_stream_t stream, const void* packed_dev, const char* layer, const void* x_dev,
                       void* y_dev, int n, int h, int w, int C, int dtype) {
  if (!packed_dev || !layer || !x_dev || !y_dev || n <= 0 || h <= 0 || w <= 0) {
    set_error("flm_fcn8_run_layer: bad argument");
    return FLM_ERR_ARG;
  }
  if (check_dtype_classes("flm_fcn8_run_layer", dtype, C)) return FLM_ERR_UNSUPPORTED;
  const Fcn8Pack L = fcn8_pack_layout(C, dtype);
  const char* blob = static_cast<const char*>(packed_dev);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (!strncmp(layer, "enc", 3) && layer[3] >= '2' && layer[3] <= '5' && layer[4] == 0)
    return conv_layer(s, blob, L.enc[layer[3] - '1'], x_dev, y_dev, n, h, w, 1, 1, 0, dtype);
  if (!strcmp(layer, "fc6")) return conv_layer(s, blob, L.fc6, x_dev, y_dev, n, h, w, 1, 0, 1, dtype);
  if (!strcmp(layer, "fc7")) return conv_layer(s, blob, L.fc7, x_dev, y_dev, n, h, w, 1, 0, 0, dtype);
  if (!strcmp(layer, "score5")) return conv_layer(s, blob, L.score5, x_dev, y_dev, n, h, w, 0, 0, 0, dtype, 1);
  if (!strcmp(layer, "score4")) return conv_layer(s, blob, L.score4, x_dev, y_dev, n, h, w, 0, 0, 0, dtype, 1);
  if (!strcmp(layer, "score3")) return conv_layer(s, blob, L.score3, x_dev, y_dev, n, h, w, 0, 0, 0, dtype, 1);
  if (!strcmp(layer, "up5") || !strcmp(layer, "up4") || !strcmp(layer, "up3")) {
    // the decoder's transposed convs, as forward_impl launches them (always launch_convt, never the fused up4 + score3):
    // up5 / up4 crop + Add in place on the skip map y_dev holds, up3 writes raw logits [n,8h+8,8w+8,C]
    if (layer[2] == '3' && (C & 3)) {
      set_error("flm_fcn8_run_layer: \"up3\" writes raw logits, which needs n_classes %% 4 == 0");
      return FLM_ERR_UNSUPPORTED;
    }
    return launch_convt(s, up_desc(L, blob, layer[2] - '0', n, h, w, static_cast<const float*>(x_dev), y_dev));
  }
  set_error("flm_fcn8_run_layer: unknown layer '%s'", layer);
  return FLM_ERR_ARG;
}

int flm_fcn8_forward(flm_stream_t stream, const void* packed_dev, const void* x_dev, int in_format, int n, int h,
                     int w, int C, int dtype, int out_mode, int decode_mode, int n_points, float thresh,
                     void* out_dev, void* workspace_dev, size_t workspace_bytes) {
  return forward_impl(stream, packed_dev, x_dev, in_format, n, h, w, C, dtype, out_mode, decode_mode, n_points, thresh,
                      out_dev, workspace_dev, workspace_bytes, FLM_ARCH_FCN8);
}
int flm_fcn_forward_opts(flm_stream_t stream, int arch, const void* packed_dev, const void* x_dev, int in_format, int n,
                         int h, int w, int C, int dtype, int out_mode, int decode_mode, int n_points, float thresh,
                         void* out_dev, void* workspace_dev, size_t workspace_bytes, const flm_forward_opts* opts) {
  return flm_fcn_forward_fb(stream, arch, packed_dev, x_dev, in_format, n, h, w, C, dtype, out_mode, decode_mode, n_points,
                            thresh, out_dev, workspace_dev, workspace_bytes, opts, nullptr);
}
int flm_fcn_forward_fb(flm_stream_t stream, int arch, const void* packed_dev, const void* x_dev, int in_format, int n,
                       int h, int w, int C, int dtype, int out_mode, int decode_mode, int n_points, float thresh,
                       void* out_dev, void* workspace_dev, size_t workspace_bytes, const flm_forward_opts* opts,
                       const flm_fallback_opts* fb) {
  return forward_impl(stream, packed_dev, x_dev, in_format, n, h, w, C, dtype, out_mode, decode_mode, n_points, thresh,
                      out_dev, workspace_dev, workspace_bytes, arch, opts, fb);
}
int flm_fcn_forward(flm_stream_t stream, int arch, const void* packed_dev, const void* x_dev, int in_format, int n,
                    int h, int w, int C, int dtype, int out_mode, int decode_mode, int n_points, float thresh,
                    void* out_dev, void* workspace_dev, size_t workspace_bytes) {
  return forward_impl(stream, packed_dev, x_dev, in_format, n, h, w, C, dtype, out_mode, decode_mode, n_points, thresh,
                      out_dev, workspace_dev, workspace_bytes, arch);
}
int flm_fcn32_forward(flm_stream_t stream, const void* packed_dev, const void* x_dev, int in_format, int n, int h,
                      int w, int C, int dtype, int out_mode, int decode_mode, int n_points, float thresh,
                      void* out_dev, void* workspace_dev, size_t workspace_bytes) {
  return forward_impl(stream, packed_dev, x_dev, in_format, n, h, w, C, dtype, out_mode, decode_mode, n_points, thresh,
                      out_dev, workspace_dev, workspace_bytes, FLM_ARCH_FCN32);
}

int flm_preprocess(flm_stream_t stream, const uint8_t* img, int n, int h, int w, int norm, float* out) {
  if (!img || !out || n <= 0 || h <= 0 || w <= 0) {
    set_error("flm_preprocess: bad argument");
    return FLM_ERR_ARG;
  }
  return launch_preprocess(static_cast<hipStream_t>(stream), img, n, h, w, norm, out);
}

size_t flm_decode_workspace_bytes(int n, int h, int w, int l, int mode, int n_points) {
  if (n <= 0 || h <= 0 || w <= 0 || l <= 0) return 0;
  return decode_ws_bytes(n, h, w, l, mode, n_points);
}

int flm_decode(flm_stream_t stream, const float* hm, int n, int h, int w, int l, int mode, int n_points,
               float thresh, double* out, void* ws, size_t ws_bytes) {
  if (!hm || !out || !ws) {
    set_error("flm_decode: null argument");
    return FLM_ERR_ARG;
  }
  return launch_decode(static_cast<hipStream_t>(stream), hm, n, h, w, l, mode, n_points, thresh, out, ws, ws_bytes);
}

// (0 for what flm_decode_stats rejects: a shape outside the kernels' reach, an unknown mode, n_points outside [1,128])
size_t flm_decode_stats_workspace_bytes(int n, int h, int w, int l, int mode, int n_points) {
  if (n <= 0 || h <= 0 || w <= 0 || l <= 0 || l > kMaxClasses || (long long)h * w >= (1ll << 31)) return 0;
  if (mode != FLM_DECODE_ALL && (mode != FLM_DECODE_TOPN || n_points < 1 || n_points > 128)) return 0;
  return decode_ws_bytes(n, h, w, l, mode, n_points, 1);
}

int flm_decode_stats(flm_stream_t stream, const float* hm, int n, int h, int w, int l, int mode, int n_points,
                     float thresh, double* rec, void* ws, size_t ws_bytes) {
  if (!hm || !rec || !ws) {
    set_error("flm_decode_stats: null argument");
    return FLM_ERR_ARG;
  }
  return launch_decode(static_cast<hipStream_t>(stream), hm, n, h, w, l, mode, n_points, thresh, rec, ws, ws_bytes,
                       nullptr, 1);
}

size_t flm_decode_sweep_workspace_bytes(int n, int h, int w, int l, const int* modes, int n_modes) {
  return decode_sweep_ws_bytes(n, h, w, l, modes, n_modes);
}

int flm_decode_sweep(flm_stream_t stream, const float* hm, int n, int h, int w, int l, const int* modes, int n_modes,
                     float thresh, double* out, void* ws, size_t ws_bytes) {
  if (!hm || !out || !ws) {
    set_error("flm_decode_sweep: null argument");
    return FLM_ERR_ARG;
  }
  return launch_decode_sweep(static_cast<hipStream_t>(stream), hm, n, h, w, l, modes, n_modes, thresh, out, ws,
                             ws_bytes);
}

int flm_gaussian_heatmaps(flm_stream_t stream, const double* kp, int n, int l, int h, int w, double two_sigma_sq,
                          float* out) {
  if (!kp || !out) {
    set_error("flm_gaussian_heatmaps: null argument");
    return FLM_ERR_ARG;
  }
  return launch_gaussian_heatmaps(static_cast<hipStream_t>(stream), kp, n, l, h, w, two_sigma_sq, out);
}

int flm_similarity_from_landmarks(flm_stream_t stream, const double* lm, const double* tmpl, int n, int k,
                                  float* m) {
  if (!lm || !tmpl || !m) {
    set_error("flm_similarity_from_landmarks: null argument");
    return FLM_ERR_ARG;
  }
  return launch_similarity(static_cast<hipStream_t>(stream), lm, tmpl, n, k, 1.0, 1.0, m);
}

int flm_similarity_from_landmarks_scaled(flm_stream_t stream, const double* lm, const double* tmpl, int n, int k,
                                         double sx, double sy, float* m) {
  if (!lm || !tmpl || !m) {
    set_error("flm_similarity_from_landmarks_scaled: null argument");
    return FLM_ERR_ARG;
  }
  return launch_similarity(static_cast<hipStream_t>(stream), lm, tmpl, n, k, sx, sy, m);
}

int flm_similarity_from_landmarks_weighted(flm_stream_t stream, const double* lm, size_t lm_stride, const double* wt,
                                           size_t w_stride, const double* tmpl, int n, int k, double sx, double sy,
                                           float* m) {
  if (!lm || !tmpl || !m) {  // (wt is optional)
    set_error("flm_similarity_from_landmarks_weighted: null argument");
    return FLM_ERR_ARG;
  }
  return launch_similarity_weighted(static_cast<hipStream_t>(stream), lm, lm_stride, wt, w_stride, tmpl, n, k, sx, sy, m);
}

int flm_warp_affine(flm_stream_t stream, const void* src, int src_is_u8, int n, int hs, int ws, const float* m,
                    float* dst, int hd, int wd) {
  if (!src || !m || !dst) {
    set_error("flm_warp_affine: null argument");
    return FLM_ERR_ARG;
  }
  return launch_warp(static_cast<hipStream_t>(stream), src, src_is_u8, n, hs, ws, m, dst, hd, wd);
}

int flm_crop_resize(flm_stream_t stream, const uint8_t* frame, int fh, int fw, const int32_t* boxes, int k,
                    uint8_t* out, int oh, int ow) {
  if (!frame || !boxes || !out) {
    set_error("flm_crop_resize: null argument");
    return FLM_ERR_ARG;
  }
  return launch_crop_resize(static_cast<hipStream_t>(stream), frame, fh, fw, boxes, k, out, oh, ow);
}

int flm_crop_resize_frames(flm_stream_t stream, const uint8_t* frames, size_t frame_stride, int nframes, int fh, int fw,
                           const int32_t* boxes, const int32_t* frame_idx, int k, uint8_t* out, int oh, int ow) {
  if (!frames || !boxes || !frame_idx || !out) {
    set_error("flm_crop_resize_frames: null argument");
    return FLM_ERR_ARG;
  }
  return launch_crop_resize(static_cast<hipStream_t>(stream), frames, fh, fw, boxes, k, out, oh, ow, frame_idx,
                            frame_stride, nframes);
}

int flm_landmarks_to_frame(flm_stream_t stream, const double* lm, const int32_t* boxes, int k, int c, int grid_h,
                           int grid_w, int fh, int fw, double* out) {
  if (!lm || !boxes || !out) {
    set_error("flm_landmarks_to_frame: null argument");
    return FLM_ERR_ARG;
  }
  return launch_landmarks_to_frame(static_cast<hipStream_t>(stream), lm, boxes, k, c, grid_h, grid_w, fh, fw, out);
}

int flm_warp_affine_frames(flm_stream_t stream, const uint8_t* frames, size_t frame_stride, int nframes, int fh, int fw,
                           const int32_t* frame_idx, const int32_t* boxes, const float* m, int k, float* dst, int hd,
                           int wd, int samples) {
  if (!frames || !m || !dst) {  // frame_idx and boxes are optional
    set_error("flm_warp_affine_frames: null argument");
    return FLM_ERR_ARG;
  }
  return launch_warp_frames(static_cast<hipStream_t>(stream), frames, frame_stride, nframes, fh, fw, frame_idx, boxes, m,
                            k, dst, hd, wd, samples);
}

void flm_image_format_init(flm_image_format* fmt) {
  if (!fmt) return;
  fmt->struct_size = (uint32_t)sizeof(flm_image_format);
  fmt->layout = FLM_LAYOUT_NHWC;
  fmt->type = FLM_PIX_F32;
  fmt->reverse_channels = 0;
  for (int c = 0; c < 3; ++c) {
    fmt->scale[c] = 1.0f;
    fmt->bias[c] = 0.0f;
  }
}

// FLM_OK, or FLM_ERR_ARG with the reason in the message; `who` names the call.
static int check_image_format(const char* who, const flm_image_format* fmt) {
  if (!fmt) {
    set_error("%s: null format", who);
    return FLM_ERR_ARG;
  }
  if (fmt->struct_size < sizeof(flm_image_format)) {
    set_error("%s: flm_image_format struct_size %u is smaller than this library's %zu (initialise with "
              "flm_image_format_init)", who, fmt->struct_size, sizeof(flm_image_format));
    return FLM_ERR_ARG;
  }
  if (fmt->layout != FLM_LAYOUT_NHWC && fmt->layout != FLM_LAYOUT_NCHW) {
    set_error("%s: unknown layout %d", who, fmt->layout);
    return FLM_ERR_ARG;
  }
  if (fmt->type != FLM_PIX_F32 && fmt->type != FLM_PIX_F16 && fmt->type != FLM_PIX_BF16 && fmt->type != FLM_PIX_U8) {
    set_error("%s: unknown pixel type %d", who, fmt->type);
    return FLM_ERR_ARG;
  }
  if (fmt->reverse_channels != 0 && fmt->reverse_channels != 1) {
    set_error("%s: reverse_channels=%d (must be 0 or 1)", who, fmt->reverse_channels);
    return FLM_ERR_ARG;
  }
  for (int c = 0; c < 3; ++c) {
    if (!std::isfinite(fmt->scale[c]) || !std::isfinite(fmt->bias[c])) {
      set_error("%s: scale and bias must be finite (channel %d: %g, %g)", who, c, (double)fmt->scale[c],
                (double)fmt->bias[c]);
      return FLM_ERR_ARG;
    }
  }
  return FLM_OK;
}

// the destination needs the alignment of its element type, no more (a slice of a larger buffer is fine)
static int check_image_dst(const char* who, const void* dst, const flm_image_format* fmt) {
  const uintptr_t esize = fmt->type == FLM_PIX_F32 ? 4 : fmt->type == FLM_PIX_U8 ? 1 : 2;
  if (reinterpret_cast<uintptr_t>(dst) % esize) {
    set_error("%s: dst is not aligned to its %d-byte element", who, (int)esize);
    return FLM_ERR_ARG;
  }
  return FLM_OK;
}

size_t flm_image_format_bytes(const flm_image_format* fmt, int n, int h, int w) {
  if (check_image_format("flm_image_format_bytes", fmt) != FLM_OK) return 0;
  if (n < 1 || h < 1 || w < 1) {
    set_error("flm_image_format_bytes: n, h, w must be >= 1 (got %d, %d, %d)", n, h, w);
    return 0;
  }
  const size_t esize = fmt->type == FLM_PIX_F32 ? 4 : fmt->type == FLM_PIX_U8 ? 1 : 2;
  return (size_t)n * (size_t)h * (size_t)w * 3 * esize;
}

int flm_warp_affine_fmt(flm_stream_t stream, const void* src, int src_is_u8, int n, int hs, int ws, const float* m,
                        void* dst, int hd, int wd, const flm_image_format* fmt) {
  if (!src || !m || !dst) {
    set_error("flm_warp_affine_fmt: null argument");
    return FLM_ERR_ARG;
  }
  if (const int rc = check_image_format("flm_warp_affine_fmt", fmt)) return rc;
  if (const int rc = check_image_dst("flm_warp_affine_fmt", dst, fmt)) return rc;
  return launch_warp_fmt(static_cast<hipStream_t>(stream), src, src_is_u8, n, hs, ws, m, dst, hd, wd, fmt);
}

int flm_warp_affine_frames_fmt(flm_stream_t stream, const uint8_t* frames, size_t frame_stride, int nframes, int fh,
                               int fw, const int32_t* frame_idx, const int32_t* boxes, const float* m, int k, void* dst,
                               int hd, int wd, int samples, const flm_image_format* fmt) {
  if (!frames || !m || !dst) {  // frame_idx and boxes are optional
    set_error("flm_warp_affine_frames_fmt: null argument");
    return FLM_ERR_ARG;
  }
  if (const int rc = check_image_format("flm_warp_affine_frames_fmt", fmt)) return rc;
  if (const int rc = check_image_dst("flm_warp_affine_frames_fmt", dst, fmt)) return rc;
  return launch_warp_frames_fmt(static_cast<hipStream_t>(stream), frames, frame_stride, nframes, fh, fw, frame_idx, boxes,
                                m, k, dst, hd, wd, samples, fmt);
}

// ---- frame formats: the ring as the decoder hands it out (flm_frames_nv12.hip) -------------------------------

void flm_frame_format_init(flm_frame_format* src) {
  if (!src) return;
  src->struct_size = (uint32_t)sizeof(flm_frame_format);
  src->pixel = FLM_FRAME_BGR24;
  src->matrix = FLM_YUV_BT601_LIMITED;
  src->y_pitch = 0;
  src->uv_pitch = 0;
  src->uv_offset = 0;
}

// FLM_OK, FLM_ERR_ARG (null, struct_size, unknown pixel or matrix) or FLM_ERR_SHAPE (a BGR24 format that is not the
// dense ring); the sizes of an NV12 format are checked against the frame by the launchers.
static int check_frame_format(const char* who, const flm_frame_format* src) {
  if (!src) {
    set_error("%s: null frame format", who);
    return FLM_ERR_ARG;
  }
  if (src->struct_size < sizeof(flm_frame_format)) {
    set_error("%s: flm_frame_format struct_size %u is smaller than this library's %zu (initialise with "
              "flm_frame_format_init)", who, src->struct_size, sizeof(flm_frame_format));
    return FLM_ERR_ARG;
  }
  if (src->pixel != FLM_FRAME_BGR24 && src->pixel != FLM_FRAME_NV12) {
    set_error("%s: unknown frame pixel format %d", who, src->pixel);
    return FLM_ERR_ARG;
  }
  if (src->matrix != FLM_YUV_BT601_LIMITED && src->matrix != FLM_YUV_BT709_LIMITED) {
    set_error("%s: unknown YUV matrix %d", who, src->matrix);
    return FLM_ERR_ARG;
  }
  if (src->pixel == FLM_FRAME_BGR24 && (src->y_pitch || src->uv_pitch || src->uv_offset)) {
    set_error("%s: a BGR24 ring is dense: y_pitch, uv_pitch and uv_offset must be 0 (got %u, %u, %llu)", who,
              src->y_pitch, src->uv_pitch, (unsigned long long)src->uv_offset);
    return FLM_ERR_SHAPE;
  }
  return FLM_OK;
}

size_t flm_frame_format_bytes(const flm_frame_format* src, int fh, int fw) {
  if (check_frame_format("flm_frame_format_bytes", src) != FLM_OK) return 0;
  if (src->pixel == FLM_FRAME_NV12) return nv12_format_bytes("flm_frame_format_bytes", src, fh, fw);
  if (fh < 1 || fw < 1) {
    set_error("flm_frame_format_bytes: frame %dx%d, needs fh, fw >= 1", fh, fw);
    return 0;
  }
  return (size_t)fh * (size_t)fw * 3;
}

int flm_frames_to_bgr(flm_stream_t stream, const uint8_t* frames, size_t frame_stride, int nframes, int fh, int fw,
                      const flm_frame_format* src, uint8_t* out) {
  if (!frames || !out) {
    set_error("flm_frames_to_bgr: null argument");
    return FLM_ERR_ARG;
  }
  if (const int rc = check_frame_format("flm_frames_to_bgr", src)) return rc;
  if (src->pixel != FLM_FRAME_NV12) {
    set_error("flm_frames_to_bgr: the source is BGR24 already (pixel must be FLM_FRAME_NV12)");
    return FLM_ERR_ARG;
  }
  return launch_frames_to_bgr_nv12(static_cast<hipStream_t>(stream), frames, frame_stride, nframes, fh, fw, src, out);
}

int flm_crop_resize_frames_src(flm_stream_t stream, const uint8_t* frames, size_t frame_stride, int nframes, int fh,
                               int fw, const int32_t* boxes, const int32_t* frame_idx, int k, uint8_t* out, int oh,
                               int ow, const flm_frame_format* src) {
  if (!frames || !boxes || !frame_idx || !out) {
    set_error("flm_crop_resize_frames_src: null argument");
    return FLM_ERR_ARG;
  }
  if (const int rc = check_frame_format("flm_crop_resize_frames_src", src)) return rc;
  if (src->pixel == FLM_FRAME_BGR24)
    return launch_crop_resize(static_cast<hipStream_t>(stream), frames, fh, fw, boxes, k, out, oh, ow, frame_idx,
                              frame_stride, nframes);
  return launch_crop_resize_nv12(static_cast<hipStream_t>(stream), frames, frame_stride, nframes, fh, fw, boxes,
                                 frame_idx, k, out, oh, ow, src);
}

int flm_warp_affine_frames_src(flm_stream_t stream, const uint8_t* frames, size_t frame_stride, int nframes, int fh,
                               int fw, const int32_t* frame_idx, const int32_t* boxes, const float* m, int k, void* dst,
                               int hd, int wd, int samples, const flm_image_format* fmt, const flm_frame_format* src) {
  if (!frames || !m || !dst) {  // frame_idx and boxes are optional
    set_error("flm_warp_affine_frames_src: null argument");
    return FLM_ERR_ARG;
  }
  if (const int rc = check_frame_format("flm_warp_affine_frames_src", src)) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (src->pixel == FLM_FRAME_BGR24 && !fmt)  // flm_warp_affine_frames, its checks and no others
    return launch_warp_frames(s, frames, frame_stride, nframes, fh, fw, frame_idx, boxes, m, k, static_cast<float*>(dst), hd,
                              wd, samples);
  flm_image_format plain;  // fmt NULL: float32 NHWC BGR, scale 1, bias 0
  flm_image_format_init(&plain);
  if (fmt) {
    if (const int rc = check_image_format("flm_warp_affine_frames_src", fmt)) return rc;
  }
  if (const int rc = check_image_dst("flm_warp_affine_frames_src", dst, fmt ? fmt : &plain)) return rc;
  if (src->pixel == FLM_FRAME_BGR24)
    return launch_warp_frames_fmt(s, frames, frame_stride, nframes, fh, fw, frame_idx, boxes, m, k, dst, hd, wd, samples,
                                  fmt);
  return launch_warp_frames_nv12(s, frames, frame_stride, nframes, fh, fw, frame_idx, boxes, m, k, dst, hd, wd, samples,
                                 fmt ? fmt : &plain, src);
}

// ---- the piecewise-affine warp over the landmark mesh (flm_mesh.hip) -------------------------------------------------

int flm_mesh_map(flm_stream_t stream, const double* pts, const int32_t* tris, int p, int t, int hd, int wd,
                 uint8_t* map) {
  if (!pts || !tris || !map) {
    set_error("flm_mesh_map: null argument");
    return FLM_ERR_ARG;
  }
  return launch_mesh_map(static_cast<hipStream_t>(stream), pts, tris, p, t, hd, wd, map);
}

int flm_mesh_affines(flm_stream_t stream, const double* lm, int lm_stride, const float* m, const double* pts,
                     const int32_t* tris, int p, int a, int t, int k, double min_det, float* aff) {
  if (!lm || !m || !pts || !tris || !aff) {
    set_error("flm_mesh_affines: null argument");
    return FLM_ERR_ARG;
  }
  return launch_mesh_affines(static_cast<hipStream_t>(stream), lm, lm_stride, m, pts, tris, p, a, t, k, min_det, aff);
}

int flm_warp_mesh_frames(flm_stream_t stream, const uint8_t* frames, size_t frame_stride, int nframes, int fh, int fw,
                         const int32_t* frame_idx, const int32_t* boxes, const double* lm, int lm_stride, const float* m,
                         const double* pts, const int32_t* tris, int p, int a, int t, const uint8_t* map, int k,
                         void* dst, int hd, int wd, int samples, const flm_image_format* fmt,
                         const flm_frame_format* src, double min_det, float* aff_out) {
  if (!frames || !lm || !m || !pts || !tris || !map || !dst) {  // frame_idx, boxes, fmt, src and aff_out are optional
    set_error("flm_warp_mesh_frames: null argument");
    return FLM_ERR_ARG;
  }
  flm_frame_format bgr;  // src NULL: the dense BGR ring
  flm_frame_format_init(&bgr);
  if (src) {
    if (const int rc = check_frame_format("flm_warp_mesh_frames", src)) return rc;
  }
  flm_image_format plain;  // fmt NULL: float32 NHWC BGR, scale 1, bias 0
  flm_image_format_init(&plain);
  if (fmt) {
    if (const int rc = check_image_format("flm_warp_mesh_frames", fmt)) return rc;
  }
  if (const int rc = check_image_dst("flm_warp_mesh_frames", dst, fmt ? fmt : &plain)) return rc;
  return launch_warp_mesh_frames(static_cast<hipStream_t>(stream), frames, frame_stride, nframes, fh, fw, frame_idx, boxes,
                                 lm, lm_stride, m, pts, tris, p, a, t, map, k, dst, hd, wd, samples, fmt ? fmt : &plain,
                                 src ? src : &bgr, min_det, aff_out);
}

// ---- tracking (flm_track.hip) ------------------------------------------------------------------------------------

void flm_track_opts_init(flm_track_opts* opts) {
  if (!opts) return;
  opts->struct_size = (uint32_t)sizeof(flm_track_opts);
  opts->min_points = 2;
  opts->min_score = 0.0;
  opts->min_side = 0.0;
  opts->max_side = HUGE_VAL;
}

int flm_track_seed(flm_stream_t stream, const int32_t* boxes, int k, int in_h, int in_w, int fh, int fw, float* m,
                   int32_t* status) {
  if (!boxes || !m || !status) {
    set_error("flm_track_seed: null argument");
    return FLM_ERR_ARG;
  }
  return launch_track_seed(static_cast<hipStream_t>(stream), boxes, k, in_h, in_w, fh, fw, m, status);
}

int flm_landmarks_from_crop(flm_stream_t stream, const double* lm, size_t lm_stride, const float* m, int k, int c,
                            double sx, double sy, double* out) {
  if (!lm || !m || !out) {
    set_error("flm_landmarks_from_crop: null argument");
    return FLM_ERR_ARG;
  }
  return launch_landmarks_from_crop(static_cast<hipStream_t>(stream), lm, lm_stride, m, k, c, sx, sy, out);
}

// The pointer and option checks of the three step entry points; *opts is replaced by `defaults` when null.
static int check_track_step_args(const char* who, const double* lm, const float* m_crop, const int32_t* boxes,
                                 const double* tmpl_crop, const double* tmpl_align, const flm_track_opts** opts,
                                 flm_track_opts* defaults, const double* lm_frame, const float* m_align,
                                 const float* m_next, const int32_t* boxes_next, const int32_t* status) {
  if (!lm || !m_crop || !boxes || !tmpl_crop || !lm_frame || !m_next || !boxes_next || !status) {  // (wt is optional)
    set_error("%s: null argument", who);
    return FLM_ERR_ARG;
  }
  if ((tmpl_align == nullptr) != (m_align == nullptr)) {
    set_error("%s: tmpl_align_dev and m_align_dev go together (both or neither)", who);
    return FLM_ERR_ARG;
  }
  flm_track_opts_init(defaults);
  if (!*opts) *opts = defaults;
  const flm_track_opts* o = *opts;
  if (o->struct_size < sizeof(flm_track_opts)) {
    set_error("%s: flm_track_opts struct_size %u is smaller than this library's %zu (initialise with "
              "flm_track_opts_init)", who, o->struct_size, sizeof(flm_track_opts));
    return FLM_ERR_ARG;
  }
  if (o->min_points < 2) {
    set_error("%s: min_points=%d, needs min_points >= 2 (a similarity takes two points)", who, o->min_points);
    return FLM_ERR_ARG;
  }
  if (std::isnan(o->min_score) || std::isnan(o->min_side) || std::isnan(o->max_side)) {
    set_error("%s: min_score, min_side and max_side must not be NaN (got %g, %g, %g)", who, o->min_score, o->min_side,
              o->max_side);
    return FLM_ERR_ARG;
  }
  return FLM_OK;
}

void flm_track_filter_init(flm_track_filter* filt) {
  if (!filt) return;
  filt->struct_size = (uint32_t)sizeof(flm_track_filter);
  filt->reserved = 0;
  filt->min_cutoff = 1.0;
  filt->beta = 15.0;
  filt->d_cutoff = 1.0;
}

// The checks of a flm_track_filter.
static int check_track_filter(const char* who, const flm_track_filter* filt) {
  if (filt->struct_size < sizeof(flm_track_filter)) {
    set_error("%s: flm_track_filter struct_size %u is smaller than this library's %zu (initialise with "
              "flm_track_filter_init)", who, filt->struct_size, sizeof(flm_track_filter));
    return FLM_ERR_ARG;
  }
  if (filt->reserved != 0) {
    set_error("%s: flm_track_filter reserved=%u, must be 0", who, filt->reserved);
    return FLM_ERR_ARG;
  }
  if (!(filt->min_cutoff > 0.0)) {
    set_error("%s: min_cutoff=%g, needs min_cutoff > 0 (+inf switches the smoothing off)", who, filt->min_cutoff);
    return FLM_ERR_ARG;
  }
  if (!(filt->beta >= 0.0 && std::isfinite(filt->beta))) {
    set_error("%s: beta=%g, needs a finite beta >= 0", who, filt->beta);
    return FLM_ERR_ARG;
  }
  if (!(filt->d_cutoff > 0.0 && std::isfinite(filt->d_cutoff))) {
    set_error("%s: d_cutoff=%g, needs a finite d_cutoff > 0", who, filt->d_cutoff);
    return FLM_ERR_ARG;
  }
  return FLM_OK;
}

static bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
  return a0 < b0 + nb && b0 < a0 + na;
}

// The three step entry points, stated once.  need_filt: filt must be given (flm_track_step_filtered; flm_track_step has
// none to give, flm_track_step_rows may or may not).  rows: the call is flm_track_step_rows -- slot and status_rows
// must be given, dt_rows may replace the scalar dt, and the compact inputs must not overlap what is written at the slots.
static int track_step(const char* who, bool need_filt, bool rows, flm_stream_t stream, const double* lm, size_t lm_stride,
                      const double* wt, size_t w_stride, const float* m_crop, const int32_t* boxes, int k, int c, double sx,
                      double sy, int in_h, int in_w, int fh, int fw, const double* tmpl_crop, const double* tmpl_align,
                      const flm_track_opts* opts, double* lm_frame, float* m_align, float* m_next, int32_t* boxes_next,
                      int32_t* status, const flm_track_filter* filt, double dt, double* state, double* lm_raw,
                      const int32_t* slot, int n_slots, const double* dt_rows, int32_t* status_rows) {
  flm_track_opts defaults;
  if (const int rc = check_track_step_args(who, lm, m_crop, boxes, tmpl_crop, tmpl_align, &opts, &defaults, lm_frame, m_align,
                                           m_next, boxes_next, status))
    return rc;
  if (rows && (!slot || !status_rows)) {
    set_error("%s: null %s", who, !slot ? "slot_dev" : "status_rows_dev");
    return FLM_ERR_ARG;
  }
  if (filt || need_filt) {
    if (!filt || !state) {  // (lm_raw is optional)
      set_error("%s: null %s", who, !filt ? "filt" : "state_dev");
      return FLM_ERR_ARG;
    }
    if (const int rc = check_track_filter(who, filt)) return rc;
    if (!dt_rows && !(dt > 0.0 && std::isfinite(dt))) {
      set_error("%s: dt=%g, needs a finite dt > 0 (seconds since the previous step)%s", who, dt, rows ? " or dt_dev" : "");
      return FLM_ERR_ARG;
    }
  } else if (state || lm_raw || dt_rows) {
    set_error("%s: state_dev, lm_raw_dev and dt_dev go with filt", who);
    return FLM_ERR_ARG;
  }
  // the compact inputs must not be the tensors the step writes at the slots (the snapshot exists to keep them apart)
  if (rows && k >= 1 && k <= 65535 && n_slots >= 1 && n_slots <= 65535 &&
      (ranges_overlap(m_crop, (size_t)k * 24, m_next, (size_t)n_slots * 24) ||
       ranges_overlap(boxes, (size_t)k * 16, boxes_next, (size_t)n_slots * 16) ||
       ranges_overlap(status_rows, (size_t)k * 4, status, (size_t)n_slots * 4))) {
    set_error("%s: m_crop_c/m_next, boxes_c/boxes_next or status_rows/status overlap (rows are read while slots are "
              "written: gather a snapshot first)", who);
    return FLM_ERR_ARG;
  }
  return launch_track_step(static_cast<hipStream_t>(stream), who, lm, lm_stride, wt, w_stride, m_crop, boxes, k, c, sx, sy, in_h,
                           in_w, fh, fw, tmpl_crop, tmpl_align, opts, lm_frame, m_align, m_next, boxes_next, status, filt, dt,
                           state, lm_raw, slot, n_slots, dt_rows, status_rows);
}

int flm_track_step(flm_stream_t stream, const double* lm, size_t lm_stride, const double* wt, size_t w_stride,
                   const float* m_crop, const int32_t* boxes, int k, int c, double sx, double sy, int in_h, int in_w,
                   int fh, int fw, const double* tmpl_crop, const double* tmpl_align, const flm_track_opts* opts,
                   double* lm_frame, float* m_align, float* m_next, int32_t* boxes_next, int32_t* status) {
  return track_step("flm_track_step", false, false, stream, lm, lm_stride, wt, w_stride, m_crop, boxes, k, c, sx, sy, in_h,
                    in_w, fh, fw, tmpl_crop, tmpl_align, opts, lm_frame, m_align, m_next, boxes_next, status, nullptr, 0.0,
                    nullptr, nullptr, nullptr, 0, nullptr, nullptr);
}

int flm_track_step_filtered(flm_stream_t stream, const double* lm, size_t lm_stride, const double* wt, size_t w_stride,
                            const float* m_crop, const int32_t* boxes, int k, int c, double sx, double sy, int in_h,
                            int in_w, int fh, int fw, const double* tmpl_crop, const double* tmpl_align,
                            const flm_track_opts* opts, double* lm_frame, float* m_align, float* m_next,
                            int32_t* boxes_next, int32_t* status, const flm_track_filter* filt, double dt, double* state,
                            double* lm_raw) {
  return track_step("flm_track_step_filtered", true, false, stream, lm, lm_stride, wt, w_stride, m_crop, boxes, k, c, sx, sy,
                    in_h, in_w, fh, fw, tmpl_crop, tmpl_align, opts, lm_frame, m_align, m_next, boxes_next, status, filt, dt,
                    state, lm_raw, nullptr, 0, nullptr, nullptr);
}

int flm_track_step_rows(flm_stream_t stream, const double* lm, size_t lm_stride, const double* wt, size_t w_stride,
                        const float* m_crop_c, const int32_t* boxes_c, int n, int c, double sx, double sy, int in_h,
                        int in_w, int fh, int fw, const double* tmpl_crop, const double* tmpl_align,
                        const flm_track_opts* opts, double* lm_frame, float* m_align, float* m_next, int32_t* boxes_next,
                        int32_t* status, const flm_track_filter* filt, double dt, double* state, double* lm_raw,
                        const int32_t* slot, int n_slots, const double* dt_rows, int32_t* status_rows) {
  return track_step("flm_track_step_rows", false, true, stream, lm, lm_stride, wt, w_stride, m_crop_c, boxes_c, n, c, sx, sy,
                    in_h, in_w, fh, fw, tmpl_crop, tmpl_align, opts, lm_frame, m_align, m_next, boxes_next, status, filt, dt,
                    state, lm_raw, slot, n_slots, dt_rows, status_rows);
}

int flm_track_gather_streams(flm_stream_t stream, const int32_t* active, int a, int s, int k,
                             const int32_t* frame_idx_stream, const double* dt_stream, const float* m_crop,
                             const int32_t* boxes, const double* best_q, int32_t* reset, int32_t* slot_c, float* m_c,
                             int32_t* boxes_c, int32_t* frame_idx_c, double* dt_c, double* best_q_c, int32_t* reset_c) {
  const char* who = "flm_track_gather_streams";
  if (!active || !m_crop || !boxes || !slot_c || !m_c || !boxes_c || !frame_idx_c) {
    set_error("%s: null argument", who);  // (frame_idx_stream and the three optional groups may be null)
    return FLM_ERR_ARG;
  }
  if ((dt_stream == nullptr) != (dt_c == nullptr) || (best_q == nullptr) != (best_q_c == nullptr) ||
      (reset == nullptr) != (reset_c == nullptr)) {
    set_error("%s: dt_stream_dev/dt_c, best_q_dev/best_q_c and reset_dev/reset_c go together (both or neither)", who);
    return FLM_ERR_ARG;
  }
  return launch_track_gather_streams(static_cast<hipStream_t>(stream), active, a, s, k, frame_idx_stream, dt_stream, m_crop,
                                     boxes, best_q, reset, slot_c, m_c, boxes_c, frame_idx_c, dt_c, best_q_c, reset_c);
}

int flm_track_gather_live(flm_stream_t stream, const int32_t* stream_on, int s, int k, int fh, int fw, int n,
                          const int32_t* frame_idx_stream, const double* dt_stream, double dt, const float* m_crop,
                          const int32_t* boxes, const double* best_q, int32_t* reset, double* age, int32_t* cursor,
                          int32_t* slot_c, float* m_c, int32_t* boxes_c, int32_t* frame_idx_c, double* dt_c,
                          double* best_q_c, int32_t* reset_c, int32_t* counts) {
  const char* who = "flm_track_gather_live";
  if (!m_crop || !boxes || !slot_c || !m_c || !boxes_c || !frame_idx_c || !counts) {
    set_error("%s: null argument", who);  // (stream_on, frame_idx_stream, cursor and the three optional groups may be null)
    return FLM_ERR_ARG;
  }
  if ((age == nullptr) != (dt_c == nullptr) || (best_q == nullptr) != (best_q_c == nullptr) ||
      (reset == nullptr) != (reset_c == nullptr)) {
    set_error("%s: age_dev/dt_c, best_q_dev/best_q_c and reset_dev/reset_c go together (both or neither)", who);
    return FLM_ERR_ARG;
  }
  if (dt_stream && !age) {
    set_error("%s: dt_stream_dev goes with age_dev", who);
    return FLM_ERR_ARG;
  }
  if (age && !dt_stream && !(dt > 0.0 && std::isfinite(dt))) {
    set_error("%s: dt=%g, needs a finite dt > 0 (seconds since the previous step) or dt_stream_dev", who, dt);
    return FLM_ERR_ARG;
  }
  TrackLiveArgs g;
  g.boxes = boxes; g.m_crop = m_crop; g.s = s; g.k = k; g.fh = fh; g.fw = fw; g.n = n;
  g.stream_on = stream_on; g.frame_idx_stream = frame_idx_stream; g.dt_stream = dt_stream; g.dt = dt;
  g.best_q = best_q; g.reset = reset; g.age = age; g.cursor = cursor;
  g.slot_c = slot_c; g.m_c = m_c; g.boxes_c = boxes_c; g.frame_idx_c = frame_idx_c;
  g.dt_c = dt_c; g.best_q_c = best_q_c; g.reset_c = reset_c; g.counts = counts;
  return launch_track_gather_live(static_cast<hipStream_t>(stream), g);
}

// ---- association (flm_track_assoc.hip) ------------------------------------------------------------------------------

void flm_track_assoc_opts_init(flm_track_assoc_opts* opts) {
  if (!opts) return;
  opts->struct_size = (uint32_t)sizeof(flm_track_assoc_opts);
  opts->max_misses = 0;
  opts->square = 1;
  opts->reserved = 0;
  opts->match_iou = 0.3;
  opts->dup_iou = 0.7;
  opts->refresh_iou = 0.0;
}

// The checks flm_track_associate and flm_track_associate_streams share; *opts is replaced by `defaults` when null.
static int track_assoc_check(const char* who, const void* det, const void* m_crop, const void* boxes, const void* status,
                             const void* misses, const void* det_slot, const void* slot_det, const void* counts,
                             const flm_track_assoc_opts** opts, flm_track_assoc_opts* defaults) {
  if (!det || !m_crop || !boxes || !status || !misses || !det_slot || !slot_det || !counts) {
    set_error("%s: null argument", who);  // (n_det_dev, state_dev and opts are optional)
    return FLM_ERR_ARG;
  }
  flm_track_assoc_opts_init(defaults);
  if (!*opts) *opts = defaults;
  if ((*opts)->struct_size < sizeof(flm_track_assoc_opts)) {
    set_error("%s: flm_track_assoc_opts struct_size %u is smaller than this library's %zu (initialise with "
              "flm_track_assoc_opts_init)", who, (*opts)->struct_size, sizeof(flm_track_assoc_opts));
    return FLM_ERR_ARG;
  }
  if ((*opts)->reserved != 0) {
    set_error("%s: flm_track_assoc_opts reserved=%d, must be 0", who, (*opts)->reserved);
    return FLM_ERR_ARG;
  }
  return FLM_OK;
}

static int track_assoc_check_sizes(const char* who, int d, int k, int c, bool has_state, int in_h, int in_w, int fh, int fw,
                                   const flm_track_assoc_opts* opts) {
  if (k < 1 || k > 1024) {
    set_error("%s: k=%d, needs 1 <= k <= 1024", who, k);
    return FLM_ERR_SHAPE;
  }
  if (d < 1 || d > 1024) {
    set_error("%s: d=%d, needs 1 <= d <= 1024", who, d);
    return FLM_ERR_SHAPE;
  }
  if (has_state && (c < 1 || c > 1024)) {
    set_error("%s: c=%d, needs 1 <= c <= 1024", who, c);
    return FLM_ERR_SHAPE;
  }
  if (in_h < 1 || in_w < 1 || fh < 1 || fw < 1) {
    set_error("%s: input %dx%d, frame %dx%d, needs in_h, in_w, fh, fw >= 1", who, in_h, in_w, fh, fw);
    return FLM_ERR_SHAPE;
  }
  if ((int64_t)fh * (int64_t)fw > (int64_t(1) << 30)) {
    set_error("%s: frame %dx%d, needs fh*fw <= 2^30 (the pair order is exact in int64 up to there)", who, fh, fw);
    return FLM_ERR_SHAPE;
  }
  if (opts->max_misses < 0) {
    set_error("%s: max_misses=%d, needs max_misses >= 0 (0 = never)", who, opts->max_misses);
    return FLM_ERR_SHAPE;
  }
  if (std::isnan(opts->match_iou) || std::isnan(opts->dup_iou) || std::isnan(opts->refresh_iou)) {
    set_error("%s: match_iou, dup_iou and refresh_iou must not be NaN (got %g, %g, %g)", who, opts->match_iou,
              opts->dup_iou, opts->refresh_iou);
    return FLM_ERR_SHAPE;
  }
  return FLM_OK;
}

int flm_track_associate(flm_stream_t stream, const int32_t* det, const int32_t* n_det, int d, int k, int c, int in_h,
                        int in_w, int fh, int fw, const flm_track_assoc_opts* opts, float* m_crop, int32_t* boxes,
                        int32_t* status, int32_t* misses, double* state, int32_t* det_slot, int32_t* slot_det,
                        int32_t* counts) {
  const char* who = "flm_track_associate";
  flm_track_assoc_opts defaults;
  int rc = track_assoc_check(who, det, m_crop, boxes, status, misses, det_slot, slot_det, counts, &opts, &defaults);
  if (rc != FLM_OK) return rc;
  rc = track_assoc_check_sizes(who, d, k, c, state != nullptr, in_h, in_w, fh, fw, opts);
  if (rc != FLM_OK) return rc;
  return launch_track_associate(static_cast<hipStream_t>(stream), det, n_det, d, k, c, in_h, in_w, fh, fw, opts, m_crop,
                                boxes, status, misses, state, det_slot, slot_det, counts);
}

int flm_track_associate_streams(flm_stream_t stream, const int32_t* det, const int32_t* n_det, int s, int d, int k, int c,
                                int in_h, int in_w, int fh, int fw, const flm_track_assoc_opts* opts, float* m_crop,
                                int32_t* boxes, int32_t* status, int32_t* misses, double* state, int32_t* det_slot,
                                int32_t* slot_det, int32_t* counts) {
  const char* who = "flm_track_associate_streams";
  flm_track_assoc_opts defaults;
  int rc = track_assoc_check(who, det, m_crop, boxes, status, misses, det_slot, slot_det, counts, &opts, &defaults);
  if (rc != FLM_OK) return rc;
  if (s < 1) {
    set_error("%s: s=%d, needs 1 <= s", who, s);
    return FLM_ERR_SHAPE;
  }
  if (k >= 1 && (int64_t)s * (int64_t)k > 65535) {
    set_error("%s: s=%d streams of k=%d slots, needs s*k <= 65535 (the capacity of the warps and the tracker)", who, s, k);
    return FLM_ERR_SHAPE;
  }
  rc = track_assoc_check_sizes(who, d, k, c, state != nullptr, in_h, in_w, fh, fw, opts);
  if (rc != FLM_OK) return rc;
  return launch_track_associate_streams(static_cast<hipStream_t>(stream), det, n_det, s, d, k, c, in_h, in_w, fh, fw, opts,
                                        m_crop, boxes, status, misses, state, det_slot, slot_det, counts);
}

// ---- best shot (flm_quality.hip) ------------------------------------------------------------------------------------

void flm_quality_opts_init(flm_quality_opts* opts) {
  if (!opts) return;
  opts->struct_size = (uint32_t)sizeof(flm_quality_opts);
  opts->dark = 16;
  opts->bright = 239;
}

int flm_face_quality(flm_stream_t stream, const void* faces, int k, int h, int w, const flm_image_format* fmt,
                     const flm_quality_opts* opts, int64_t* rec) {
  const char* who = "flm_face_quality";
  if (!faces || !rec) {
    set_error("%s: null argument", who);  // (fmt and opts are optional)
    return FLM_ERR_ARG;
  }
  flm_image_format plain;
  flm_image_format_init(&plain);
  if (!fmt) fmt = &plain;
  if (const int rc = check_image_format(who, fmt)) return rc;
  const uintptr_t esize = fmt->type == FLM_PIX_F32 ? 4 : fmt->type == FLM_PIX_U8 ? 1 : 2;
  if (reinterpret_cast<uintptr_t>(faces) % esize) {
    set_error("%s: faces is not aligned to its %d-byte element", who, (int)esize);
    return FLM_ERR_ARG;
  }
  for (int c = 0; c < 3; ++c) {
    if (fmt->scale[c] == 0.0f) {
      set_error("%s: scale[%d] is 0, needs a scale that can be undone (scale != 0)", who, c);
      return FLM_ERR_ARG;
    }
  }
  flm_quality_opts defaults;
  flm_quality_opts_init(&defaults);
  if (!opts) opts = &defaults;
  if (opts->struct_size < sizeof(flm_quality_opts)) {
    set_error("%s: flm_quality_opts struct_size %u is smaller than this library's %zu (initialise with "
              "flm_quality_opts_init)", who, opts->struct_size, sizeof(flm_quality_opts));
    return FLM_ERR_ARG;
  }
  if (opts->dark < 0 || opts->dark > 255 || opts->bright < 0 || opts->bright > 255) {
    set_error("%s: dark=%d, bright=%d, needs both in [0, 255]", who, opts->dark, opts->bright);
    return FLM_ERR_ARG;
  }
  return launch_face_quality(static_cast<hipStream_t>(stream), faces, k, h, w, fmt, opts, rec);
}

void flm_best_opts_init(flm_best_opts* opts) {
  if (!opts) return;
  opts->struct_size = (uint32_t)sizeof(flm_best_opts);
  opts->reserved = 0;
  opts->sharp_ref = 100.0;
  opts->min_exposed = 0.5;
}

// The option and size checks flm_track_best_update and flm_track_best_update_rows share; *popts is replaced by `defaults`
// when null.  kname: what the call names its number of faces.
static int check_best_args(const char* who, const flm_best_opts** popts, flm_best_opts* defaults, const char* kname, int k,
                           int c, size_t face_bytes, size_t lm_stride, const double* wt, size_t w_stride) {
  flm_best_opts_init(defaults);
  if (!*popts) *popts = defaults;
  const flm_best_opts* opts = *popts;
  if (opts->struct_size < sizeof(flm_best_opts)) {
    set_error("%s: flm_best_opts struct_size %u is smaller than this library's %zu (initialise with "
              "flm_best_opts_init)", who, opts->struct_size, sizeof(flm_best_opts));
    return FLM_ERR_ARG;
  }
  if (opts->reserved != 0) {
    set_error("%s: flm_best_opts reserved=%d, must be 0", who, opts->reserved);
    return FLM_ERR_ARG;
  }
  if (!(opts->sharp_ref > 0.0)) {
    set_error("%s: sharp_ref=%g, needs sharp_ref > 0", who, opts->sharp_ref);
    return FLM_ERR_ARG;
  }
  if (std::isnan(opts->min_exposed)) {
    set_error("%s: min_exposed must not be NaN", who);
    return FLM_ERR_ARG;
  }
  if (k < 1 || k > 65535) {
    set_error("%s: %s=%d, needs 1 <= %s <= 65535", who, kname, k, kname);
    return FLM_ERR_SHAPE;
  }
  if (c < 1) {
    set_error("%s: c=%d, needs c >= 1", who, c);
    return FLM_ERR_SHAPE;
  }
  if (face_bytes < 1) {
    set_error("%s: face_bytes=0, needs face_bytes >= 1", who);
    return FLM_ERR_SHAPE;
  }
  if (lm_stride < 2 || (wt && w_stride < 1)) {
    set_error("%s: lm_stride=%zu, w_stride=%zu, needs lm_stride >= 2 and w_stride >= 1", who, lm_stride, w_stride);
    return FLM_ERR_SHAPE;
  }
  return FLM_OK;
}

int flm_track_best_update(flm_stream_t stream, const void* faces, size_t face_bytes, int k, const int64_t* rec,
                          const int32_t* status, const int32_t* reset, const double* lm, size_t lm_stride,
                          const double* wt, size_t w_stride, int c, const double* factor, const float* m,
                          int64_t frame_id, const flm_best_opts* opts, const double* best_q_in, double* best_q_out,
                          void* gallery, int64_t* best_frame, float* best_m, double* best_lm, int64_t* best_rec) {
  const char* who = "flm_track_best_update";
  if (!faces || !rec || !lm || !best_q_in || !best_q_out || !gallery || !best_frame) {
    set_error("%s: null argument", who);  // (status, reset, w, factor, m, opts and the last three outputs are optional)
    return FLM_ERR_ARG;
  }
  if (best_m && !m) {
    set_error("%s: best_m_dev needs m_dev", who);
    return FLM_ERR_ARG;
  }
  flm_best_opts defaults;
  if (const int rc = check_best_args(who, &opts, &defaults, "k", k, c, face_bytes, lm_stride, wt, w_stride)) return rc;
  if (ranges_overlap(best_q_in, (size_t)k * sizeof(double), best_q_out, (size_t)k * sizeof(double))) {
    set_error("%s: best_q_in and best_q_out overlap (every workgroup of a slot reads best_q_in: swap two buffers)", who);
    return FLM_ERR_ARG;
  }
  if (ranges_overlap(faces, (size_t)k * face_bytes, gallery, (size_t)k * face_bytes)) {
    set_error("%s: faces_dev and gallery_dev overlap", who);
    return FLM_ERR_ARG;
  }
  return launch_track_best_update(static_cast<hipStream_t>(stream), faces, face_bytes, k, rec, status, reset, lm, lm_stride,
                                  wt, w_stride, c, factor, m, frame_id, opts, nullptr, 0, best_q_in, best_q_out, gallery,
                                  best_frame, best_m, best_lm, best_rec);
}

int flm_track_best_update_rows(flm_stream_t stream, const void* faces, size_t face_bytes, int n, const int64_t* rec,
                               const int32_t* status_rows, const int32_t* reset_c, const double* lm, size_t lm_stride,
                               const double* wt, size_t w_stride, int c, const double* factor, const float* m,
                               int64_t frame_id, const flm_best_opts* opts, const int32_t* slot, int n_slots,
                               const double* best_q_c, double* best_q, void* gallery, int64_t* best_frame, float* best_m,
                               double* best_lm, int64_t* best_rec) {
  const char* who = "flm_track_best_update_rows";
  if (!faces || !rec || !lm || !slot || !best_q_c || !best_q || !gallery || !best_frame) {
    set_error("%s: null argument", who);  // (status, reset, w, factor, m, opts and the last three outputs are optional)
    return FLM_ERR_ARG;
  }
  if (best_m && !m) {
    set_error("%s: best_m_dev needs m_dev", who);
    return FLM_ERR_ARG;
  }
  flm_best_opts defaults;
  if (const int rc = check_best_args(who, &opts, &defaults, "n", n, c, face_bytes, lm_stride, wt, w_stride)) return rc;
  if (n_slots < 1 || n_slots > 65535) {
    set_error("%s: n_slots=%d, needs 1 <= n_slots <= 65535", who, n_slots);
    return FLM_ERR_SHAPE;
  }
  if (ranges_overlap(best_q_c, (size_t)n * sizeof(double), best_q, (size_t)n_slots * sizeof(double))) {
    set_error("%s: best_q_c and best_q overlap (every workgroup of a row reads best_q_c: it is the snapshot)", who);
    return FLM_ERR_ARG;
  }
  if (ranges_overlap(faces, (size_t)n * face_bytes, gallery, (size_t)n_slots * face_bytes)) {
    set_error("%s: faces_dev and gallery_dev overlap", who);
    return FLM_ERR_ARG;
  }
  return launch_track_best_update(static_cast<hipStream_t>(stream), faces, face_bytes, n, rec, status_rows, reset_c, lm,
                                  lm_stride, wt, w_stride, c, factor, m, frame_id, opts, slot, n_slots, best_q_c, best_q,
                                  gallery, best_frame, best_m, best_lm, best_rec);
}

// ---- finished tracks (flm_track_exit.hip) -----------------------------------------------------------------------------

void flm_exit_opts_init(flm_exit_opts* opts) {
  if (!opts) return;
  opts->struct_size = (uint32_t)sizeof(flm_exit_opts);
  opts->reserved = 0;
  opts->min_q = 0.0;
}

int flm_track_retire(flm_stream_t stream, const int32_t* boxes, const int32_t* status, int k, int fh, int fw,
                     const double* best_q, const void* gallery, size_t face_bytes, const int64_t* best_frame,
                     const float* best_m, const double* best_lm, int c, const int64_t* best_rec, int64_t frame_id,
                     int flush, const flm_exit_opts* opts, int32_t* born, int64_t* track_id, int64_t* born_frame,
                     int64_t* head, int q, void* x_gallery, int64_t* x_meta, double* x_q, float* x_m, double* x_lm,
                     int64_t* x_rec, int32_t* exit_row) {
  const char* who = "flm_track_retire";
  if (!boxes || !status || !best_q || !gallery || !best_frame || !born || !track_id || !born_frame || !head ||
      !x_gallery || !x_meta || !x_q || !exit_row) {
    set_error("%s: null argument", who);  // (opts and the three pairs best_m/x_m, best_lm/x_lm, best_rec/x_rec are optional)
    return FLM_ERR_ARG;
  }
  if (!best_m != !x_m || !best_lm != !x_lm || !best_rec != !x_rec) {
    set_error("%s: best_m_dev goes with x_m, best_lm_dev with x_lm and best_rec_dev with x_rec: both or neither", who);
    return FLM_ERR_ARG;
  }
  flm_exit_opts defaults;
  flm_exit_opts_init(&defaults);
  if (!opts) opts = &defaults;
  if (opts->struct_size < sizeof(flm_exit_opts)) {
    set_error("%s: flm_exit_opts struct_size %u is smaller than this library's %zu (initialise with "
              "flm_exit_opts_init)", who, opts->struct_size, sizeof(flm_exit_opts));
    return FLM_ERR_ARG;
  }
  if (opts->reserved != 0) {
    set_error("%s: flm_exit_opts reserved=%u, must be 0", who, opts->reserved);
    return FLM_ERR_ARG;
  }
  if (!(opts->min_q >= 0.0)) {
    set_error("%s: min_q=%g, needs min_q >= 0", who, opts->min_q);
    return FLM_ERR_ARG;
  }
  if (k < 1 || k > 65535) {
    set_error("%s: k=%d, needs 1 <= k <= 65535", who, k);
    return FLM_ERR_SHAPE;
  }
  if (q < 1 || q > 65535) {
    set_error("%s: q=%d, needs 1 <= q <= 65535", who, q);
    return FLM_ERR_SHAPE;
  }
  if (c < 1 || c > 1024) {
    set_error("%s: c=%d, needs 1 <= c <= 1024", who, c);
    return FLM_ERR_SHAPE;
  }
  if (face_bytes < 1) {
    set_error("%s: face_bytes=0, needs face_bytes >= 1", who);
    return FLM_ERR_SHAPE;
  }
  if (fh < 1 || fw < 1) {
    set_error("%s: frame %dx%d, needs fh, fw >= 1", who, fh, fw);
    return FLM_ERR_SHAPE;
  }
  const size_t sk = (size_t)k, sq = (size_t)q, sc = (size_t)c;
  const struct { const void* p; size_t bytes; const char* name; } bufs[] = {
      {boxes, sk * 16, "boxes_dev"}, {status, sk * 4, "status_dev"}, {best_q, sk * 8, "best_q_dev"},
      {gallery, sk * face_bytes, "gallery_dev"}, {best_frame, sk * 8, "best_frame_dev"}, {best_m, sk * 24, "best_m_dev"},
      {best_lm, sk * sc * 16, "best_lm_dev"}, {best_rec, sk * FLM_QUALITY_REC * 8, "best_rec_dev"},
      {born, sk * 4, "born_dev"}, {track_id, sk * 8, "track_id_dev"}, {born_frame, sk * 8, "born_frame_dev"},
      {head, 4 * 8, "head_dev"}, {x_gallery, sq * face_bytes, "x_gallery"}, {x_meta, sq * FLM_EXIT_META * 8, "x_meta"},
      {x_q, sq * 8, "x_q"}, {x_m, sq * 24, "x_m"}, {x_lm, sq * sc * 16, "x_lm"},
      {x_rec, sq * FLM_QUALITY_REC * 8, "x_rec"}, {exit_row, sk * 4, "exit_row_dev"}};
  const int nb = (int)(sizeof(bufs) / sizeof(bufs[0]));
  for (int i = 0; i < nb; ++i)
    for (int j = i + 1; j < nb; ++j)
      if (bufs[i].p && bufs[j].p && ranges_overlap(bufs[i].p, bufs[i].bytes, bufs[j].p, bufs[j].bytes)) {
        set_error("%s: %s and %s overlap (no two arguments may)", who, bufs[i].name, bufs[j].name);
        return FLM_ERR_ARG;
      }
  TrackExitArgs g;
  g.boxes = boxes; g.status = status; g.k = k; g.fh = fh; g.fw = fw; g.c = c; g.q = q;
  g.face_bytes = face_bytes;
  g.best_q = best_q; g.gallery = static_cast<const unsigned char*>(gallery); g.best_frame = best_frame;
  g.best_m = best_m; g.best_lm = best_lm; g.best_rec = best_rec;
  g.frame_id = frame_id; g.flush = flush; g.min_q = opts->min_q;
  g.born = born; g.track_id = track_id; g.born_frame = born_frame; g.head = head;
  g.x_gallery = static_cast<unsigned char*>(x_gallery); g.x_meta = x_meta; g.x_q = x_q;
  g.x_m = x_m; g.x_lm = x_lm; g.x_rec = x_rec; g.exit_row = exit_row;
  return launch_track_retire(static_cast<hipStream_t>(stream), g);
}

// ---- head pose (flm_pose.hip) ---------------------------------------------------------------------------------------

void flm_pose_opts_init(flm_pose_opts* opts) {
  if (!opts) return;
  opts->struct_size = (uint32_t)sizeof(flm_pose_opts);
  opts->reserved = 0;
  opts->min_volume = 1e-6;
  opts->min_frontal = 0.0;
}

int flm_head_pose(flm_stream_t stream, const double* lm, size_t lm_stride, const double* wt, size_t w_stride, int n, int c,
                  const int32_t* idx, const double* xyz, int p, const flm_pose_opts* opts, const int32_t* slot,
                  int n_slots, double* pose, double* factor) {
  const char* who = "flm_head_pose";
  if (!lm || !idx || !xyz || !pose) {
    set_error("%s: null argument", who);  // (w, opts, slot and factor_out are optional)
    return FLM_ERR_ARG;
  }
  flm_pose_opts defaults;
  flm_pose_opts_init(&defaults);
  if (!opts) opts = &defaults;
  if (opts->struct_size < sizeof(flm_pose_opts)) {
    set_error("%s: flm_pose_opts struct_size %u is smaller than this library's %zu (initialise with "
              "flm_pose_opts_init)", who, opts->struct_size, sizeof(flm_pose_opts));
    return FLM_ERR_ARG;
  }
  if (opts->reserved != 0) {
    set_error("%s: flm_pose_opts reserved=%u, must be 0", who, opts->reserved);
    return FLM_ERR_ARG;
  }
  if (!(opts->min_volume >= 0.0)) {
    set_error("%s: min_volume=%g, needs min_volume >= 0", who, opts->min_volume);
    return FLM_ERR_ARG;
  }
  if (!(opts->min_frontal >= 0.0 && opts->min_frontal <= 1.0)) {
    set_error("%s: min_frontal=%g, needs 0 <= min_frontal <= 1", who, opts->min_frontal);
    return FLM_ERR_ARG;
  }
  if (n < 1 || n > 65535) {
    set_error("%s: n=%d, needs 1 <= n <= 65535", who, n);
    return FLM_ERR_SHAPE;
  }
  if (c < 1 || c > 1024) {
    set_error("%s: c=%d, needs 1 <= c <= 1024", who, c);
    return FLM_ERR_SHAPE;
  }
  if (p < 4 || p > 256) {
    set_error("%s: p=%d, needs 4 <= p <= 256", who, p);
    return FLM_ERR_SHAPE;
  }
  if (lm_stride < 2 || (wt && w_stride < 1)) {
    set_error("%s: lm_stride=%zu, w_stride=%zu, needs lm_stride >= 2 and w_stride >= 1", who, lm_stride, w_stride);
    return FLM_ERR_SHAPE;
  }
  if (slot && (n_slots < 1 || n_slots > 65535)) {
    set_error("%s: n_slots=%d, needs 1 <= n_slots <= 65535", who, n_slots);
    return FLM_ERR_SHAPE;
  }
  const size_t last = (size_t)n * c - 1;  // the last landmark read
  const struct { const void* p; size_t bytes; const char* name; } in[] = {
      {lm, (last * lm_stride + 2) * sizeof(double), "lm_dev"},
      {wt, wt ? (last * w_stride + 1) * sizeof(double) : 0, "w_dev"},
      {idx, (size_t)p * sizeof(int32_t), "idx_dev"},
      {xyz, (size_t)p * 3 * sizeof(double), "xyz_dev"},
      {slot, slot ? (size_t)n * sizeof(int32_t) : 0, "slot_dev"}};
  const size_t pose_bytes = (size_t)(slot ? n_slots : n) * FLM_POSE_REC * sizeof(double);
  const size_t factor_bytes = factor ? (size_t)n * sizeof(double) : 0;
  for (const auto& a : in) {
    if (!a.p) continue;
    if (ranges_overlap(pose, pose_bytes, a.p, a.bytes) || (factor && ranges_overlap(factor, factor_bytes, a.p, a.bytes))) {
      set_error("%s: pose_dev or factor_out overlaps %s", who, a.name);
      return FLM_ERR_ARG;
    }
  }
  if (factor && ranges_overlap(pose, pose_bytes, factor, factor_bytes)) {
    set_error("%s: pose_dev and factor_out overlap", who);
    return FLM_ERR_ARG;
  }
  return launch_head_pose(static_cast<hipStream_t>(stream), lm, lm_stride, wt, w_stride, n, c, idx, xyz, p, opts, slot,
                          n_slots, pose, factor);
}

// ---- pose-binned best shots (flm_track_views.hip) -------------------------------------------------------------------

void flm_views_opts_init(flm_views_opts* opts) {
  if (!opts) return;
  memset(opts, 0, sizeof(*opts));
  opts->struct_size = (uint32_t)sizeof(flm_views_opts);
  opts->sharp_ref = 100.0;
  opts->min_exposed = 0.5;
  opts->n_u = 2;
  opts->u_edge[0] = -0.3420201433256687;  // -+sin(20 degrees): right, frontal, left
  opts->u_edge[1] = 0.3420201433256687;
  opts->n_v = 0;
}

static int check_view_edges(const char* who, const char* axis, int n, const double* edge) {
  if (n < 0 || n > FLM_VIEWS_MAX_EDGES) {
    set_error("%s: n_%s=%d, needs 0 <= n_%s <= %d", who, axis, n, axis, FLM_VIEWS_MAX_EDGES);
    return FLM_ERR_ARG;
  }
  for (int i = 0; i < n; ++i) {
    if (!(edge[i] > -1.0 && edge[i] < 1.0)) {  // (false for a NaN and for an infinity)
      set_error("%s: %s_edge[%d]=%g, needs a finite edge inside (-1, 1)", who, axis, i, edge[i]);
      return FLM_ERR_ARG;
    }
    if (i > 0 && !(edge[i] > edge[i - 1])) {
      set_error("%s: %s_edge[%d]=%g after %g, needs strictly ascending edges", who, axis, i, edge[i], edge[i - 1]);
      return FLM_ERR_ARG;
    }
  }
  return FLM_OK;
}

struct NamedRange {
  const void* p;
  size_t bytes;
  const char* name;
};

int flm_track_views_update(flm_stream_t stream, const void* faces, size_t face_bytes, int n, const int64_t* rec,
                           const int32_t* status_rows, const int32_t* reset, const double* lm, size_t lm_stride,
                           const double* wt, size_t w_stride, int c, const float* m, int64_t frame_id,
                           const flm_views_opts* opts, const int32_t* slot, int n_slots, const double* pose, double* view_q,
                           int64_t* view_frame, void* view_gallery, float* view_m, double* view_lm, double* view_pose,
                           int32_t* take) {
  const char* who = "flm_track_views_update";
  if (!faces || !rec || !lm || !pose || !view_q || !view_frame || !view_gallery || !take) {
    set_error("%s: null argument", who);  // (status, reset, w, m, opts, slot and the three view_m/lm/pose are optional)
    return FLM_ERR_ARG;
  }
  if (view_m && !m) {
    set_error("%s: view_m needs m_dev", who);
    return FLM_ERR_ARG;
  }
  flm_views_opts defaults;
  flm_views_opts_init(&defaults);
  if (!opts) opts = &defaults;
  if (opts->struct_size < sizeof(flm_views_opts)) {
    set_error("%s: flm_views_opts struct_size %u is smaller than this library's %zu (initialise with "
              "flm_views_opts_init)", who, opts->struct_size, sizeof(flm_views_opts));
    return FLM_ERR_ARG;
  }
  if (opts->reserved != 0) {
    set_error("%s: flm_views_opts reserved=%u, must be 0", who, opts->reserved);
    return FLM_ERR_ARG;
  }
  if (!(opts->sharp_ref > 0.0)) {
    set_error("%s: sharp_ref=%g, needs sharp_ref > 0", who, opts->sharp_ref);
    return FLM_ERR_ARG;
  }
  if (std::isnan(opts->min_exposed)) {
    set_error("%s: min_exposed must not be NaN", who);
    return FLM_ERR_ARG;
  }
  if (const int rc = check_view_edges(who, "u", opts->n_u, opts->u_edge)) return rc;
  if (const int rc = check_view_edges(who, "v", opts->n_v, opts->v_edge)) return rc;
  if (n < 1 || n > 65535) {
    set_error("%s: n=%d, needs 1 <= n <= 65535", who, n);
    return FLM_ERR_SHAPE;
  }
  if (slot && (n_slots < 1 || n_slots > 65535)) {
    set_error("%s: n_slots=%d, needs 1 <= n_slots <= 65535", who, n_slots);
    return FLM_ERR_SHAPE;
  }
  if (!slot) n_slots = n;
  if (c < 1 || c > 1024) {
    set_error("%s: c=%d, needs 1 <= c <= 1024", who, c);
    return FLM_ERR_SHAPE;
  }
  if (face_bytes < 1) {
    set_error("%s: face_bytes=0, needs face_bytes >= 1", who);
    return FLM_ERR_SHAPE;
  }
  if (lm_stride < 2 || (wt && w_stride < 1)) {
    set_error("%s: lm_stride=%zu, w_stride=%zu, needs lm_stride >= 2 and w_stride >= 1", who, lm_stride, w_stride);
    return FLM_ERR_SHAPE;
  }
  const int bins = (opts->n_u + 1) * (opts->n_v + 1);
  const size_t sn = (size_t)n, ss = (size_t)n_slots * bins, sc = (size_t)c;
  const size_t last = sn * sc - 1;  // the last landmark read
  const NamedRange in[] = {
      {faces, sn * face_bytes, "faces_dev"}, {rec, sn * FLM_QUALITY_REC * 8, "rec_dev"},
      {status_rows, sn * 4, "status_rows_dev"}, {reset, sn * 4, "reset_dev"},
      {lm, (last * lm_stride + 2) * sizeof(double), "lm_dev"}, {wt, (last * w_stride + 1) * sizeof(double), "w_dev"},
      {m, sn * 24, "m_dev"}, {slot, sn * 4, "slot_dev"}, {pose, (size_t)n_slots * FLM_POSE_REC * 8, "pose_dev"}};
  const NamedRange out[] = {
      {view_q, ss * 8, "view_q"}, {view_frame, ss * 8, "view_frame"}, {view_gallery, ss * face_bytes, "view_gallery"},
      {view_m, ss * 24, "view_m"}, {view_lm, ss * sc * 16, "view_lm"}, {view_pose, ss * FLM_POSE_REC * 8, "view_pose"},
      {take, sn * 4, "take_dev"}};
  const int n_out = (int)(sizeof(out) / sizeof(out[0]));
  for (int i = 0; i < n_out; ++i) {
    if (!out[i].p) continue;
    for (const auto& a : in)
      if (a.p && ranges_overlap(out[i].p, out[i].bytes, a.p, a.bytes)) {
        set_error("%s: %s and %s overlap (no output may overlap an input)", who, out[i].name, a.name);
        return FLM_ERR_ARG;
      }
    for (int j = i + 1; j < n_out; ++j)
      if (out[j].p && ranges_overlap(out[i].p, out[i].bytes, out[j].p, out[j].bytes)) {
        set_error("%s: %s and %s overlap (no two outputs may)", who, out[i].name, out[j].name);
        return FLM_ERR_ARG;
      }
  }
  TrackViewsArgs g;
  g.faces = static_cast<const unsigned char*>(faces);
  g.face_bytes = face_bytes;
  g.n = n; g.n_slots = n_slots; g.c = c; g.bins = bins;
  g.rec = rec; g.status = status_rows; g.reset = reset;
  g.lm = lm; g.lm_stride = lm_stride; g.wt = wt; g.w_stride = w_stride; g.m = m; g.frame_id = frame_id;
  g.sharp_ref = opts->sharp_ref; g.min_exposed = opts->min_exposed;
  g.n_u = opts->n_u; g.n_v = opts->n_v;
  for (int i = 0; i < FLM_VIEWS_MAX_EDGES; ++i) {  // (the edges not in use are never compared: zeros keep the struct defined)
    g.u_edge[i] = i < opts->n_u ? opts->u_edge[i] : 0.0;
    g.v_edge[i] = i < opts->n_v ? opts->v_edge[i] : 0.0;
  }
  g.slot = slot; g.pose = pose;
  g.view_q = view_q; g.view_frame = view_frame; g.view_gallery = static_cast<unsigned char*>(view_gallery);
  g.view_m = view_m; g.view_lm = view_lm; g.view_pose = view_pose; g.take = take;
  return launch_track_views_update(static_cast<hipStream_t>(stream), g);
}

int flm_track_exit_views(flm_stream_t stream, const int32_t* exit_row, int k, int q, int bins, size_t face_bytes, int c,
                         const double* view_q, const int64_t* view_frame, const void* view_gallery, const float* view_m,
                         const double* view_lm, const double* view_pose, double* x_view_q, int64_t* x_view_frame,
                         void* x_view_gallery, float* x_view_m, double* x_view_lm, double* x_view_pose) {
  const char* who = "flm_track_exit_views";
  if (!exit_row || !view_q || !view_frame || !view_gallery || !x_view_q || !x_view_frame || !x_view_gallery) {
    set_error("%s: null argument", who);  // (the three pairs view_m/x_view_m, view_lm/x_view_lm, view_pose/x_view_pose are optional)
    return FLM_ERR_ARG;
  }
  if (!view_m != !x_view_m || !view_lm != !x_view_lm || !view_pose != !x_view_pose) {
    set_error("%s: view_m goes with x_view_m, view_lm with x_view_lm and view_pose with x_view_pose: both or neither", who);
    return FLM_ERR_ARG;
  }
  if (k < 1 || k > 65535) {
    set_error("%s: k=%d, needs 1 <= k <= 65535", who, k);
    return FLM_ERR_SHAPE;
  }
  if (q < 1 || q > 65535) {
    set_error("%s: q=%d, needs 1 <= q <= 65535", who, q);
    return FLM_ERR_SHAPE;
  }
  if (bins < 1 || bins > 64) {
    set_error("%s: bins=%d, needs 1 <= bins <= 64", who, bins);
    return FLM_ERR_SHAPE;
  }
  if (c < 1 || c > 1024) {
    set_error("%s: c=%d, needs 1 <= c <= 1024", who, c);
    return FLM_ERR_SHAPE;
  }
  if (face_bytes < 1) {
    set_error("%s: face_bytes=0, needs face_bytes >= 1", who);
    return FLM_ERR_SHAPE;
  }
  const size_t sk = (size_t)k * bins, sq = (size_t)q * bins, sc = (size_t)c;
  const NamedRange bufs[] = {
      {exit_row, (size_t)k * 4, "exit_row_dev"}, {view_q, sk * 8, "view_q"}, {view_frame, sk * 8, "view_frame"},
      {view_gallery, sk * face_bytes, "view_gallery"}, {view_m, sk * 24, "view_m"}, {view_lm, sk * sc * 16, "view_lm"},
      {view_pose, sk * FLM_POSE_REC * 8, "view_pose"}, {x_view_q, sq * 8, "x_view_q"},
      {x_view_frame, sq * 8, "x_view_frame"}, {x_view_gallery, sq * face_bytes, "x_view_gallery"},
      {x_view_m, sq * 24, "x_view_m"}, {x_view_lm, sq * sc * 16, "x_view_lm"},
      {x_view_pose, sq * FLM_POSE_REC * 8, "x_view_pose"}};
  const int nb = (int)(sizeof(bufs) / sizeof(bufs[0]));
  for (int i = 0; i < nb; ++i)
    for (int j = i + 1; j < nb; ++j)
      if (bufs[i].p && bufs[j].p && ranges_overlap(bufs[i].p, bufs[i].bytes, bufs[j].p, bufs[j].bytes)) {
        set_error("%s: %s and %s overlap (no two arguments may)", who, bufs[i].name, bufs[j].name);
        return FLM_ERR_ARG;
      }
  TrackExitViewsArgs g;
  g.exit_row = exit_row; g.k = k; g.q = q; g.bins = bins; g.c = c; g.face_bytes = face_bytes;
  g.view_q = view_q; g.view_frame = view_frame; g.view_gallery = static_cast<const unsigned char*>(view_gallery);
  g.view_m = view_m; g.view_lm = view_lm; g.view_pose = view_pose;
  g.x_view_q = x_view_q; g.x_view_frame = x_view_frame; g.x_view_gallery = static_cast<unsigned char*>(x_view_gallery);
  g.x_view_m = x_view_m; g.x_view_lm = x_view_lm; g.x_view_pose = x_view_pose;
  return launch_track_exit_views(static_cast<hipStream_t>(stream), g);
}

// ---- frame annotation (flm_annotate.hip) ------------------------------------------------------------------------------

void flm_annotate_opts_init(flm_annotate_opts* opts) {
  if (!opts) return;
  memset(opts, 0, sizeof(*opts));
  opts->struct_size = (uint32_t)sizeof(flm_annotate_opts);
  opts->marks = 1;
  opts->box = 0;
  opts->redact = 0;
  opts->margin[0] = 0.1; opts->margin[1] = 0.35; opts->margin[2] = 0.1; opts->margin[3] = 0.1;
  opts->mark_bgr[0] = 0; opts->mark_bgr[1] = 255; opts->mark_bgr[2] = 0;
  opts->box_bgr[0] = 0; opts->box_bgr[1] = 255; opts->box_bgr[2] = 0;
}

int flm_bgr_to_yuv(int matrix, const uint8_t bgr[3], uint8_t yuv[3]) {
  if (!bgr || !yuv) {
    set_error("flm_bgr_to_yuv: null argument");
    return FLM_ERR_ARG;
  }
  if (matrix != FLM_YUV_BT601_LIMITED && matrix != FLM_YUV_BT709_LIMITED) {
    set_error("flm_bgr_to_yuv: unknown YUV matrix %d", matrix);
    return FLM_ERR_ARG;
  }
  annot_bgr_to_yuv(matrix, bgr, yuv);
  return FLM_OK;
}

int flm_frames_annotate(flm_stream_t stream, uint8_t* frames, size_t frame_stride, int nframes, int fh, int fw,
                        const flm_frame_format* src, const int32_t* frame_idx, const double* lm, size_t lm_stride, int k,
                        int c, const flm_annotate_opts* opts, int32_t* regions) {
  const char* who = "flm_frames_annotate";
  if (!frames || !lm || !regions) {  // src, frame_idx and opts are optional
    set_error("%s: null argument", who);
    return FLM_ERR_ARG;
  }
  flm_frame_format bgr;
  flm_frame_format_init(&bgr);
  if (!src) src = &bgr;
  const int rc_fmt = check_frame_format(who, src);
  if (rc_fmt == FLM_ERR_ARG) return rc_fmt;  // (a BGR24 format with a pitch is a shape error: after the options)
  flm_annotate_opts defaults;
  flm_annotate_opts_init(&defaults);
  if (!opts) opts = &defaults;
  if (opts->struct_size < sizeof(flm_annotate_opts)) {
    set_error("%s: flm_annotate_opts struct_size %u is smaller than this library's %zu (initialise with "
              "flm_annotate_opts_init)", who, opts->struct_size, sizeof(flm_annotate_opts));
    return FLM_ERR_ARG;
  }
  if (opts->marks != 0 && opts->marks != 1) {
    set_error("%s: marks=%d (must be 0 or 1)", who, opts->marks);
    return FLM_ERR_ARG;
  }
  if (opts->box < 0 || opts->box > 16) {
    set_error("%s: box=%d outside 0 <= box <= 16", who, opts->box);
    return FLM_ERR_ARG;
  }
  if (opts->redact != 0 && (opts->redact < 2 || opts->redact > 64 || (opts->redact & 1))) {
    set_error("%s: redact=%d (must be 0, or even and 2 <= redact <= 64)", who, opts->redact);
    return FLM_ERR_ARG;
  }
  for (int i = 0; i < 4; ++i)
    if (!(opts->margin[i] >= 0.0 && opts->margin[i] <= 4.0)) {  // (NaN fails the test)
      set_error("%s: margin[%d]=%g outside 0 <= margin <= 4", who, i, opts->margin[i]);
      return FLM_ERR_ARG;
    }
  if (k < 1 || k > 65535) {
    set_error("%s: k=%d outside 1 <= k <= 65535", who, k);
    return FLM_ERR_SHAPE;
  }
  if (opts->redact && k > 4096) {
    set_error("%s: k=%d with redact, needs k <= 4096 (every workgroup of the mosaic scans the faces before its own)", who,
              k);
    return FLM_ERR_SHAPE;
  }
  if (c < 1 || c > 1024) {
    set_error("%s: c=%d outside 1 <= c <= 1024", who, c);
    return FLM_ERR_SHAPE;
  }
  if (lm_stride < 2) {
    set_error("%s: lm_stride=%zu, needs lm_stride >= 2", who, lm_stride);
    return FLM_ERR_SHAPE;
  }
  if (rc_fmt) return check_frame_format(who, src);  // (sets the message again)
  if (nframes < 1) {
    set_error("%s: nframes=%d, needs nframes >= 1", who, nframes);
    return FLM_ERR_SHAPE;
  }
  AnnotateArgs g;
  memset(&g, 0, sizeof(g));
  if (src->pixel == FLM_FRAME_NV12) {
    const size_t bytes = nv12_format_bytes(who, src, fh, fw);  // fh, fw even and >= 2, the pitches, slot bytes < 2^31
    if (!bytes) return FLM_ERR_SHAPE;
    if (frame_stride < bytes) {
      set_error("%s: frame_stride=%zu, needs frame_stride >= flm_frame_format_bytes = %zu", who, frame_stride, bytes);
      return FLM_ERR_SHAPE;
    }
    g.nv12 = 1;
    g.y_pitch = src->y_pitch ? src->y_pitch : (unsigned)fw;
    g.uv_pitch = src->uv_pitch ? src->uv_pitch : g.y_pitch;
    g.uv_off = src->uv_offset ? (unsigned)src->uv_offset : g.y_pitch * (unsigned)fh;
    annot_bgr_to_yuv(src->matrix, opts->mark_bgr, g.mark_px);
    annot_bgr_to_yuv(src->matrix, opts->box_bgr, g.box_px);
  } else {
    if (fh < 1 || fw < 2) {
      set_error("%s: frame %dx%d, needs fh >= 1 and fw >= 2", who, fh, fw);
      return FLM_ERR_SHAPE;
    }
    if ((long long)fh * fw * 3 >= (1ll << 31)) {
      set_error("%s: frame %dx%d, needs fh*fw*3 < 2^31", who, fh, fw);
      return FLM_ERR_SHAPE;
    }
    if (frame_stride < (size_t)fh * fw * 3) {
      set_error("%s: frame_stride=%zu, needs frame_stride >= fh*fw*3 = %zu", who, frame_stride, (size_t)fh * fw * 3);
      return FLM_ERR_SHAPE;
    }
    for (int i = 0; i < 3; ++i) {
      g.mark_px[i] = opts->mark_bgr[i];
      g.box_px[i] = opts->box_bgr[i];
    }
  }
  g.frames = frames; g.frame_stride = frame_stride; g.nframes = nframes; g.fh = fh; g.fw = fw;
  g.frame_idx = frame_idx; g.lm = lm; g.lm_stride = lm_stride; g.k = k; g.c = c;
  g.marks = opts->marks; g.box = opts->box; g.redact = opts->redact;
  for (int i = 0; i < 4; ++i) g.margin[i] = opts->margin[i];
  g.regions = regions;
  return launch_frames_annotate(static_cast<hipStream_t>(stream), g);
}

// ---- landmark flow (flm_flow.hip; the flow launch of both calls is in flm_flow_rows.hip) ----------------------------

size_t flm_flow_pyramid_bytes(int h, int w, int levels) {
  if (h < 1 || w < 1 || levels < 1 || levels > 6) return 0;
  size_t bytes = 0;
  for (int l = 0; l < levels; ++l) bytes += (size_t)(h >> l) * (size_t)(w >> l);
  return bytes;
}

// The geometry both flow calls share.
static int check_flow_geometry(const char* who, int h, int w, int levels) {
  if (levels < 1 || levels > 6) {
    set_error("%s: levels=%d, needs 1 <= levels <= 6", who, levels);
    return FLM_ERR_SHAPE;
  }
  const int t = 1 << (levels - 1);
  if (h < 1 || w < 1 || h > 32768 || w > 32768 || h % t || w % t || (h >> (levels - 1)) < 2 || (w >> (levels - 1)) < 2) {
    set_error("%s: crop %dx%d with %d levels, needs h and w <= 32768, multiples of 2^(levels-1) = %d and at least %d",
              who, h, w, levels, t, 2 * t);
    return FLM_ERR_SHAPE;
  }
  return FLM_OK;
}

int flm_flow_pyramid(flm_stream_t stream, const uint8_t* src, int n, int h, int w, int ch, int levels, uint8_t* pyr) {
  const char* who = "flm_flow_pyramid";
  if (!src || !pyr) {
    set_error("%s: null argument", who);
    return FLM_ERR_ARG;
  }
  if (n < 1 || n > 131070) {
    set_error("%s: n=%d, needs 1 <= n <= 131070", who, n);
    return FLM_ERR_SHAPE;
  }
  if (ch != 1 && ch != 3) {
    set_error("%s: ch=%d, needs ch 1 (luma) or 3 (BGR)", who, ch);
    return FLM_ERR_SHAPE;
  }
  if (int rc = check_flow_geometry(who, h, w, levels)) return rc;
  const long long tiles = (long long)((h + 31) / 32) * ((w + 31) / 32) * n;
  if (tiles >= (1ll << 31)) {
    set_error("%s: %d crops of %dx%d are %lld tiles of 32x32, needs fewer than 2^31", who, n, h, w, tiles);
    return FLM_ERR_SHAPE;
  }
  if (ranges_overlap(src, (size_t)n * h * w * ch, pyr, (size_t)n * flm_flow_pyramid_bytes(h, w, levels))) {
    set_error("%s: pyr_dev overlaps src_dev", who);
    return FLM_ERR_ARG;
  }
  return launch_flow_pyramid(static_cast<hipStream_t>(stream), src, n, h, w, ch, levels, pyr);
}

void flm_flow_opts_init(flm_flow_opts* opts) {
  if (!opts) return;
  opts->struct_size = (uint32_t)sizeof(flm_flow_opts);
  opts->reserved = 0;
  opts->levels = 4;
  opts->radius = 7;
  opts->max_iter = 10;
  opts->pad = 0;
  opts->eps = 0.03;
  opts->min_eig = 0.5;
  opts->max_err = 12.0;
  opts->max_move = 64.0;
}

// The options every flow call takes: the struct's header and the four numbers.
static int check_flow_opts(const char* who, const flm_flow_opts* opts) {
  if (opts->struct_size < sizeof(flm_flow_opts)) {
    set_error("%s: flm_flow_opts struct_size %u is smaller than this library's %zu (initialise with "
              "flm_flow_opts_init)", who, opts->struct_size, sizeof(flm_flow_opts));
    return FLM_ERR_ARG;
  }
  if (opts->reserved != 0 || opts->pad != 0) {
    set_error("%s: flm_flow_opts reserved=%u, pad=%d, both must be 0", who, opts->reserved, opts->pad);
    return FLM_ERR_ARG;
  }
  if (!(opts->eps > 0.0)) {
    set_error("%s: eps=%g, needs eps > 0", who, opts->eps);
    return FLM_ERR_ARG;
  }
  if (!(opts->min_eig >= 0.0)) {
    set_error("%s: min_eig=%g, needs min_eig >= 0", who, opts->min_eig);
    return FLM_ERR_ARG;
  }
  if (!(opts->max_err >= 0.0)) {
    set_error("%s: max_err=%g, needs max_err >= 0", who, opts->max_err);
    return FLM_ERR_ARG;
  }
  if (!(opts->max_move > 0.0)) {
    set_error("%s: max_move=%g, needs max_move > 0", who, opts->max_move);
    return FLM_ERR_ARG;
  }
  return FLM_OK;
}

// The window of every flow call: radius and max_iter (after the call's own sizes, the order flm_landmark_flow had).
static int check_flow_window(const char* who, const flm_flow_opts* opts) {
  if (opts->radius < 1 || opts->radius > 7) {
    set_error("%s: radius=%d, needs 1 <= radius <= 7", who, opts->radius);
    return FLM_ERR_SHAPE;
  }
  if (opts->max_iter < 1 || opts->max_iter > 64) {
    set_error("%s: max_iter=%d, needs 1 <= max_iter <= 64", who, opts->max_iter);
    return FLM_ERR_SHAPE;
  }
  return FLM_OK;
}

// Every output against every input and every other output; null entries are skipped.
static int check_no_overlap(const char* who, const NamedRange* in, size_t n_in, const NamedRange* out, size_t n_out) {
  for (size_t a = 0; a < n_out; ++a) {
    if (!out[a].p) continue;
    for (size_t b = 0; b < n_in; ++b) {
      if (in[b].p && ranges_overlap(out[a].p, out[a].bytes, in[b].p, in[b].bytes)) {
        set_error("%s: %s overlaps %s", who, out[a].name, in[b].name);
        return FLM_ERR_ARG;
      }
    }
    for (size_t b = a + 1; b < n_out; ++b) {
      if (out[b].p && ranges_overlap(out[a].p, out[a].bytes, out[b].p, out[b].bytes)) {
        set_error("%s: %s overlaps %s", who, out[a].name, out[b].name);
        return FLM_ERR_ARG;
      }
    }
  }
  return FLM_OK;
}

int flm_landmark_flow(flm_stream_t stream, const uint8_t* pyr_prev, const uint8_t* pyr_cur, int k, int h, int w,
                      const double* lm_prev, const double* w_prev, const float* m, int c, const flm_flow_opts* opts,
                      double* lm_out, double* w_out, int32_t* err_out, int32_t* flags_out) {
  const char* who = "flm_landmark_flow";
  if (!pyr_prev || !pyr_cur || !lm_prev || !m || !lm_out || !flags_out) {
    set_error("%s: null argument", who);  // (w_prev, opts, w_out and err_out are optional)
    return FLM_ERR_ARG;
  }
  flm_flow_opts defaults;
  flm_flow_opts_init(&defaults);
  if (!opts) opts = &defaults;
  if (int rc = check_flow_opts(who, opts)) return rc;
  if (k < 1 || k > 65535) {
    set_error("%s: k=%d, needs 1 <= k <= 65535", who, k);
    return FLM_ERR_SHAPE;
  }
  if (c < 1 || c > 1024) {
    set_error("%s: c=%d, needs 1 <= c <= 1024", who, c);
    return FLM_ERR_SHAPE;
  }
  if (int rc = check_flow_window(who, opts)) return rc;
  if (int rc = check_flow_geometry(who, h, w, opts->levels)) return rc;
  const size_t pyr = (size_t)k * flm_flow_pyramid_bytes(h, w, opts->levels), kc = (size_t)k * c;
  const NamedRange in[] = {{pyr_prev, pyr, "pyr_prev_dev"}, {pyr_cur, pyr, "pyr_cur_dev"},
                           {lm_prev, kc * 16, "lm_prev_dev"}, {w_prev, w_prev ? kc * 8 : 0, "w_prev_dev"},
                           {m, (size_t)k * 24, "m_dev"}};
  const NamedRange out[] = {{lm_out, kc * 16, "lm_out_dev"}, {w_out, kc * 8, "w_out_dev"},
                            {err_out, kc * 4, "err_out_dev"}, {flags_out, kc * 4, "flags_out_dev"}};
  if (int rc = check_no_overlap(who, in, sizeof(in) / sizeof(in[0]), out, sizeof(out) / sizeof(out[0]))) return rc;
  return launch_landmark_flow_rows(static_cast<hipStream_t>(stream), pyr_prev, pyr_cur, k, h, w, nullptr, k, lm_prev,
                                   w_prev, m, c, opts, 0.0, lm_out, w_out, err_out, nullptr, flags_out);
}

// ---- the flow tick on rows (flm_flow_rows.hip) ------------------------------------------------------------------------

int flm_track_gather_flow(flm_stream_t stream, const int32_t* stream_on, int s, int k, int fh, int fw, int n,
                          const int32_t* frame_idx_stream, const double* dt_stream, double dt, const float* m_crop,
                          const int32_t* boxes, const double* best_q, int32_t* reset, double* age, int32_t* cursor,
                          const int32_t* flow_frame, int32_t* flow_ready, int32_t* slot_c, float* m_c, int32_t* boxes_c,
                          int32_t* frame_idx_c, int32_t* prev_frame_idx_c, double* dt_c, double* best_q_c, int32_t* reset_c,
                          int32_t* counts) {
  const char* who = "flm_track_gather_flow";
  if (!m_crop || !boxes || !flow_frame || !flow_ready || !slot_c || !m_c || !boxes_c || !frame_idx_c || !prev_frame_idx_c ||
      !counts) {
    set_error("%s: null argument", who);  // (stream_on, frame_idx_stream, cursor and the three optional groups may be null)
    return FLM_ERR_ARG;
  }
  if ((age == nullptr) != (dt_c == nullptr) || (best_q == nullptr) != (best_q_c == nullptr) ||
      (reset == nullptr) != (reset_c == nullptr)) {
    set_error("%s: age_dev/dt_c, best_q_dev/best_q_c and reset_dev/reset_c go together (both or neither)", who);
    return FLM_ERR_ARG;
  }
  if (dt_stream && !age) {
    set_error("%s: dt_stream_dev goes with age_dev", who);
    return FLM_ERR_ARG;
  }
  if (age && !dt_stream && !(dt > 0.0 && std::isfinite(dt))) {
    set_error("%s: dt=%g, needs a finite dt > 0 (seconds since the previous step) or dt_stream_dev", who, dt);
    return FLM_ERR_ARG;
  }
  TrackFlowArgs g;
  g.boxes = boxes; g.m_crop = m_crop; g.s = s; g.k = k; g.fh = fh; g.fw = fw; g.n = n;
  g.stream_on = stream_on; g.frame_idx_stream = frame_idx_stream; g.dt_stream = dt_stream; g.dt = dt;
  g.best_q = best_q; g.reset = reset; g.age = age; g.cursor = cursor; g.flow_frame = flow_frame; g.flow_ready = flow_ready;
  g.slot_c = slot_c; g.m_c = m_c; g.boxes_c = boxes_c; g.frame_idx_c = frame_idx_c; g.prev_frame_idx_c = prev_frame_idx_c;
  g.dt_c = dt_c; g.best_q_c = best_q_c; g.reset_c = reset_c; g.counts = counts;
  if (n >= 1 && n <= 65535 && s >= 1 && k >= 1 && (long long)s * k <= 65535) {   // (the launcher names a size outside)
    const size_t ns = (size_t)s * k, nr = (size_t)n;
    const NamedRange in[] = {{stream_on, stream_on ? (size_t)s * 4 : 0, "stream_on_dev"},
                             {frame_idx_stream, frame_idx_stream ? (size_t)s * 4 : 0, "frame_idx_stream_dev"},
                             {dt_stream, dt_stream ? (size_t)s * 8 : 0, "dt_stream_dev"}, {m_crop, ns * 24, "m_crop_dev"},
                             {boxes, ns * 16, "boxes_dev"}, {best_q, best_q ? ns * 8 : 0, "best_q_dev"},
                             {flow_frame, ns * 4, "flow_frame_dev"}};
    const NamedRange out[] = {{reset, ns * 4, "reset_dev"}, {age, ns * 8, "age_dev"}, {cursor, 4, "cursor_dev"},
                              {flow_ready, ns * 4, "flow_ready_dev"}, {slot_c, nr * 4, "slot_c"}, {m_c, nr * 24, "m_c"},
                              {boxes_c, nr * 16, "boxes_c"}, {frame_idx_c, nr * 4, "frame_idx_c"},
                              {prev_frame_idx_c, nr * 4, "prev_frame_idx_c"}, {dt_c, nr * 8, "dt_c"},
                              {best_q_c, nr * 8, "best_q_c"}, {reset_c, nr * 4, "reset_c"}, {counts, 24, "counts_dev"}};
    if (int rc = check_no_overlap(who, in, sizeof(in) / sizeof(in[0]), out, sizeof(out) / sizeof(out[0]))) return rc;
  }
  return launch_track_gather_flow(static_cast<hipStream_t>(stream), g);
}

int flm_landmark_flow_rows(flm_stream_t stream, const uint8_t* pyr_prev, const uint8_t* pyr_cur, int n, int h, int w,
                           const int32_t* slot, int n_slots, const double* lm_prev, const double* w_prev, const float* m,
                           int c, const flm_flow_opts* opts, double max_fb, double* lm_out, double* w_out,
                           int32_t* err_out, double* fb_out, int32_t* flags_out) {
  const char* who = "flm_landmark_flow_rows";
  if (!pyr_prev || !pyr_cur || !slot || !lm_prev || !m || !lm_out || !fb_out || !flags_out) {
    set_error("%s: null argument", who);  // (w_prev, opts, w_out and err_out are optional)
    return FLM_ERR_ARG;
  }
  flm_flow_opts defaults;
  flm_flow_opts_init(&defaults);
  if (!opts) opts = &defaults;
  if (int rc = check_flow_opts(who, opts)) return rc;
  if (!(max_fb >= 0.0 && std::isfinite(max_fb))) {
    set_error("%s: max_fb=%g, needs a finite max_fb >= 0 (0: no forward-backward check)", who, max_fb);
    return FLM_ERR_ARG;
  }
  if (n < 1 || n > 65535) {
    set_error("%s: n=%d, needs 1 <= n <= 65535", who, n);
    return FLM_ERR_SHAPE;
  }
  if (n_slots < 1 || n_slots > 65535) {
    set_error("%s: n_slots=%d, needs 1 <= n_slots <= 65535", who, n_slots);
    return FLM_ERR_SHAPE;
  }
  if (c < 1 || c > 1024) {
    set_error("%s: c=%d, needs 1 <= c <= 1024", who, c);
    return FLM_ERR_SHAPE;
  }
  if (int rc = check_flow_window(who, opts)) return rc;
  if (int rc = check_flow_geometry(who, h, w, opts->levels)) return rc;
  const size_t pyr = (size_t)n * flm_flow_pyramid_bytes(h, w, opts->levels), nc = (size_t)n * c, sc = (size_t)n_slots * c;
  const NamedRange in[] = {{pyr_prev, pyr, "pyr_prev_dev"}, {pyr_cur, pyr, "pyr_cur_dev"}, {slot, (size_t)n * 4, "slot_dev"},
                           {lm_prev, sc * 16, "lm_prev_dev"}, {w_prev, w_prev ? sc * 8 : 0, "w_prev_dev"},
                           {m, (size_t)n * 24, "m_dev"}};
  const NamedRange out[] = {{lm_out, nc * 16, "lm_out_dev"}, {w_out, nc * 8, "w_out_dev"}, {err_out, nc * 4, "err_out_dev"},
                            {fb_out, nc * 8, "fb_out_dev"}, {flags_out, nc * 4, "flags_out_dev"}};
  if (int rc = check_no_overlap(who, in, sizeof(in) / sizeof(in[0]), out, sizeof(out) / sizeof(out[0]))) return rc;
  return launch_landmark_flow_rows(static_cast<hipStream_t>(stream), pyr_prev, pyr_cur, n, h, w, slot, n_slots, lm_prev,
                                   w_prev, m, c, opts, max_fb, lm_out, w_out, err_out, fb_out, flags_out);
}

int flm_track_flow_history_put(flm_stream_t stream, const int32_t* slot, const int32_t* status_rows,
                               const int32_t* frame_idx_c, const double* lm_rows, const double* w_rows, int n, int n_slots,
                               int c, double* hist_lm, double* hist_w, int32_t* flow_frame, int32_t* flow_ready) {
  const char* who = "flm_track_flow_history_put";
  if (!slot || !status_rows || !frame_idx_c || !flow_frame || !flow_ready) {
    set_error("%s: null argument", who);  // (lm_rows/hist_lm_dev and w_rows/hist_w_dev are optional)
    return FLM_ERR_ARG;
  }
  if ((lm_rows == nullptr) != (hist_lm == nullptr) || (w_rows == nullptr) != (hist_w == nullptr)) {
    set_error("%s: lm_rows_dev/hist_lm_dev and w_rows_dev/hist_w_dev go together (both or neither)", who);
    return FLM_ERR_ARG;
  }
  if (w_rows && !lm_rows) {
    set_error("%s: w_rows_dev goes with lm_rows_dev", who);
    return FLM_ERR_ARG;
  }
  if (n < 1 || n > 65535) {
    set_error("%s: n=%d, needs 1 <= n <= 65535", who, n);
    return FLM_ERR_SHAPE;
  }
  if (n_slots < 1 || n_slots > 65535) {
    set_error("%s: n_slots=%d, needs 1 <= n_slots <= 65535", who, n_slots);
    return FLM_ERR_SHAPE;
  }
  if (c < 1 || c > 1024) {
    set_error("%s: c=%d, needs 1 <= c <= 1024", who, c);
    return FLM_ERR_SHAPE;
  }
  const size_t nc = (size_t)n * c, sc = (size_t)n_slots * c;
  const NamedRange in[] = {{slot, (size_t)n * 4, "slot_dev"}, {status_rows, (size_t)n * 4, "status_rows_dev"},
                           {frame_idx_c, (size_t)n * 4, "frame_idx_c"}, {lm_rows, nc * 16, "lm_rows_dev"},
                           {w_rows, nc * 8, "w_rows_dev"}};
  const NamedRange out[] = {{hist_lm, sc * 16, "hist_lm_dev"}, {hist_w, sc * 8, "hist_w_dev"},
                            {flow_frame, (size_t)n_slots * 4, "flow_frame_dev"},
                            {flow_ready, (size_t)n_slots * 4, "flow_ready_dev"}};
  if (int rc = check_no_overlap(who, in, sizeof(in) / sizeof(in[0]), out, sizeof(out) / sizeof(out[0]))) return rc;
  FlowPutArgs g;
  g.slot = slot; g.status_rows = status_rows; g.frame_idx_c = frame_idx_c; g.lm_rows = lm_rows; g.w_rows = w_rows;
  g.n = n; g.n_slots = n_slots; g.c = c; g.hist_lm = hist_lm; g.hist_w = hist_w; g.flow_frame = flow_frame;
  g.flow_ready = flow_ready;
  return launch_flow_history_put(static_cast<hipStream_t>(stream), g);
}

}  // extern "C"
