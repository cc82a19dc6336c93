// extern "C" entry points of the network (see include/flm.h): pack, workspace layout and offsets, the forward's launch
// sequence and its public forms, single layers, preprocessing, the decodes, target heatmaps.
#include <cstdio>
#include <cstring>

#include "flm_api_checks.h"
#include "flm_api_prof.h"

namespace flm {

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
  if (!p || !packed_dev) return null_argument("flm_fcn8_pack");
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
  if (!p) return null_argument("flm_fcn8_pack");
  const flm_fcn_params q = from_fcn8(p);
  return pack_impl(stream, &q, n_classes, dtype, packed_dev, packed_bytes, FLM_ARCH_FCN8);
}
int flm_fcn32_pack(flm_stream_t stream, const flm_fcn8_params* p, int n_classes, int dtype, void* packed_dev,
                   size_t packed_bytes) {
  if (!p) return null_argument("flm_fcn32_pack");
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
  if (!info) return null_argument("flm_fcn_encoder_layer");
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
  if (!packed_dev || !x_dev || !out_dev || !workspace_dev) return null_argument("flm_fcn8_forward");
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
  if (!hm || !out || !ws) return null_argument("flm_decode");
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
  if (!hm || !rec || !ws) return null_argument("flm_decode_stats");
  return launch_decode(static_cast<hipStream_t>(stream), hm, n, h, w, l, mode, n_points, thresh, rec, ws, ws_bytes,
                       nullptr, 1);
}

size_t flm_decode_sweep_workspace_bytes(int n, int h, int w, int l, const int* modes, int n_modes) {
  return decode_sweep_ws_bytes(n, h, w, l, modes, n_modes);
}

int flm_decode_sweep(flm_stream_t stream, const float* hm, int n, int h, int w, int l, const int* modes, int n_modes,
                     float thresh, double* out, void* ws, size_t ws_bytes) {
  if (!hm || !out || !ws) return null_argument("flm_decode_sweep");
  return launch_decode_sweep(static_cast<hipStream_t>(stream), hm, n, h, w, l, modes, n_modes, thresh, out, ws,
                             ws_bytes);
}

int flm_gaussian_heatmaps(flm_stream_t stream, const double* kp, int n, int l, int h, int w, double two_sigma_sq,
                          float* out) {
  if (!kp || !out) return null_argument("flm_gaussian_heatmaps");
  return launch_gaussian_heatmaps(static_cast<hipStream_t>(stream), kp, n, l, h, w, two_sigma_sq, out);
}

}  // extern "C"
