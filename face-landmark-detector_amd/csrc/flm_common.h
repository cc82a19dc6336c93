// Shared declarations of libflm_hip.so (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <atomic>
#include <mutex>

#include "flm.h"

namespace flm {

void set_error(const char* fmt, ...);
int hip_fail(hipError_t e, const char* what);

#define FLM_HIP(call)                                            \
  do {                                                           \
    hipError_t e_ = (call);                                      \
    if (e_ != hipSuccess) return ::flm::hip_fail(e_, #call);     \
  } while (0)

#define FLM_LAUNCH_CHECK(what)                                   \
  do {                                                           \
    hipError_t e_ = hipGetLastError();                           \
    if (e_ != hipSuccess) return ::flm::hip_fail(e_, what);      \
  } while (0)

// hipFuncSetAttribute (dynamic LDS above 64 KiB) once per kernel instantiation AND device, safe under concurrent
// callers: a launcher keeps one static FuncAttrOnce and calls FLM_FUNC_ATTR_ONCE(flag, kernel, lds) before launching.
struct FuncAttrOnce {
  std::atomic<unsigned> done{0};  // one bit per device ordinal
  std::mutex mu;
};
#define FLM_FUNC_ATTR_ONCE(flag, kernel, lds_bytes)                                                        \
  do {                                                                                                     \
    int dev_ = 0;                                                                                          \
    FLM_HIP(hipGetDevice(&dev_));                                                                          \
    const unsigned bit_ = 1u << (dev_ & 31);                                                               \
    if (!((flag).done.load(std::memory_order_acquire) & bit_)) {                                           \
      std::lock_guard<std::mutex> lock_((flag).mu);                                                        \
      if (!((flag).done.load(std::memory_order_relaxed) & bit_)) {                                         \
        FLM_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),                                 \
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)(lds_bytes)));        \
        (flag).done.fetch_or(bit_, std::memory_order_release);                                             \
      }                                                                                                    \
    }                                                                                                      \
  } while (0)

static inline int cdiv(int a, int b) { return (a + b - 1) / b; }
static inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

constexpr float kBnEps = 1e-3f;  // keras BatchNormalization default epsilon

// ---- architecture constants (networks/fcn.py:13,34,43,98,100) ------------------------------
constexpr int kFc = 4096;
constexpr int kMaxClasses = 96;
constexpr int kMaxEnc = 64;

// Encoder description: a list of layers; layer i reads the output of layer `src` (default: i-1, or the
// network input for i = 0) and may add the output of layer `res` before its activation.
enum EncKind {
  ENC_FIRST3 = 0,    // 3-channel Conv2D 3x3 'same' + (BN) + ReLU (+ MaxPool 2x2): enc1_kernel
  ENC_CONV3 = 1,     // Conv2D 3x3 'same' + (BN) + ReLU (+ MaxPool 2x2): igemm_kernel
  ENC_MB_CONV1 = 2,  // MobileNet conv1: pad 1, 3x3 stride 2, no bias, BN, ReLU6 (3 -> 32)
  ENC_MB_DW = 3,     // MobileNet depthwise 3x3 (stride 1|2), no bias, BN, ReLU6
  ENC_MB_PW = 4,     // MobileNet pointwise 1x1, no bias, BN, ReLU6: igemm_kernel
  ENC_RN_CONV1 = 5,  // ResNet conv1: pad 3, 7x7 stride 2, bias, BN, ReLU (3 -> 64)
  ENC_MAXPOOL3 = 6,  // MaxPooling2D 3x3 stride 2 'valid' (no parameters)
  ENC_CONV = 7       // generic Conv2D k x k (k = 1|3, stride 1|2, 'same' when stride 1) + bias + BN (+ residual)
                     // (+ ReLU): igemm_kernel
};
struct EncLayer {
  int cin, cout, bn, pool;
  int kind, stride;
  int k, relu;   // ENC_CONV: kernel size and whether a ReLU follows
  int src, res;  // layer indices (-1: previous layer / none)
};
struct ArchSpec {
  int n_enc;
  EncLayer enc[kMaxEnc];
  int f_idx[5];  // index of the layer whose (pooled) output is f1..f5 (f1, f2 are not used by the decoders)
  int fcn32;     // one 64x64 stride-32 transposed conv instead of the FCN-8 skip decoder
  int valid;
};
// Output grid of every encoder layer for an h x w input.
void enc_dims(const ArchSpec& A, int h, int w, int* hs, int* ws);
inline int enc_has_params(const EncLayer& e) { return e.kind != ENC_MAXPOOL3; }
// FLM_ARCH_FCN8 / FCN32: vanilla_encoder (networks/fcn.py:10-51); *_VGG: get_vgg_encoder (networks/vgg16.py:17-81);
// *_MOBILENET: get_mobilenet_encoder (networks/mobilenet.py:59-114); *_RESNET50: get_resnet50_encoder
// (networks/resnet50.py:122-182)
ArchSpec arch_spec(int arch);

// Geometry of the transposed-conv kernels for a class count C.
struct ConvTGeom {
  int C;   // classes
  int Cp;  // channel stride of the (fp32) score / fuse buffers: multiple of 4 (fp32) or 8 (bf16)
  int MT;  // 16-row class tiles
  int G;   // k groups over K = 4 taps * Cp: 16 deep (fp32, 16x16x4 MFMA x4) or 32 deep (bf16, 16x16x32)
  int bf16;
};
ConvTGeom convt_geom(int C, int dtype);

// One implicit-GEMM conv layer inside the packed blob (offsets in bytes).
struct ConvPack {
  size_t w;      // fp32 or bf16 [coutpad][kh*kw*cin], k = (ky*kw+kx)*cin + c
  size_t scale;  // float [coutpad]
  size_t shift;  // float [coutpad]
  int cin, cout, coutpad, kh, kw, pad;
};

struct Fcn8Pack {
  size_t enc1_w;  // float [64][32], k = ky*9+kx*3+c (c in RGB order), zero for k >= 27
  size_t enc1_scale, enc1_shift;
  ConvPack enc[kMaxEnc];  // enc[i] packs encoder layer i for i >= 1 (layer 0 is the 3-channel first conv)
  ConvPack fc6, fc7, score5, score4, score3;
  size_t up5, up4, up3;  // [s*s phases][G][MT][64 lanes][16 bytes: 4 fp32 or 8 bf16]
  ConvTGeom g;
  int dtype;
  int arch;
  ArchSpec spec;
  size_t total;
};
Fcn8Pack fcn8_pack_layout(int C, int dtype, int arch = 0);

// Workspace of the forward (offsets in bytes).
struct Fcn8Ws {
  size_t act[kMaxEnc];  // output of every encoder layer
  size_t f[5];          // = act[spec.f_idx[k]]
  size_t fc6, fc7, score5, fuse4, seg;
  size_t splitk;  // split-K partial sums of the score convs
  size_t splitk_bytes;
  size_t probs;   // logits/probs when they are not the call's output (else == SIZE_MAX)
  size_t decode;  // decode partials
  // landmark mode without the probability tensor (flm_convt.hip); cand == SIZE_MAX when not used
  size_t sub, tau, cand, cand_cnt;
  int cand_cap;
  // per-face fallback (flm_fallback_opts, faces = fb_faces > 0 on the candidate path); SIZE_MAX / 0 otherwise.  fb_counts
  // holds {R, served, batch, B} and behind them the two gate words: [4] rows_gate = (0 < R <= B), [5] batch_gate = (R > B)
  size_t cand_redo, fb_rows, fb_counts, fb_decode;
  int fb_faces;
  int cand_sub;  // phases the sampling launch takes per tile
  size_t total;
  int oh, ow;
};
// `opts` (NULL = defaults) carries the per-call options that change the layout (include/flm.h: flm_forward_opts).
Fcn8Ws fcn8_ws_layout(int n, int h, int w, int C, int dtype, int out_mode, int decode_mode, int n_points,
                      int arch = 0, const flm_forward_opts* opts = nullptr, const flm_fallback_opts* fb = nullptr);

// ---- A/B knobs (flm_set_tuning / flm_get_tuning; include/flm.h documents every key) ----------
// One row per knob in the table of flm_api.hip, in this order.  A launcher reads each knob it uses exactly ONCE per
// launch, into a local const int, and decides from that: calls may run concurrently with a setter, and a launch must not
// mix two configurations.
enum KnobId {
  KNOB_BF16_BIG_TILES, KNOB_BF16_LDS_DMA, KNOB_BF16_MFMA16, KNOB_BF16_HALO_MFMA16, KNOB_F32_TWO_LEVEL, KNOB_F32_LEAN_TILE,
  KNOB_BF16_GROUP_N, KNOB_BF16_CONV3_HALO, KNOB_BF16_SCORE1X1, KNOB_BF16_FUSED_TAIL, KNOB_DECODE_LDS_DMA,
  KNOB_POSMAJOR_ORDER, KNOB_WARP_ROWS, KNOB_UP3_CAND8, KNOB_UP3_CAND8_ROWS, KNOB_UP3_WREG, KNOB_F32_FC6_ROWS,
  KNOB_COUNT
};
int tuning(KnobId id);  // the knob's current value (relaxed load)

// ---- kernel launchers (each returns FLM_OK or an error) --------------------------------------
// "The caller" below is the extern "C" entry point: flm_api_fcn.hip (network), flm_api_image.hip (fits, warps, frames,
// mesh, annotation) or flm_api_track.hip (tracker, quality, pose, views, flow), each through flm_api_checks.h.
int launch_pack_fcn(hipStream_t s, const flm_fcn_params& p, int C, const Fcn8Pack& L, char* blob);

int launch_enc1(hipStream_t s, const void* x, int in_format, int n, int h, int w, const float* w1p,
                const float* scale, const float* shift, void* f1, int out_bf16, int pool);

struct IgemmDesc {
  const void* x;       // [n,h,w,cin] fp32, or bf16 when `bf16`
  const void* wt;      // [coutpad][K], same type as x
  const float* scale;  // [coutpad]
  const float* shift;  // [coutpad]
  void* y;             // [n,ho,wo,ldc]  (ho,wo = h,w or h/2,w/2 when pooled); bf16 unless out_f32
  int bf16;            // operands are bf16 (v_mfma_f32_32x32x16_bf16), accumulate fp32
  int out_f32;         // bf16 path: store fp32 (score convs feeding the fp32 decoder buffers)
  int n, h, w, cin;
  int cout;     // columns stored
  int coutpad;  // rows of wt (multiple of 128)
  int ldc;      // channel stride of y
  int kh, kw, pad;
  int relu, pool, posmajor;  // relu: 0 none, 1 ReLU, 2 ReLU6
  int stride;               // 1 (0 = 1); 2 only in the row-major order (ResNet's strided 1x1 convs)
  const void* res;          // optional residual [n,ho,wo,ldc] added before the activation
  float* splitk_ws;        // optional scratch for split-K partial sums (null: never split)
  size_t splitk_ws_bytes;
};
int launch_igemm(hipStream_t s, const IgemmDesc& d);
int igemm_occupancy(size_t lds_bytes);
// rows per tile (64 | 128) of the most recent fp32 position-major launch of this process, 0 before the first (tests)
int igemm_posmajor_rows_last();
// seg_feats = crop(up4(fuse4)) + score3(f3) in one launch (flm_tail_bf16.hip; bf16, 68 classes, 256-channel f3):
// 1 launched, 0 shape left to the two-launch form, < 0 error
int launch_seg_fused_bf16(hipStream_t s, const float* fuse4, const void* w4_packed, const void* f3, const void* w3,
                          const float* scale3, const float* shift3, float* seg, int n, int h4, int w4d, int C, int Cp,
                          int G, int cin3, int coutpad3);

struct ConvTDesc {
  const float* x;     // [n,hi,wi,Cp]
  const void* wf;     // fragment-packed weights (fp32 or bf16 per g.bf16)
  const float* skip;  // [n,ho,wo,Cp] added to the result, or null
  void* y;            // logits/probs float [n,ho,wo,ldy] or int32 class map [n,ho,wo]
  int n, hi, wi;      // input grid
  int ho, wo;         // output grid after the crop (<= s*(hi+1))
  int s;              // stride; kernel = 2s
  int ldy;            // channel stride of y (C for the final layer, Cp for score buffers)
  int epilogue;       // 0 raw (+skip), 1 softmax probs, 2 argmax class map, 3 top-n candidates (no map written),
                      // 4 per-wave class maxima of a sampling launch (sub > 0)
  ConvTGeom g;
  // landmark mode without the probability tensor (see flm_convt.hip); all zero / null otherwise
  int sub = 0;                         // > 0: sampling launch, `sub` phases per tile, compact [n][sub][hi+1][wi+1][C] output
  const float* tau = nullptr;          // [n][C] thresholds (epilogue 3)
  unsigned long long* cand = nullptr;  // [n][cand_cap] candidate keys
  unsigned* cand_cnt = nullptr;        // [n] + overflow flag at [n]
  int cand_cap = 0;
  const unsigned* gate = nullptr;      // launch is a no-op unless *gate != 0
  void* scratch = nullptr;             // epilogue 3: memory the launch may use (the bf16 input copy of up3_wreg_kernel), or null
  size_t scratch_bytes = 0;
  unsigned* cand_redo = nullptr;       // epilogue 3: [n] per-face form of the overflow flag (set where it is raised), or null
  // epilogue 1 of the 68-class kernels on a compact batch: n is the row budget, row r reads x of face rows[r] and writes
  // map row r; rows at index *rows_cnt and beyond do nothing.  Both null otherwise.
  const int* rows = nullptr;
  const unsigned* rows_cnt = nullptr;
};
int launch_convt(hipStream_t s, const ConvTDesc& d);
int convt_candidates_supported(const ConvTGeom& g);
// 68-class kernels with a stride that is a multiple of 4 (up3: 8, fcn_32: 32) share the fifth class tile between
// four consecutive phases (flm_convt.hip, flm_pack.hip).
__host__ __device__ inline int convt_share_layout(const ConvTGeom& g, int s) {
  return g.C == 68 && (g.bf16 ? g.G == 9 : g.G == 17) && (s % 4) == 0;
}
int convt_sample_slots(const ConvTGeom& g, int hi, int wi, int sub);
int launch_cand_tau(hipStream_t s, const unsigned* wave_max, int n, int slots, int ld, int l, int n_points, float* tau);

// (activations fp32, or bf16 when `bf16`)
int launch_mb_conv1(hipStream_t s, const void* x, int in_format, int n, int h, int w, const float* wgt,
                    const float* scale, const float* shift, void* y, int bf16);
int launch_mb_depthwise(hipStream_t s, const void* x, int n, int h, int w, int c, int stride, const float* wgt,
                        const float* scale, const float* shift, void* y, int bf16);
int launch_rn_conv1(hipStream_t s, const void* x, int in_format, int n, int h, int w, const float* wgt,
                    const float* scale, const float* shift, void* y, int bf16);
int launch_maxpool3(hipStream_t s, const void* x, int n, int h, int w, int c, void* y, int bf16);

// `stats`: `out` takes landmark records [n][l][FLM_LANDMARK_REC] instead of [n][l][2] (flm_decode_stats; include/flm.h)
size_t decode_ws_bytes(int n, int h, int w, int l, int mode, int n_points, int stats = 0);
int launch_decode(hipStream_t s, const float* hm, int n, int h, int w, int l, int mode, int n_points, float thresh,
                  double* out, void* ws, size_t ws_bytes, const unsigned* gate = nullptr, int stats = 0,
                  const int* rows = nullptr, const unsigned* rows_cnt = nullptr);
// (rows / rows_cnt, top-n only: hm is a compact batch of n rows; rows at index *rows_cnt and beyond are skipped and row
// r's result goes to out[rows[r]])
size_t decode_sweep_ws_bytes(int n, int h, int w, int l, const int* modes, int n_modes);
int launch_decode_sweep(hipStream_t s, const float* hm, int n, int h, int w, int l, const int* modes, int n_modes,
                        float thresh, double* out, void* ws, size_t ws_bytes);
int launch_gaussian_heatmaps(hipStream_t s, const double* kp, int n, int l, int h, int w, double two_sigma_sq,
                             float* out);
int launch_cand_merge(hipStream_t s, const unsigned long long* cand, unsigned* cand_cnt, int n, int w, int l,
                      int n_points, float thresh, int cap, double* out, int stats = 0, unsigned* cand_redo = nullptr);
// The faces cand_redo[0..n) marks, ascending, into rows[0..budget) (-1 from index R on); counts = {R, R <= budget ? R : 0,
// R > budget, budget}, counts[4] = (0 < R <= budget), counts[5] = (R > budget): the gates of the two redo paths.
int launch_fallback_plan(hipStream_t s, const unsigned* cand_redo, int n, int budget, int* rows, unsigned* counts);

int launch_preprocess(hipStream_t s, const uint8_t* img, int n, int h, int w, int norm, float* out);
int launch_similarity(hipStream_t s, const double* lm, const double* tmpl, int n, int k, double sx, double sy, float* m);
int launch_similarity_weighted(hipStream_t s, const double* lm, size_t lm_stride, const double* wt, size_t w_stride,
                               const double* tmpl, int n, int k, double sx, double sy, float* m);
int launch_warp(hipStream_t s, const void* src, int src_is_u8, int n, int hs, int ws, const float* m, float* dst,
                int hd, int wd);
int launch_crop_resize(hipStream_t s, const uint8_t* frame, int fh, int fw, const int32_t* boxes, int k,
                       uint8_t* out, int oh, int ow, const int32_t* frame_idx = nullptr, size_t frame_stride = 0,
                       int nframes = 0);
// frame-space tail (flm_frames.hip)
int launch_landmarks_to_frame(hipStream_t s, const double* lm, const int32_t* boxes, int k, int c, int grid_h,
                              int grid_w, int fh, int fw, double* out);
int launch_warp_frames(hipStream_t s, const uint8_t* frames, size_t frame_stride, int nframes, int fh, int fw,
                       const int32_t* frame_idx, const int32_t* boxes, const float* m, int k, float* dst, int hd,
                       int wd, int samples);
// the two warps with the output format in the epilogue (flm_warp_fmt.hip); the format has been checked by the caller
int launch_warp_fmt(hipStream_t s, const void* src, int src_is_u8, int n, int hs, int ws, const float* m, void* dst, int hd,
                    int wd, const flm_image_format* fmt);
int launch_warp_frames_fmt(hipStream_t s, const uint8_t* frames, size_t frame_stride, int nframes, int fh, int fw,
                           const int32_t* frame_idx, const int32_t* boxes, const float* m, int k, void* dst, int hd,
                           int wd, int samples, const flm_image_format* fmt);

// the limits of a dense BGR24 ring (flm_warp_fmt.hip): FLM_OK or FLM_ERR_SHAPE with the limit named after `who`
int bgr_ring_check(const char* who, size_t frame_stride, int nframes, int fh, int fw);

// NV12 frame slots as the source (flm_frames_nv12.hip); struct_size, pixel and matrix of `src` and the image format have
// been checked by the caller
int launch_frames_to_bgr_nv12(hipStream_t s, const uint8_t* frames, size_t frame_stride, int nframes, int fh, int fw,
                              const flm_frame_format* src, uint8_t* out);
int launch_crop_resize_nv12(hipStream_t s, const uint8_t* frames, size_t frame_stride, int nframes, int fh, int fw,
                            const int32_t* boxes, const int32_t* frame_idx, int k, uint8_t* out, int oh, int ow,
                            const flm_frame_format* src);
int launch_warp_frames_nv12(hipStream_t s, const uint8_t* frames, size_t frame_stride, int nframes, int fh, int fw,
                            const int32_t* frame_idx, const int32_t* boxes, const float* m, int k, void* dst, int hd,
                            int wd, int samples, const flm_image_format* fmt, const flm_frame_format* src);
// 0 when the format's sizes are rejected (the reason is in flm_last_error())
size_t nv12_format_bytes(const char* who, const flm_frame_format* src, int fh, int fw);
// the ring's checks of the calls above, and the slot geometry with the defaults resolved (flm_nv12_dev.h)
struct Nv12Geom;
int nv12_ring_geometry(const char* who, const flm_frame_format* src, size_t frame_stride, int nframes, int fh, int fw,
                       Nv12Geom* g);

// the piecewise-affine warp over the landmark mesh (flm_mesh.hip); null pointers, the image format (never null here)
// and struct_size, pixel and matrix of `src` have been checked by the caller
int launch_mesh_map(hipStream_t s, const double* pts, const int32_t* tris, int p, int t, int hd, int wd, uint8_t* map);
int launch_mesh_affines(hipStream_t s, const double* lm, int lm_stride, const float* m, const double* pts,
                        const int32_t* tris, int p, int a, int t, int k, double min_det, float* aff);
int launch_warp_mesh_frames(hipStream_t s, const uint8_t* frames, size_t frame_stride, int nframes, int fh, int fw,
                            const int32_t* frame_idx, const int32_t* boxes, const double* lm, int lm_stride,
                            const float* m, const double* pts, const int32_t* tris, int p, int a, int t,
                            const uint8_t* map, int k, void* dst, int hd, int wd, int samples,
                            const flm_image_format* fmt, const flm_frame_format* src, double min_det, float* aff_out);

// face parts and openness (flm_parts.hip); null pointers, the formats (never null here), the option struct and the
// overlaps have been checked by the caller
int launch_part_affines(hipStream_t s, const double* lm, size_t lm_stride, const double* wt, size_t w_stride, int k, int c,
                        const int32_t* idx, const double* tmpl, const int32_t* part_n, int r, float* aff, int32_t* ok);
int launch_warp_parts_frames(hipStream_t s, const uint8_t* frames, size_t frame_stride, int nframes, int fh, int fw,
                             const int32_t* frame_idx, const int32_t* boxes, const double* lm, size_t lm_stride,
                             const double* wt, size_t w_stride, int c, const int32_t* idx, const double* tmpl,
                             const int32_t* part_n, int r, int k, void* dst, int ph, int pw, int samples,
                             const flm_image_format* fmt, const flm_frame_format* src, float* aff_out, int32_t* ok_out);
int launch_face_openness(hipStream_t s, const double* lm, size_t lm_stride, const double* wt, size_t w_stride, int n, int c,
                         const flm_open_opts* opts, const int32_t* slot, int n_slots, double* rec, double* state,
                         int32_t* reset, const double* dt_dev, double dt, const int32_t* status, int64_t frame_id);

// tracking (flm_track.hip); null pointers and the option struct have been checked by the caller, `opts` is never null
int launch_track_seed(hipStream_t s, const int32_t* boxes, int k, int in_h, int in_w, int fh, int fw, float* m,
                      int32_t* status);
int launch_landmarks_from_crop(hipStream_t s, const double* lm, size_t lm_stride, const float* m, int k, int c, double sx,
                               double sy, double* out);
// who: the entry point, for the messages
int launch_track_step(hipStream_t s, const char* who, const double* lm, size_t lm_stride, const double* wt, size_t w_stride,
                      const float* m_crop, const int32_t* boxes, int k, int c, double sx, double sy, int in_h, int in_w,
                      int fh, int fw, const double* tmpl_crop, const double* tmpl_align, const flm_track_opts* opts,
                      double* lm_frame, float* m_align, float* m_next, int32_t* boxes_next, int32_t* status,
                      const flm_track_filter* filt /*null = unfiltered*/, double dt, double* state, double* lm_raw,
                      const int32_t* slot /*null = the dense step: row == slot, the next three unused*/, int n_slots,
                      const double* dt_rows, int32_t* status_rows);
int launch_track_gather_streams(hipStream_t s, const int32_t* active, int a, int n_streams, int k,
                                const int32_t* frame_idx_stream, const double* dt_stream, const float* m_crop,
                                const int32_t* boxes, const double* best_q, int32_t* reset, int32_t* slot_c, float* m_c,
                                int32_t* boxes_c, int32_t* frame_idx_c, double* dt_c, double* best_q_c, int32_t* reset_c);
// flm_track_gather_live's arguments under the names of include/flm.h (the kernel takes the struct as it is)
struct TrackLiveArgs {
  const int32_t* boxes;             // [S*K,4]
  const float* m_crop;              // [S*K,2,3]
  int s, k, fh, fw, n;              // n: the budget, the number of rows
  const int32_t* stream_on;         // [S] or null
  const int32_t* frame_idx_stream;  // [S] or null
  const double* dt_stream;          // [S] or null
  double dt;
  const double* best_q;             // [S*K] or null
  int32_t* reset;                   // [S*K] or null, in/out
  double* age;                      // [S*K] or null, in/out
  int32_t* cursor;                  // [1] or null, in/out
  int32_t* slot_c;
  float* m_c;
  int32_t* boxes_c;
  int32_t* frame_idx_c;
  double* dt_c;
  double* best_q_c;
  int32_t* reset_c;
  int32_t* counts;                  // [4]
};
int launch_track_gather_live(hipStream_t s, const TrackLiveArgs& g);

// association (flm_track_assoc.hip); pointers, sizes and the option struct have been checked by the caller
int launch_track_associate(hipStream_t s, const int32_t* det, const int32_t* n_det, int d, int k, int c, int in_h, int in_w,
                           int fh, int fw, const flm_track_assoc_opts* opts, float* m_crop, int32_t* boxes, int32_t* status,
                           int32_t* misses, double* state, int32_t* det_slot, int32_t* slot_det, int32_t* counts);
int launch_track_associate_streams(hipStream_t s, const int32_t* det, const int32_t* n_det, int n_streams, int d, int k,
                                   int c, int in_h, int in_w, int fh, int fw, const flm_track_assoc_opts* opts,
                                   float* m_crop, int32_t* boxes, int32_t* status, int32_t* misses, double* state,
                                   int32_t* det_slot, int32_t* slot_det, int32_t* counts);

// best shot (flm_quality.hip); pointers, the format, the option structs and overlaps have been checked by the caller
int launch_face_quality(hipStream_t s, const void* faces, int k, int h, int w, const flm_image_format* fmt,
                        const flm_quality_opts* opts, int64_t* rec);
int launch_track_best_update(hipStream_t s, const void* faces, size_t face_bytes, int k, const int64_t* rec,
                             const int32_t* status, const int32_t* reset, const double* lm, size_t lm_stride,
                             const double* wt, size_t w_stride, int c, const double* factor, const float* m,
                             int64_t frame_id, const flm_best_opts* opts,
                             const int32_t* slot /*null = flm_track_best_update: k slots, row == slot*/, int n_slots,
                             const double* best_q_in, double* best_q_out, void* gallery, int64_t* best_frame, float* best_m,
                             double* best_lm, int64_t* best_rec);

// flm_track_retire's arguments under the names of include/flm.h (flm_track_exit.hip; both kernels take the struct as it
// is); pointers, their pairing, the option struct, sizes and overlaps have been checked by the caller
struct TrackExitArgs {
  const int32_t* boxes;        // [K,4]
  const int32_t* status;       // [K]
  int k, fh, fw, c, q;
  size_t face_bytes;
  const double* best_q;        // [K]
  const unsigned char* gallery;
  const int64_t* best_frame;   // [K]
  const float* best_m;         // [K,2,3] or null, with x_m
  const double* best_lm;       // [K,C,2] or null, with x_lm
  const int64_t* best_rec;     // [K,8] or null, with x_rec
  int64_t frame_id;
  int flush;
  double min_q;
  int32_t* born;               // [K] in/out
  int64_t* track_id;           // [K] in/out
  int64_t* born_frame;         // [K] in/out
  int64_t* head;               // [4] in/out
  unsigned char* x_gallery;    // [Q,face_bytes]
  int64_t* x_meta;             // [Q,8]
  double* x_q;                 // [Q]
  float* x_m;
  double* x_lm;
  int64_t* x_rec;
  int32_t* exit_row;           // [K]
};
int launch_track_retire(hipStream_t s, const TrackExitArgs& g);

// head pose (flm_pose.hip); pointers, the option struct, sizes, strides and overlaps have been checked by the caller
int launch_head_pose(hipStream_t s, const double* lm, size_t lm_stride, const double* wt, size_t w_stride, int n, int c,
                     const int32_t* idx, const double* xyz, int p, const flm_pose_opts* opts,
                     const int32_t* slot /*null: row r writes record r*/, int n_slots, double* pose, double* factor);

// pose-binned best shots (flm_track_views.hip): the arguments of the two calls under the names of include/flm.h; pointers,
// their pairing, the option struct, sizes and overlaps have been checked by the caller
struct TrackViewsArgs {
  const unsigned char* faces;  // [N,face_bytes]
  size_t face_bytes;
  int n, n_slots, c, bins;
  const int64_t* rec;          // [N,8]
  const int32_t* status;       // [N] or null
  const int32_t* reset;        // [N] or null
  const double* lm;
  size_t lm_stride;
  const double* wt;            // or null
  size_t w_stride;
  const float* m;              // [N,2,3] or null
  int64_t frame_id;
  double sharp_ref, min_exposed;
  int n_u, n_v;
  double u_edge[FLM_VIEWS_MAX_EDGES], v_edge[FLM_VIEWS_MAX_EDGES];
  const int32_t* slot;         // [N] or null: row == slot
  const double* pose;          // [n_slots,18]
  double* view_q;              // [n_slots,B] in/out
  int64_t* view_frame;         // [n_slots,B]
  unsigned char* view_gallery; // [n_slots,B,face_bytes]
  float* view_m;               // [n_slots,B,2,3] or null
  double* view_lm;             // [n_slots,B,C,2] or null
  double* view_pose;           // [n_slots,B,18] or null
  int32_t* take;               // [N]
};
int launch_track_views_update(hipStream_t s, const TrackViewsArgs& g);

struct TrackExitViewsArgs {
  const int32_t* exit_row;     // [K]
  int k, q, bins, c;
  size_t face_bytes;
  const double* view_q;        // [K,B]
  const int64_t* view_frame;   // [K,B]
  const unsigned char* view_gallery;
  const float* view_m;         // [K,B,2,3] or null, with x_view_m
  const double* view_lm;       // [K,B,C,2] or null, with x_view_lm
  const double* view_pose;     // [K,B,18] or null, with x_view_pose
  double* x_view_q;            // [Q,B]
  int64_t* x_view_frame;       // [Q,B]
  unsigned char* x_view_gallery;
  float* x_view_m;
  double* x_view_lm;
  double* x_view_pose;
};
int launch_track_exit_views(hipStream_t s, const TrackExitViewsArgs& g);

// flm_frames_annotate (flm_annotate.hip); every argument has been checked by the caller (flm_api_image.hip), which resolves
// the frame format's defaults and converts the two colours for an NV12 ring
struct AnnotateArgs {
  uint8_t* frames;
  size_t frame_stride;
  int nframes, fh, fw;
  int nv12;                           // 0: dense BGR24; 1: y_pitch, uv_pitch, uv_off below hold
  unsigned y_pitch, uv_pitch, uv_off;
  const int32_t* frame_idx;           // [K] or null = slot 0
  const double* lm;
  size_t lm_stride;
  int k, c;
  int marks, box, redact;
  double margin[4];
  uint8_t mark_px[3], box_px[3];      // B,G,R for a BGR ring, Y,U,V for an NV12 ring
  int32_t* regions;                   // [K,4]
};
int launch_frames_annotate(hipStream_t s, const AnnotateArgs& g);

// landmark flow (flm_flow.hip); sizes, options, pointers and overlaps have been checked by the caller (flm_api_track.hip)
int launch_flow_pyramid(hipStream_t s, const uint8_t* src, int n, int h, int w, int ch, int levels, uint8_t* pyr);

// the flow tick on rows (flm_flow_rows.hip; flm_flow_rows_dev.h holds the two argument structs); pointers, their pairing,
// sizes, options and overlaps have been checked by the caller (flm_api_track.hip), except the sizes launch_track_gather_flow
// names.  launch_landmark_flow_rows is the landmark flow of both calls: flm_landmark_flow passes slot and fb_out null
struct TrackFlowArgs;
struct FlowPutArgs;
int launch_track_gather_flow(hipStream_t s, const TrackFlowArgs& g);
int launch_landmark_flow_rows(hipStream_t s, const uint8_t* pyr_prev, const uint8_t* pyr_cur, int n, int h, int w,
                              const int32_t* slot, int n_slots, const double* lm_prev, const double* w_prev, const float* m,
                              int c, const flm_flow_opts* opts, double max_fb, double* lm_out, double* w_out,
                              int32_t* err_out, double* fb_out, int32_t* flags_out);
int launch_flow_history_put(hipStream_t s, const FlowPutArgs& g);

// Bijective XCD-aware remap of a 1-D grid: blocks that the dispatcher deals to the same XCD
// (b % 8) receive consecutive logical ids, so neighbours in logical order share an L2.
__device__ __forceinline__ int xcd_remap(int b, int nblk) {
  const int q = nblk >> 3, r = nblk & 7;
  const int xcd = b & 7, loc = b >> 3;
  const int base = (xcd < r) ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
  return base + loc;
}

}  // namespace flm
