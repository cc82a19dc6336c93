/*
 * flm.h -- C ABI of the MI355X-native facial-landmark hot path (libflm_hip.so).
 *
 * The reference (sandyz1000/face-landmark-detector) is pure Python on
 * TensorFlow/Keras: it has no FFI, plugin or operator registry.  The boundary it
 * offers is a duck-typed model object plus a few functions; each entry point below
 * names the reference interface it replaces (paths relative to the reference root).
 * The Python host side (package `face-landmark-detector_amd`) binds these with
 * ctypes; INTEGRATION.md shows the binding a reference maintainer would add.
 *
 * Conventions
 *  - plain pointers and sizes only; every pointer named *_dev is DEVICE memory
 *    borrowed for the duration of the call; nothing is retained.
 *  - every launch goes to the caller's stream (hipStream_t passed as void*);
 *    no call synchronises the device or allocates memory.
 *  - scratch memory is a caller-owned workspace sized by the matching
 *    *_workspace_bytes query.
 *  - return value: 0 = FLM_OK, negative = error; flm_last_error() returns a
 *    thread-local message for the last failing call on this thread.
 *  - reentrancy: calls on different streams may run concurrently from different threads.
 *    Process state is limited to (1) the thread-local error string, (2) the A/B
 *    performance knobs of flm_set_tuning -- integers that every launch reads once, at
 *    launch time, and that never change results or memory layouts, (3) the measurement hook flm_profile_*
 *    (off by default; a measurement aid, NOT thread-safe).  Everything that changes
 *    results' provenance or the workspace layout is an argument (flm_forward_opts).
 *  - layouts are NHWC ("channels_last", networks/config.py:5) throughout.
 */
#ifndef FLM_H_
#define FLM_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FLM_ABI_VERSION 2

typedef void* flm_stream_t; /* hipStream_t */

enum flm_status {
  FLM_OK = 0,
  FLM_ERR_ARG = -1,         /* null pointer / bad enum */
  FLM_ERR_SHAPE = -2,       /* shape outside what the kernels cover */
  FLM_ERR_WORKSPACE = -3,   /* workspace too small */
  FLM_ERR_HIP = -4,         /* a HIP runtime call failed */
  FLM_ERR_UNSUPPORTED = -5  /* valid request this build does not implement */
};

/* Arithmetic of the conv stack.  FLM_F32: exact fp32 on v_mfma_f32_*_f32 (the parity path).
 * FLM_BF16: bf16 operands (weights and the activations f1..f5/fc6/fc7 stored as bf16), fp32
 * accumulation, BatchNorm/bias/softmax/decode in fp32 (BASELINE configs[2]); inputs and outputs of
 * flm_fcn8_forward keep the same types in both modes. */
enum flm_dtype { FLM_F32 = 0, FLM_BF16 = 1 };

/* Input formats of the forward. */
enum flm_input_format {
  FLM_IN_U8_BGR = 0,  /* raw cv2 crop, uint8 [N,H,W,3] BGR: the sub_mean preprocess of
                         get_image_array (data/generator.py:52-61) is fused into the
                         first conv's loader */
  FLM_IN_F32_RGB = 1  /* already preprocessed float32 [N,H,W,3], what model.predict
                         receives at prediction.py:208 */
};

/* What flm_fcn8_forward writes to `out_dev`. */
enum flm_output_mode {
  FLM_OUT_PROBS = 0,     /* float32 [N, H'*W', C]: model.predict (networks/utils.py:28-30) */
  FLM_OUT_CLASSMAP = 1,  /* int32 [N, H', W']: pr.argmax(axis=2) (prediction.py:209) */
  FLM_OUT_LANDMARKS = 2, /* float64 [N, C, 2] (x,y): transfer_target (utils/metrics.py:102-109) */
  FLM_OUT_LOGITS = 3,    /* float32 [N, H', W', C] before the softmax (debug / tests) */
  FLM_OUT_LANDMARKS_STATS = 4 /* float64 [N, C, FLM_LANDMARK_REC] landmark records (below, at flm_decode_stats): the
                                 landmarks of FLM_OUT_LANDMARKS, bit for bit, with their score and spread */
};

enum flm_decode_mode {
  FLM_DECODE_ALL = 0, /* n_points < 1: full-map weighted centroid (utils/metrics.py:58-64) */
  FLM_DECODE_TOPN = 1 /* weighted centroid of the n largest pixels (utils/metrics.py:66-77) */
};

enum flm_image_norm { /* imgNorm of get_image_array (data/generator.py:50-65) */
  FLM_NORM_SUB_MEAN = 0,
  FLM_NORM_SUB_AND_DIVIDE = 1,
  FLM_NORM_DIVIDE = 2
};

int flm_abi_version(void);
const char* flm_last_error(void);

/* ---- weights -------------------------------------------------------------------
 * Replaces keras `model.load_weights` (prediction.py:128).  Parameters arrive as
 * device tensors in the KERAS layouts and are repacked on the device into one blob
 * in the layouts the kernels read (OHWI rows for the implicit GEMMs, MFMA fragment
 * order for the transposed convs, BatchNorm folded to scale/shift with eps = 1e-3).
 */
typedef struct flm_conv_params {
  const float* kernel; /* Conv2D: HWIO (kh,kw,in,out) */
  const float* bias;   /* [out] */
  const float* gamma;  /* BatchNormalization, NULL for layers without BN */
  const float* beta;
  const float* mean;   /* moving_mean */
  const float* var;    /* moving_variance */
} flm_conv_params;

typedef struct flm_fcn8_params {
  flm_conv_params enc[5];  /* vanilla_encoder, networks/fcn.py:10-51: 3x3, F=64,128,256,256,256 */
  flm_conv_params fc6;     /* fcn.py:98  7x7x256x4096 */
  flm_conv_params fc7;     /* fcn.py:100 1x1x4096x4096 */
  flm_conv_params score5;  /* fcn.py:103 1x1x4096xC */
  flm_conv_params score4;  /* fcn.py:108 1x1x256xC on f4 */
  flm_conv_params score3;  /* fcn.py:117 1x1x256xC on f3 */
  const float* up5;        /* fcn.py:104 Conv2DTranspose (4,4,C,C) = (kh,kw,out,in), stride 2 */
  const float* up4;        /* fcn.py:114 (4,4,C,C), stride 2 */
  const float* up3;        /* fcn.py:121 (16,16,C,C), stride 8 */
} flm_fcn8_params;

size_t flm_fcn8_packed_bytes(int n_classes, int dtype);
int flm_fcn8_pack(flm_stream_t stream, const flm_fcn8_params* params_dev_ptrs, int n_classes,
                  int dtype, void* packed_dev, size_t packed_bytes);

/* ---- forward -------------------------------------------------------------------
 * Replaces `model.predict(x)` of the model built by fcn_8 + vanilla_encoder +
 * get_segmentation_model (networks/fcn.py:89-126, networks/utils.py:6-39;
 * call site prediction.py:208), optionally continued through the argmax of
 * prediction.py:209 or the decode of utils/metrics.py:102-109.
 * H and W must be multiples of 32; the output grid is H' = H+8, W' = W+8.
 *
 * What a call may assume about its buffers -- and what it may not.  A workspace is a recycled block, not a fresh page.
 * In one call of a forward (every flm_fcn*_forward*), of a pack (flm_fcn*_pack) or of a decode (flm_decode,
 * flm_decode_stats, flm_decode_sweep):
 *  1. the result does not depend on what the workspace held before the call;
 *  2. it does not depend on what the output held;
 *  3. it does not depend on what the gaps between the regions of the packed blob hold (a pack writes every byte a
 *     forward reads and leaves the rest of packed_dev as it found it);
 *  4. it does not depend on memory adjacent to any operand: nothing before the first or after the last byte of the
 *     input, the blob, the workspace or the output is read into a result, not even multiplied by a packed zero;
 *  5. nothing outside [workspace_dev, workspace_dev + workspace_bytes) and the output is written; packed_dev and x_dev
 *     are read only.
 * "The result" is the output and every intermediate flm_fcn_workspace_offset_opts names, pad class columns included.
 * Alignment: workspace_dev and packed_dev must be 256-byte aligned (their layouts count in 256-byte steps from the
 * start), x_dev and out_dev 16-byte aligned; the decodes' maps 16-byte aligned as stated there, their workspaces
 * 256-byte and their outputs 8-byte aligned.  The image calls further down (warps, crops, frame conversion) take 16-byte
 * aligned sources and float32 destinations -- every face of a batch then starts wherever its size puts it -- and, in the
 * *_fmt calls, a destination aligned to its element, as stated there; they use no workspace, and points 2, 4 and 5 hold
 * for them too.  tests/test_gpu_buffer_independence.py holds all of this with the operands carved from one allocation
 * pre-filled with 0x00, 0x4B and 0xFF, each between 4 MiB guards, at exactly these alignments and no better.
 */
size_t flm_fcn8_workspace_bytes(int n, int h, int w, int n_classes, int dtype, int out_mode,
                                int decode_mode, int n_points);
int flm_fcn8_forward(flm_stream_t stream, const void* packed_dev, const void* x_dev, int in_format,
                     int n, int h, int w, int n_classes, int dtype, int out_mode, int decode_mode,
                     int n_points, float thresh, void* out_dev, void* workspace_dev,
                     size_t workspace_bytes);
/* Byte offset inside the workspace of a named intermediate ("f1".."f5","fc6","fc7",
 * "score5","fuse4","seg_feats","probs"), or -1: lets tests compare layer by layer. */
int64_t flm_fcn8_workspace_offset(const char* name, int n, int h, int w, int n_classes, int dtype,
                                  int out_mode, int decode_mode, int n_points);

/* ---- fcn_32 (networks/fcn.py:129-150) ------------------------------------------------------------
 * Same encoder and head; no skip branches; one Conv2DTranspose(C, 64x64, stride 32) then the
 * softmax: output grid H' = H+32, W' = W+32.  Parameters: flm_fcn8_params with `up3` holding the
 * (64,64,C,C) kernel; score4, score3, up5, up4 are ignored.  Same contracts as the fcn8 calls. */
size_t flm_fcn32_packed_bytes(int n_classes, int dtype);
int flm_fcn32_pack(flm_stream_t stream, const flm_fcn8_params* params_dev_ptrs, int n_classes, int dtype,
                   void* packed_dev, size_t packed_bytes);
size_t flm_fcn32_workspace_bytes(int n, int h, int w, int n_classes, int dtype, int out_mode,
                                 int decode_mode, int n_points);
int flm_fcn32_forward(flm_stream_t stream, const void* packed_dev, const void* x_dev, int in_format,
                      int n, int h, int w, int n_classes, int dtype, int out_mode, int decode_mode,
                      int n_points, float thresh, void* out_dev, void* workspace_dev,
                      size_t workspace_bytes);

/* ---- architecture-generic entry points ------------------------------------------------------------
 * The registry of the reference (networks/basic_models.py:59-64, networks/fcn.py:153-192) builds the same
 * FCN head on several encoders.  `arch` selects the graph; the flm_fcn8_* / flm_fcn32_* calls above are
 * these with arch = FLM_ARCH_FCN8 / FLM_ARCH_FCN32.  Encoder convs arrive in network order in `enc`:
 * 5 layers for the vanilla encoder (BatchNorm tensors required), 13 for VGG16 (block1_conv1 ..
 * block5_conv3, networks/vgg16.py:27-72, no BatchNorm: gamma..var NULL), 27 for MobileNet-v1 (conv1, then
 * conv_dw_i / conv_pw_i for i = 1..13, networks/mobilenet.py:79-102; no biases: bias NULL; the depthwise
 * kernels are the Keras (3,3,C,1) tensors), 53 for ResNet50 (conv1, then per bottleneck block the shortcut
 * conv `res<stage><block>_branch1` when the block has one, then branch2a, 2b, 2c; networks/resnet50.py:
 * 145-170; every conv has bias and BatchNorm). */
enum flm_arch {
  FLM_ARCH_FCN8 = 0, FLM_ARCH_FCN32 = 1, FLM_ARCH_FCN8_VGG = 2, FLM_ARCH_FCN32_VGG = 3,
  FLM_ARCH_FCN8_MOBILENET = 4, FLM_ARCH_FCN32_MOBILENET = 5,
  FLM_ARCH_FCN8_RESNET50 = 6, FLM_ARCH_FCN32_RESNET50 = 7     /* every architecture builds in fp32 and bf16 */
};
typedef struct flm_fcn_params {
  const flm_conv_params* enc; /* host array of n_enc entries (the pointers inside are device pointers) */
  int n_enc;
  flm_conv_params fc6, fc7, score5, score4, score3;
  const float *up5, *up4, *up3; /* FCN-32 variants: only up3 = the (64,64,C,C) kernel */
} flm_fcn_params;
size_t flm_fcn_packed_bytes(int arch, int n_classes, int dtype);
int flm_fcn_pack(flm_stream_t stream, int arch, const flm_fcn_params* params, int n_classes, int dtype,
                 void* packed_dev, size_t packed_bytes);
size_t flm_fcn_workspace_bytes(int arch, int n, int h, int w, int n_classes, int dtype, int out_mode,
                               int decode_mode, int n_points);
int flm_fcn_forward(flm_stream_t stream, int arch, const void* packed_dev, const void* x_dev, int in_format,
                    int n, int h, int w, int n_classes, int dtype, int out_mode, int decode_mode,
                    int n_points, float thresh, void* out_dev, void* workspace_dev, size_t workspace_bytes);

/* Per-call options of the forward that change the WORKSPACE LAYOUT (never the results): pass the same struct to the
 * workspace query and to the forward.  NULL = defaults.  Initialise with flm_forward_opts_init (sets struct_size, which
 * lets the struct grow without breaking callers).
 *   landmark_candidates   1 (default): FLM_OUT_LANDMARKS with top-n, n <= 32, on the 68-class FCN-8 kernels selects
 *                         from candidate keys emitted by the last transposed conv instead of materialising the
 *                         [N,H'*W',C] probabilities (bit-identical landmarks, gated fallback) -- under those
 *                         conditions and the output map has fewer than 2^17 pixels: 352 x 352 is the largest square
 *                         input (a candidate key holds the pixel index in 17 bits).  Larger maps, the default
 *                         416 x 608 geometry (424 x 616 = 261,184 pixels) among them, always materialise the
 *                         probabilities: their layout holds no cand_* buffers and is the same for both values.
 *                         0: always materialise
 *                         and decode (the decode of utils/metrics.py:102-109 on model.predict's output, literally)
 *   candidate_sub_phases  phases per tile in that path's sampling launch (1..16; 0 = by n_points: 4 up to n = 8 (fp32: 2),
 *                         6 up to 15, 8 beyond)
 *   candidate_cap_div     shrink the candidate lists by this factor (>= 1; tests of the overflow fallback) */
typedef struct flm_forward_opts {
  uint32_t struct_size;
  int32_t landmark_candidates;
  int32_t candidate_sub_phases;
  int32_t candidate_cap_div;
} flm_forward_opts;
void flm_forward_opts_init(flm_forward_opts* opts);
size_t flm_fcn_workspace_bytes_opts(int arch, int n, int h, int w, int n_classes, int dtype, int out_mode,
                                    int decode_mode, int n_points, const flm_forward_opts* opts);
int flm_fcn_forward_opts(flm_stream_t stream, int arch, const void* packed_dev, const void* x_dev, int in_format,
                         int n, int h, int w, int n_classes, int dtype, int out_mode, int decode_mode,
                         int n_points, float thresh, void* out_dev, void* workspace_dev, size_t workspace_bytes,
                         const flm_forward_opts* opts);
int64_t flm_fcn8_workspace_offset_opts(const char* name, int n, int h, int w, int n_classes, int dtype,
                                       int out_mode, int decode_mode, int n_points, const flm_forward_opts* opts);

/* Per-face fallback of the candidate path (landmark_candidates = 1 above).  One word, cand_cnt[n], guards the whole batch
 * there: when any face raises it, every face is redone through the materialised probabilities.  With `faces` = B > 0 the
 * forward records WHICH faces raised (cand_redo), compacts them on the device into at most B rows (fallback_rows) and
 * redoes only those -- the materialising up3 and the decode run on a batch of B rows whose row r reads face
 * fallback_rows[r], writes probability row r (the first B rows of "probs") and puts its landmarks at face
 * fallback_rows[r].  When more than B faces raised, today's whole-batch redo runs instead.  Every launch shape is a host
 * number; nothing is downloaded.  Landmarks are bit for bit those of faces = 0 in every case.
 *   faces   0 (default, and NULL): the flm_fcn_*_opts entry points, launch for launch and byte for byte of layout.
 *           < 0: FLM_ERR_ARG.  > n: n.  Where the call does not take the candidate path (another class count, fcn_32, the
 *           all-pixel mode, n_points > 32, landmark_candidates = 0, a map of 2^17 pixels or more) the option adds nothing.
 * The same struct goes to the workspace query and to the forward, as flm_forward_opts does.  Regions it adds, after
 * cand_cnt (no other name moves), by flm_fcn_workspace_offset_fb:
 *   "cand_redo"        uint32 [n]: 1 where the face raised (every site that raises cand_cnt[n] sets it)
 *   "fallback_rows"    int32 [B]: the faces that raised, ascending; -1 from index R on (R > B: the first B of them)
 *   "fallback_counts"  uint32 [4]: { R faces raised, faces served per face (R when R <= B, else 0), whole-batch redo
 *                      taken 0 | 1, B }
 * cand_cnt[0..n-1] and cand_cnt[n] keep their meaning and values.  Profile records: "fallback_plan", "up3_rows",
 * "decode_rows", then "up3_fallback" and "decode_fallback". */
typedef struct flm_fallback_opts {
  uint32_t struct_size;  /* as flm_forward_opts: lets the struct grow */
  int32_t faces;
} flm_fallback_opts;
void flm_fallback_opts_init(flm_fallback_opts* fb);
size_t flm_fcn_workspace_bytes_fb(int arch, int n, int h, int w, int n_classes, int dtype, int out_mode,
                                  int decode_mode, int n_points, const flm_forward_opts* opts,
                                  const flm_fallback_opts* fb);
int64_t flm_fcn_workspace_offset_fb(int arch, const char* name, int n, int h, int w, int n_classes, int dtype,
                                    int out_mode, int decode_mode, int n_points, const flm_forward_opts* opts,
                                    const flm_fallback_opts* fb);
int flm_fcn_forward_fb(flm_stream_t stream, int arch, const void* packed_dev, const void* x_dev, int in_format,
                       int n, int h, int w, int n_classes, int dtype, int out_mode, int decode_mode,
                       int n_points, float thresh, void* out_dev, void* workspace_dev, size_t workspace_bytes,
                       const flm_forward_opts* opts, const flm_fallback_opts* fb);

/* ---- where every layer's output lies, for every architecture (tests compare layer by layer) ------------------------
 * flm_fcn_workspace_offset_opts: byte offset inside the workspace of a named intermediate of `arch`, or -1 (null or
 * unknown name, unknown architecture, a shape or option struct the workspace query refuses, a tensor this call's layout
 * does not hold).  Names: "f1".."f5", "fc6", "fc7", "score5", "fuse4", "seg_feats" (both -1 for the fcn_32 graphs, which
 * have no skip stages), "probs", "cand_sub" / "cand_tau" / "cand_keys" / "cand_cnt" / "cand_cap" (the last returns the
 * list capacity, not an offset), and "act<i>" (decimal, no leading zeros): the output of encoder layer i -- every layer
 * has a region of its own, nothing is reused, so all of them survive the forward.  Encoder outputs, fc6 and fc7 are
 * [n, out_h, out_w, cout] in the operand type (float32 | bfloat16); score5 / fuse4 / seg_feats are float32 with the
 * padded class count as channel stride.  The flm_fcn8_workspace_offset* calls are this one with FLM_ARCH_FCN8.
 *
 * flm_fcn_encoder_layers: the number of encoder layers of `arch` (5 | 13 | 27 | 54: ResNet50's parameter-free max-pool
 * is layer 1 of its 54), or -1.  flm_fcn_encoder_layer: layer `index` for an h x w input (multiples of 32), in network
 * order -- the order of flm_fcn_params::enc with the max-pool inserted.  Read-only; launches nothing. */
enum flm_enc_kind {
  FLM_ENC_FIRST3 = 0,   /* 3-channel Conv2D 3x3 'same' (+ BatchNorm) + ReLU (+ MaxPool 2x2) */
  FLM_ENC_CONV3 = 1,    /* Conv2D 3x3 'same' (+ BatchNorm) + ReLU (+ MaxPool 2x2) */
  FLM_ENC_MB_CONV1 = 2, /* MobileNet conv1: pad 1, 3x3 stride 2, BatchNorm, ReLU6 */
  FLM_ENC_MB_DW = 3,    /* MobileNet depthwise: pad 1, 3x3 stride 1 | 2, BatchNorm, ReLU6 */
  FLM_ENC_MB_PW = 4,    /* MobileNet pointwise 1x1, BatchNorm, ReLU6 */
  FLM_ENC_RN_CONV1 = 5, /* ResNet50 conv1: pad 3, 7x7 stride 2, bias, BatchNorm, ReLU */
  FLM_ENC_MAXPOOL3 = 6, /* MaxPooling2D 3x3 stride 2 'valid' */
  FLM_ENC_CONV = 7      /* Conv2D k x k (pad k/2, stride 1 | 2), bias, BatchNorm (+ residual) (+ ReLU) */
};
typedef struct flm_enc_layer_info {
  int32_t kind;          /* enum flm_enc_kind */
  int32_t cin, cout;
  int32_t kernel;        /* k of the k x k window */
  int32_t stride;
  int32_t activation;    /* 0 none, 1 ReLU, 2 ReLU6 */
  int32_t pool;          /* 1: a 2x2 max-pool closes the layer (its output grid is the pooled one) */
  int32_t src;           /* index of the layer whose output this one reads; -1: the network input */
  int32_t res;           /* index of the layer whose output is added before the activation; -1: none */
  int32_t in_h, in_w;    /* grid of the input */
  int32_t out_h, out_w;  /* grid of the stored output */
} flm_enc_layer_info;
int64_t flm_fcn_workspace_offset_opts(int arch, const char* name, int n, int h, int w, int n_classes, int dtype,
                                      int out_mode, int decode_mode, int n_points, const flm_forward_opts* opts);
int flm_fcn_encoder_layers(int arch);
int flm_fcn_encoder_layer(int arch, int index, int h, int w, flm_enc_layer_info* info);

/* One named Conv2D layer of the model in isolation ("enc2".."enc5" with BN+ReLU+pool fused,
 * "fc6", "fc7", "score5", "score4", "score3"), exactly the launch the forward makes for it except that no
 * split-K scratch is passed (the layer never splits K here).  For tests and developer tools that run or time one layer.
 * Types follow the forward's own intermediates -- the call converts nothing:
 *   FLM_F32:  x_dev float32 [n,h,w,Cin] -> y_dev float32 [n,ho,wo,Cout]
 *   FLM_BF16: x_dev bfloat16 [n,h,w,Cin] (what the previous layer stored) -> y_dev bfloat16 [n,ho,wo,Cout] for
 *             "enc2".."enc5", "fc6", "fc7"; float32 for "score5", "score4", "score3"
 * ho x wo = h x w (h/2 x w/2 for the pooled "enc" layers).  Cout of the score layers is the padded class count of the
 * configuration (n_classes = 68: 68 in FLM_F32, 72 in FLM_BF16; otherwise 16 * ceil(n_classes / 16)); the columns from
 * n_classes on are written as exact zeros.  tests/test_gpu_bf16_layers.py holds fc6, fc7 and the score layers to an
 * integer reference bit for bit in both types.
 *
 * The decoder's Conv2DTranspose layers, with the forward's own launch (kernel 2s x 2s, stride s, crop to the top-left
 * window fused); n, h, w are the INPUT grid.  Both types take and write float32 maps -- FLM_BF16 re-reads x_dev as a
 * bf16 operand, as the forward does.  Cp is the padded class count above:
 *   "up5", "up4":  x_dev float32 [n,h,w,Cp]; y_dev float32 [n,2h,2w,Cp] HOLDS THE SKIP MAP ON ENTRY and the call adds
 *                  crop(convT(x)) onto it in place (s = 2; fuse4 = up5(score5) + score4, seg_feats = up4(fuse4) + score3).
 *                  Pad columns of x_dev and y_dev must be zeros and stay exact zeros.  ("up4" is always the stand-alone
 *                  launch; the 68-class bf16 forward may fuse it with score3 -- same bits.)
 *   "up3":         x_dev float32 [n,h,w,Cp] -> y_dev float32 [n,8h+8,8w+8,n_classes] raw logits (s = 8);
 *                  FLM_ERR_UNSUPPORTED unless n_classes % 4 == 0, as FLM_OUT_LOGITS. */
int flm_fcn8_run_layer(flm_stream_t stream, const void* packed_dev, const char* layer, const void* x_dev,
                       void* y_dev, int n, int h, int w, int n_classes, int dtype);

/* ---- measurement hook (bench.py) --------------------------------------------------
 * When enabled, flm_fcn8_forward brackets each of its kernel launches with a hipEvent pair on
 * the caller's stream (no synchronisation).  flm_profile_read(i, ...) waits for record i and
 * returns its layer name and duration in ms; it returns 1 past the last record.
 * Process-global, not thread-safe: a measurement aid, off by default. */
int flm_profile_enable(int max_records);
/* Bracket only the launches of one layer ("fc6", ...; NULL or "" = every launch).  Every event pair costs a few
 * microseconds of stream time, so a timed region that only needs the dominant kernel's duration filters on it. */
int flm_profile_filter(const char* layer);
/* A/B performance knobs: they never change memory layouts, and -- with the one exception of "f32_two_level", which
 * selects between two fp32 summation orders -- never results; key "none" is always accepted, unknown keys
 * fail.  A launch reads each knob it depends on exactly once, when it is issued: a setter running concurrently with
 * launches on other threads takes effect between launches, never inside one.  A rejected value leaves the knob as it
 * was.  Meant for A/B runs (tools/tune.py) and for tests that force a code path:
 *   "bf16_big_tiles"        0 off | 1 auto (default) | 2 whenever the shape allows | 3 auto + 256x128 tiles
 *                           256-row bf16 implicit-GEMM tiles (csrc/flm_igemm_bf16.hip)
 *   "bf16_lds_dma"          1 (default): the 256x256 tiles fetch their operands with buffer_load ... lds (no staging
 *                           registers, no LDS write pass); 0: global -> registers -> LDS
 *   "bf16_mfma16"           1 (default): the LDS-DMA form of those tiles computes with v_mfma_f32_16x16x32_bf16;
 *                           0: with 32x32x16.  Same bits
 *   "bf16_halo_mfma16"      1 (default): the halo-resident 3x3 kernel (enc2) computes with v_mfma_f32_16x16x32_bf16 too;
 *                           0: with 32x32x16.  Same bits
 *   "f32_two_level"         1 (default): the fp32 implicit GEMMs sum every 32-product k-step from zero and add the step
 *                           sums into a second accumulator set (chains of 32 + K/32 roundings, operands by LDS-DMA;
 *                           csrc/flm_igemm.hip); 0: one fmaf chain of K per output (round 2's kernel).  Both are valid
 *                           fp32 evaluations of the layer; the bits differ
 *   "f32_lean_tile"         1 (default): the row-major and pooled layers of that kernel enter and leave the k-loop by a
 *                           shorter path -- no integer division and, where the launcher proves every tap in bounds for
 *                           every tile, no tap-mask loop in the set-up; the first operand requests issued before anything
 *                           they do not need; full tiles stored without per-element tests (csrc/flm_igemm.hip, LEAN);
 *                           0: the set-up and write-out as they were.  Same bits
 *   "bf16_group_n"          weight panels per tile group of that kernel (0 default, else a power of two <= 32)
 *   "bf16_conv3_halo"       0 off | 1 auto (default) | 2 always: halo-resident 3x3 kernel for 64-channel inputs
 *   "bf16_score1x1"         1 (default): 1x1 classifiers on 256-channel bf16 maps (score4, score3) run the kernel that
 *                           keeps the weights in registers (csrc/flm_score1x1.hip); 0: the implicit GEMM.  Same bits
 *   "bf16_fused_tail"       1 (default): seg_feats = crop(up4(fuse4)) + score3(f3) is ONE launch in the bf16 configuration
 *                           of the 68-class models (csrc/flm_tail_bf16.hip); 0: score3, then up4 with the skip add.
 *                           Same bits
 *   "decode_lds_dma"        1 (default): the standalone decode of 68-landmark maps brings its tiles into a three-slot LDS
 *                           ring by buffer_load ... lds (csrc/flm_decode.hip, decode_partial_dma_kernel); 0: one tile of
 *                           register prefetch.  Same results
 *   "posmajor_order"        1 (default): position-major layers (fc6) at batches smaller than a tile's rows take the map
 *                           positions that share a tile in an order chosen for their common filter taps
 *                           (csrc/flm_igemm_args.h, posmajor_fill_perm); 0: map order.  Same bits
 *   "warp_rows"             1 (default): uint8 warps whose destination width is a multiple of 64 run a wave per
 *                           64-pixel row segment, 2 rows per wave (csrc/flm_misc.hip, warp_u8_rows_kernel; 4: four rows
 *                           per wave); 0: the pixel-list kernel.  Same bits
 *   "up3_cand8"             bit 0: the bf16 candidate launch of the last transposed conv runs the 8-wave kernel
 *                           (csrc/flm_convt.hip, up3_cand8_kernel); bit 2: its 4-wave x 2-workgroup shape; default 1;
 *                           0: the generic kernel.  Same keys either way.  Bit 1 (an fp32 form of that kernel) is
 *                           accepted and ignored: the fp32 path always runs the generic kernel
 *   "up3_cand8_rows"        phase rows one workgroup of that kernel walks with the same input fragments: 0 (default)
 *                           chosen from the batch, else 1, 2, 4 or 8
 *   "up3_wreg"              1: that launch runs the weights-in-registers kernel instead (csrc/flm_up3_wreg.hip: a wave keeps
 *                           one phase's weights for its whole life, the input streams past through LDS) where its
 *                           conditions hold (stride 8, 68 classes; the probability region of the workspace is its
 *                           scratch); 0 (default).  Same keys
 * One knob is a size, not a switch (0, 64 or 128; anything else is rejected):
 *     "f32_fc6_rows"        rows per tile of the fp32 position-major implicit GEMM (fc6; csrc/flm_igemm.hip, BMT): 0
 *                           (default) the launcher's model decides per launch -- the list schedule of the tile weights on
 *                           the resident workgroups for both forms plus a surcharge on the 64-row form's extra operand
 *                           requests (csrc/flm_igemm_args.h, posmajor_pick_rows); split-K launches and batches of 128
 *                           faces and more keep 128 rows --; 64 or 128: that form wherever it can run (a forced 64 also
 *                           in split-K launches, whose slices do not move).  Same bits
 * The options that change the workspace layout ("landmark_candidates", "candidate_*") are per-call arguments:
 * flm_forward_opts above. */
int flm_set_tuning(const char* key, int value);
/* The current value of a knob listed above: FLM_OK, or FLM_ERR_ARG (null pointer, unknown key) with a message. */
int flm_get_tuning(const char* key, int* value);
/* Diagnostics for developers ("igemm_occupancy", arg = dynamic LDS bytes -> workgroups per CU; "igemm_posmajor_rows" ->
 * rows per tile, 64 or 128, of this process's most recent fp32 position-major launch, 0 before the first). */
int flm_debug_query(const char* key, int arg);
int flm_profile_reset(void);
int flm_profile_read(int index, char* name_out, int name_cap, float* ms_out);
int flm_profile_disable(void);

/* ---- preprocess ----------------------------------------------------------------
 * get_image_array (data/generator.py:29-69) for crops already at model size:
 * uint8 BGR [N,H,W,3] -> float32 [N,H,W,3] (RGB for sub_mean). */
int flm_preprocess(flm_stream_t stream, const uint8_t* img_bgr_dev, int n, int h, int w, int norm,
                   float* out_dev);

/* ---- decode --------------------------------------------------------------------
 * transfer_target / transfer_xy_coord / get_average_xy (utils/metrics.py:46-109):
 * float32 heatmaps [N,H,W,L] -> float64 [N,L,2] (x,y) in heatmap pixel units,
 * (-1,-1) where mean(selected) <= thresh.  Ties at the n-th place: pixels are ordered
 * by (value, flat index), the n largest are kept. */
size_t flm_decode_workspace_bytes(int n, int h, int w, int l, int mode, int n_points);
int flm_decode(flm_stream_t stream, const float* hm_dev, int n, int h, int w, int l, int mode,
               int n_points, float thresh, double* out_dev, void* workspace_dev,
               size_t workspace_bytes);

/* ---- the landmark record -----------------------------------------------------------
 * The decode with what it knows about every landmark kept: float64 [N,L,FLM_LANDMARK_REC], one row per landmark,
 *   x, y, score, var_x, var_y, cov_xy
 * in heatmap pixel units (px and px^2); score is the mean selected value the reject test of utils/metrics.py:78-79
 * compares.  Operation by operation (-ffp-contract=off: only the fma named below fuses):
 *  top-n (n_points >= 1), keys visited rank n-1 down to rank 0, empty slots skipped:
 *    hsum (float32) += hv;  i0 += (double)row * (double)hv;  i1 += (double)col * (double)hv
 *    x = i1 / (double)hsum;  y = i0 / (double)hsum                      -- flm_decode's chain and bits
 *    score = (double)(hsum / (float)n_points)                           -- the float32 quotient, widened
 *    rejected (hsum / (float)n_points <= thresh):  x = y = -1, var_x = var_y = -1, cov_xy = 0; score is still written
 *    else a second walk in the same order: dx = (double)col - x, dy = (double)row - y,
 *      vxx += (double)hv * (dx*dx);  vyy += (double)hv * (dy*dy);  vxy += (double)hv * (dx*dy)
 *      var_x = vxx / (double)hsum;  var_y = vyy / (double)hsum;  cov_xy = vxy / (double)hsum
 *    (centred on purpose: every term of vxx and vyy is non-negative, nothing cancels; n_points = 1 gives exact zeros)
 *  all-pixel (n_points < 1):
 *    per lane and chunk, in pixel order, float64: S0 += hv, Sx = fma(hv, col, Sx), Sy = fma(hv, row, Sy) as flm_decode,
 *    and beside them Sxx = fma(hv, col*col, Sxx), Syy = fma(hv, row*row, Syy), Sxy = fma(hv, col*row, Sxy); lanes are
 *    added by the same fixed-order butterfly, chunks in chunk order
 *    hsum = (float)S0;  x = Sx / (double)hsum;  y = Sy / (double)hsum   -- flm_decode's bits
 *    score = (double)(hsum / (float)(H*W));  rejected rows as above
 *    var_x = max(0, Sxx / (double)hsum - x*x);  var_y = max(0, Syy / (double)hsum - y*y);  cov_xy = Sxy / (double)hsum - x*y
 * A map on which flm_decode yields NaN (hsum == 0 under a negative thresh) yields NaN moments too.
 * flm_decode_stats has flm_decode's contracts and error codes (l <= 96, n_points <= 128, 16-byte aligned maps) and
 * reads the maps once; its workspace differs from flm_decode's only by the all-pixel partial sums (six instead of
 * three).  The workspace query returns 0 for arguments the call rejects. */
#define FLM_LANDMARK_REC 6
size_t flm_decode_stats_workspace_bytes(int n, int h, int w, int l, int mode, int n_points);
int flm_decode_stats(flm_stream_t stream, const float* hm_dev, int n, int h, int w, int l, int mode, int n_points,
                     float thresh, double* rec_dev /*[N,L,6]*/, void* workspace_dev, size_t workspace_bytes);

/* One read of the maps, up to FLM_SWEEP_MAX_MODES decodes (the n_points experiment of utils/metrics.py:118-154).
 * `modes` (host memory, n_modes entries, duplicates and any order allowed): 0 = all-pixel centroid, 1..128 = top-n.
 * out: float64 [n_modes, N, L, 2], slice m for modes[m].  A top-n slice is byte for byte what flm_decode(TOPN, n)
 * writes (same selection under the (value, flat index) order, the same float32 hsum chain, float64 index sums and reject
 * test); an all-pixel slice agrees with flm_decode(ALL) within 1e-9 px (float64 partial sums added in another order).
 * Errors: FLM_ERR_ARG for a null or empty list, more than FLM_SWEEP_MAX_MODES entries, or a misaligned map;
 * FLM_ERR_UNSUPPORTED for a mode outside 0..128; FLM_ERR_SHAPE / FLM_ERR_WORKSPACE as flm_decode.  The workspace query
 * returns 0 for arguments the call rejects. */
#define FLM_SWEEP_MAX_MODES 16
size_t flm_decode_sweep_workspace_bytes(int n, int h, int w, int l, const int* modes, int n_modes);
int flm_decode_sweep(flm_stream_t stream, const float* hm_dev, int n, int h, int w, int l, const int* modes,
                     int n_modes, float thresh, double* out_dev, void* workspace_dev, size_t workspace_bytes);

/* Gaussian target maps: generate_hm(height, width, keypoints, s) (data/generator.py:274-296) on the device.
 * kp_dev float64 [N,L,2] (x,y) in grid pixels -> out_dev float32 [N,H,W,L] (channel last, hm[:, :, i]):
 * out[r,c,i] = float32(exp(-((c - x0)**2 + (r - y0)**2) / two_sigma_sq)), evaluated in float64 in that order;
 * two_sigma_sq is the caller's `2 * sigma**2`.  A keypoint equal to (-1,-1) gives an all-zero map.  x runs along
 * the width (the reference passes (height, width) into gaussian_k's (width, height) slots, :293, so it only runs
 * on square maps, where the two agree).  out_dev must be 16-byte aligned. */
int flm_gaussian_heatmaps(flm_stream_t stream, const double* kp_dev, int n, int l, int h, int w, double two_sigma_sq,
                          float* out_dev);

/* ---- alignment (no reference implementation: README.md:1 states the intent only) --
 * Least-squares similarity (Umeyama, 4 dof) mapping each face's K landmarks onto a
 * template, returned as the 2x3 matrix M that maps SOURCE pixel coords to ALIGNED
 * coords; and the inverse-map bilinear warp with edge clamp (the skimage
 * `warp(..., mode="edge")` shape of data/generator.py:192-200). */
int flm_similarity_from_landmarks(flm_stream_t stream, const double* lm_dev /*[N,K,2]*/,
                                  const double* tmpl_dev /*[K,2]*/, int n, int k,
                                  float* m_dev /*[N,2,3]*/);
/* Same fit with the landmarks first taken from output-grid to crop pixel units: x * sx, y * sy in float64 (the
 * reference leaves decoded coordinates in grid units); points the decode rejected, (-1,-1), stay rejected. */
int flm_similarity_from_landmarks_scaled(flm_stream_t stream, const double* lm_dev /*[N,K,2]*/,
                                         const double* tmpl_dev /*[K,2]*/, int n, int k, double sx, double sy,
                                         float* m_dev /*[N,2,3]*/);
/* The same fit with a weight per point, read at element strides: point i of face f is the two doubles at
 * lm_dev + (f*k + i)*lm_stride, its weight the double at w_dev + (f*k + i)*w_stride; w_dev == NULL: every weight is 1.
 * With strides of FLM_LANDMARK_REC and w_dev = rec_dev + 2 the fit reads the forward's landmark records in place,
 * weighted by their scores.  A point takes part when both coordinates are >= 0 and its weight is > 0 (a NaN weight
 * fails that test and is left out).  float64, sequential sums in landmark order over the participating points, the
 * coordinates first multiplied by sx, sy as in the _scaled call:
 *   W = sum w;  mpx = sum(w*px) / W, likewise mpy, mqx, mqy (q: the template);  p' = p - mp, q' = q - mq
 *   sa = sum w*(px'*qx' + py'*qy');  sb = sum w*(px'*qy' - py'*qx');  var = sum w*(px'*px' + py'*py')
 *   a = sa / var, b = sb / var, tx = mqx - (a*mpx - b*mpy), ty = mqy - (b*mpx + a*mpy);  M = [[a,-b,tx],[b,a,ty]]
 * Fewer than two participating points, or var <= 0, gives the identity.  With unit weights every product by w is exact
 * and W is the count: the bits of flm_similarity_from_landmarks_scaled.
 * Errors: null lm, tmpl or m -> FLM_ERR_ARG; lm_stride < 2, w_stride < 1, n < 1 or k outside [1,1024] -> FLM_ERR_SHAPE. */
int flm_similarity_from_landmarks_weighted(flm_stream_t stream, const double* lm_dev, size_t lm_stride,
                                           const double* w_dev, size_t w_stride, const double* tmpl_dev /*[K,2]*/,
                                           int n, int k, double sx, double sy, float* m_dev /*[N,2,3]*/);
int flm_warp_affine(flm_stream_t stream, const void* src_dev /*[N,Hs,Ws,3]*/, int src_is_u8, int n,
                    int hs, int ws, const float* m_dev /*[N,2,3] src->dst*/,
                    float* dst_dev /*[N,Hd,Wd,3]*/, int hd, int wd);

/* ---- crop front-end (detect_marks pre-processing, prediction.py:76-83; get_image_array's resize,
 * data/generator.py:53) ---------------------------------------------------------------------------
 * `img[y0:y1, x0:x1]` + `cv2.resize(., (out_w, out_h))` (default INTER_LINEAR on uint8) for K boxes of one
 * uint8 BGR frame, into the model's input batch (uint8 BGR [K,out_h,out_w,3]); boxes are (x0,y0,x1,y1)
 * int32, already squared by the host-side box maths, clipped to the frame here (a box that misses the frame
 * gives zeros).  Integer fixed point: OpenCV's 11-bit-weight algorithm restated (csrc/flm_misc.hip states
 * every operation), bit-exact against oracle/warp_ref.py; parity with the cv2 binary itself is unpinned. */
int flm_crop_resize(flm_stream_t stream, const uint8_t* frame_dev, int fh, int fw,
                    const int32_t* boxes_dev /*[K,4]*/, int k, uint8_t* out_dev, int out_h, int out_w);
/* The same for the faces of SEVERAL frames in one launch (the multi-face stream of prediction.py:99-113, one launch
 * sequence per group of frames): `frames_dev` holds `nframes` uint8 BGR frames of fh x fw, `frame_stride` bytes apart
 * (a ring of stream frames in one allocation); box k is cut from frame frame_idx_dev[k] (an index outside [0, nframes)
 * gives zeros). */
int flm_crop_resize_frames(flm_stream_t stream, const uint8_t* frames_dev, size_t frame_stride, int nframes, int fh, int fw,
                           const int32_t* boxes_dev /*[K,4]*/, const int32_t* frame_idx_dev /*[K]*/, int k,
                           uint8_t* out_dev, int out_h, int out_w);

/* ---- frame-space tail of the multi-face stream ----------------------------------------------------------
 * The stream pipeline crops faces out of a ring of frames (flm_crop_resize_frames) and decodes landmarks on the
 * model's output grid.  These two calls finish it in FRAME coordinates: the landmarks of every face in pixels of its
 * frame, and the aligned face sampled from the frame itself -- one bilinear resampling of the original pixels instead
 * of the crop's resize followed by a warp, and real frame pixels where the rotated aligned square leaves the box.
 * flm_similarity_from_landmarks on the frame-space landmarks gives the M (frame px -> aligned px) the warp takes.
 *
 * flm_landmarks_to_frame: lm_dev float64 [K,C,2] (x,y) in output-grid pixels -> out_dev float64 [K,C,2] in frame
 * pixels (out_dev may equal lm_dev).  Per face the box (x0,y0,x1,y1) is clipped to the frame exactly as
 * flm_crop_resize clips it: cx0 = min(max(x0,0),fw), cx1 = min(max(x1,0),fw), cw = cx1-cx0 (same for y with fh).
 * Then, in float64 and in this order,
 *   xf = (double)cx0 + x * ((double)cw / grid_w);   yf = (double)cy0 + y * ((double)ch / grid_h)
 * -- the pure-scale convention of the reference's back-projection (prediction.py:91-94) before its float32 rounding
 * and truncation, on the region that was actually cropped.  A point the decode rejected (either coordinate negative)
 * stays (-1,-1); a face whose clipped box is empty gets (-1,-1) everywhere.
 * Errors: null pointer -> FLM_ERR_ARG; k, c, grid_h, grid_w, fh or fw below 1 -> FLM_ERR_SHAPE. */
int flm_landmarks_to_frame(flm_stream_t stream, const double* lm_dev /*[K,C,2] output-grid px*/,
                           const int32_t* boxes_dev /*[K,4]*/, int k, int c, int grid_h, int grid_w, int fh, int fw,
                           double* out_dev /*[K,C,2]*/);
/* flm_warp_affine_frames: the alignment warp with a per-face source frame.  The source of face f is frame
 * frame_idx_dev[f] of the ring (frames_dev + idx*frame_stride, uint8 BGR fh x fw: the layout flm_crop_resize_frames
 * reads; frame_idx_dev NULL = frame 0 for every face).  An index outside [0, nframes) gives zeros; with boxes_dev
 * given, a face whose clipped box is empty gives zeros too (it had no pixels to find landmarks in).
 *   samples == 1: per output pixel the arithmetic of flm_warp_affine (csrc/flm_misc.hip states it operation by
 *     operation: det, idet, the inverse, the two fmaf chains, clamp to [0,fw-1] x [0,fh-1], floor, the three fmafs
 *     of the bilinear blend) with the frame as the source: the same bits as flm_warp_affine on that frame.
 *   samples == 2 | 4: an s x s grid of such samples per output pixel, for faces that shrink on their way to the
 *     aligned size.  Sub-sample (i,j), i the row, is taken at destination coordinates xd + (2j+1-s)/(2s),
 *     yd + (2i+1-s)/(2s) (float32 sums; the offsets are exact), the sample values are added in float32 in row-major
 *     order starting from the first sample, and the sum is multiplied by 1/(s*s).
 * Errors: null frames / m / dst, or any other `samples` -> FLM_ERR_ARG; FLM_ERR_SHAPE (the limit is named in
 * flm_last_error()) unless 1 <= k <= 65535, nframes >= 1, fh >= 1, fw >= 2, fh*fw*3 < 2^31,
 * frame_stride >= fh*fw*3, hd, wd >= 1 and hd*wd*12 < 2^31. */
int flm_warp_affine_frames(flm_stream_t stream, const uint8_t* frames_dev, size_t frame_stride, int nframes, int fh,
                           int fw, const int32_t* frame_idx_dev /*[K] or NULL = frame 0*/,
                           const int32_t* boxes_dev /*[K,4] or NULL*/, const float* m_dev /*[K,2,3] frame px -> aligned px*/,
                           int k, float* dst_dev /*[K,hd,wd,3]*/, int hd, int wd, int samples);

/* ---- aligned faces in the consumer's format ---------------------------------------------------------------
 * flm_warp_affine and flm_warp_affine_frames write float32 [n,hd,wd,3], NHWC, in the source's channel order (BGR),
 * values as sampled (0..255 for uint8 sources).  The two calls below are the same warps with the conversion to what
 * reads the faces next -- an embedding network's planar, RGB, normalised float16 / bfloat16 input, or uint8 for
 * storage -- in the store of the warp itself, so that the single resampling of the original pixels is also the single
 * write of the result.  The format travels with the call: */
enum flm_pixel_layout { FLM_LAYOUT_NHWC = 0, FLM_LAYOUT_NCHW = 1 };
enum flm_pixel_type { FLM_PIX_F32 = 0, FLM_PIX_F16 = 1, FLM_PIX_BF16 = 2, FLM_PIX_U8 = 3 };
typedef struct flm_image_format {
  uint32_t struct_size;      /* as flm_forward_opts: lets the struct grow */
  int32_t layout, type;      /* flm_pixel_layout, flm_pixel_type */
  int32_t reverse_channels;  /* 0: output channel c = source channel c (BGR stays BGR); 1: source channel 2-c (RGB) */
  float scale[3], bias[3];   /* indexed by OUTPUT channel */
} flm_image_format;
/* NHWC, F32, reverse_channels 0, scale 1, bias 0: with these the calls below store the bits of the calls above. */
void flm_image_format_init(flm_image_format* fmt);
/* Bytes of n faces of h x w in this format (n*h*w*3 elements of 4, 2, 2 or 1 bytes); 0 for a format the calls below
 * reject (null, struct_size, unknown layout or type, reverse_channels, non-finite scale or bias) and for n, h or w
 * below 1. */
size_t flm_image_format_bytes(const flm_image_format* fmt, int n, int h, int w);
/* The contract, for output pixel (row, col) of face f, output channel c, source channel s = reverse_channels ? 2-c : c:
 *   v   the float32 value flm_warp_affine (flm_warp_affine_frames) writes for that pixel and channel s: the same
 *       operations in the same order, the same bits -- for samples = 2 | 4 including the float32 sum of the samples
 *       and the multiply by 1/(s*s).  A face those calls fill with zeros (a ring slot outside the ring, an empty
 *       clipped box) has v = 0, which goes through the next steps like any other value.
 *   t = v * scale[c]      float32 multiply, rounded
 *   u = t + bias[c]       float32 add, rounded: two operations, two roundings, never a fused multiply-add
 *   stored value:
 *     FLM_PIX_F32   u
 *     FLM_PIX_F16   u rounded to IEEE binary16, to nearest, ties to even; subnormals are gradual, overflow gives +-inf
 *     FLM_PIX_BF16  u rounded to bfloat16, to nearest, ties to even (on the float32 bits b:
 *                   (b + 0x7fff + ((b >> 16) & 1)) >> 16); a NaN stays a NaN
 *     FLM_PIX_U8    rintf(u) (ties to even) clamped to [0, 255]; a NaN u stores 0
 *   at element  FLM_LAYOUT_NHWC  ((f*hd + row)*wd + col)*3 + c          dense [n,hd,wd,3]
 *               FLM_LAYOUT_NCHW  (((f*3 + c)*hd + row)*wd + col         dense [n,3,hd,wd]
 * dst_dev needs the alignment of its element type and no more: it may be a slice of a larger buffer.  The kernels
 * choose 16-byte stores from the actual address of every run they write and fall back to element stores elsewhere;
 * no byte outside the n faces is written.
 * Errors, all found before anything is launched: a null src / frames / m / dst or fmt, an unknown layout or type, a
 * reverse_channels outside {0, 1}, a non-finite scale or bias, a dst that is not aligned to its element, or (frames
 * call) `samples` outside {1, 2, 4} -> FLM_ERR_ARG; a struct_size smaller than this library's -> FLM_ERR_ARG with
 * "struct_size" in the message.  FLM_ERR_SHAPE, the limit named in flm_last_error(), unless
 *   flm_warp_affine_fmt         1 <= n <= 65535, hs, ws >= 1, hs*ws*3*4 < 2^31, hd, wd >= 1, hd*wd*3*4 < 2^31
 *   flm_warp_affine_frames_fmt  1 <= k <= 65535, nframes >= 1, fh >= 1, fw >= 2, fh*fw*3 < 2^31,
 *                               frame_stride >= fh*fw*3, hd, wd >= 1, hd*wd*3*4 < 2^31
 * -- the limits of the float32 calls; the aligned-size limit counts float32 bytes whatever the type. */
int flm_warp_affine_fmt(flm_stream_t stream, const void* src_dev /*[N,Hs,Ws,3]*/, int src_is_u8, int n, int hs, int ws,
                        const float* m_dev /*[N,2,3] src->dst*/, void* dst_dev, int hd, int wd,
                        const flm_image_format* fmt);
int flm_warp_affine_frames_fmt(flm_stream_t stream, const uint8_t* frames_dev, size_t frame_stride, int nframes, int fh,
                               int fw, const int32_t* frame_idx_dev /*[K] or NULL = frame 0*/,
                               const int32_t* boxes_dev /*[K,4] or NULL*/,
                               const float* m_dev /*[K,2,3] frame px -> aligned px*/, int k, void* dst_dev, int hd,
                               int wd, int samples, const flm_image_format* fmt);

/* ---- the decoder's surface as the ring: NV12 frame slots ------------------------------------------------------
 * Video decoders hand out NV12: an 8-bit luma plane and an interleaved half-resolution U,V plane, rows `pitch` bytes
 * apart, the U,V plane at an aligned row offset.  The calls below read such slots directly, so that the one resampling
 * of the original pixels starts from the decoder's bytes and no BGR copy of a whole frame is made.  Their contract: THE
 * BITS ARE THOSE OF THE BGR CALL ON THE FRAME THAT THE INTEGER CONVERSION BELOW PRODUCES.
 *
 * For pixel (x, y) of an fh x fw slot at byte address s (all arithmetic int32, >> an arithmetic shift):
 *   Y = s[y*y_pitch + x]
 *   U = s[uv_offset + (y>>1)*uv_pitch + (x & ~1)];  V = the byte after U
 *       (chroma is replicated over its 2x2 block, not interpolated)
 *   yy = max(Y - 16, 0) * CY;   u = U - 128;   v = V - 128
 *   B = clamp((yy + CUB*u         + (1<<19)) >> 20, 0, 255)
 *   G = clamp((yy + CVG*v + CUG*u + (1<<19)) >> 20, 0, 255)
 *   R = clamp((yy + CVR*v         + (1<<19)) >> 20, 0, 255)
 * with (CY, CUB, CUG, CVG, CVR) =
 *   FLM_YUV_BT601_LIMITED  (1220542, 2116026, -409993, -852492, 1673527): 1.164 / 2.018 / -0.391 / -0.813 / 1.596 x 2^20,
 *                          the published fixed-point form of OpenCV's COLOR_YUV2BGR_NV12 (parity with a cv2 binary is
 *                          unpinned, as for the resize)
 *   FLM_YUV_BT709_LIMITED  (1220945, 2215014, -223607, -558796, 1879825): round(exact coefficient x 2^20) with
 *                          Kr = 0.2126, Kb = 0.0722 -- what 1080p decoders tag
 * Over all 2^24 (Y,U,V) the accumulators stay within +-573,636,921 < 2^31; Y=16, U=V=128 gives 0 and Y=235 gives 255. */
enum flm_frame_pixel { FLM_FRAME_BGR24 = 0, FLM_FRAME_NV12 = 1 };
enum flm_yuv_matrix { FLM_YUV_BT601_LIMITED = 0, FLM_YUV_BT709_LIMITED = 1 };
typedef struct flm_frame_format {
  uint32_t struct_size; /* as flm_image_format */
  int32_t pixel, matrix; /* flm_frame_pixel, flm_yuv_matrix (the matrix is not used by FLM_FRAME_BGR24) */
  uint32_t y_pitch;     /* bytes between luma rows, 0 = fw */
  uint32_t uv_pitch;    /* bytes between U,V rows, 0 = y_pitch */
  uint64_t uv_offset;   /* slot start -> first U,V row, 0 = y_pitch*fh */
} flm_frame_format;
/* FLM_FRAME_BGR24, everything else 0: the dense uint8 BGR ring of flm_crop_resize_frames. */
void flm_frame_format_init(flm_frame_format* src);
/* Bytes of a slot that the kernels may read: fh*fw*3 for BGR24; for NV12 uv_offset + (fh/2 - 1)*uv_pitch + fw with the
 * defaults resolved (the last U,V row ends after its fw bytes, not after its pitch).  No kernel reads a byte outside
 * [slot, slot + this).  0 for a format or size the calls below reject. */
size_t flm_frame_format_bytes(const flm_frame_format* src, int fh, int fw);
/* flm_frames_to_bgr: slots 0..nframes-1 of an NV12 ring -> out_dev uint8 BGR [nframes,fh,fw,3], dense: B,G,R of the
 *   conversion above.  The path an NV12 caller has without the two calls below.  (A BGR24 `src` is rejected with
 *   FLM_ERR_ARG: there is nothing to convert.)
 * flm_crop_resize_frames_src: flm_crop_resize_frames with the ring in the format `src`.
 * flm_warp_affine_frames_src: flm_warp_affine_frames_fmt with the ring in the format `src`; fmt NULL = float32 NHWC
 *   BGR, scale 1, bias 0, the bits of flm_warp_affine_frames.
 * FLM_FRAME_BGR24: y_pitch, uv_pitch and uv_offset must be 0; the calls are the existing ones, with their limits and
 *   their bits.
 * FLM_FRAME_NV12: bit for bit what flm_crop_resize_frames / flm_warp_affine_frames_fmt give on the converted frame --
 *   samples 1 | 2 | 4, every layout, type, channel order, scale and bias, and the zero fill for a slot outside the
 *   ring and for an empty clipped box included.
 * Errors, all found before anything is launched: a null pointer (frames, boxes, frame_idx, out; frames, m, dst; src),
 *   an unknown pixel or matrix, a struct_size smaller than this library's, and what flm_warp_affine_frames_fmt answers
 *   with FLM_ERR_ARG -> FLM_ERR_ARG.  FLM_ERR_SHAPE, the limit named in flm_last_error(), unless (NV12)
 *   fh and fw even and >= 2, y_pitch >= fw, uv_pitch >= fw, uv_offset >= y_pitch*fh, slot bytes < 2^31,
 *   frame_stride >= flm_frame_format_bytes, nframes >= 1, 1 <= k <= 65535, oh, ow >= 1 and oh*ow*3 < 2^31 (crop),
 *   hd, wd >= 1 and hd*wd*3*4 < 2^31 (warp); a BGR24 format with a non-zero pitch or offset is FLM_ERR_SHAPE too. */
int flm_frames_to_bgr(flm_stream_t stream, const uint8_t* frames_dev, size_t frame_stride, int nframes, int fh, int fw,
                      const flm_frame_format* src, uint8_t* out_dev /*[nframes,fh,fw,3]*/);
int flm_crop_resize_frames_src(flm_stream_t stream, const uint8_t* frames_dev, size_t frame_stride, int nframes, int fh,
                               int fw, const int32_t* boxes_dev /*[K,4]*/, const int32_t* frame_idx_dev /*[K]*/, int k,
                               uint8_t* out_dev, int out_h, int out_w, const flm_frame_format* src);
int flm_warp_affine_frames_src(flm_stream_t stream, const uint8_t* frames_dev, size_t frame_stride, int nframes, int fh,
                               int fw, const int32_t* frame_idx_dev /*[K] or NULL = frame 0*/,
                               const int32_t* boxes_dev /*[K,4] or NULL*/,
                               const float* m_dev /*[K,2,3] frame px -> aligned px*/, int k, void* dst_dev, int hd,
                               int wd, int samples, const flm_image_format* fmt /* NULL = float32 NHWC BGR */,
                               const flm_frame_format* src);

/* ---- shape-normalised faces: a piecewise-affine warp over the landmark mesh -------------------------------------------
 * The similarity warps above use four degrees of freedom of a face's landmarks.  The calls below use all of them: the
 * aligned rectangle is cut into triangles whose corners are the landmarks' TEMPLATE positions, and every triangle is
 * filled from the frame by the affine that takes this face's landmarks in this frame onto its three corners -- so every
 * landmark's texture lands on its template pixel, whatever the expression and the pose the similarity left.  (An
 * addition to ABI version 2: no existing call, struct or bit changes.)
 *
 * A MESH is P = C + A points, float64 [P,2] in aligned pixels, and T triangles, int32 [T,3] of point indices, with
 * 3 <= P <= 256, 0 <= A <= P, 1 <= T <= 255.  Points 0..C-1 are the template positions of landmarks 0..C-1; points
 * C..P-1 are ANCHORS, template positions without a landmark, whose place in the frame is M^-1 of their template
 * position -- with anchors on the border of the aligned rectangle the mesh covers it and meets the similarity warp there.
 * Triangles are positively oriented ((bx-ax)*(cy-ay) - (by-ay)*(cx-ax) > 0) and not degenerate in the template; the
 * Python class alignment.FaceMesh checks both.  A triangle that names a point outside [0,P) is never dereferenced: the
 * map skips it and its matrix is the face's M.
 *
 * All mesh arithmetic is float64, one IEEE operation per written operator, in the written order, no fused multiply-add.
 *
 * flm_mesh_map, once per mesh and aligned size: map[y][x] = the LOWEST t whose three edge functions at the integer
 *   point q = (x, y) are all >= 0, 255 if none is.  For corners a, b, c of triangle t, in that order, the edges are
 *   a->b, b->c, c->a and
 *     E_ab(q) = (bx-ax)*(qy-ay) - (by-ay)*(qx-ax)          two products, one subtraction, in that order
 *   (a point on a shared edge or vertex has E = 0 in every triangle that shares it: the lowest index wins).
 *
 * flm_mesh_affines: aff[f][t], float32 [K,T,2,3], the forward matrix FRAME px -> ALIGNED px of every (face, triangle).
 *   Landmark j of face f is lm_dev[(f*C + j)*lm_stride + {0,1}] (lm_stride float64 elements between points, >= 2: a
 *   dense [K,C,2] tensor has 2, the x,y of a landmark record tensor FLM_LANDMARK_REC).  m_dev is the face's similarity M,
 *   float32 [K,2,3], frame px -> aligned px (flm_similarity_from_landmarks*, flm_track_step).  The source s_v of mesh
 *   vertex v with template position d_v:
 *     v < C    s_v = the face's landmark v
 *     v >= C   det = m00*m11 - m01*m10;  i00 = m11/det, i01 = (-m01)/det, i10 = (-m10)/det, i11 = m00/det
 *              sx = i00*(dx-m02) + i01*(dy-m12);  sy = i10*(dx-m02) + i11*(dy-m12)      (M widened to float64 first)
 *   and for triangle (v0, v1, v2) with e1 = s1-s0, e2 = s2-s0, g1 = d1-d0, g2 = d2-d0, det = e1x*e2y - e1y*e2x:
 *     a00 = (g1x*e2y - g2x*e1y)/det     a01 = (g2x*e1x - g1x*e2x)/det     a02 = d0x - (a00*s0x + a01*s0y)
 *     a10 = (g1y*e2y - g2y*e1y)/det     a11 = (g2y*e1x - g1y*e2x)/det     a12 = d0y - (a10*s0x + a11*s0y)
 *   each of the six rounded to float32 (nearest even).  When !(fabs(det) >= min_det) -- collapsed, collinear or NaN
 *   landmarks -- the triangle takes the face's M unchanged.  min_det >= 0; 1e-6 is the Python default.
 *
 * flm_warp_mesh_frames: the faces, in ONE launch.  THE CONTRACT: for output pixel (x, y) of face f with
 *   map[y][x] = t < T, the stored element has the bits that flm_warp_affine_frames_src stores at (x, y) of face f when
 *   it is given m = aff[f][t] and the same frames, frame_idx, boxes, samples, fmt and src.  A pixel's triangle is chosen
 *   at its centre and used for all its samples x samples sub-samples.  A pixel with map[y][x] >= T (255: no triangle)
 *   stores what a zero face stores: v = 0 through the format's epilogue.  A ring slot outside [0,nframes) and an empty
 *   clipped box give a zero face as they do there.  fmt NULL = float32 NHWC BGR, scale 1, bias 0; src NULL = the dense
 *   BGR24 ring.  map_dev is flm_mesh_map's for this mesh at hd x wd.  aff_out_dev, when not NULL, receives
 *   [K,T,2,3]: the bits of flm_mesh_affines, zero faces included.  No atomics, no allocation, no byte outside the K
 *   faces (and aff_out) written.
 *
 * Errors, all found before anything is launched: those of flm_warp_affine_frames_src with their codes (null frames / m /
 *   dst, formats, samples -> FLM_ERR_ARG; ring, k and aligned-size limits -> FLM_ERR_SHAPE); in addition a null
 *   lm / pts / tris / map (aff for flm_mesh_affines), t outside [1,255], p outside [3,256], a outside [0,p],
 *   lm_stride < 2 and a min_det that is negative or NaN -> FLM_ERR_ARG.  flm_mesh_map: hd, wd >= 1 and
 *   hd*wd*3*4 < 2^31, else FLM_ERR_SHAPE; flm_mesh_affines: 1 <= k <= 65535, else FLM_ERR_SHAPE. */
int flm_mesh_map(flm_stream_t stream, const double* pts_dev /*[P,2]*/, const int32_t* tris_dev /*[T,3]*/, int p, int t,
                 int hd, int wd, uint8_t* map_dev /*[hd,wd]*/);
int flm_mesh_affines(flm_stream_t stream, const double* lm_dev, int lm_stride, const float* m_dev /*[K,2,3]*/,
                     const double* pts_dev /*[P,2]*/, const int32_t* tris_dev /*[T,3]*/, int p, int a, int t, int k,
                     double min_det, float* aff_dev /*[K,T,2,3]*/);
int flm_warp_mesh_frames(flm_stream_t stream, const uint8_t* frames_dev, size_t frame_stride, int nframes, int fh, int fw,
                         const int32_t* frame_idx_dev /*[K] or NULL = frame 0*/,
                         const int32_t* boxes_dev /*[K,4] or NULL*/, const double* lm_dev, int lm_stride,
                         const float* m_dev /*[K,2,3] frame px -> aligned px*/, const double* pts_dev /*[P,2]*/,
                         const int32_t* tris_dev /*[T,3]*/, int p, int a, int t, const uint8_t* map_dev /*[hd,wd]*/,
                         int k, void* dst_dev, int hd, int wd, int samples,
                         const flm_image_format* fmt /* NULL = float32 NHWC BGR */,
                         const flm_frame_format* src /* NULL = BGR24 */, double min_det,
                         float* aff_out_dev /*[K,T,2,3] or NULL*/);

/* ---- tracking: the next frame's crop from this frame's landmarks --------------------------------------------------
 * The stream above starts every frame from detector boxes on the host.  The calls below keep a face's crop on the
 * device instead: the network input of frame t+1 is cut from the frame by the similarity that takes the landmarks of
 * frame t onto a template in input pixels (upright, centred, at a fixed scale), sampled by flm_warp_affine_frames_src
 * with a uint8 NHWC flm_image_format.  A detector is needed to seed a track and to re-seed one that was lost
 * (flm_track_associate, at the end of this section, does both from boxes on the device).  Per
 * face the state is a crop matrix M (float32 [2,3], FRAME px -> network-INPUT px), a box (int32 x0,y0,x1,y1: the frame
 * region the crop covers; empty = the slot holds no face, and the frame warps fill such a face with zeros) and a status
 * word.  Everything below is float64, one IEEE operation per written operator, in the written order, no fused
 * multiply-add; (float) and (double) are the conversions, (float) rounding to nearest even.  "Clipped" is the clip of
 * flm_landmarks_to_frame: cx0 = min(max(x0,0),fw), cx1 = min(max(x1,0),fw), cy0, cy1 with fh; empty: cx1-cx0 <= 0 or
 * cy1-cy0 <= 0. */
enum flm_track_status {      /* bits of a status word; 0 = the face is tracked */
  FLM_TRACK_DEAD = 1,        /* the incoming box, clipped, is empty: the slot held no face */
  FLM_TRACK_FEW_POINTS = 2,  /* fewer than min_points landmarks took part in the fit */
  FLM_TRACK_LOW_SCORE = 4,   /* mean weight of the participating landmarks below min_score */
  FLM_TRACK_SCALE = 8,       /* the next crop's side in frame px outside [min_side, max_side] */
  FLM_TRACK_OUTSIDE = 16,    /* the next crop's centre lies outside the frame */
  /* set by flm_track_associate alone (below); flm_track_step never sets them */
  FLM_TRACK_DUPLICATE = 32,  /* a live track in a lower slot covers the same face */
  FLM_TRACK_UNCONFIRMED = 64 /* no detection matched the track in max_misses consecutive calls */
};
typedef struct flm_track_opts {
  uint32_t struct_size;      /* as flm_forward_opts: lets the struct grow */
  int32_t min_points;        /* >= 2 */
  double min_score, min_side, max_side;
} flm_track_opts;
/* min_points = 2, min_score = 0, min_side = 0, max_side = +inf: only the geometric tests can lose a track. */
void flm_track_opts_init(flm_track_opts* opts);

/* flm_track_seed: detector boxes (squared by the host-side box maths, as for flm_crop_resize) -> crop matrices.
 *   bw = x1-x0, bh = y1-y0;  sx = (double)in_w / (double)bw;  sy = (double)in_h / (double)bh
 *   M = [[(float)sx, 0, (float)((0.5 - (double)x0)*sx - 0.5)], [0, (float)sy, (float)((0.5 - (double)y0)*sy - 0.5)]]
 * -- the pixel-centre convention of the resize that flm_crop_resize restates: input pixel xd samples the frame at
 * x0 + (xd+0.5)/sx - 0.5.  status = 0.  A box that is empty after clipping gives the identity matrix and
 * status = FLM_TRACK_DEAD.  (For a box inside the frame and no smaller than the input the uint8 warp with M samples
 * where flm_crop_resize samples; float bilinear against 11-bit fixed-point weights can differ by one in a pixel's
 * value.  A smaller box is enlarged: its outermost input pixels sample up to half a source pixel beyond the box, where
 * flm_crop_resize replicates the box's edge and the warp reads the frame.)
 * Errors: null pointer -> FLM_ERR_ARG; FLM_ERR_SHAPE unless 1 <= k <= 65535 and in_h, in_w, fh, fw >= 1. */
int flm_track_seed(flm_stream_t stream, const int32_t* boxes_dev /*[K,4]*/, int k, int in_h, int in_w, int fh, int fw,
                   float* m_dev /*[K,2,3]*/, int32_t* status_dev /*[K]*/);

/* flm_landmarks_from_crop: landmarks on the model's output grid -> frame pixels through a crop matrix; the affine
 * counterpart of flm_landmarks_to_frame.  Point i of face f is the two doubles at lm_dev + (f*c + i)*lm_stride (2 for
 * plain landmarks, FLM_LANDMARK_REC for landmark records, as the weighted fit reads them); sx = in_w/grid_w and
 * sy = in_h/grid_h take grid px to input px; out_dev is dense float64 [K,C,2] and must not overlap lm_dev.
 *   per face:   m00..m12 = (double) of the six floats;  det = m00*m11 - m01*m10
 *   per point:  xi = x*sx;  yi = y*sy;  u = xi - m02;  v = yi - m12
 *               xf = (m11*u - m01*v) / det;   yf = (m00*v - m10*u) / det
 * A point is written as (-1,-1) when the decode rejected it (x < 0 or y < 0), when xf or yf is negative or not finite
 * (a rotated crop may reach past the frame's edge: "negative means rejected" holds in frame px too), and -- every
 * point of the face -- when det is zero or not finite.
 * The warp that cut the crop inverts M in float32 (csrc/flm_misc.hip states it), this call inverts it in float64: on
 * a 1080p frame the two positions of one input pixel differ at the 1e-4 px level.
 * Errors: null pointer -> FLM_ERR_ARG; FLM_ERR_SHAPE unless 1 <= k <= 65535, 1 <= c <= 1024, lm_stride >= 2 and
 * sx, sy > 0. */
int flm_landmarks_from_crop(flm_stream_t stream, const double* lm_dev, size_t lm_stride, const float* m_dev /*[K,2,3]*/,
                            int k, int c, double sx, double sy, double* out_dev /*[K,C,2]*/);

/* flm_track_step: everything between the forward of frame t and the two warps that follow it, in ONE launch (a
 * workgroup of one wave per face).
 * In:  lm_dev at lm_stride and w_dev at w_stride (NULL = unit weights), as flm_similarity_from_landmarks_weighted takes
 *      them; m_crop_dev [K,2,3] and boxes_dev [K,4], the matrices and boxes this frame's crops were cut with; sx, sy as
 *      above; tmpl_crop_dev float64 [C,2] in input px, where the landmarks should sit in the NEXT crop; tmpl_align_dev
 *      float64 [C,2] in aligned px (NULL together with m_align_dev: no aligned fit); opts (NULL = the defaults).
 * Out: lm_frame_dev float64 [K,C,2]; m_align_dev float32 [K,2,3] frame px -> aligned px; m_next_dev float32 [K,2,3]
 *      frame px -> input px of the next crop (may be m_crop_dev); boxes_next_dev int32 [K,4] (may be boxes_dev);
 *      status_dev int32 [K].  No other overlap of an output with an input or another output is allowed.
 * Contract, in this order:
 *  1. dead = the clipped boxes_dev[f] is empty.  lm_frame = what flm_landmarks_from_crop writes, bit for bit; (-1,-1)
 *     everywhere for a dead face.
 *  2. m_align, m_next = what flm_similarity_from_landmarks_weighted writes for lm_frame (stride 2) with these weights,
 *     sx = sy = 1 and tmpl_align, tmpl_crop, bit for bit.  cnt is that fit's number of participating points and W its
 *     sequential weight sum (the same for both templates; cnt = 0, W = 0 for a dead face, whose fits are the identity).
 *  3. status = the OR of
 *       FLM_TRACK_DEAD        dead
 *       FLM_TRACK_FEW_POINTS  cnt < min_points
 *       FLM_TRACK_LOW_SCORE   w_dev given and !(W / (double)cnt >= min_score)            (0/0 = NaN sets it)
 *       FLM_TRACK_SCALE       a = (double)m_next[0][0], b = (double)m_next[1][0];
 *                             side = (double)in_w / sqrt(a*a + b*b);  !(side >= min_side && side <= max_side)
 *       FLM_TRACK_OUTSIDE     the centre ((double)(in_w-1)/2, (double)(in_h-1)/2) taken to the frame by back(), is not
 *                             inside: !(det finite, det != 0, 0 <= xf <= fw-1 and 0 <= yf <= fh-1)
 *     every test made on m_next as fitted in 2, whatever the other tests say.  back(x, y), with m00..m12 the floats of
 *     m_next widened: det = m00*m11 - m01*m10; u = x - m02; v = y - m12; xf = (m11*u - m01*v)/det;
 *     yf = (m00*v - m10*u)/det -- the formula of flm_landmarks_from_crop.
 *  4. status == 0: with back() of the corner centres (0,0), (in_w-1,0), (0,in_h-1), (in_w-1,in_h-1), in that order,
 *       mn = first; mn = (next < mn) ? next : mn; ... likewise mx with >, per coordinate
 *       boxes_next = ((int32)cl(floor(mnx)), (int32)cl(floor(mny)), (int32)cl(ceil(mxx) + 1.0), (int32)cl(ceil(mxy) + 1.0))
 *       cl(t) = min(max(t, -2^30), 2^30)
 *     -- the crop's bounding box in the frame; it holds the centre, which is inside, so its clip is never empty.
 *  5. status != 0, the track is lost: boxes_next = (0,0,0,0) and m_next is the identity; m_align keeps the fit of 2
 *     (the identity for a dead face).  The empty box makes the slot dead at the next step, and harmless: the frame
 *     warps fill a face whose clipped box is empty with zeros, and its matrix is finite.
 * Errors, all found before anything is launched: a null lm, m_crop, boxes, tmpl_crop, lm_frame, m_next, boxes_next or
 * status, m_align_dev without tmpl_align_dev or the reverse, a struct_size smaller than this library's ("struct_size"
 * in the message), min_points < 2, or a NaN min_score, min_side or max_side -> FLM_ERR_ARG.  FLM_ERR_SHAPE, the limit
 * named in flm_last_error(), unless 1 <= k <= 65535, 1 <= c <= 1024, lm_stride >= 2, w_stride >= 1, sx, sy > 0 and
 * in_h, in_w, fh, fw >= 1. */
int flm_track_step(flm_stream_t stream, const double* lm_dev, size_t lm_stride, const double* w_dev, size_t w_stride,
                   const float* m_crop_dev /*[K,2,3]*/, const int32_t* boxes_dev /*[K,4]*/, int k, int c, double sx,
                   double sy, int in_h, int in_w, int fh, int fw, const double* tmpl_crop_dev /*[C,2]*/,
                   const double* tmpl_align_dev /*[C,2] or NULL*/, const flm_track_opts* opts,
                   double* lm_frame_dev /*[K,C,2]*/, float* m_align_dev /*[K,2,3] or NULL*/,
                   float* m_next_dev /*[K,2,3]*/, int32_t* boxes_next_dev /*[K,4]*/, int32_t* status_dev /*[K]*/);

/* flm_track_step_filtered: flm_track_step with a One-Euro filter (Casiez, Roussel, Vogel 2012: a first-order low-pass
 * whose cutoff rises with the point's speed) on every landmark, inside the same single launch: between step 1 and step 2
 * of flm_track_step's contract.  The filter runs per landmark in 2-D, in frame px, in float64; speed is the length of
 * the 2-D velocity (a rolled head is treated like an upright one), measured in CROP SIDES per second (beta means the
 * same at every face size); the velocity is taken from the previous RAW position, as the authors' implementation does.
 * State per point, state_dev float64 [K,C,6], read and written: (xh, yh, vx, vy, xr, yr) -- the previous filtered
 * position, the filtered velocity in px/s, the previous raw position.  A point HAS NO HISTORY when xh < 0, yh < 0 or any
 * of the six is not finite: a state buffer filled with -1 is a reset.  dt is the time since the previous step in
 * seconds.  lm_raw_dev float64 [K,C,2] (or NULL) receives the raw points.
 * Contract: one IEEE float64 operation per written operator, in the written order, nothing fused;
 * TWO_PI is the double 6.283185307179586.
 *   raw (x, y) = what step 1 of flm_track_step writes for this point (frame px; (-1,-1) = rejected, or a dead face)
 *   side       = (double)in_w / sqrt(m00*m00 + m10*m10)        m00, m10 of THIS frame's m_crop, widened
 *   rejected raw:        out = (-1,-1);  state = (-1,-1,0,0,-1,-1)
 *   raw ok, no history:  out = (x, y);   state = (x, y, 0, 0, x, y)
 *   raw ok, history:
 *     rx = (x - xr) / dt;  ry = (y - yr) / dt
 *     ad = 1.0 / (1.0 + (1.0 / (TWO_PI * d_cutoff)) / dt)
 *     vx' = ad*rx + (1.0 - ad)*vx;   vy' = ad*ry + (1.0 - ad)*vy
 *     fc = min_cutoff + beta * (sqrt(vx'*vx' + vy'*vy') / side)
 *     a  = 1.0 / (1.0 + (1.0 / (TWO_PI * fc)) / dt)
 *     xh' = a*x + (1.0 - a)*xh;      yh' = a*y + (1.0 - a)*yh
 *     xh', yh', vx', vy' all finite:  out = (xh', yh');  state = (xh', yh', vx', vy', x, y)
 *     otherwise:                      as "no history"
 * lm_frame = out, lm_raw = raw, and steps 2 to 5 of flm_track_step (both fits, the status tests, the box) run on out.
 * out is a convex combination of non-negative numbers, so "negative means rejected" still holds in frame px.
 * Two properties follow from the arithmetic and are part of the contract: when no point has history (the first frame
 * after a seed), and at every step when min_cutoff = +inf (1/(TWO_PI*inf) = 0, so a = 1 and 1*x + 0*xh = x), the five
 * outputs of flm_track_step are flm_track_step's, bit for bit.
 * Defaults (flm_track_filter_init): min_cutoff = 1 Hz, beta = 15, d_cutoff = 1 Hz.  A point moving steadily at v sides/s
 * lags by side*v / (2 pi (min_cutoff + beta*v)) < side / (2 pi beta): 1.06 % of the crop side at any speed.  At rest and
 * 30 frames/s a = 0.173: white noise leaves with sqrt(a/(2-a)) = 0.31 of its standard deviation.
 * state_dev and lm_raw_dev must not overlap each other or any other argument.
 * Errors, all found before anything is launched: those of flm_track_step; a null filt or state_dev, a struct_size
 * smaller than this library's or a non-zero reserved -> FLM_ERR_ARG; FLM_ERR_ARG, the field named in flm_last_error(),
 * unless min_cutoff > 0 (+inf allowed), beta >= 0 and finite, d_cutoff > 0 and finite, dt > 0 and finite. */
typedef struct flm_track_filter {
  uint32_t struct_size;      /* as flm_track_opts */
  uint32_t reserved;         /* 0 */
  double min_cutoff, beta, d_cutoff;
} flm_track_filter;
void flm_track_filter_init(flm_track_filter* filt);   /* min_cutoff = 1.0, beta = 15.0, d_cutoff = 1.0 */
int flm_track_step_filtered(flm_stream_t stream, const double* lm_dev, size_t lm_stride, const double* w_dev,
                            size_t w_stride, const float* m_crop_dev /*[K,2,3]*/, const int32_t* boxes_dev /*[K,4]*/,
                            int k, int c, double sx, double sy, int in_h, int in_w, int fh, int fw,
                            const double* tmpl_crop_dev /*[C,2]*/, const double* tmpl_align_dev /*[C,2] or NULL*/,
                            const flm_track_opts* opts, double* lm_frame_dev /*[K,C,2]*/,
                            float* m_align_dev /*[K,2,3] or NULL*/, float* m_next_dev /*[K,2,3]*/,
                            int32_t* boxes_next_dev /*[K,4]*/, int32_t* status_dev /*[K]*/,
                            const flm_track_filter* filt, double dt, double* state_dev /*[K,C,6]*/,
                            double* lm_raw_dev /*[K,C,2] or NULL*/);

/* ---- rows: stepping a subset of the slots, each on its own clock --------------------------------------------------------
 * A tracker of S streams steps, on a tick, only the streams that delivered a frame.  The host knows which; the three
 * calls below do the rest on the device without a synchronisation.  A ROW r in [0, N) is one face of the compacted
 * batch; slot_dev int32 [N] names its global SLOT g.  A row is VALID when 0 <= g < n_slots and INERT otherwise.  Rows
 * must name distinct slots: where two valid rows name one slot, that slot's results are one of the rows' values per
 * written element, nothing else is affected and nothing is accessed out of bounds.
 *
 * flm_track_gather_streams: the step's snapshot, in ONE launch (a thread per row; a copy).  For streams, N = A*K and
 * row a*K + j is slot active[a]*K + j.
 * In:  active_dev int32 [A], the stream ids; a, s, k (slots PER STREAM); frame_idx_stream_dev int32 [S] or NULL (ring
 *      slot 0 for every row); dt_stream_dev float64 [S] or NULL; m_crop_dev float32 [S*K,2,3]; boxes_dev int32 [S*K,4];
 *      best_q_dev float64 [S*K] or NULL.
 * In/out: reset_dev int32 [S*K] or NULL.
 * Out, compact: slot_c int32 [A*K], m_c float32 [A*K,2,3], boxes_c int32 [A*K,4], frame_idx_c int32 [A*K], and, each
 *      required exactly when its input is given, dt_c float64 [A*K], best_q_c float64 [A*K], reset_c int32 [A*K].
 * Contract:
 *  1. active[a] in [0, S): with g = active[a]*K + j and r = a*K + j, slot_c[r] = g, m_c[r], boxes_c[r], best_q_c[r]
 *     and reset_c[r] are bit copies of the entries at g, frame_idx_c[r] = frame_idx_stream[active[a]] (0 without it)
 *     and dt_c[r] = dt_stream[active[a]], bit copies too.  reset_dev[g] is then set to 0: the pending reset MOVES into
 *     the snapshot.
 *  2. active[a] outside [0, S): slot_c = -1, m_c = the identity, boxes_c = (0,0,0,0), frame_idx_c = 0, dt_c = 0.0,
 *     best_q_c = -1.0, reset_c = 0 for the K rows; nothing global is read or written for them.
 *  3. A stream that is not named is neither read nor written.
 *  4. Stream ids must be distinct.  Where one is repeated, the compact rows are still the copies of 1 except reset_c,
 *     which is one of (the pending value, 0) per row; nothing else is affected and nothing is accessed out of bounds.
 *  5. One launch, no workspace, no allocation, no synchronisation.  No two arguments may overlap.
 * Errors, all found before anything is launched: a null active_dev, m_crop_dev, boxes_dev, slot_c, m_c, boxes_c or
 * frame_idx_c, or an optional output without its input or the reverse -> FLM_ERR_ARG.  FLM_ERR_SHAPE, the limit named in
 * flm_last_error(), unless 1 <= a, 1 <= s, 1 <= k, a*k <= 65535 and s*k <= 65535. */
int flm_track_gather_streams(flm_stream_t stream, const int32_t* active_dev /*[A]*/, int a, int s, int k /*slots PER STREAM*/,
                             const int32_t* frame_idx_stream_dev /*[S] or NULL*/, const double* dt_stream_dev /*[S] or NULL*/,
                             const float* m_crop_dev /*[S*K,2,3]*/, const int32_t* boxes_dev /*[S*K,4]*/,
                             const double* best_q_dev /*[S*K] or NULL*/, int32_t* reset_dev /*[S*K] or NULL, in/out*/,
                             int32_t* slot_c /*[A*K]*/, float* m_c /*[A*K,2,3]*/, int32_t* boxes_c /*[A*K,4]*/,
                             int32_t* frame_idx_c /*[A*K]*/, double* dt_c /*[A*K] or NULL*/,
                             double* best_q_c /*[A*K] or NULL*/, int32_t* reset_c /*[A*K] or NULL*/);

/* flm_track_gather_live: flm_track_gather_streams with the row map computed from the slots' LIVENESS instead of read from
 * active_dev, in ONE launch (one workgroup; a prefix count over the slots, no atomics: the row order is a function of the
 * inputs alone).  Which slots hold a face is known only on the device -- flm_track_step loses tracks there,
 * flm_track_associate* starts them there --, so the map is made there: the live slots are compacted into a batch of the
 * fixed size N (the BUDGET, a host number: every launch shape that follows is known without a synchronisation).  Live
 * slots beyond the budget sit the call out with their state intact and are served first by the next call.
 * In:  stream_on_dev int32 [S] or NULL (NULL: every stream is on); s, k (slots PER STREAM), fh, fw; n, the budget = the
 *      number of rows; frame_idx_stream_dev int32 [S] or NULL; dt_stream_dev float64 [S] or NULL, with the scalar dt;
 *      m_crop_dev float32 [S*K,2,3]; boxes_dev int32 [S*K,4]; best_q_dev float64 [S*K] or NULL.
 * In/out: reset_dev int32 [S*K] or NULL; age_dev float64 [S*K] or NULL, the seconds every slot has waited unserved;
 *      cursor_dev int32 [1] or NULL, the slot the order starts from.
 * Out, compact: slot_c int32 [N], m_c float32 [N,2,3], boxes_c int32 [N,4], frame_idx_c int32 [N], and, each required
 *      exactly when its input is given, dt_c float64 [N] (age_dev), best_q_c float64 [N] (best_q_dev), reset_c int32 [N]
 *      (reset_dev); counts_dev int32 [4].
 * Contract:
 *  1. Slot g belongs to stream i = g / K.  It is ELIGIBLE when (stream_on_dev is NULL or stream_on_dev[i] != 0) and the
 *     clip of boxes_dev[g] to fh x fw -- the clip of flm_landmarks_to_frame -- is not empty: the negation of the DEAD test
 *     of flm_track_step, step 1.  E = the number of eligible slots.
 *  2. c0 = cursor_dev[0]; 0 without a cursor or when the value lies outside [0, S*K).  The eligible slots are ranked in
 *     the cyclic order c0, c0+1, ..., S*K-1, 0, ..., c0-1; the first served = min(E, N) of them become the rows
 *     0 .. served-1, in that order.
 *  3. A served row r of slot g: slot_c[r] = g; m_c[r], boxes_c[r], best_q_c[r] and reset_c[r] are bit copies of the
 *     entries at g; frame_idx_c[r] = frame_idx_stream[i] (0 without it).  reset_dev[g] is then set to 0: the pending reset
 *     MOVES into the snapshot, as in flm_track_gather_streams.
 *  4. A row r >= served is inert exactly as rule 2 there: slot_c = -1, m_c = the identity, boxes_c = (0,0,0,0),
 *     frame_idx_c = 0, dt_c = 0.0, best_q_c = -1.0, reset_c = 0; nothing global is read or written for it.
 *  5. Time, only with age_dev.  d = dt_stream_dev ? dt_stream_dev[i] : dt; d is GOOD when it is > 0 and finite.
 *       served slot:                 dt_c[r] = good ? d + age[g] : d   (one IEEE add);  then age[g] = 0.0
 *       eligible, not served:        age[g] = good ? age[g] + d : NaN  (the quiet NaN 0x7ff8000000000000)
 *       on, not eligible:            age[g] = 0.0
 *       slot of a stream that is off: neither read nor written -- boxes_dev included
 *     A NaN age reaches dt_c when the slot is served later, and rule 2 of flm_track_step_rows then restarts that slot's
 *     filter history: a wait of unknown length is no history.
 *  6. counts = (E, served, E - served, cursor_out); cursor_out = (the last served slot + 1) mod S*K when E > N, otherwise
 *     c0; cursor_dev[0] = cursor_out.  Over consecutive calls on an unchanged set of E > N eligible slots
 *     every one of them is served within ceil(E/N) calls.
 *  7. A slot that is not served keeps every bit of m_crop, boxes, best_q and reset.  No two arguments may overlap.  One
 *     launch, no workspace, no allocation, no synchronisation.
 * Errors, all found before anything is launched: a null m_crop_dev, boxes_dev, slot_c, m_c, boxes_c, frame_idx_c or
 * counts_dev, an optional output without its input or the reverse, dt_stream_dev without age_dev, or, with age_dev and
 * without dt_stream_dev, a dt that is not > 0 and finite -> FLM_ERR_ARG.  FLM_ERR_SHAPE, the limit named in
 * flm_last_error(), unless 1 <= n <= 65535, 1 <= s, 1 <= k, s*k <= 65535 and fh, fw >= 1. */
int flm_track_gather_live(flm_stream_t stream, const int32_t* stream_on_dev /*[S] or NULL*/, int s, int k /*slots PER STREAM*/,
                          int fh, int fw, int n /*the budget*/, const int32_t* frame_idx_stream_dev /*[S] or NULL*/,
                          const double* dt_stream_dev /*[S] or NULL*/, double dt, const float* m_crop_dev /*[S*K,2,3]*/,
                          const int32_t* boxes_dev /*[S*K,4]*/, const double* best_q_dev /*[S*K] or NULL*/,
                          int32_t* reset_dev /*[S*K] or NULL, in/out*/, double* age_dev /*[S*K] or NULL, in/out*/,
                          int32_t* cursor_dev /*[1] or NULL, in/out*/, int32_t* slot_c /*[N]*/, float* m_c /*[N,2,3]*/,
                          int32_t* boxes_c /*[N,4]*/, int32_t* frame_idx_c /*[N]*/, double* dt_c /*[N] or NULL*/,
                          double* best_q_c /*[N] or NULL*/, int32_t* reset_c /*[N] or NULL*/, int32_t* counts_dev /*[4]*/);

/* flm_track_step_rows: flm_track_step / flm_track_step_filtered on rows, in ONE launch (a workgroup of one wave per row;
 * the kernel runs the body of the two calls above, so the arithmetic is stated once).
 * The arguments are those of flm_track_step_filtered with k replaced by n, plus slot_dev int32 [N], n_slots, dt_dev
 * float64 [N] or NULL (NULL: the scalar dt for every row, checked on the host as there) and status_rows_dev int32 [N].
 * filt may be NULL: then state_dev, lm_raw_dev and dt_dev are NULL, dt is not read, and the step is flm_track_step's.
 * Where each argument lives:
 *   compact, read at row r:      lm_dev, w_dev, m_crop_c_dev [N,2,3], boxes_c_dev [N,4]
 *   compact, written at row r:   lm_frame_dev [N,C,2], m_align_dev [N,2,3], lm_raw_dev [N,C,2], status_rows_dev [N]
 *   global, written at slot g:   m_next_dev [n_slots,2,3], boxes_next_dev [n_slots,4], status_dev [n_slots]
 *   global, read and written at slot g:  state_dev [n_slots,C,6]
 * Contract:
 *  1. VALID row: every value written is, bit for bit, what flm_track_step_filtered (flm_track_step without filt) writes
 *     for ONE face with the inputs of row r, the state rows of slot g and dt = dt_dev ? dt_dev[r] : dt.
 *     status_rows[r] and status[g] both receive the status.
 *  2. The one new rule: a row whose dt_dev[r] is not > 0 and finite treats every point as having NO HISTORY -- a raw point
 *     that is ok gives out = raw and state = (x, y, 0, 0, x, y), a rejected one (-1,-1) and (-1,-1,0,0,-1,-1) as there.
 *     Nothing else of the row changes.
 *  3. INERT row: lm_frame and lm_raw are (-1,-1) everywhere, m_align is the identity, status_rows = FLM_TRACK_DEAD;
 *     nothing global is read or written.
 *  4. A slot no row names keeps every bit of m_next, boxes_next, status and state.
 *  5. With slot[r] = r, n = n_slots and dt_dev NULL every output is flm_track_step_filtered's (flm_track_step's), bit for
 *     bit, and status_rows equals status.
 *  6. m_next_dev and boxes_next_dev may be the tensors the snapshot m_crop_c_dev / boxes_c_dev was gathered FROM (that is
 *     what the snapshot is for); no other overlap of two arguments is allowed, and the call refuses m_crop_c_dev inside
 *     m_next_dev, boxes_c_dev inside boxes_next_dev and status_rows_dev inside status_dev.
 *  7. One launch, no workspace, no allocation, no synchronisation.
 * Errors, all found before anything is launched: those of flm_track_step_filtered (of flm_track_step without filt; the
 * dt test only without dt_dev); a null slot_dev or status_rows_dev, state_dev, lm_raw_dev or dt_dev without filt, or one
 * of the overlaps of 6 -> FLM_ERR_ARG; FLM_ERR_SHAPE unless 1 <= n <= 65535 and 1 <= n_slots <= 65535. */
int flm_track_step_rows(flm_stream_t stream, const double* lm_dev, size_t lm_stride, const double* w_dev, size_t w_stride,
                        const float* m_crop_c_dev /*[N,2,3]*/, const int32_t* boxes_c_dev /*[N,4]*/, int n, int c,
                        double sx, double sy, int in_h, int in_w, int fh, int fw, const double* tmpl_crop_dev /*[C,2]*/,
                        const double* tmpl_align_dev /*[C,2] or NULL*/, const flm_track_opts* opts,
                        double* lm_frame_dev /*[N,C,2]*/, float* m_align_dev /*[N,2,3] or NULL*/,
                        float* m_next_dev /*[n_slots,2,3]*/, int32_t* boxes_next_dev /*[n_slots,4]*/,
                        int32_t* status_dev /*[n_slots]*/, const flm_track_filter* filt /*or NULL*/, double dt,
                        double* state_dev /*[n_slots,C,6] or NULL*/, double* lm_raw_dev /*[N,C,2] or NULL*/,
                        const int32_t* slot_dev /*[N]*/, int n_slots, const double* dt_dev /*[N] or NULL*/,
                        int32_t* status_rows_dev /*[N]*/);

/* ---- association: detector boxes against live tracks --------------------------------------------------------------
 * flm_track_associate: what a tracker does at the moment a detector has run again -- pair its boxes with the live
 * slots, end the slots that sit on the same face as a lower one, end the slots no detection has confirmed for a while,
 * and start a track in a free slot for every detection nobody claimed -- in ONE launch of one workgroup, on boxes that
 * never leave the device.  It edits the state flm_track_step carries from frame to frame (m_crop, boxes, status, and
 * the filter state of flm_track_step_filtered) plus a miss counter per slot, between any two steps.
 * Integers only, except the two places marked (F): int32 coordinates, int64 areas and products.
 * In:  det_dev int32 [D,4] x0,y0,x1,y1; n_det_dev NULL or one int32 on the device (a detector with a fixed output
 *      buffer says here how many rows it filled); opts (NULL = the defaults).
 * In/out: m_crop_dev [K,2,3], boxes_dev [K,4], status_dev [K], misses_dev int32 [K], state_dev NULL or float64 [K,C,6].
 * Out: det_slot_dev int32 [D], slot_det_dev int32 [K], counts_dev int32 [8].  No two arguments may overlap.
 * Contract, in this order:
 *  1. nd = n_det_dev ? min(max(*n_det_dev, 0), d) : d.  Rows j >= nd are never read; their det_slot is -1.
 *  2. Detection j < nd is VOID when a coordinate lies outside [-2^28, 2^28].  Otherwise, with opts->square, it passes
 *     through the box maths of the reference's detect_marks (what the host does before flm_track_seed):
 *       off = (int)fabs((double)(y1-y0) * 0.1)                                                              (F)
 *       y0 += off;  y1 += off;  diff = (y1-y0) - (x1-x0);  delta = |diff| >> 1;  odd = |diff| & 1
 *       diff > 0:  x0 -= delta;  x1 += delta + odd          diff < 0:  y0 -= delta;  y1 += delta + odd
 *     (every intermediate stays inside int32).  A detection whose box is then empty after the clip of the tracking
 *     section is void too.  A void detection takes no part below; its det_slot is -1.
 *  3. All boxes are clipped first.  area(a) = (int64)(cx1-cx0)*(cy1-cy0); inter(a,b) = the area of the intersection of
 *     the clipped boxes (0 when they do not overlap); uni = area(a) + area(b) - inter.
 *       "IoU(a,b) >= t"  means  inter > 0 && (double)inter >= t * (double)uni                               (F)
 *     -- one float64 multiplication.  ORDER: pair p = (slot, detection) comes before pair q when
 *     inter_p*uni_q > inter_q*uni_p, exact in int64 (fh*fw <= 2^30 keeps every product below 2^61); on equality the
 *     lower slot comes first, then the lower detection.
 *  4. A slot is LIVE when its clipped box is not empty (the test of flm_track_step), whatever its status says.
 *  5. A live slot t is a DUPLICATE when any live slot s < t has IoU(s,t) >= dup_iou; s counts whether or not it is a
 *     duplicate itself (no serial dependence).  A duplicate is killed: boxes = (0,0,0,0), m_crop = the identity,
 *     status |= FLM_TRACK_DUPLICATE, misses = 0, slot_det = -1.
 *  6. MATCHING, among the live slots that survived 5 and the detections that are not void: over the pairs with
 *     IoU >= match_iou, in the ORDER of 3, take the first pair, remove its slot and its detection, repeat until no pair
 *     is left (greedy assignment).
 *  7. A matched slot t with detection j: slot_det[t] = j, det_slot[j] = t, misses = 0.  If refresh_iou > 0 and NOT
 *     IoU(t,j) >= refresh_iou the track RESTARTS from the detection: m_crop[t] and status[t] are what flm_track_seed
 *     writes for the detection's box of 2 (not clipped), boxes[t] is that box, and the slot's C*6 doubles of state_dev
 *     become -1.0.  Otherwise m_crop, boxes, status and state of the slot are untouched.
 *  8. A surviving live slot without a detection: slot_det = -1, misses = (int32)((uint32)misses + 1).  If max_misses > 0
 *     and misses >= max_misses it is killed as in 5 with FLM_TRACK_UNCONFIRMED, and misses = 0.
 *  9. BIRTHS: the detections that are neither void nor matched, in ascending index, pair off one to one with the slots
 *     that were not live at entry, in ascending index (a slot killed in this call is not reused in it: its status stays
 *     readable).  A born slot t with detection j gets m_crop, boxes and status exactly as in the restart of 7
 *     (status = 0), misses = 0, its state rows -1.0, slot_det[t] = j and det_slot[j] = t.  A detection left without a
 *     slot gets det_slot = -2.
 * 10. Everything else is untouched: a slot that was not live at entry and is not born keeps m_crop, boxes, status and
 *     misses (its slot_det is -1), and the state rows of every slot neither born nor restarted keep their bits.
 *     counts = { matched (restarted ones included), born, restarted, duplicates, unconfirmed, dropped (det_slot -2),
 *     void (among the rows j < nd), 0 }.
 * Defaults (flm_track_assoc_opts_init): max_misses = 0 (never), square = 1, match_iou = 0.3 (the customary gate of box
 * trackers), dup_iou = 0.7, refresh_iou = 0 (never).  None of them has been tuned against a trained model: a track's
 * box is the bounding box of a rotated, template-scaled crop square (twice the square's area at 45 degrees of roll),
 * a detection's box is the detector's square, and how the two overlap for one face has not been measured.
 * dup_iou > 1 switches 5 off (inter <= uni).
 * The call allocates nothing, synchronises nothing and makes one launch whatever the data; the matching inside it takes
 * as many rounds as the data needs (at most min(k, d); DESIGN 4.5f has the time of the worst case).
 * Errors, all found before anything is launched: a null pointer other than n_det_dev, state_dev and opts, a
 * struct_size smaller than this library's or a non-zero reserved -> FLM_ERR_ARG.  FLM_ERR_SHAPE, the limit named in
 * flm_last_error(), unless 1 <= k <= 1024, 1 <= d <= 1024, 1 <= c <= 1024 (read only when state_dev is given),
 * in_h, in_w, fh, fw >= 1, (int64)fh*fw <= 2^30, max_misses >= 0 and none of the three thresholds is NaN. */
typedef struct flm_track_assoc_opts {
  uint32_t struct_size;      /* as flm_track_opts */
  int32_t max_misses;        /* 0 = never give a track up for want of a detection */
  int32_t square;            /* 1: detections pass through the reference's box maths first; 0: used as given */
  int32_t reserved;          /* 0 */
  double match_iou;          /* a detection and a track may pair when IoU >= match_iou */
  double dup_iou;            /* two live tracks with IoU >= dup_iou are one face; > 1 = off */
  double refresh_iou;        /* a matched pair with IoU below it: the track restarts from the detection; 0 = never */
} flm_track_assoc_opts;
void flm_track_assoc_opts_init(flm_track_assoc_opts* opts);
int flm_track_associate(flm_stream_t stream, const int32_t* det_dev /*[D,4]*/, const int32_t* n_det_dev /*NULL or [1]*/,
                        int d, int k, int c, int in_h, int in_w, int fh, int fw,
                        const flm_track_assoc_opts* opts /*NULL = defaults*/, float* m_crop_dev /*[K,2,3] in/out*/,
                        int32_t* boxes_dev /*[K,4] in/out*/, int32_t* status_dev /*[K] in/out*/,
                        int32_t* misses_dev /*[K] in/out*/, double* state_dev /*NULL or [K,C,6] in/out*/,
                        int32_t* det_slot_dev /*[D] out*/, int32_t* slot_det_dev /*[K] out*/,
                        int32_t* counts_dev /*[8] out*/);

/* flm_track_associate_streams: the association above for S streams (cameras) that share one tracker of S*K slots, in
 * ONE launch of S workgroups -- one per stream, on LDS sized to max(k, d) (64, 256 or 1024 items), so that many
 * streams of a camera-sized tracker share a CU.  opts and every size but s are common to all streams.
 * In:  det_dev int32 [S,D,4]; n_det_dev NULL or int32 [S] on the device; opts (NULL = the defaults).
 * In/out: m_crop_dev [S*K,2,3], boxes_dev [S*K,4], status_dev [S*K], misses_dev int32 [S*K], state_dev NULL or float64
 *      [S*K,C,6].
 * Out: det_slot_dev int32 [S,D], slot_det_dev int32 [S*K], counts_dev int32 [S,8].  No two arguments may overlap.
 * Contract:
 *  1. Stream i owns the slots [i*K, (i+1)*K) of the five state tensors and of slot_det, and the rows det[i], n_det[i],
 *     det_slot[i] and counts[i].  k is the number of slots PER STREAM.
 *  2. For every stream that is not skipped (4) the call writes on the stream's blocks what
 *       flm_track_associate(det[i], n_det ? &n_det[i] : NULL, d, k, ...)
 *     writes on those slices, bit for bit, with one difference (3).
 *  3. det_slot[i][j], where it names a slot, holds the GLOBAL slot i*K + t, the index into the [S*K] tensors; -1 (void
 *     or unread) and -2 (no free slot) keep their meaning.  slot_det[i*K + t] stays the row j inside det[i].
 *  4. n_det[i] < 0: stream i is SKIPPED -- its detector did not run this time.  Nothing of its state is read or
 *     written: m_crop, boxes, status, misses and state keep their bits.
 *  5. A skipped stream's outputs: det_slot[i][:] = -1, slot_det[i*K ..] = -1, counts[i][:] = 0.
 *  6. With n_det_dev NULL no stream is skipped.  n_det[i] == 0 means "ran and found nothing": item 1 of
 *     flm_track_associate gives nd = 0, every surviving live slot counts a miss (item 8 there).
 *  7. No pair of two different streams is ever evaluated: a face at the same pixels of two cameras is two faces, and a
 *     detection of one stream neither confirms nor restarts nor starts a track of another.
 *  8. Every stream's result is the same whichever LDS size the launcher picks (integers and fixed float64 products
 *     only), and does not depend on the other streams.
 *  9. One launch whatever the data, no workspace, no allocation, no synchronisation.
 * 10. Errors, all found before anything is launched: the null, struct_size and reserved checks of flm_track_associate
 *     -> FLM_ERR_ARG.  FLM_ERR_SHAPE, the limit named in flm_last_error(), unless 1 <= s, s*k <= 65535 (the capacity
 *     cap of the warps and the tracker), 1 <= k <= 1024, 1 <= d <= 1024, and the c, size, 2^30, max_misses and NaN
 *     rules of flm_track_associate hold. */
int flm_track_associate_streams(flm_stream_t stream, const int32_t* det_dev /*[S,D,4]*/,
                                const int32_t* n_det_dev /*NULL or [S]*/, int s, int d, int k /*slots PER STREAM*/, int c,
                                int in_h, int in_w, int fh, int fw, const flm_track_assoc_opts* opts /*NULL = defaults*/,
                                float* m_crop_dev /*[S*K,2,3]*/, int32_t* boxes_dev /*[S*K,4]*/,
                                int32_t* status_dev /*[S*K]*/, int32_t* misses_dev /*[S*K]*/,
                                double* state_dev /*NULL or [S*K,C,6]*/, int32_t* det_slot_dev /*[S,D] out*/,
                                int32_t* slot_det_dev /*[S*K] out*/, int32_t* counts_dev /*[S,8] out*/);

/* ---- the best shot of a track: face quality and gallery ---------------------------------------------------------------
 * A matcher embeds a track's best face, not every face.  The two calls below judge the aligned faces where the warp
 * left them and keep, per slot, the best one seen so far -- three launches per step, no workspace, no allocation, no
 * synchronisation.  Every reduction is an exact integer sum, so the results do not depend on how they are scheduled.
 *
 * flm_face_quality: rec_dev int64 [K,8] from K faces of h x w as flm_warp_affine_fmt / flm_warp_affine_frames_fmt store
 * them under `fmt` (NULL = what flm_image_format_init gives: NHWC float32 BGR, scale 1, bias 0).  On the host, once:
 *   inv[c] = 1.0f / fmt->scale[c]                              float32 division
 * For stored element x of output channel c of a pixel (the element index is that of the warps' contract):
 *   xf = (float)x                                              exact for uint8, binary16 and bfloat16
 *   t  = xf - bias[c]                                          float32, rounded
 *   v  = t * inv[c]                                            float32, rounded: two operations, never fused
 *   p  = (int32)min(max(rintf(v * 16.0f), 0), 4080)            ties to even; a NaN gives 0; +-inf clamp
 *        -- the source pixel value in sixteenths of an 8-bit level
 * The source channel of output channel c is s = reverse_channels ? 2-c : c, and B, G, R are s = 0, 1, 2.  Per pixel
 *   Y = (1868*B + 9617*G + 4899*R + 8192) >> 14                BT.601 weights x 2^14 (sum 16384); 0 <= Y <= 4080
 * and for the interior pixels (1 <= row <= h-2 and 1 <= col <= w-2)
 *   L = Y(row-1,col) + Y(row+1,col) + Y(row,col-1) + Y(row,col+1) - 4*Y(row,col)
 * The record of a face, every entry an exact int64 sum (the largest stays below 2^56):
 *   { n_pix = h*w, sum Y, sum Y*Y, n_lap = max(h-2,0)*max(w-2,0), sum L, sum L*L, #(Y < 16*dark), #(Y > 16*bright) }
 * opts (NULL = the defaults of flm_quality_opts_init: dark = 16, bright = 239): the 8-bit levels below and above which
 * a pixel counts as under- and over-exposed.
 * faces_dev needs the alignment of its element and no more: it may be a slice of a larger buffer.  The kernel uses
 * 16-byte loads where the actual address of a run of elements allows them and element loads elsewhere; no byte
 * outside the K faces is read.  Two launches (the records' constants and zeros, then the sums).
 * Errors, all found before anything is launched: a null faces_dev or rec_dev, a format flm_warp_affine_fmt rejects, a
 * faces_dev that is not aligned to its element, a scale[c] of 0, a struct_size smaller than this library's, or dark or
 * bright outside [0, 255] -> FLM_ERR_ARG.  FLM_ERR_SHAPE, the limit named in flm_last_error(), unless
 * 1 <= k <= 65535, h, w >= 1 and h*w*3*4 < 2^31 (the warp's limit). */
#define FLM_QUALITY_REC 8
typedef struct flm_quality_opts {
  uint32_t struct_size;  /* as flm_track_opts */
  int32_t dark, bright;  /* 8-bit levels: Y < 16*dark is under-exposed, Y > 16*bright over-exposed */
} flm_quality_opts;
void flm_quality_opts_init(flm_quality_opts* opts);
int flm_face_quality(flm_stream_t stream, const void* faces_dev, int k, int h, int w,
                     const flm_image_format* fmt /*NULL = NHWC f32 BGR*/, const flm_quality_opts* opts /*NULL = defaults*/,
                     int64_t* rec_dev /*[K,8]*/);

/* flm_track_best_update: per slot, "keep this face if it beats what the slot holds", in ONE launch.
 * In:  faces_dev, K faces of face_bytes bytes each (any format: they are copied as bytes); rec_dev int64 [K,8], their
 *      records; status_dev int32 [K] or NULL; reset_dev int32 [K] or NULL (non-zero: the slot forgets its best first);
 *      lm_dev, lm_stride, w_dev, w_stride, c: the landmarks and their weights as flm_track_step reads them (point i of
 *      slot f at lm_dev[(f*c+i)*lm_stride + {0,1}], its weight at w_dev[(f*c+i)*w_stride]; w_dev may be NULL);
 *      factor_dev float64 [K] or NULL: a term of the caller's own (head pose, say); m_dev float32 [K,2,3] or NULL;
 *      frame_id; best_q_in float64 [K].
 * Per slot, in float64, one IEEE operation per written operator, in the written order, no contraction; max and min
 * are fmax and fmin; (double) of an int64 rounds to nearest:
 *   mu    = (double)S_L / (double)n_lap
 *   var   = (double)S_LL / (double)n_lap - mu*mu
 *   sharp = max(var / 256.0, 0.0)        the variance of the Laplacian in 8-bit levels squared: the customary focus measure
 *   s     = min(sharp / sharp_ref, 1.0)
 *   e     = (double)(n_pix - n_dark - n_bright) / (double)n_pix
 *   wbar  = the mean of w over the landmarks whose (x, y) is not (-1,-1), summed in ascending landmark index from 0.0,
 *           then divided by their number; 1.0 when w_dev is NULL; 0.0 when w_dev is given and no landmark took part
 *   f     = factor_dev ? factor_dev[slot] : 1.0
 *   q     = ((s * e) * wbar) * f
 * The slot is ELIGIBLE when status_dev is NULL or status == 0, n_lap > 0, e >= min_exposed, q is not NaN and q >= 0.
 * prev = (reset_dev && reset_dev[slot] != 0) ? -1.0 : best_q_in[slot]; -1.0 means "holds no best".
 * The slot is TAKEN when it is eligible and q > prev (strict: on a tie the earlier frame stays).  Then
 *   gallery_dev[slot*face_bytes ..] = the face's face_bytes bytes, best_q_out = q, best_frame_dev = frame_id, and, each
 *   where its pointer is given, best_m_dev = the slot's six floats of m_dev, best_lm_dev = the slot's C*2 doubles of
 *   lm_dev, best_rec_dev = the slot's record.
 * Otherwise best_q_out = prev and nothing else of the slot is written: its gallery bytes keep their bits.
 * best_q_in and best_q_out must not overlap (the launch is race-free because every workgroup of a slot derives the same
 * decision from inputs nobody writes); no output may overlap an input.  The grid is (chunk, slot); the workgroups of a
 * slot that is not taken return at once; the copy uses 16-byte accesses where both addresses allow them.
 * Defaults (flm_best_opts_init): sharp_ref = 100, the customary blur threshold of this measure (a face at or above it
 * counts as fully sharp), and min_exposed = 0.5, a guess.  Neither has been tuned against real footage.
 * Errors, all found before anything is launched: a null faces_dev, rec_dev, lm_dev, best_q_in, best_q_out, gallery_dev
 * or best_frame_dev, a best_m_dev without m_dev, a struct_size smaller than this library's, a non-zero reserved, a
 * sharp_ref that is not > 0, a NaN min_exposed, best_q_in overlapping best_q_out, or faces_dev overlapping gallery_dev
 * -> FLM_ERR_ARG.  FLM_ERR_SHAPE, the limit named in flm_last_error(), unless 1 <= k <= 65535, c >= 1, face_bytes >= 1,
 * lm_stride >= 2 and (with w_dev) w_stride >= 1. */
typedef struct flm_best_opts {
  uint32_t struct_size;  /* as flm_track_opts */
  int32_t reserved;      /* 0 */
  double sharp_ref;      /* sharpness (8-bit levels squared) at and above which a face counts as fully sharp */
  double min_exposed;    /* the least share of pixels that are neither dark nor bright */
} flm_best_opts;
void flm_best_opts_init(flm_best_opts* opts);
int flm_track_best_update(flm_stream_t stream, const void* faces_dev, size_t face_bytes, int k,
                          const int64_t* rec_dev /*[K,8]*/, const int32_t* status_dev /*[K] or NULL*/,
                          const int32_t* reset_dev /*[K] or NULL*/, const double* lm_dev, size_t lm_stride,
                          const double* w_dev /*or NULL*/, size_t w_stride, int c,
                          const double* factor_dev /*[K] or NULL*/, const float* m_dev /*[K,2,3] or NULL*/,
                          int64_t frame_id, const flm_best_opts* opts /*NULL = defaults*/,
                          const double* best_q_in /*[K]*/, double* best_q_out /*[K]*/, void* gallery_dev /*[K,face_bytes]*/,
                          int64_t* best_frame_dev /*[K]*/, float* best_m_dev /*[K,2,3] or NULL*/,
                          double* best_lm_dev /*[K,C,2] or NULL*/, int64_t* best_rec_dev /*[K,8] or NULL*/);

/* flm_track_best_update_rows: flm_track_best_update on rows (see "rows" in the tracking section), in ONE launch.
 *   compact, read at row r:   faces_dev [N,face_bytes], rec_dev [N,8], status_rows_dev [N] or NULL, reset_c_dev [N] or
 *                             NULL, lm_dev, w_dev, factor_dev [N] or NULL, m_dev [N,2,3] or NULL, and best_q_c float64
 *                             [N]: the SNAPSHOT of the slots' best quality, the `prev` below, which nobody writes during
 *                             the launch (flm_track_gather_streams makes it)
 *   global, written at slot g = slot_dev[r]:  best_q_dev float64 [n_slots], gallery_dev [n_slots,face_bytes],
 *                             best_frame_dev [n_slots], best_m_dev, best_lm_dev, best_rec_dev (each or NULL)
 * Contract: q and ELIGIBLE are those of flm_track_best_update, word for word, computed from row r;
 * prev = (reset_c_dev && reset_c_dev[r] != 0) ? -1.0 : best_q_c[r]; TAKEN = eligible and q > prev.  For a valid row
 * best_q_dev[g] = taken ? q : prev, and when taken the face's bytes, frame_id and, each where its pointer is given, the
 * row's matrix, landmarks and record go to slot g.  An inert row, and a slot no row names, write nothing: gallery,
 * best_q and the rest keep their bits.
 * Reading prev from the snapshot is what keeps the launch race-free with best_q written IN PLACE: as in
 * flm_track_best_update, several workgroups of a row each derive the decision again, and they agree because they
 * derive it from inputs nobody writes -- there best_q_in, a second buffer; here best_q_c.  best_q_c must not overlap
 * best_q_dev; no output may overlap an input.
 * Errors, all found before anything is launched: those of flm_track_best_update with n for k and best_q_c, best_q_dev for
 * best_q_in, best_q_out; a null slot_dev -> FLM_ERR_ARG; FLM_ERR_SHAPE unless 1 <= n_slots <= 65535. */
int flm_track_best_update_rows(flm_stream_t stream, const void* faces_dev, size_t face_bytes, int n,
                               const int64_t* rec_dev /*[N,8]*/, const int32_t* status_rows_dev /*[N] or NULL*/,
                               const int32_t* reset_c_dev /*[N] or NULL*/, const double* lm_dev, size_t lm_stride,
                               const double* w_dev /*or NULL*/, size_t w_stride, int c,
                               const double* factor_dev /*[N] or NULL*/, const float* m_dev /*[N,2,3] or NULL*/,
                               int64_t frame_id, const flm_best_opts* opts /*NULL = defaults*/,
                               const int32_t* slot_dev /*[N]*/, int n_slots, const double* best_q_c /*[N]*/,
                               double* best_q_dev /*[n_slots]*/, void* gallery_dev /*[n_slots,face_bytes]*/,
                               int64_t* best_frame_dev /*[n_slots]*/, float* best_m_dev /*[n_slots,2,3] or NULL*/,
                               double* best_lm_dev /*[n_slots,C,2] or NULL*/, int64_t* best_rec_dev /*[n_slots,8] or NULL*/);

/* flm_track_retire: retires the tracks that have ended and gives identities to the ones that have begun -- the exit
 * queue of the best shots.  A slot is an index; this call says WHO a slot is (track_id) and THAT a track is over (one ring
 * row per finished track, holding its best face, delivered once).  At most two launches (the decision, one workgroup;
 * the copy of the faces), no atomics, no workspace, no allocation, no synchronisation; every launch shape is a host number.
 * Read:   boxes_dev int32 [K,4], status_dev int32 [K], fh, fw: the tracker's state; best_q_dev float64 [K], gallery_dev
 *         [K,face_bytes], best_frame_dev int64 [K]: the best shots as flm_track_best_update* keep them; best_m_dev float32
 *         [K,2,3], best_lm_dev float64 [K,C,2], best_rec_dev int64 [K,8]: each may be NULL, but only together with its ring
 *         counterpart x_m, x_lm, x_rec; frame_id; flush; opts (NULL = the defaults).
 * In/out: born_dev int32 [K]: non-zero means a track was started in the slot since the last call (the caller sets it
 *         where it starts a track; the call clears it); track_id_dev int64 [K]: -1 means the slot holds no track;
 *         born_frame_dev int64 [K]; head_dev int64 [4] = {seq, next_id, discarded, overrun}, all zero before the first call.
 * Out:    the exit ring of Q rows: x_gallery [Q,face_bytes], x_meta int64 [Q,FLM_EXIT_META], x_q float64 [Q], and x_m
 *         float32 [Q,2,3], x_lm float64 [Q,C,2], x_rec int64 [Q,8] (each may be NULL); exit_row_dev int32 [K].
 * No two arguments may overlap.
 * Contract, per slot t, in this order; everything is a function of the inputs at entry:
 *  1. live = the clipped boxes_dev[t] is not empty: the clip of this section, the negation of the DEAD test of
 *     flm_track_step, step 1, and the test of item 4 of flm_track_associate.  born = born_dev[t] != 0.
 *     held = track_id_dev[t] >= 0.
 *  2. The slot's track ENDS when held && (born || !live || flush != 0).
 *  3. An ending track is EMITTED when best_q_dev[t] >= min_q.  Otherwise it is DISCARDED: exit_row = -2, and it is counted
 *     in head[2].  The comparison is false for NaN, and false for the -1 of a slot without a best, since min_q >= 0.
 *  4. The E emitted tracks of the call are ranked by ascending slot: r = 0 .. E-1.  With seq0 = head[0] at entry, the
 *     track of rank r has sequence number seq0 + r and ring row (seq0 + r) % Q (the non-negative remainder).  It is
 *     WRITTEN when r >= E - Q, so that no two tracks of one call share a row; then exit_row = its row.  Otherwise it is
 *     OVERRUN: exit_row = -3, and it is counted in head[3].  head[0] += E: overrun tracks are included, so a consumer that
 *     keeps its own cursor sees what it missed.
 *  5. A written row receives the slot's face_bytes gallery bytes; x_q = best_q_dev[t]; each of the matrix, the landmarks and
 *     the record where its pointer is given; and
 *       x_meta = { track_id, t, born_frame[t], frame_id, best_frame[t], end, seq0 + r, 0 }
 *     end = status_dev[t] for a track that ended dead and was not born; -1 when the slot was restarted before its end was
 *     seen (born); -2 for a live, not born track ended by flush.
 *  6. Births: the slots with born && live are ranked by ascending slot, b = 0 .. B-1, and next_id = head[1] at entry.  For
 *     these track_id[t] = next_id + b and born_frame[t] = frame_id; head[1] += B.  A slot that ended and was not born so
 *     gets track_id = -1; so does a slot that was born with an empty box.  born_dev[t] = 0 for every slot.  A slot that
 *     neither ends nor is born keeps every bit and has exit_row = -1 (a born slot that held no track has exit_row = -1 too);
 *     born_frame is written for births alone.
 *  7. Ring rows that no track of this call was written to keep their bits.
 * gallery_dev and x_gallery need byte alignment only: the copy uses 16-byte accesses where both addresses allow them and
 * element accesses elsewhere, and no byte outside a row is read or written.
 * Defaults (flm_exit_opts_init): min_q = 0: every track that has a best shot is emitted.
 * Errors, all found before any launch: a null pointer other than the optional triples and opts, an optional source
 * without its ring buffer or the reverse, a struct_size smaller than this library's, a non-zero reserved, a min_q that is
 * negative or NaN, or two arguments that overlap -> FLM_ERR_ARG.  FLM_ERR_SHAPE, the limit named in flm_last_error(),
 * unless 1 <= k <= 65535, 1 <= q <= 65535, 1 <= c <= 1024, face_bytes >= 1 and fh, fw >= 1. */
#define FLM_EXIT_META 8
typedef struct flm_exit_opts {
  uint32_t struct_size;  /* as flm_track_opts */
  uint32_t reserved;     /* 0 */
  double min_q;          /* >= 0: an ending track whose best quality lies below it is discarded */
} flm_exit_opts;
void flm_exit_opts_init(flm_exit_opts* opts);   /* min_q = 0.0 */
int flm_track_retire(flm_stream_t stream, const int32_t* boxes_dev /*[K,4]*/, const int32_t* status_dev /*[K]*/, int k,
                     int fh, int fw, const double* best_q_dev /*[K]*/, const void* gallery_dev /*[K,face_bytes]*/,
                     size_t face_bytes, const int64_t* best_frame_dev /*[K]*/, const float* best_m_dev /*[K,2,3] or NULL*/,
                     const double* best_lm_dev /*[K,C,2] or NULL*/, int c, const int64_t* best_rec_dev /*[K,8] or NULL*/,
                     int64_t frame_id, int flush, const flm_exit_opts* opts /*NULL = defaults*/,
                     int32_t* born_dev /*[K] in/out*/, int64_t* track_id_dev /*[K] in/out*/,
                     int64_t* born_frame_dev /*[K] in/out*/, int64_t* head_dev /*[4] in/out*/, int q,
                     void* x_gallery /*[Q,face_bytes]*/, int64_t* x_meta /*[Q,8]*/, double* x_q /*[Q]*/,
                     float* x_m /*[Q,2,3] or NULL*/, double* x_lm /*[Q,C,2] or NULL*/, int64_t* x_rec /*[Q,8] or NULL*/,
                     int32_t* exit_row_dev /*[K]*/);

/* ---- head pose: where a face looks, from its landmarks ------------------------------------------------------------------
 * flm_head_pose: a scaled-orthographic pose (the linear step of POS: DeMenthon, Davis 1995) of every face from its 2-D
 * landmarks and a rigid 3-D model of P points, in ONE launch (a workgroup of one wave per row), no workspace, no
 * allocation, no atomics, no synchronisation.  It produces the `factor_dev` of flm_track_best_update.
 * Model frame: X to the image's right, Y down, Z away from the camera; a face looking straight into the camera has
 * R = identity.  Model point p names landmark idx_dev[p] and has the coordinates X[p] = xyz_dev[3p .. 3p+2] (any unit).
 * Landmarks and weights are read at element strides exactly as flm_similarity_from_landmarks_weighted reads them: point
 * i of row r is the two doubles at lm_dev + (r*c + i)*lm_stride, its weight the double at w_dev + (r*c + i)*w_stride;
 * w_dev == NULL: every weight is 1.  Model point p TAKES PART when 0 <= idx[p] < c, both coordinates of landmark idx[p]
 * are >= 0 and its weight is > 0 (a NaN weight fails that test); cnt is the number of participating points.
 * float64, one IEEE operation per written operator, in the written order, nothing fused; every sum runs sequentially from
 * 0.0 in ascending model index p over the participating points:
 *   W = sum w;  mX = sum(w*X)/W (three means);  mx = sum(w*x)/W;  my = sum(w*y)/W
 *   X' = X - mX;  x' = x - mx;  y' = y - my
 *   a00 = sum w*(X'0*X'0), likewise a01, a02, a11, a12, a22
 *   bxk = sum w*(X'k*x');  byk = sum w*(X'k*y')                                              k = 0, 1, 2
 *   c00 = a11*a22 - a12*a12;  c01 = a02*a12 - a01*a22;  c02 = a01*a12 - a02*a11
 *   c11 = a00*a22 - a02*a02;  c12 = a01*a02 - a00*a12;  c22 = a00*a11 - a01*a01             (c symmetric: ckl = clk)
 *   det = (a00*c00 + a01*c01) + a02*c02;   vol = det / ((a00*a11)*a22)
 *   Ik = ((ck0*bx0 + ck1*bx1) + ck2*bx2) / det;  Jk likewise from by
 *   nI = sqrt((I0*I0 + I1*I1) + I2*I2);  nJ likewise;  s = sqrt(nI*nJ)
 *   i = I/nI;  j = J/nJ;  e = i + j;  f = i - j;  ne = |e|, nf = |f| (as nI);  e = e/ne;  f = f/nf
 *   r1 = (e + f)*H;  r2 = (e - f)*H;  H = 0.7071067811865476
 *   r3 = (r1[1]*r2[2] - r1[2]*r2[1], r1[2]*r2[0] - r1[0]*r2[2], r1[0]*r2[1] - r1[1]*r2[0]);   R = rows r1, r2, r3
 *   ex = s*((r1[0]*X'0 + r1[1]*X'1) + r1[2]*X'2) - x';  ey likewise with r2 and y'
 *   rms = sqrt(sum w*(ex*ex + ey*ey) / W)
 *   yaw = atan2(-R[2][0], R[2][2]);  pitch = asin(min(max(R[2][1], -1), 1));  roll = atan2(-R[0][1], R[1][1])
 * i.e. R = Rz(roll) Rx(pitch) Ry(yaw), and x = s*(r1 . X') + mx, y = s*(r2 . X') + my is the model in the image.  |i| =
 * |j| = 1 makes e and f orthogonal, so the bisector step returns an orthonormal R in closed form: up to the three angles
 * (the platform's atan2 and asin) the record is made of + - * / sqrt alone and is the same on every conforming machine.
 * The fit is OK when cnt >= 4; W, det, nI, nJ, ne and nf are all finite and > 0; vol >= min_volume; and all of R, s and
 * rms are finite.  By Hadamard's inequality vol lies in [0, 1] and does not depend on the model's unit; it is 0 for
 * coplanar points.
 * The record, FLM_POSE_REC doubles per face:
 *   { R[0][0..2], R[1][0..2], R[2][0..2], s, mx, my, rms, (double)cnt, ok ? 1.0 : 0.0, yaw, pitch, roll }
 * A fit that is not ok gives the identity for R, s = 0, mx = my = -1, rms = 0, the true cnt, ok = 0 and three angles of 0.
 * Frontality is R[2][2], the cosine between the face's normal and the optical axis:
 *   factor_out[r] = (ok && R[2][2] >= min_frontal) ? R[2][2] : 0.0
 * Without slot_dev row r writes the record pose_dev[r].  With slot_dev int32 [N] the "rows" rules of the tracking section
 * hold: a valid row writes its record at slot g = slot_dev[r] of pose_dev [n_slots,18], an inert row writes no record, a
 * slot no row names keeps its bits.  factor_out is written by ROW in both cases -- where flm_track_best_update and
 * flm_track_best_update_rows read factor_dev --, 0.0 for an inert row.
 * Defaults (flm_pose_opts_init): min_volume = 1e-6 (the six points of a frontal face model give 0.9, their worst
 * non-planar four 6e-3, four coplanar ones 0 up to rounding), min_frontal = 0.
 * Errors, all found before anything is launched: a null lm_dev, idx_dev, xyz_dev or pose_dev (n_slots is not
 * read without slot_dev), a struct_size smaller than this library's, a non-zero reserved, a min_volume or min_frontal that is NaN or
 * negative, min_frontal > 1, or pose_dev or factor_out overlapping an input or each other -> FLM_ERR_ARG.  FLM_ERR_SHAPE,
 * the limit named in flm_last_error(), unless 1 <= n <= 65535, 1 <= c <= 1024, 4 <= p <= 256, lm_stride >= 2, w_stride >= 1
 * (with w_dev) and, with slot_dev, 1 <= n_slots <= 65535. */
#define FLM_POSE_REC 18
typedef struct flm_pose_opts {
  uint32_t struct_size;  /* as flm_track_opts */
  uint32_t reserved;     /* 0 */
  double min_volume;     /* the least vol at which the model's participating points count as non-planar */
  double min_frontal;    /* in [0, 1]: below this R[2][2] the factor is 0 */
} flm_pose_opts;
void flm_pose_opts_init(flm_pose_opts* opts);   /* min_volume = 1e-6, min_frontal = 0.0 */
int flm_head_pose(flm_stream_t stream, const double* lm_dev, size_t lm_stride, const double* w_dev /*or NULL*/,
                  size_t w_stride, int n, int c, const int32_t* idx_dev /*[P]*/, const double* xyz_dev /*[P,3]*/, int p,
                  const flm_pose_opts* opts /*NULL = defaults*/, const int32_t* slot_dev /*[N] or NULL*/, int n_slots,
                  double* pose_dev /*[N or n_slots,18]*/, double* factor_out /*[N] or NULL*/);

/* ---- pose-binned best shots: one best face per view of every track ------------------------------------------------------
 * A matcher that enrols from video wants the best frontal face of a track AND its best left and right (up and down) views,
 * so that a profile probe meets a profile template.  flm_track_views_update keeps, per slot, one best face per POSE BIN;
 * flm_track_exit_views moves the bins of a finished track into the exit ring beside the row flm_track_retire wrote.
 *
 * The bin of a face, from the slot's pose record as flm_head_pose wrote it, by comparisons of doubles alone (the
 * platform's atan2 and asin play no part, so the bin is the same on every machine):
 *   ok = pose[14] == 1.0
 *   u  = -pose[6]        -R[2][0] = cos(pitch)*sin(yaw): the sign of yaw.  u > 0: the face is turned to the image's LEFT
 *   v  =  pose[7]         R[2][1] = sin(pitch).                            v > 0: the face looks DOWN in the image
 *   iu = the number of edges e among u_edge[0 .. n_u) with u >= e;  iv likewise from v_edge[0 .. n_v)
 *   B  = (n_u + 1) * (n_v + 1)  (at most 64);   bin = iv * (n_u + 1) + iu
 * A face is NOT BINNED when !ok, or when u or v is NaN.  The edges are strictly ascending finite numbers in (-1, 1), at
 * most FLM_VIEWS_MAX_EDGES per axis; an edge sin(a) on u is the yaw a exactly at pitch 0.
 *
 * flm_track_views_update: at most two launches, no atomics, no workspace, no allocation, no synchronisation; every launch
 * shape is a host number.
 * In, read at row r as flm_track_best_update_rows reads them: faces_dev [N,face_bytes], rec_dev int64 [N,8],
 *   status_rows_dev int32 [N] or NULL, reset_dev int32 [N] or NULL, lm_dev, lm_stride, w_dev (or NULL), w_stride, c, m_dev
 *   float32 [N,2,3] or NULL, frame_id; slot_dev int32 [N] or NULL.  NULL: g = r and n_slots = n (the argument is not read).
 *   Otherwise the "rows" rules of the tracking section hold: a valid row writes at slot g = slot_dev[r], an inert row and a
 *   slot no row names write nothing.  pose_dev float64 [n_slots,18], read at slot g, where flm_head_pose wrote it.
 * In/out, indexed [g][b]: view_q float64 [n_slots,B] (-1: the bin holds nothing), view_frame int64 [n_slots,B],
 *   view_gallery [n_slots,B,face_bytes], and, each optional, view_m float32 [n_slots,B,2,3], view_lm float64
 *   [n_slots,B,C,2], view_pose float64 [n_slots,B,18].
 * Out: take_dev int32 [N].
 * Per valid row r, in float64, one IEEE operation per written operator, in the written order, nothing fused:
 *   if reset_dev && reset_dev[r] != 0: every view_q[g][*] = -1.0 first; nothing else of the slot is cleared.
 *   q = (s * e) * wbar, with s, e and wbar word for word those of flm_track_best_update.  There is NO caller factor: the
 *       bin is what accounts for pose, and a sharp profile must be able to win its own bin.
 *   ELIGIBLE: status_rows_dev is NULL or status == 0, n_lap > 0, e >= min_exposed, q is not NaN and q >= 0, and the face
 *       is binned.
 *   TAKEN: eligible and q > view_q[g][bin] (strict: on a tie the earlier frame stays).  Then view_q[g][bin] = q,
 *       view_frame[g][bin] = frame_id, the face's bytes go to view_gallery[g][bin], the row's matrix and landmarks and the
 *       slot's 18 pose doubles go where their pointers are given, and take_dev[r] = bin.
 *   Otherwise take_dev[r] = -1 and the bin keeps every bit.  An inert row has take_dev[r] = -1.
 * Launch 1, the decision, one thread per row: thread r is the only reader and writer of slot g's [B] entries -- which is
 * why view_q is updated IN PLACE, without the snapshot or second buffer of flm_track_best_update* -- and writes take,
 * view_frame, view_m, view_lm and view_pose.  Launch 2, the copy, grid (chunk, row): it reads take_dev and returns at
 * once for take < 0; 16-byte accesses where both addresses allow them and element accesses elsewhere; no byte outside
 * the bin's row is touched.  faces_dev and view_gallery need byte alignment only.
 * Defaults (flm_views_opts_init): sharp_ref = 100 and min_exposed = 0.5 as flm_best_opts; n_u = 2, u_edge = -+sin(20 deg)
 * (right, frontal, left); n_v = 0.
 * Errors, all found before any launch: a null faces_dev, rec_dev, lm_dev, pose_dev, view_q, view_frame, view_gallery or
 * take_dev; a view_m without m_dev; a struct_size smaller than this library's; a non-zero reserved; a sharp_ref that is
 * not > 0; a NaN min_exposed; n_u or n_v outside [0, 7]; edges that are not finite, not inside (-1, 1) or not strictly
 * ascending; an output overlapping an input or another output -> FLM_ERR_ARG.  FLM_ERR_SHAPE, the limit named in
 * flm_last_error(), unless 1 <= n <= 65535, (with slot_dev) 1 <= n_slots <= 65535, 1 <= c <= 1024, face_bytes >= 1,
 * lm_stride >= 2 and (with w_dev) w_stride >= 1. */
#define FLM_VIEWS_MAX_EDGES 7
typedef struct flm_views_opts {
  uint32_t struct_size;  /* as flm_track_opts */
  uint32_t reserved;     /* 0 */
  double sharp_ref;      /* as flm_best_opts */
  double min_exposed;    /* as flm_best_opts */
  int32_t n_u, n_v;      /* edges in use per axis, 0 .. FLM_VIEWS_MAX_EDGES */
  double u_edge[FLM_VIEWS_MAX_EDGES]; /* strictly ascending, in (-1, 1) */
  double v_edge[FLM_VIEWS_MAX_EDGES];
} flm_views_opts;
void flm_views_opts_init(flm_views_opts* opts);
int flm_track_views_update(flm_stream_t stream, const void* faces_dev, size_t face_bytes, int n,
                           const int64_t* rec_dev /*[N,8]*/, const int32_t* status_rows_dev /*[N] or NULL*/,
                           const int32_t* reset_dev /*[N] or NULL*/, const double* lm_dev, size_t lm_stride,
                           const double* w_dev /*or NULL*/, size_t w_stride, int c, const float* m_dev /*[N,2,3] or NULL*/,
                           int64_t frame_id, const flm_views_opts* opts /*NULL = defaults*/,
                           const int32_t* slot_dev /*[N] or NULL*/, int n_slots, const double* pose_dev /*[n_slots,18]*/,
                           double* view_q /*[n_slots,B]*/, int64_t* view_frame /*[n_slots,B]*/,
                           void* view_gallery /*[n_slots,B,face_bytes]*/, float* view_m /*[n_slots,B,2,3] or NULL*/,
                           double* view_lm /*[n_slots,B,C,2] or NULL*/, double* view_pose /*[n_slots,B,18] or NULL*/,
                           int32_t* take_dev /*[N]*/);

/* flm_track_exit_views: the views of the tracks flm_track_retire has just written, into the exit ring, in ONE launch.
 * Called directly after flm_track_retire, it reads that call's exit_row_dev int32 [K].  For every slot t with
 * 0 <= exit_row[t] < Q, ring row exit_row[t] receives all `bins` values of view_q[t] and view_frame[t], and for each bin
 * with view_q[t][b] >= 0 also the bin's face bytes and, where given, its matrix, landmarks and pose.  A bin with
 * view_q < 0 (or NaN) leaves its ring bytes as they were: the consumer reads x_view_q.  Slots with a negative exit_row
 * (nothing ended, discarded, overrun) write nothing, and ring rows no slot was written to keep every bit.
 * flm_track_retire guarantees that the rows written in one call are distinct.  The ring: x_view_q float64 [Q,bins],
 * x_view_frame int64 [Q,bins], x_view_gallery [Q,bins,face_bytes], and x_view_m, x_view_lm, x_view_pose, each given
 * together with its source and only so.  The grid is (chunk x bin, slot); the copy is that of flm_track_retire.
 * Errors, found before the launch: a null exit_row_dev, view_q, view_frame, view_gallery, x_view_q, x_view_frame or
 * x_view_gallery, an optional source without its ring buffer or the reverse, or two arguments that overlap ->
 * FLM_ERR_ARG.  FLM_ERR_SHAPE, the limit named in flm_last_error(), unless 1 <= k <= 65535, 1 <= q <= 65535,
 * 1 <= bins <= 64, 1 <= c <= 1024 and face_bytes >= 1. */
int flm_track_exit_views(flm_stream_t stream, const int32_t* exit_row_dev /*[K]*/, int k, int q, int bins,
                         size_t face_bytes, int c, const double* view_q /*[K,bins]*/,
                         const int64_t* view_frame /*[K,bins]*/, const void* view_gallery /*[K,bins,face_bytes]*/,
                         const float* view_m /*[K,bins,2,3] or NULL*/, const double* view_lm /*[K,bins,C,2] or NULL*/,
                         const double* view_pose /*[K,bins,18] or NULL*/, double* x_view_q /*[Q,bins]*/,
                         int64_t* x_view_frame /*[Q,bins]*/, void* x_view_gallery /*[Q,bins,face_bytes]*/,
                         float* x_view_m /*[Q,bins,2,3] or NULL*/, double* x_view_lm /*[Q,bins,C,2] or NULL*/,
                         double* x_view_pose /*[Q,bins,18] or NULL*/);

/* ---- frame annotation: marks, boxes and mosaics written into the ring ---------------------------------------------------
 * The reference's frame loop (prediction.py:99-113) ends every frame with draw_marks(img, marks) (utils/plots.py) on a
 * host frame.  flm_frames_annotate writes the same marks -- and an outline and a mosaic of every face -- into the ring
 * slots themselves, BGR24 or NV12, from the landmarks in frame pixels that flm_track_step (or flm_landmarks_to_frame)
 * left on the device: at most four launches, no atomics, no download, no synchronisation, no allocation, no workspace.
 * It is the one call of this library that WRITES a frame: the slot is changed for every later reader.
 *
 *  1. Accepted landmark.  A landmark (x, y) is accepted when x >= 0 && y >= 0 && x <= 2^30 && y <= 2^30.  The rejected
 *     point (-1,-1) of flm_landmarks_from_crop fails this test, and so do NaN and +-inf.  Point i of face f is the two
 *     doubles at lm_dev + (f*c + i)*lm_stride, as flm_track_step reads it; lm_stride is 2 or FLM_LANDMARK_REC.
 *  2. Region of a face, float64, one IEEE operation per written operator, nothing fused:
 *       mnx, mny, mxx, mxy = min and max over the accepted points;  side = max(mxx - mnx, mxy - mny)
 *       R = (floor(mnx - margin[0]*side), floor(mny - margin[1]*side),
 *            ceil(mxx + margin[2]*side) + 1, ceil(mxy + margin[3]*side) + 1)
 *     each value clamped to +-2^30 and cast to int32, the form of boxes_next in flm_track_step.  A face without an
 *     accepted point has R = (0,0,0,0).  regions_dev receives R of every face, whatever its frame index.
 *     P = R intersected with [0,fw) x [0,fh).  A face TAKES PART when P is not empty and its frame index
 *     (frame_idx_dev[f], or 0 for a NULL frame_idx_dev) lies in [0, nframes).
 *  3. Layer 1, the mosaic (redact = s).  Cells lie on a grid anchored at the frame's origin: cell (cx,cy) covers
 *     [cx*s, min((cx+1)*s, fw)) x [cy*s, min((cy+1)*s, fh)).  A cell is mosaicked when it intersects P of at least one
 *     face of that frame that takes part.  Every such cell is replaced ONCE, by (sum + (n>>1)) / n of its ORIGINAL bytes,
 *     n its pixel count.  BGR24: per channel.  NV12: the luma bytes of the cell as above; the U bytes and the V bytes of
 *     the m = n/4 chroma samples under it each by (sum + (m>>1)) / m (sizes and s are even: a cell never splits a sample).
 *  4. Layer 2, the outline (box = t): the pixels (x,y) of P with x < R.x0+t || x >= R.x1-t || y < R.y0+t || y >= R.y1-t,
 *     in box_bgr.  R is the unclipped region: a face cut by the frame's border shows no edge along that border.
 *  5. Layer 3, the marks: for every accepted landmark of a face that takes part, the pixels ((int)x + dx, (int)y + dy)
 *     with dx*dx + dy*dy <= 5 -- rows of 3, 5, 5, 5, 3 pixels, what utils/plots.draw_marks paints -- clipped to the
 *     frame, in mark_bgr.
 *  6. Order: all mosaics, then all outlines, then all marks, over all faces.  A layer has one colour per call, so a
 *     pixel's final value does not depend on the order of the faces: the call is deterministic without atomics.
 *  7. Painting NV12.  The colour's (Y,U,V) is computed once, on the host, by flm_bgr_to_yuv with the format's matrix.  A
 *     painted pixel gets the luma byte Y, and the U,V pair of its 2x2 block gets U,V; a later layer that paints any pixel
 *     of the block overwrites the pair.
 *  8. flm_bgr_to_yuv (host only, no GPU), int32 throughout, >> an arithmetic shift:
 *       Y = clamp(16  + ((cB*B + cG*G + cR*R + 2^15) >> 16), 16, 235);  U, V likewise with 128, clamped to [16, 240]
 *     coefficients round(exact x 2^16) of the limited-range forward matrix with the format's Kr and Kb, over (B,G,R):
 *       FLM_YUV_BT601_LIMITED  Y (6416, 33039, 16829)  U (28784, -19071, -9714)  V (-4681, -24103, 28784)
 *       FLM_YUV_BT709_LIMITED  Y (4064, 40254, 11966)  U (28784, -22189, -6596)  V (-2639, -26145, 28784)
 *     Through the conversion of the NV12 section above, every one of the 2^24 colours returns within 2 per channel, for
 *     both matrices (tests/native/annotate_host.cpp runs all of them).
 *  9. Bytes left alone.  No byte of the ring outside the cells, outlines and discs above is written: not the pitch
 *     padding, not the rows between the luma plane and uv_offset, not a slot that no face that takes part names.  With
 *     marks = 0, box = 0 and redact = 0 only regions_dev is written.
 * 10. Errors, all found before any launch.  FLM_ERR_ARG: a null frames_dev, lm_dev or regions_dev; a struct_size smaller
 *     than this library's (either struct); an unknown pixel or matrix; marks outside {0, 1}; box outside [0, 16]; a redact
 *     that is neither 0 nor even and in [2, 64]; a margin outside [0, 4] or NaN.  FLM_ERR_SHAPE, the limit named in
 *     flm_last_error(), unless 1 <= k <= 65535 (k <= 4096 when redact != 0: every workgroup of the mosaic scans the faces
 *     before its own), 1 <= c <= 1024, lm_stride >= 2, and the frame geometry flm_warp_affine_frames_src accepts for the
 *     same src: nframes >= 1 and (BGR24) fh >= 1, fw >= 2, fh*fw*3 < 2^31, frame_stride >= fh*fw*3, pitches and offset 0,
 *     (NV12) fh and fw even and >= 2, y_pitch >= fw, uv_pitch >= fw, uv_offset >= y_pitch*fh, slot bytes < 2^31,
 *     frame_stride >= flm_frame_format_bytes.
 * lm_dev and regions_dev must not overlap the ring or each other; frames_dev needs byte alignment only. */
typedef struct flm_annotate_opts {
  uint32_t struct_size;  /* as flm_forward_opts: lets the struct grow */
  int32_t marks;         /* 0 or 1: the 21-pixel disc of the reference's draw_marks at every accepted landmark */
  int32_t box;           /* outline thickness in px, 0 = none, <= 16 */
  int32_t redact;        /* mosaic cell in px, 0 = none, else even and 2..64 */
  double margin[4];      /* left, top, right, bottom, as fractions of the landmark box's longer side; each in [0, 4] */
  uint8_t mark_bgr[3], box_bgr[3];
  uint8_t reserved[2];   /* pads the colours to 8 bytes */
} flm_annotate_opts;
/* marks 1, box 0, redact 0, margin {0.1, 0.35, 0.1, 0.1}, both colours (0,255,0). */
void flm_annotate_opts_init(flm_annotate_opts* opts);
int flm_bgr_to_yuv(int matrix, const uint8_t bgr[3], uint8_t yuv[3]);
int flm_frames_annotate(flm_stream_t stream, uint8_t* frames_dev, size_t frame_stride, int nframes, int fh, int fw,
                        const flm_frame_format* src /* NULL = BGR24 */, const int32_t* frame_idx_dev /*[K] or NULL = 0*/,
                        const double* lm_dev, size_t lm_stride, int k, int c,
                        const flm_annotate_opts* opts /* NULL = defaults */, int32_t* regions_dev /*[K,4], out*/);

/* ---- landmark flow: carrying the landmarks from one frame to the next without a forward --------------------------------
 * Between two forwards the landmarks of a track can be carried by sparse optical flow: a pyramidal, translation-only
 * Lucas-Kanade step per landmark between two crops cut from two frames with the SAME matrix.  flm_flow_pyramid makes the
 * luma pyramids of the crops (one launch), flm_landmark_flow moves every landmark (one launch, a wave per landmark); no
 * workspace, no allocation, no atomics, no synchronisation.  The result is landmarks in CROP pixels with "negative means
 * rejected", which flm_track_step takes as landmarks on a grid of the crop's own size (sx = sy = 1).
 *
 * Arithmetic.  Integers are int64 unless a range is given; everything summed over a window is an exact integer, so the
 * order of a sum does not matter.  float64 lines are one IEEE operation per written operator, in the written order,
 * nothing fused.  >> is an arithmetic shift.
 *  Luma.  ch = 3 (B, G, R bytes): Y = (1868*b + 9617*g + 4899*r + 8192) >> 14, the weights of flm_face_quality's luma;
 *    ch = 1: Y is the byte.
 *  Pyramid.  Level 0 is Y [h,w]; level l+1 at (y,x) is (a + b + c + d + 2) >> 2 of the 2x2 block of level l at (2y,2x);
 *    level l has (h >> l) x (w >> l) bytes.  The pyramid of one image is its levels 0 .. levels-1 one after the other,
 *    dense: flm_flow_pyramid_bytes(h, w, levels) = sum over l of (h >> l)*(w >> l) bytes (0 for sizes < 1 or levels
 *    outside [1, 6]); image i of a call starts at i times that.  A level-l coordinate is x_l = (x_0 + 0.5) / 2^l - 0.5.
 *  Sample S(I, x, y) on a level of Hl x Wl:  ix = floor(x), ax = (int)((x - ix) * 32.0), likewise iy, ay; the four reads
 *    are at ix, ix+1, iy, iy+1, each clamped to the level (the edge is replicated);
 *    S = (32-ax)*(32-ay)*p00 + ax*(32-ay)*p01 + (32-ax)*ay*p10 + ax*ay*p11, an int32 in [0, 255*1024].
 *  Per point (x, y) = lm_prev of face f, m = m_dev[f] widened to double, r = radius, n = (2r+1)^2, window offsets
 *  i, j in [-r, r]:
 *    NO_HISTORY (1) unless x >= 0 and y >= 0 and both are finite.  Otherwise
 *    p0 = ((m00*x + m01*y) + m02, (m10*x + m11*y) + m12); NOT_FINITE (32) unless both |p0| <= 2^20.  Otherwise
 *    for l = levels-1 down to 0:
 *      p_l = (p0 + 0.5) / 2^l - 0.5;  at the top level the guess is q = p_l
 *      T = S(prev_l, p_l + (i, j));  Gx = S(prev_l, p_l + (i+1, j)) - S(prev_l, p_l + (i-1, j));  Gy likewise in j
 *        (twice the gradient; "p_l + (i, j)" is the float64 sum of the coordinate and the integer)
 *      A = sum Gx*Gx, B = sum Gx*Gy, C = sum Gy*Gy (< 2^47), each converted to double;  det = A*C - B*B
 *      e = (((A + C) - sqrt((A-C)*(A-C) + 4.0*B*B)) / 2.0) / ((double)n * 4194304.0)
 *        (the smaller eigenvalue of the structure tensor per pixel, in grey levels squared)
 *      if !(e >= min_eig): at l > 0 the level is skipped and q carried; at l = 0 LOW_TEXTURE (2) is set.  Otherwise
 *      up to max_iter times:
 *        D = T - S(cur_l, q + (i, j));  bx = sum D*Gx, by = sum D*Gy, each converted to double
 *        dx = 2.0*(C*bx - B*by)/det;  dy = 2.0*(A*by - B*bx)/det;  q = q + (dx, dy)
 *        unless both |q| <= 2^20 (a NaN fails): NOT_FINITE (32), and the point ends here, err = -1
 *        stop after the update when dx*dx + dy*dy < eps*eps
 *      between levels (l > 0): q = 2.0*q + 0.5
 *    err = sum |T - S(cur_0, q + (i, j))| with the T of level 0 (<= 58.7 M: an int32)
 *    RESIDUAL (4) if !((double)err / ((double)n * 1024.0) <= max_err)
 *    OUTSIDE  (8) unless 0 <= qx <= w-1 and 0 <= qy <= h-1
 *    MOVED   (16) if !((qx-p0x)*(qx-p0x) + (qy-p0y)*(qy-p0y) <= max_move*max_move)
 *  Outputs.  flags == 0: lm_out = q and w_out = w_prev (1.0 for a NULL w_prev_dev).  Otherwise lm_out = (-1,-1), w_out =
 *  0 and flags_out says why.  err_out is the SAD above, or -1 where it was not reached (NO_HISTORY, NOT_FINITE); a point
 *  with LOW_TEXTURE has passed through the end and carries its err and gates.  An accepted point is non-negative.
 * The matrix maps FRAME px to CROP px and must be the one BOTH crops were cut with; lm_prev_dev is in frame px.
 * Defaults (flm_flow_opts_init): levels 4, radius 7, max_iter 10, eps 0.03, min_eig 0.5, max_err 12, max_move 64.  On
 * synthetic multi-scale texture three levels lost shifts of 14 px in a 256 px crop to far-away minima that a residual gate
 * accepted, four levels did not.  max_err and max_move are GUESSES: nothing has measured them on real faces.  radius,
 * max_iter, eps and min_eig are the customary values of pyramidal Lucas-Kanade trackers, not measured here either.
 * Errors, all found before anything is launched.  FLM_ERR_ARG: a null pointer other than the optional ones; a struct_size
 * smaller than this library's; a non-zero reserved or pad; unless eps > 0, min_eig >= 0, max_err >= 0, max_move > 0 (a NaN
 * fails each); an output overlapping an input or another output.  FLM_ERR_SHAPE, the limit named in flm_last_error(),
 * unless 1 <= k <= 65535, 1 <= c <= 1024, 1 <= levels <= 6, 1 <= radius <= 7, 1 <= max_iter <= 64, h and w are
 * multiples of 2^(levels-1) with (h >> (levels-1)) >= 2 and (w >> (levels-1)) >= 2, and h, w <= 32768;
 * flm_flow_pyramid: 1 <= n <= 131070 (two crops of 65535 faces), ch 1 or 3, and fewer than 2^31 tiles of 32x32. */
#define FLM_FLOW_NO_HISTORY 1
#define FLM_FLOW_LOW_TEXTURE 2
#define FLM_FLOW_RESIDUAL 4
#define FLM_FLOW_OUTSIDE 8
#define FLM_FLOW_MOVED 16
#define FLM_FLOW_NOT_FINITE 32
size_t flm_flow_pyramid_bytes(int h, int w, int levels);
int flm_flow_pyramid(flm_stream_t stream, const uint8_t* src_dev /*[N,H,W,ch]*/, int n, int h, int w, int ch /*1 | 3*/,
                     int levels, uint8_t* pyr_dev /*[N, flm_flow_pyramid_bytes]*/);
typedef struct flm_flow_opts {
  uint32_t struct_size;  /* as flm_track_opts */
  uint32_t reserved;     /* 0 */
  int32_t levels;        /* pyramid levels, 1..6 */
  int32_t radius;        /* window radius r, 1..7: a window of (2r+1)^2 pixels */
  int32_t max_iter;      /* iterations per level, 1..64 */
  int32_t pad;           /* 0 */
  double eps;            /* a level stops when the update is shorter than eps px */
  double min_eig;        /* the least eigenvalue per pixel, grey levels squared, at which a level is solved */
  double max_err;        /* the largest mean absolute residual, grey levels, of an accepted point (a guess) */
  double max_move;       /* the longest move, crop px, of an accepted point (a guess) */
} flm_flow_opts;
void flm_flow_opts_init(flm_flow_opts* opts);
int flm_landmark_flow(flm_stream_t stream, const uint8_t* pyr_prev_dev, const uint8_t* pyr_cur_dev, int k, int h, int w,
                      const double* lm_prev_dev /*[K,C,2] frame px*/, const double* w_prev_dev /*[K,C] or NULL*/,
                      const float* m_dev /*[K,2,3] frame px -> crop px*/, int c, const flm_flow_opts* opts /*NULL = defaults*/,
                      double* lm_out_dev /*[K,C,2] crop px*/, double* w_out_dev /*[K,C] or NULL*/,
                      int32_t* err_out_dev /*[K,C] or NULL*/, int32_t* flags_out_dev /*[K,C]*/);

/* ---- the flow tick on rows: flow for the slots that hold a face and have a history ------------------------------------
 * THE HISTORY RULE.  Beside the history store -- hist_lm float64 [n_slots,C,2], the raw landmarks of a slot's last tick in
 * frame px, and hist_w float64 [n_slots,C] -- a tracker keeps flow_frame int32 [n_slots], the ring slot those landmarks
 * were found in, and flow_ready int32 [n_slots]:
 *     flow_ready[g] == 1 exactly when slot g was served with status 0 by the last tick of its stream, key or flow, and
 *     nothing has written its crop matrix since.
 * Every tick clears flow_ready for all slots of the streams it steps and then sets it for the rows it served alive
 * (flm_track_flow_history_put); whoever writes a crop matrix (a seed, a birth or a restart of the association) clears the
 * slot's entry.  A live slot a budget left out thereby loses its history -- its landmarks are older than the previous
 * frame --, a slot of a stream that was not stepped keeps it.
 *
 * flm_track_gather_flow: flm_track_gather_live with one more condition and two more columns, in ONE launch (the same
 * one-workgroup prefix count: the row order is a function of the inputs alone).  The arguments are those of
 * flm_track_gather_live plus flow_frame_dev int32 [S*K] (in), flow_ready_dev int32 [S*K] (in/out) and prev_frame_idx_c
 * int32 [N] (out); counts_dev is int32 [6]; cursor_dev is a cursor of the flow ticks' own.  Its contract is rules 1-7
 * there with these changes:
 *  1. Slot g is LIVE when it is eligible by rule 1 there.  It is ELIGIBLE here when it is live and flow_ready_dev[g] != 0.
 *     L = the number of live slots, E = the number of eligible ones.
 *  2-4. unchanged, over the eligible slots of this rule 1.  A served row r of slot g additionally gets prev_frame_idx_c[r]
 *     = flow_frame_dev[g]; an inert row gets 0.
 *  5. Time: a live slot that is not served -- it has no history, or it is beyond the budget -- ages as "eligible, not
 *     served" there; a served slot and a slot that is on and not live as there.
 *  5a. After its ranking, flow_ready_dev[g] = 0 for EVERY slot of a stream that is on.  A slot of a stream that is off is
 *     neither read nor written, flow_ready_dev and flow_frame_dev included.
 *  6. counts = (L, E, served, E - served, L - E, cursor_out), cursor_out as there with E and N.
 *  7. unchanged; flow_frame_dev is only read.
 * Errors as flm_track_gather_live, with flow_frame_dev, flow_ready_dev and prev_frame_idx_c among the required pointers,
 * and FLM_ERR_ARG where an output overlaps an input or another output. */
int flm_track_gather_flow(flm_stream_t stream, const int32_t* stream_on_dev /*[S] or NULL*/, int s, int k /*slots PER STREAM*/,
                          int fh, int fw, int n /*the budget*/, const int32_t* frame_idx_stream_dev /*[S] or NULL*/,
                          const double* dt_stream_dev /*[S] or NULL*/, double dt, const float* m_crop_dev /*[S*K,2,3]*/,
                          const int32_t* boxes_dev /*[S*K,4]*/, const double* best_q_dev /*[S*K] or NULL*/,
                          int32_t* reset_dev /*[S*K] or NULL, in/out*/, double* age_dev /*[S*K] or NULL, in/out*/,
                          int32_t* cursor_dev /*[1] or NULL, in/out*/, const int32_t* flow_frame_dev /*[S*K]*/,
                          int32_t* flow_ready_dev /*[S*K], in/out*/, int32_t* slot_c /*[N]*/, float* m_c /*[N,2,3]*/,
                          int32_t* boxes_c /*[N,4]*/, int32_t* frame_idx_c /*[N]*/, int32_t* prev_frame_idx_c /*[N]*/,
                          double* dt_c /*[N] or NULL*/, double* best_q_c /*[N] or NULL*/, int32_t* reset_c /*[N] or NULL*/,
                          int32_t* counts_dev /*[6]*/);

/* flm_landmark_flow_rows: flm_landmark_flow on the rows of a compacted batch, with an optional forward-backward check, in
 * ONE launch (a wave per landmark of a row; no workspace, no allocation, no atomics, no synchronisation).
 * Where the arguments live: pyr_prev_dev, pyr_cur_dev [N, flm_flow_pyramid_bytes] and m_dev [N,2,3] are read at row r;
 * lm_prev_dev [n_slots,C,2] and w_prev_dev [n_slots,C] -- the history store itself, never copied -- at slot g =
 * slot_dev[r]; every output is compact, at row r.
 * A row whose slot lies outside [0, n_slots) is INERT (flm_track_gather_* write -1): it reads nothing and writes (-1,-1),
 * weight 0, err -1, fb -1.0 and FLM_FLOW_NO_HISTORY for each of its C points.
 * Forward pass: "Per point" of flm_landmark_flow, word for word.  With slot_dev[r] = r, n = n_slots and max_fb = 0 every
 * output equals flm_landmark_flow's bit for bit.
 * Forward-backward check, max_fb > 0, only for a point whose forward flags are 0: the same per-point procedure -- "for l =
 * levels-1 down to 0" with the same levels, radius, max_iter, eps and min_eig -- with the two images exchanged, from
 * p0' = q (q is in crop px: no matrix is applied), gives q' and the backward pass's own LOW_TEXTURE / NOT_FINITE.
 *     fb2 = (q'x - p0x)*(q'x - p0x) + (q'y - p0y)*(q'y - p0y)     (one IEEE operation per operator, in this order)
 *     FB (64) if the backward pass ended with NOT_FINITE or LOW_TEXTURE, or if !(fb2 <= max_fb*max_fb)
 *   The backward pass's residual, OUTSIDE and MOVED gates are not applied.  A point with FB is rejected as any other:
 *   (-1,-1), weight 0; err_out keeps the forward pass's SAD.
 * fb_out_dev float64 [N,C]: fb2, or -1.0 where the backward pass did not run (max_fb = 0, an inert row, forward flags) or
 * did not finish (NOT_FINITE).
 * max_fb = 0 switches the check off, and off is the default of everything built on this call: the value a user would
 * start from, 1 px as in median-flow trackers, is a GUESS that -- like max_err and max_move -- nothing has measured on
 * real faces.
 * Errors, all found before anything is launched: those of flm_landmark_flow with k read as n; FLM_ERR_ARG for a null
 * slot_dev or fb_out_dev and unless max_fb is finite and >= 0; FLM_ERR_SHAPE unless 1 <= n_slots <= 65535. */
#define FLM_FLOW_FB 64
int flm_landmark_flow_rows(flm_stream_t stream, const uint8_t* pyr_prev_dev, const uint8_t* pyr_cur_dev, int n, int h, int w,
                           const int32_t* slot_dev /*[N]*/, int n_slots, const double* lm_prev_dev /*[n_slots,C,2] frame px*/,
                           const double* w_prev_dev /*[n_slots,C] or NULL*/, const float* m_dev /*[N,2,3] frame px -> crop px*/,
                           int c, const flm_flow_opts* opts /*NULL = defaults*/, double max_fb /*crop px; 0 = off*/,
                           double* lm_out_dev /*[N,C,2] crop px*/, double* w_out_dev /*[N,C] or NULL*/,
                           int32_t* err_out_dev /*[N,C] or NULL*/, double* fb_out_dev /*[N,C]*/,
                           int32_t* flags_out_dev /*[N,C]*/);

/* flm_track_flow_history_put: the rows of a tick moved to the history of their slots, in ONE launch (a wave per row).
 * For a row r with g = slot_dev[r] in [0, n_slots):
 *   status_rows_dev[r] == 0:  hist_lm_dev[g] = lm_rows_dev[r] (the RAW landmarks of the track step, frame px) and
 *                             hist_w_dev[g] = w_rows_dev[r], each where given; flow_frame_dev[g] = frame_idx_c[r];
 *                             flow_ready_dev[g] = 1
 *   otherwise:                flow_ready_dev[g] = 0, nothing else
 * A row whose slot lies outside [0, n_slots) writes nothing; a slot no row names keeps every bit.  The rows name
 * distinct slots.  lm_rows_dev and hist_lm_dev may both be NULL -- the all-slots ticks, which copy their landmarks
 * themselves, then write flow_frame and flow_ready alone, with slot_dev[r] = r --, and so may w_rows_dev and hist_w_dev;
 * weights go with landmarks.
 * Errors, all found before anything is launched: FLM_ERR_ARG for a null slot_dev, status_rows_dev, frame_idx_c,
 * flow_frame_dev or flow_ready_dev, a rows tensor without its store or the reverse, weights without landmarks, or an output
 * overlapping an input or another output; FLM_ERR_SHAPE unless 1 <= n <= 65535, 1 <= n_slots <= 65535, 1 <= c <= 1024. */
int flm_track_flow_history_put(flm_stream_t stream, const int32_t* slot_dev /*[N]*/, const int32_t* status_rows_dev /*[N]*/,
                               const int32_t* frame_idx_c /*[N]*/, const double* lm_rows_dev /*[N,C,2] or NULL*/,
                               const double* w_rows_dev /*[N,C] or NULL*/, int n, int n_slots, int c,
                               double* hist_lm_dev /*[n_slots,C,2] or NULL*/, double* hist_w_dev /*[n_slots,C] or NULL*/,
                               int32_t* flow_frame_dev /*[n_slots]*/, int32_t* flow_ready_dev /*[n_slots]*/);

/* ---- face parts: eye and mouth patches straight from the frames ---------------------------------------------------------
 * A gaze, liveness or lip-reading network reads patches of the eyes and the mouth.  flm_warp_parts_frames cuts R patches
 * per face, each under a similarity fitted to the part's OWN landmarks, in ONE launch with ONE output tensor.
 *
 * A SET OF PARTS: R parts, 1 <= R <= FLM_PARTS_MAX (8).  Part r names part_n[r] landmarks, 2 <= part_n[r] <=
 * FLM_PART_MAX_POINTS (32): part_idx_dev int32 [R,32] holds their numbers and part_tmpl_dev float64 [R,32,2] where each
 * belongs in PATCH pixels (x, y); part_n is an array of R ints in HOST memory, read during the call (it sizes the checks
 * and travels to the kernel by value).  The entries of a row past part_n[r] -- padded with -1 by convention -- are never
 * read.  All parts share one patch size ph x pw.
 *
 * flm_part_affines: aff_dev float32 [K,R,2,3], the matrix FRAME px -> PATCH px of every (face, part), and part_ok_dev
 * int32 [K,R].  The matrix of (f, r) is word for word the arithmetic of flm_similarity_from_landmarks_weighted with
 * sx = sy = 1 (so no product by sx, sy is made), over the part's entries i = 0 .. part_n[r]-1 IN THE ORDER part_idx LISTS
 * THEM: point i is landmark id = part_idx[r][i] of face f, the two doubles at lm_dev + (f*c + id)*lm_stride, its weight
 * the double at w_dev + (f*c + id)*w_stride (w_dev == NULL: 1), its template point part_tmpl[r][i].  An entry takes part
 * when 0 <= id < c, both coordinates are >= 0 and the weight is > 0 (a NaN fails each test).  float64, one IEEE operation
 * per written operator, nothing fused, every sum sequential from 0.0 over the participating entries in ascending i:
 *   W = sum w;  mpx = sum(w*px) / W, likewise mpy, mqx, mqy (q: the template);  p' = p - mp, q' = q - mq
 *   sa = sum w*(px'*qx' + py'*qy');  sb = sum w*(px'*qy' - py'*qx');  var = sum w*(px'*px' + py'*py')
 *   a = sa / var, b = sb / var, tx = mqx - (a*mpx - b*mpy), ty = mqy - (b*mpx + a*mpy);  M = [[a,-b,tx],[b,a,ty]]
 * each of the six rounded to float32 once.  part_ok = 1 when two entries or more take part and var > 0 (a NaN var fails
 * the test); otherwise part_ok = 0 and the matrix is the identity.  An index may appear in several parts, and twice in one.
 *
 * flm_warp_parts_frames: dst_dev [K,R,...] -- K*R faces of ph x pw in the image format, face f*R + r being patch (f, r)
 * -- in ONE launch of K*R workgroups; the fit above is part of that launch and runs ONCE per (face, part).  aff_out_dev
 * and part_ok_out_dev, each optional, receive the bits of flm_part_affines, zero faces included.
 *   THE CONTRACT: patch (f, r) has, pixel for pixel, the bits flm_warp_affine_frames_src stores for a face whose matrix
 *   is aff[f][r], with hd = ph, wd = pw, face f's frame_idx_dev[f] and boxes_dev[f] (each optional, as there), and the
 *   same samples, fmt and src (NULL: the dense BGR24 ring; or NV12).  A part that is not ok stores a ZERO face -- what
 *   that call stores for a slot outside the ring or an empty clipped box, which give a zero face here too.
 * No atomics, no allocation, no workspace; no byte outside the outputs is written; every launch shape is a host number.
 * Errors, all found before anything is launched, with the codes of flm_warp_affine_frames_src for what it shares with
 * that call (samples, ring, formats, dst alignment).  FLM_ERR_ARG: a null frames / lm / part_idx / part_tmpl / part_n /
 * dst (aff and part_ok for flm_part_affines), r outside [1,8], a part_n[r] outside [2,32].  FLM_ERR_SHAPE, the limit named
 * in flm_last_error(): lm_stride < 2, w_stride < 1 (with w_dev), k outside [1,65535], c outside [1,1024], ph or pw
 * outside [1,256]. */
#define FLM_PARTS_MAX 8
#define FLM_PART_MAX_POINTS 32
#define FLM_PART_MAX_SIDE 256
int flm_part_affines(flm_stream_t stream, const double* lm_dev, size_t lm_stride, const double* w_dev /*or NULL*/,
                     size_t w_stride, int k, int c, const int32_t* part_idx_dev /*[R,32]*/,
                     const double* part_tmpl_dev /*[R,32,2]*/, const int32_t* part_n /*HOST [R]*/, int r,
                     float* aff_dev /*[K,R,2,3]*/, int32_t* part_ok_dev /*[K,R]*/);
int flm_warp_parts_frames(flm_stream_t stream, const uint8_t* frames_dev, size_t frame_stride, int nframes, int fh, int fw,
                          const int32_t* frame_idx_dev /*[K] or NULL*/, const int32_t* boxes_dev /*[K,4] or NULL*/,
                          const double* lm_dev, size_t lm_stride, const double* w_dev /*or NULL*/, size_t w_stride, int c,
                          const int32_t* part_idx_dev /*[R,32]*/, const double* part_tmpl_dev /*[R,32,2]*/,
                          const int32_t* part_n /*HOST [R]*/, int r, int k, void* dst_dev /*[K,R,...]*/, int ph, int pw,
                          int samples, const flm_image_format* fmt /*or NULL*/, const flm_frame_format* src /*or NULL*/,
                          float* aff_out_dev /*[K,R,2,3] or NULL*/, int32_t* part_ok_out_dev /*[K,R] or NULL*/);

/* ---- openness and blink state: how open the eyes and the mouth are, and a count of closures -----------------------------
 * flm_face_openness, ONE launch (one thread per row, looping over the measures), no workspace, no allocation, no atomics.
 *
 * A MEASURE g is a width pair of landmarks (width[g][0], width[g][1]) and V = n_pairs[g] pairs (upper[g][v], lower[g][v]),
 * 1 <= V <= FLM_OPEN_MAX_PAIRS (4); flm_open_opts holds G = n_measures of them, 1 <= G <= FLM_OPEN_MAX_MEASURES (8).
 * Landmarks and weights are read at element strides as flm_head_pose reads them, and a landmark TAKES PART as there: its
 * index lies in [0, c), both coordinates are >= 0 and its weight (1 without w_dev) is > 0; a NaN fails each test.
 * Per row and measure, float64, one IEEE operation per written operator, in the written order, nothing fused:
 *   dist(i, j) = sqrt(dx*dx + dy*dy),  dx = x_i - x_j,  dy = y_i - y_j
 *   dw  = dist(width[g][0], width[g][1])
 *   sum = 0.0;  sum = sum + dist(upper[g][v], lower[g][v])  for v = 0 .. V-1 in ascending v
 *   o   = (sum / (double)V) / dw
 *   OK  = every landmark the measure names takes part, dw >= min_width, and o is finite
 * For six eye points with V = 2, o is the eye aspect ratio of Soukupova and Cech (2016).
 * The record, FLM_OPEN_REC = 4 doubles: { o, dw, ok ? 1.0 : 0.0, sum }.  When not ok, o = -1; when a named landmark does not
 * take part nothing was measured and dw = sum = -1 as well.  (Coordinates are expected finite: +inf takes part and yields
 * NaNs whose sign the platform chooses.)
 * Rows and slots follow flm_head_pose: without slot_dev row r writes rec_dev[r] ([N,G,4]); with slot_dev int32 [N] a valid
 * row writes at slot s = slot_dev[r] of rec_dev [n_slots,G,4], an inert row (s outside [0, n_slots)) writes nothing, and a
 * slot no row names keeps its bits.  Valid rows name distinct slots.
 *
 * STATE, optional, in the same launch: state_dev float64 [N or n_slots,G,FLM_OPEN_STATE = 8], indexed as rec_dev,
 *   { closed, run, events, last_closed, closed_total, seen_total, last_event_frame, 0 }
 * with reset_dev int32 [N or n_slots] (in/out, required with state_dev), dt_dev float64 [N] by ROW or NULL (NULL: the scalar
 * dt for every row), status_rows_dev int32 [N] by row or NULL (NULL: 0), and frame_id.  The thread of row r is the ONLY
 * reader and writer of its slot's G entries and of its reset flag, which is why the state is updated in place; it reads
 * the flag once, walks g = 0 .. G-1, and stores 0 to the flag after the last measure -- program order within one thread,
 * no atomics.  Per valid row:
 *   if reset_dev[s] != 0: every measure's state becomes { 0, 0, 0, -1, 0, 0, -1, 0 } first, whatever follows; the flag
 *     is then set to 0.  An inert row and a slot no row names leave flag and state alone: a pending reset waits.
 *   if the measure is not ok, or status != 0, or the row's dt is not finite and > 0: the state keeps every bit.
 *   otherwise seen_total = seen_total + dt, then one of four cases:
 *     closed == 0 and o < close_below:   closed = 1;  run = 0;  closed_total = closed_total + dt
 *     closed == 0 otherwise:             run = run + dt
 *     closed != 0 and o > open_above:    d = run + dt;  last_closed = d;
 *                                        if min_closed <= d && d <= max_closed: events = events + 1,
 *                                                                               last_event_frame = (double)frame_id
 *                                        closed = 0;  run = 0
 *     closed != 0 otherwise:             run = run + dt;  closed_total = closed_total + dt
 * Defaults (flm_open_opts_init): the three measures of the 68-point layout -- right eye: width (36,39), pairs (37,41)
 * (38,40); left eye: width (42,45), pairs (43,47) (44,46); inner mouth: width (60,64), pairs (61,67) (62,66) (63,65) --
 * close_below = 0.18, open_above = 0.22, min_closed = 0.03 s, max_closed = 0.5 s, min_width = 4 px.  These five numbers
 * are UNMEASURED GUESSES: there is no trained checkpoint and no labelled blink data behind them.
 * Errors, all found before anything is launched.  FLM_ERR_ARG: a null lm_dev or rec_dev, state_dev without reset_dev,
 * a struct_size smaller than this library's, a non-zero reserved, n_measures outside [1,8], an n_pairs outside [1,4],
 * close_below not below open_above (or either NaN), a min_closed, max_closed or min_width that is NaN or negative,
 * max_closed < min_closed, with state_dev and without dt_dev a dt that is not finite and > 0, an output overlapping an
 * input or another output.  FLM_ERR_SHAPE: lm_stride < 2, w_stride < 1 (with w_dev), n outside [1,65535], c outside
 * [1,1024], with slot_dev n_slots outside [1,65535]. */
#define FLM_OPEN_REC 4
#define FLM_OPEN_STATE 8
#define FLM_OPEN_MAX_MEASURES 8
#define FLM_OPEN_MAX_PAIRS 4
typedef struct flm_open_opts {
  uint32_t struct_size;  /* as flm_track_opts */
  uint32_t reserved;     /* 0 */
  int32_t n_measures;    /* G */
  int32_t n_pairs[FLM_OPEN_MAX_MEASURES];                    /* V of measure g */
  int32_t width[FLM_OPEN_MAX_MEASURES][2];
  int32_t upper[FLM_OPEN_MAX_MEASURES][FLM_OPEN_MAX_PAIRS];
  int32_t lower[FLM_OPEN_MAX_MEASURES][FLM_OPEN_MAX_PAIRS];
  double close_below;    /* an open measure closes when o < close_below */
  double open_above;     /* a closed measure opens when o > open_above; close_below < open_above */
  double min_closed;     /* a closure of min_closed <= d <= max_closed (the unit of dt) counts as an event */
  double max_closed;
  double min_width;      /* frame px: below this dw the measure is not ok */
} flm_open_opts;
void flm_open_opts_init(flm_open_opts* opts);
int flm_face_openness(flm_stream_t stream, const double* lm_dev, size_t lm_stride, const double* w_dev /*or NULL*/,
                      size_t w_stride, int n, int c, const flm_open_opts* opts /*NULL = defaults*/,
                      const int32_t* slot_dev /*[N] or NULL*/, int n_slots, double* rec_dev /*[N or n_slots,G,4]*/,
                      double* state_dev /*[N or n_slots,G,8] or NULL*/, int32_t* reset_dev /*[N or n_slots] or NULL*/,
                      const double* dt_dev /*[N] or NULL*/, double dt, const int32_t* status_rows_dev /*[N] or NULL*/,
                      int64_t frame_id);

#ifdef __cplusplus
}
#endif
#endif /* FLM_H_ */
