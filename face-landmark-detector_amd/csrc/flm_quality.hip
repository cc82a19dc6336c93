// flm_face_quality and flm_track_best_update (include/flm.h states every operation; flm_quality_dev.h holds the per-pixel
// pieces; the comments here only say how the work is laid out).
//
// flm_face_quality, two launches, no workspace:
//   quality_init_kernel   writes {n_pix, 0, 0, n_lap, 0, 0, 0, 0} into every record;
//   face_quality_kernel   a grid of (tile, face) workgroups of 256 threads.  A tile is 8 rows x 128 columns of a face, so a
//     112 x 112 face is 14 workgroups and a tracker of 16 slots 224.  The workgroup (1) copies the tile and its one-pixel
//     halo, as stored, from global memory into LDS: the tile is a set of runs of consecutive elements (one per row for
//     NHWC, one per row and plane for NCHW), every run is cut at the 16-byte boundaries of its ACTUAL address, a piece that
//     lies wholly inside the run is one 16-byte load and the pieces at its two ends are element loads -- no byte outside
//     the run, hence outside the face, is read; (2) turns every pixel of tile and halo into its luma Y (uint16 in LDS);
//     (3) every thread takes four pixels of the tile: Y, Y*Y, the two exposure counts and, for interior pixels, the
//     Laplacian from the four neighbours in LDS; (4) the six sums are reduced over the wave with shuffles, over the four
//     waves through LDS, and leave the workgroup as ONE 64-bit integer atomic per entry.  Integer sums: the order of
//     arrival does not matter.
//
// flm_track_best_update, one launch: a grid of (chunk, slot) workgroups.  Thread 0 of every workgroup derives the slot's
// decision from the inputs (nobody writes them: the workgroups of a slot agree); a slot that is not taken costs its
// workgroups that and nothing else.  Chunk 0 writes the slot's scalars; every chunk copies its 4 KiB pieces of the face,
// cut at 16-byte boundaries as above, with 16-byte accesses where source and destination are congruent modulo 16.
// flm_track_best_update_rows is the same body on the rows of a compacted batch: everything the decision reads lies at the
// ROW, everything written at the row's SLOT; an inert row's workgroups return before they read anything else.
#include "flm_best_dev.h"
#include "flm_common.h"
#include "flm_copy_dev.h"
#include "flm_quality_dev.h"

namespace flm {

typedef unsigned q4v __attribute__((ext_vector_type(4)));

constexpr int kQTileRows = 8, kQTileCols = 128, kQThreads = 256;
constexpr int kQHaloRows = kQTileRows + 2, kQHaloCols = kQTileCols + 2;

// The staging area of one tile: RUNS runs of at most RUN_ELEMS elements, each at the offset its address has in its
// 16-byte line (so global and LDS pieces are congruent), STRIDE bytes apart.
template <int LAYOUT, int ES> struct QStage {
  static constexpr int RUNS = LAYOUT == FLM_LAYOUT_NHWC ? kQHaloRows : 3 * kQHaloRows;
  static constexpr int RUN_ELEMS = LAYOUT == FLM_LAYOUT_NHWC ? 3 * kQHaloCols : kQHaloCols;
  static constexpr int CHUNKS = (RUN_ELEMS * ES + 15) / 16 + 1;  // 16-byte pieces a run can touch
  static constexpr int STRIDE = CHUNKS * 16;
};

struct QualityArgs {
  float bias[3], inv[3];  // by OUTPUT channel
  int reverse;
  int dark16, bright16;   // 16*dark, 16*bright
};

__global__ __launch_bounds__(kQThreads) void quality_init_kernel(int64_t* __restrict__ rec, int k, int64_t n_pix,
                                                                 int64_t n_lap) {
  const int i = blockIdx.x * kQThreads + threadIdx.x;
  if (i >= k * FLM_QUALITY_REC) return;
  const int e = i & (FLM_QUALITY_REC - 1);
  rec[i] = e == 0 ? n_pix : e == 3 ? n_lap : 0;
}

template <int LAYOUT, int TYPE>
__global__ __launch_bounds__(kQThreads) void face_quality_kernel(const typename QPix<TYPE>::T* __restrict__ faces, int h,
                                                                 int w, int tiles_c, const QualityArgs a,
                                                                 unsigned long long* __restrict__ rec) {
  typedef typename QPix<TYPE>::T T;
  constexpr int ES = (int)sizeof(T);
  typedef QStage<LAYOUT, ES> S;
  __shared__ __attribute__((aligned(16))) unsigned char stage[S::RUNS * S::STRIDE];
  __shared__ uint16_t luma[kQHaloRows * kQHaloCols];
  __shared__ long long part[kQThreads / 64][6];

  const int tid = threadIdx.x, f = blockIdx.y;
  const int tr = blockIdx.x / tiles_c, tc = blockIdx.x - tr * tiles_c;
  const int r0 = tr * kQTileRows, c0 = tc * kQTileCols;  // the tile's first pixel (inside the face)
  // tile and halo, clipped to the face: rows [hr0, hr0+nrow), columns [hc0, hc0+ncol)
  const int hr0 = r0 > 0 ? r0 - 1 : 0, hc0 = c0 > 0 ? c0 - 1 : 0;
  const int hr1 = r0 + kQTileRows + 1 < h ? r0 + kQTileRows + 1 : h;
  const int hc1 = c0 + kQTileCols + 1 < w ? c0 + kQTileCols + 1 : w;
  const int nrow = hr1 - hr0, ncol = hc1 - hc0;
  const int npix = h * w;  // (h*w*12 < 2^31: every element index inside a face fits int32)
  const T* face = faces + (size_t)f * 3 * npix;
  const int run_elems = LAYOUT == FLM_LAYOUT_NHWC ? 3 * ncol : ncol;
  // run -> its first element: NHWC run = halo row; NCHW run = plane * kQHaloRows + halo row
  auto run_first = [&](int run) -> const T* {
    if (LAYOUT == FLM_LAYOUT_NHWC) return face + ((hr0 + run) * w + hc0) * 3;
    const int plane = run / kQHaloRows, rr = run - plane * kQHaloRows;
    return face + plane * npix + (hr0 + rr) * w + hc0;
  };

  // ---- (1) the runs, as stored, into LDS ----
  for (int i = tid; i < S::RUNS * S::CHUNKS; i += kQThreads) {
    const int run = i / S::CHUNKS, j = i - run * S::CHUNKS;
    const int rr = LAYOUT == FLM_LAYOUT_NHWC ? run : run % kQHaloRows;
    if (rr >= nrow) continue;
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(run_first(run));
    const uintptr_t a1 = a0 + (uintptr_t)run_elems * ES;
    const uintptr_t lo = (a0 & ~(uintptr_t)15) + 16u * (unsigned)j, hi = lo + 16;
    unsigned char* d = stage + run * S::STRIDE + 16 * j;
    if (lo >= a0 && hi <= a1) {
      *reinterpret_cast<q4v*>(d) = *reinterpret_cast<const q4v*>(lo);
    } else if (hi > a0 && lo < a1) {  // an end of the run: its elements one by one (an element never straddles a piece)
      const uintptr_t s = lo > a0 ? lo : a0, e = hi < a1 ? hi : a1;
      for (uintptr_t q = s; q < e; q += ES) *reinterpret_cast<T*>(d + (q - lo)) = *reinterpret_cast<const T*>(q);
    }
  }
  __syncthreads();

  // ---- (2) luma of tile and halo ----
  for (int i = tid; i < kQHaloRows * kQHaloCols; i += kQThreads) {
    const int rr = i / kQHaloCols, cc = i - rr * kQHaloCols;
    if (rr >= nrow || cc >= ncol) continue;
    int p[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int run = LAYOUT == FLM_LAYOUT_NHWC ? rr : c * kQHaloRows + rr;
      const int lead = (int)(reinterpret_cast<uintptr_t>(run_first(run)) & 15u);
      const int el = LAYOUT == FLM_LAYOUT_NHWC ? cc * 3 + c : cc;
      const T x = *reinterpret_cast<const T*>(stage + run * S::STRIDE + lead + el * ES);
      p[c] = quality_quant(QPix<TYPE>::load(x), a.bias[c], a.inv[c]);
    }
    const int b = a.reverse ? p[2] : p[0], r = a.reverse ? p[0] : p[2];
    luma[rr * kQHaloCols + cc] = (uint16_t)quality_luma(b, p[1], r);
  }
  __syncthreads();

  // ---- (3) four pixels of the tile per thread ----
  long long s[6] = {0, 0, 0, 0, 0, 0};  // Y, Y*Y, L, L*L, dark, bright
  const int col = c0 + (tid & (kQTileCols - 1));
#pragma unroll
  for (int q = 0; q < kQTileRows / 2; ++q) {
    const int row = r0 + (tid >> 7) + 2 * q;
    if (row >= h || col >= w) continue;
    const uint16_t* y = luma + (row - hr0) * kQHaloCols + (col - hc0);
    const int yc = y[0];
    s[0] += yc;
    s[1] += yc * yc;
    s[4] += yc < a.dark16;
    s[5] += yc > a.bright16;
    if (row >= 1 && row <= h - 2 && col >= 1 && col <= w - 2) {
      const int l = (int)y[-kQHaloCols] + (int)y[kQHaloCols] + (int)y[-1] + (int)y[1] - 4 * yc;
      s[2] += l;
      s[3] += l * l;  // (< 2^28)
    }
  }

  // ---- (4) wave, workgroup, one atomic per entry ----
#pragma unroll
  for (int e = 0; e < 6; ++e) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s[e] += __shfl_down(s[e], off, 64);
  }
  if ((tid & 63) == 0) {
#pragma unroll
    for (int e = 0; e < 6; ++e) part[tid >> 6][e] = s[e];
  }
  __syncthreads();
  if (tid < 6) {
    long long t = 0;
    for (int wv = 0; wv < kQThreads / 64; ++wv) t += part[wv][tid];
    const int entry = tid < 2 ? 1 + tid : 2 + tid;  // Y, Y*Y -> 1, 2;  L, L*L, dark, bright -> 4..7
    if (t != 0) atomicAdd(rec + (size_t)f * FLM_QUALITY_REC + entry, (unsigned long long)t);
  }
}

// The format, the options and the alignment of faces are checked by the caller in flm_api.hip.
int launch_face_quality(hipStream_t s, const void* faces, int k, int h, int w, const flm_image_format* fmt,
                        const flm_quality_opts* opts, int64_t* rec) {
  if (k < 1 || k > 65535) {
    set_error("face_quality: k=%d outside 1 <= k <= 65535", k);
    return FLM_ERR_SHAPE;
  }
  if (h < 1 || w < 1 || (long long)h * w * 12 >= (1ll << 31)) {
    set_error("face_quality: faces of %dx%d, needs h, w >= 1 and h*w*3*4 < 2^31", h, w);
    return FLM_ERR_SHAPE;
  }
  QualityArgs a;
  for (int c = 0; c < 3; ++c) {
    a.bias[c] = fmt->bias[c];
    a.inv[c] = 1.0f / fmt->scale[c];
  }
  a.reverse = fmt->reverse_channels;
  a.dark16 = 16 * opts->dark;
  a.bright16 = 16 * opts->bright;
  const int64_t n_lap = (int64_t)(h > 2 ? h - 2 : 0) * (int64_t)(w > 2 ? w - 2 : 0);
  quality_init_kernel<<<cdiv(k * FLM_QUALITY_REC, kQThreads), kQThreads, 0, s>>>(rec, k, (int64_t)h * w, n_lap);
  FLM_LAUNCH_CHECK("quality_init_kernel");
  const int tiles_r = cdiv(h, kQTileRows), tiles_c = cdiv(w, kQTileCols);  // (tiles_r * tiles_c <= h*w < 2^28)
  const dim3 grid(tiles_r * tiles_c, k);
  unsigned long long* urec = reinterpret_cast<unsigned long long*>(rec);
#define FLM_CALL(L, P) \
  face_quality_kernel<L, P><<<grid, kQThreads, 0, s>>>(static_cast<const QPix<P>::T*>(faces), h, w, tiles_c, a, urec)
  if (fmt->layout == FLM_LAYOUT_NHWC) {
    switch (fmt->type) {
      case FLM_PIX_F32: FLM_CALL(FLM_LAYOUT_NHWC, FLM_PIX_F32); break;
      case FLM_PIX_F16: FLM_CALL(FLM_LAYOUT_NHWC, FLM_PIX_F16); break;
      case FLM_PIX_BF16: FLM_CALL(FLM_LAYOUT_NHWC, FLM_PIX_BF16); break;
      default: FLM_CALL(FLM_LAYOUT_NHWC, FLM_PIX_U8); break;
    }
  } else {
    switch (fmt->type) {
      case FLM_PIX_F32: FLM_CALL(FLM_LAYOUT_NCHW, FLM_PIX_F32); break;
      case FLM_PIX_F16: FLM_CALL(FLM_LAYOUT_NCHW, FLM_PIX_F16); break;
      case FLM_PIX_BF16: FLM_CALL(FLM_LAYOUT_NCHW, FLM_PIX_BF16); break;
      default: FLM_CALL(FLM_LAYOUT_NCHW, FLM_PIX_U8); break;
    }
  }
#undef FLM_CALL
  FLM_LAUNCH_CHECK("face_quality_kernel");
  return FLM_OK;
}

// ---- flm_track_best_update ------------------------------------------------------------------------------------------

struct BestArgs {
  const unsigned char* faces;
  size_t face_bytes;
  const int64_t* rec;
  const int32_t* status;
  const int32_t* reset;
  const double* lm;
  size_t lm_stride;
  const double* wt;
  size_t w_stride;
  int c;
  const double* factor;
  const float* m;
  int64_t frame_id;
  double sharp_ref, min_exposed;
  const double* best_q_in;
  double* best_q_out;
  unsigned char* gallery;
  int64_t* best_frame;
  float* best_m;
  double* best_lm;
  int64_t* best_rec;
};

constexpr int kBestThreads = 256, kBestChunk = kBestThreads * 16;  // bytes a workgroup copies per trip

// The quality of slot `slot` as the header states it, one float64 operation per line (flm_best_dev.h holds the terms
// flm_track_views_update shares); *eligible says whether it counts.
__device__ __forceinline__ double best_quality(const BestArgs& g, int slot, bool* eligible) {
  const BestTerms t = best_terms(g.rec + (size_t)slot * FLM_QUALITY_REC, g.lm + (size_t)slot * g.c * g.lm_stride,
                                 g.lm_stride, g.wt ? g.wt + (size_t)slot * g.c * g.w_stride : nullptr, g.w_stride, g.c,
                                 g.sharp_ref);
  const double f = g.factor ? g.factor[slot] : 1.0;
  const double q = t.sew * f;
  *eligible = (!g.status || g.status[slot] == 0) && t.n_lap > 0 && t.e >= g.min_exposed && q >= 0.0;  // (q >= 0: no NaN)
  return q;
}

// The body track_best_kernel and track_best_rows_kernel share: `slot` is the ROW the faces, records, landmarks, status,
// reset, factor, matrices and best_q_in are read at, `gs` the SLOT best_q_out, the gallery and the other outputs are
// written at (track_best_kernel: the same number).
__device__ __forceinline__ void track_best_body(const BestArgs& g, int slot, size_t gs) {
  __shared__ int s_taken;
  const int tid = threadIdx.x;
  if (tid == 0) {
    bool eligible;
    const double q = best_quality(g, slot, &eligible);
    const double prev = (g.reset && g.reset[slot] != 0) ? -1.0 : g.best_q_in[slot];
    const bool taken = eligible && q > prev;
    s_taken = taken;
    if (blockIdx.x == 0) g.best_q_out[gs] = taken ? q : prev;
  }
  __syncthreads();
  if (!s_taken) return;

  if (blockIdx.x == 0) {  // the slot's scalars
    if (tid == 0) g.best_frame[gs] = g.frame_id;
    if (g.best_m && tid < 6) g.best_m[gs * 6 + tid] = g.m[(size_t)slot * 6 + tid];
    if (g.best_rec && tid >= 64 && tid < 64 + FLM_QUALITY_REC)
      g.best_rec[gs * FLM_QUALITY_REC + (tid - 64)] = g.rec[(size_t)slot * FLM_QUALITY_REC + (tid - 64)];
    if (g.best_lm) {
      const double* lm = g.lm + (size_t)slot * g.c * g.lm_stride;
      double* o = g.best_lm + gs * g.c * 2;
      for (int i = tid; i < 2 * g.c; i += kBestThreads) o[i] = lm[(size_t)(i >> 1) * g.lm_stride + (i & 1)];
    }
  }

  // the face: pieces of 16 bytes at the 16-byte lines of the SOURCE address (flm_copy_dev.h)
  copy_row_bytes(g.faces + (size_t)slot * g.face_bytes, g.gallery + gs * g.face_bytes, g.face_bytes,
                 (size_t)blockIdx.x * kBestThreads + tid, (size_t)gridDim.x * kBestThreads);
}

__global__ __launch_bounds__(kBestThreads) void track_best_kernel(const BestArgs g) {
  track_best_body(g, blockIdx.y, blockIdx.y);
}

// best_q_in is the SNAPSHOT of the rows (nobody writes it), best_q_out the tracker's own tensor, written at the slot.
__global__ __launch_bounds__(kBestThreads) void track_best_rows_kernel(const BestArgs g, const int32_t* __restrict__ slot,
                                                                       int n_slots) {
  const int gs = slot[blockIdx.y];
  if (gs < 0 || gs >= n_slots) return;  // an inert row: the whole workgroup leaves
  track_best_body(g, blockIdx.y, (size_t)gs);
}

// Pointers, options and overlaps are checked by the caller in flm_api.hip.
// slot == null: flm_track_best_update (k slots, row == slot); else flm_track_best_update_rows (k rows).
int launch_track_best_update(hipStream_t s, const void* faces, size_t face_bytes, int k, const int64_t* rec,
                             const int32_t* status, const int32_t* reset, const double* lm, size_t lm_stride,
                             const double* wt, size_t w_stride, int c, const double* factor, const float* m,
                             int64_t frame_id, const flm_best_opts* opts, const int32_t* slot, int n_slots,
                             const double* best_q_in, double* best_q_out, void* gallery, int64_t* best_frame, float* best_m,
                             double* best_lm, int64_t* best_rec) {
  BestArgs g;
  g.faces = static_cast<const unsigned char*>(faces);
  g.face_bytes = face_bytes;
  g.rec = rec; g.status = status; g.reset = reset;
  g.lm = lm; g.lm_stride = lm_stride; g.wt = wt; g.w_stride = w_stride; g.c = c;
  g.factor = factor; g.m = m; g.frame_id = frame_id;
  g.sharp_ref = opts->sharp_ref; g.min_exposed = opts->min_exposed;
  g.best_q_in = best_q_in; g.best_q_out = best_q_out;
  g.gallery = static_cast<unsigned char*>(gallery);
  g.best_frame = best_frame; g.best_m = best_m; g.best_lm = best_lm; g.best_rec = best_rec;
  size_t chunks = (face_bytes + 15 + kBestChunk - 1) / kBestChunk;  // (+15: the lead-in of an unaligned face)
  if (chunks > 1024) chunks = 1024;
  if (slot) {
    track_best_rows_kernel<<<dim3((unsigned)chunks, k), kBestThreads, 0, s>>>(g, slot, n_slots);
    FLM_LAUNCH_CHECK("track_best_rows_kernel");
  } else {
    track_best_kernel<<<dim3((unsigned)chunks, k), kBestThreads, 0, s>>>(g);
    FLM_LAUNCH_CHECK("track_best_kernel");
  }
  return FLM_OK;
}

}  // namespace flm
