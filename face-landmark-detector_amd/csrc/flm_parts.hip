// Face parts on the device: flm_part_affines, flm_warp_parts_frames (eye and mouth patches under a similarity of the
// part's own landmarks) and flm_face_openness (aspect ratios and a closure count).  include/flm.h states the contract;
// flm_parts_dev.h holds the float64 arithmetic (shared with the host program tests/native/parts_host.cpp),
// flm_warp_sample_dev.h / flm_nv12_dev.h the sampling and flm_warp_store_dev.h the store, all three unchanged: a pixel of
// patch (f, r) has the bits flm_warp_affine_frames_src stores when its matrix is aff[f][r].
//
// Shape of the warp kernel: ONE workgroup per (face, part) -- blockIdx.z the face, blockIdx.y the part, gridDim.x = 1 --
// that walks the whole patch with the pixel loop of warp_fmt_u8_kernel / warp_nv12_kernel (a thread holds UNR pixels x
// S*S samples, a wave's 64 lanes hold 64 consecutive pixels, every gather of a thread issued before the first is
// consumed).  The prologue is the fit: the part's entries are staged in LDS by the first part_n threads, thread 0 runs
// part_fit's two sequential passes and leaves the float32 matrix and ok in LDS.  Because the workgroup is the only one of
// its (face, part), the float64 fit runs once, not once per strip of the patch (the mesh warp lost half of its excess
// to a prologue that every workgroup of a face repeated).  A patch is at most 256 x 256, 64 trips of the UNR = 4 loop.
#include "flm_nv12_dev.h"
#include "flm_parts_dev.h"
#include "flm_warp_sample_dev.h"
#include "flm_warp_store_dev.h"

namespace flm {

struct PartArgs {
  const double* lm;
  size_t lm_stride;
  const double* wt;  // or null
  size_t w_stride;
  int c, r;
  const int32_t* idx;   // [R,32]
  const double* tmpl;   // [R,32,2]
  int n[FLM_PARTS_MAX];  // entries per part
  float* aff;           // [K,R,2,3] or null
  int32_t* ok;          // [K,R] or null
};

// The prologue of both kernels: stage, fit, publish.  Every thread of the workgroup calls it; returns ok, the matrix in
// m_s.  pt_s: kPartPt * FLM_PART_MAX_POINTS doubles, m_s: 6 floats, ok_s: one int, all in LDS.
__device__ __forceinline__ bool part_prologue(const PartArgs& g, int f, int r, double* pt_s, float* m_s, int* ok_s) {
  const int n = g.n[r];
  if ((int)threadIdx.x < n) {
    const int i = threadIdx.x;
    part_stage(pt_s + kPartPt * i, g.lm, g.lm_stride, g.wt, g.w_stride, (size_t)f, g.c,
               g.idx[r * FLM_PART_MAX_POINTS + i], g.tmpl + 2 * (size_t)(r * FLM_PART_MAX_POINTS + i));
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float m[6];
    const bool ok = part_fit(pt_s, n, m);
#pragma unroll
    for (int j = 0; j < 6; ++j) m_s[j] = m[j];
    *ok_s = ok ? 1 : 0;
    const size_t e = (size_t)f * g.r + r;
    if (g.aff) {
#pragma unroll
      for (int j = 0; j < 6; ++j) g.aff[e * 6 + j] = m[j];
    }
    if (g.ok) g.ok[e] = ok ? 1 : 0;
  }
  __syncthreads();
  return *ok_s != 0;
}

// ---- flm_part_affines: a workgroup of one wave per (face, part) ----------------------------------------------------------
__global__ __launch_bounds__(64) void part_affines_kernel(const PartArgs g) {
  __shared__ double pt_s[kPartPt * FLM_PART_MAX_POINTS];
  __shared__ float m_s[6];
  __shared__ int ok_s;
  part_prologue(g, blockIdx.y, blockIdx.x, pt_s, m_s, &ok_s);
}

// ---- flm_warp_parts_frames --------------------------------------------------------------------------------------------
template <bool NV12> struct PartTaps { typedef WarpTapsU8 T; };
template <> struct PartTaps<true> { typedef Nv12Taps T; };

// g.fh, g.fw: the frame, for both sources; the pitches and kc are read by the NV12 kernels alone.
template <bool NV12, int S, int UNR, int LAYOUT, int TYPE>
__global__ __launch_bounds__(256, 4) void warp_parts_kernel(const uint8_t* __restrict__ frames, size_t frame_stride,
                                                            int nframes, Nv12Geom g, Nv12Coef kc,
                                                            const int32_t* __restrict__ frame_idx,
                                                            const int32_t* __restrict__ boxes, PartArgs pa,
                                                            typename Pix<TYPE>::T* __restrict__ dst, int hd, int wd,
                                                            FmtArgs a) {
  typedef typename PartTaps<NV12>::T Taps;
  constexpr int NS = S * S;
  constexpr int NQ = (NV12 && NS > 8) ? 8 : NS;  // samples gathered together (warp_nv12_kernel says why)
  __shared__ __attribute__((aligned(16))) unsigned char stage[4][192 * sizeof(typename Pix<TYPE>::T)];
  __shared__ double pt_s[kPartPt * FLM_PART_MAX_POINTS];
  __shared__ float m_s[6];
  __shared__ int ok_s;
  const int f = blockIdx.z, r = blockIdx.y;
  const int face = f * pa.r + r;  // the patch's place in dst
  const int npix = hd * wd;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int fi = frame_idx ? frame_idx[f] : 0;
  bool zero = (unsigned)fi >= (unsigned)nframes;  // a slot outside the ring
  if (boxes) {                                    // a clipped box without pixels
    const int cx0 = min(max(boxes[4 * f + 0], 0), g.fw), cy0 = min(max(boxes[4 * f + 1], 0), g.fh);
    const int cx1 = min(max(boxes[4 * f + 2], 0), g.fw), cy1 = min(max(boxes[4 * f + 3], 0), g.fh);
    zero = zero || cx1 - cx0 <= 0 || cy1 - cy0 <= 0;
  }
  // the fit: a zero face has no pixels to warp, but its matrix and ok are still owed to the optional outputs
  bool ok = false;
  if (!zero || pa.aff != nullptr || pa.ok != nullptr) ok = part_prologue(pa, f, r, pt_s, m_s, &ok_s);
  if (zero || !ok) {  // (workgroup-uniform)
    store_zero_face<LAYOUT, TYPE>(dst, face, npix, a, stage[wv]);
    return;
  }
  const uint8_t* s8 = frames + (size_t)fi * frame_stride;
  const WarpInverse inv = warp_inverse(m_s);
  const float xmax = (float)(g.fw - 1), ymax = (float)(g.fh - 1);
  const int pend = (npix + 63) & ~63;  // whole waves run the loop together (the staging needs every lane's pixel)
  const int stride = blockDim.x;       // gridDim.x == 1
  for (int p0 = threadIdx.x; p0 < pend; p0 += UNR * stride) {
    float o3[UNR][3];
#pragma unroll
    for (int q0 = 0; q0 < NS; q0 += NQ) {
      Taps taps[UNR][NQ];
#pragma unroll
      for (int k = 0; k < UNR; ++k) {
        const int p = p0 + k * stride;
        const int pc = p < npix ? p : npix - 1;  // a pixel past the face is computed from the clamped index, never stored
        const int py = pc / wd;
        const float x = (float)(pc - py * wd), y = (float)py;
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
          float xd, yd;
          warp_subsample<S>(x, y, q0 + q, xd, yd);
          if constexpr (NV12) {
            const WarpPos wp = warp_position(inv, xd, yd, xmax, ymax);
            nv12_gather(s8, g, wp.x0, wp.y0, wp.fx, wp.fy, taps[k][q]);
          } else {
            warp_gather_u8(s8, g.fh, g.fw, inv, xd, yd, taps[k][q]);
          }
          // (as warp_fmt_u8_kernel: a sample's loads go out before the next sample's offsets are worked out)
          if (S == 4) __builtin_amdgcn_sched_barrier(0);
        }
      }
      // every gather above is issued before the first is consumed below (warp_frames_kernel says what happens otherwise)
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int k = 0; k < UNR; ++k) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
          float v[3];
          if constexpr (NV12) nv12_blend(taps[k][q], kc, v);
          else warp_blend_u8(taps[k][q], v);
#pragma unroll
          for (int c = 0; c < 3; ++c) o3[k][c] = q0 + q == 0 ? v[c] : o3[k][c] + v[c];
        }
      }
      if (NQ < NS) __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int k = 0; k < UNR; ++k) {
      const int p = p0 + k * stride;
      if (S > 1) {
#pragma unroll
        for (int c = 0; c < 3; ++c) o3[k][c] *= 1.0f / (float)NS;
      }
      // (the lane index is handed over opaque for the reason warp_fmt_u8_kernel gives: the store offsets are worked out
      // here instead of being held in registers across the gathers)
      int ln = lane;
      asm volatile("" : "+v"(ln));
      store_pixel<LAYOUT, TYPE>(dst, face, npix, p - lane, ln, p < npix, o3[k], a, stage[wv]);
    }
  }
}

// ---- flm_face_openness: one thread per row, the measures in order ------------------------------------------------------
struct OpenArgs {
  const double* lm;
  size_t lm_stride;
  const double* wt;  // or null
  size_t w_stride;
  int n, c;
  flm_open_opts o;
  const int32_t* slot;  // [N] or null
  int n_slots;
  double* rec;          // [N or n_slots,G,4]
  double* state;        // [N or n_slots,G,8] or null
  int32_t* reset;       // with state
  const double* dt_dev;  // [N] or null
  double dt;
  const int32_t* status;  // [N] or null
  int64_t frame_id;
};

__global__ __launch_bounds__(64) void face_openness_kernel(const OpenArgs g) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= g.n) return;
  size_t s = (size_t)r;
  if (g.slot) {
    const int v = g.slot[r];
    if (v < 0 || v >= g.n_slots) return;  // an inert row
    s = (size_t)v;
  }
  const int G = g.o.n_measures;
  const bool reset = g.state && g.reset[s] != 0;
  const double dt = g.dt_dev ? g.dt_dev[r] : g.dt;
  const int status = g.status ? g.status[r] : 0;
  const OpenThresholds th{g.o.close_below, g.o.open_above, g.o.min_closed, g.o.max_closed};
  for (int m = 0; m < G; ++m) {
    double rec[FLM_OPEN_REC];
    const bool ok = open_record(g.lm, g.lm_stride, g.wt, g.w_stride, (size_t)r, g.c, g.o.width[m][0], g.o.width[m][1],
                                g.o.n_pairs[m], g.o.upper[m], g.o.lower[m], g.o.min_width, rec);
    double* ro = g.rec + (s * G + m) * FLM_OPEN_REC;
#pragma unroll
    for (int i = 0; i < FLM_OPEN_REC; ++i) ro[i] = rec[i];
    if (g.state) {
      double* so = g.state + (s * G + m) * FLM_OPEN_STATE;
      double st[FLM_OPEN_STATE];
      if (reset) {
        open_state_reset(st);
      } else {
#pragma unroll
        for (int i = 0; i < FLM_OPEN_STATE; ++i) st[i] = so[i];
      }
      open_state_step(st, ok, rec[0], status, dt, th, g.frame_id);
#pragma unroll
      for (int i = 0; i < FLM_OPEN_STATE; ++i) so[i] = st[i];
    }
  }
  if (reset) g.reset[s] = 0;  // after the last measure has used the flag: the same thread, in program order
}

// ---- host side ---------------------------------------------------------------------------------------------------------
static int check_part_set(const char* who, size_t lm_stride, const double* wt, size_t w_stride, int k, int c,
                          const int32_t* part_n, int r) {
  if (r < 1 || r > FLM_PARTS_MAX) {
    set_error("%s: r=%d outside 1 <= r <= %d", who, r, FLM_PARTS_MAX);
    return FLM_ERR_ARG;
  }
  for (int i = 0; i < r; ++i)
    if (part_n[i] < 2 || part_n[i] > FLM_PART_MAX_POINTS) {
      set_error("%s: part_n[%d]=%d, a part has 2 to %d indices", who, i, part_n[i], FLM_PART_MAX_POINTS);
      return FLM_ERR_ARG;
    }
  if (lm_stride < 2 || (wt && w_stride < 1)) {
    set_error("%s: lm_stride=%zu, w_stride=%zu, needs lm_stride >= 2 and w_stride >= 1", who, lm_stride, w_stride);
    return FLM_ERR_SHAPE;
  }
  if (k < 1 || k > 65535) {
    set_error("%s: k=%d outside 1 <= k <= 65535", who, k);
    return FLM_ERR_SHAPE;
  }
  if (c < 1 || c > 1024) {
    set_error("%s: c=%d outside 1 <= c <= 1024", who, c);
    return FLM_ERR_SHAPE;
  }
  return FLM_OK;
}

static PartArgs part_args(const double* lm, size_t lm_stride, const double* wt, size_t w_stride, int c, const int32_t* idx,
                          const double* tmpl, const int32_t* part_n, int r, float* aff, int32_t* ok) {
  PartArgs g{};
  g.lm = lm; g.lm_stride = lm_stride; g.wt = wt; g.w_stride = w_stride; g.c = c; g.r = r;
  g.idx = idx; g.tmpl = tmpl; g.aff = aff; g.ok = ok;
  for (int i = 0; i < FLM_PARTS_MAX; ++i) g.n[i] = i < r ? part_n[i] : 0;
  return g;
}

// Null pointers have been checked by the caller (flm_api_image.hip).
int launch_part_affines(hipStream_t s, const double* lm, size_t lm_stride, const double* wt, size_t w_stride, int k, int c,
                        const int32_t* idx, const double* tmpl, const int32_t* part_n, int r, float* aff, int32_t* ok) {
  if (const int rc = check_part_set("part_affines", lm_stride, wt, w_stride, k, c, part_n, r)) return rc;
  part_affines_kernel<<<dim3(r, k), 64, 0, s>>>(part_args(lm, lm_stride, wt, w_stride, c, idx, tmpl, part_n, r, aff, ok));
  FLM_LAUNCH_CHECK("part_affines_kernel");
  return FLM_OK;
}

template <bool NV12, int S, int UNR>
static void launch_parts(hipStream_t s, dim3 grid, const uint8_t* frames, size_t frame_stride, int nframes,
                         const Nv12Geom& g, const Nv12Coef& kc, const int32_t* frame_idx, const int32_t* boxes,
                         const PartArgs& pa, void* dst, int hd, int wd, const flm_image_format* fmt) {
  const FmtArgs a = fmt_args(fmt);
#define FLM_CALL(L, P)                                                                                              \
  warp_parts_kernel<NV12, S, UNR, L, P><<<grid, 256, 0, s>>>(frames, frame_stride, nframes, g, kc, frame_idx, boxes, \
                                                             pa, static_cast<typename Pix<P>::T*>(dst), hd, wd, a)
  FMT_DISPATCH(FLM_CALL);
#undef FLM_CALL
}

// The image format (the default one for a NULL fmt) and the frame format's struct_size, pixel and matrix have been
// checked by the caller (flm_api_image.hip), null pointers too.
int launch_warp_parts_frames(hipStream_t s, const uint8_t* frames, size_t frame_stride, int nframes, int fh, int fw,
                             const int32_t* frame_idx, const int32_t* boxes, const double* lm, size_t lm_stride,
                             const double* wt, size_t w_stride, int c, const int32_t* idx, const double* tmpl,
                             const int32_t* part_n, int r, int k, void* dst, int ph, int pw, int samples,
                             const flm_image_format* fmt, const flm_frame_format* src, float* aff_out, int32_t* ok_out) {
  const char* who = "warp_parts_frames";
  if (samples != 1 && samples != 2 && samples != 4) {
    set_error("%s: samples=%d (must be 1, 2 or 4)", who, samples);
    return FLM_ERR_ARG;
  }
  if (const int rc = check_part_set(who, lm_stride, wt, w_stride, k, c, part_n, r)) return rc;
  Nv12Geom g{};
  Nv12Coef kc{};
  const bool nv12 = src->pixel == FLM_FRAME_NV12;
  if (nv12) {
    if (const int rc = nv12_ring_geometry(who, src, frame_stride, nframes, fh, fw, &g)) return rc;
    kc = nv12_coef(src->matrix);
  } else {  // the limits of flm_warp_affine_frames_fmt, by its own check
    if (const int rc = bgr_ring_check(who, frame_stride, nframes, fh, fw)) return rc;
    g.fh = fh;
    g.fw = fw;
  }
  if (ph < 1 || pw < 1 || ph > FLM_PART_MAX_SIDE || pw > FLM_PART_MAX_SIDE) {
    set_error("%s: patch size %dx%d, needs 1 <= ph, pw <= %d", who, ph, pw, FLM_PART_MAX_SIDE);
    return FLM_ERR_SHAPE;
  }
  const PartArgs pa = part_args(lm, lm_stride, wt, w_stride, c, idx, tmpl, part_n, r, aff_out, ok_out);
  const dim3 grid(1, r, k);  // one workgroup per (face, part)
#define FLM_PARTS(NV)                                                                                                      \
  do {                                                                                                                     \
    if (samples == 1) launch_parts<NV, 1, 4>(s, grid, frames, frame_stride, nframes, g, kc, frame_idx, boxes, pa, dst, ph, pw, fmt); \
    else if (samples == 2) launch_parts<NV, 2, 2>(s, grid, frames, frame_stride, nframes, g, kc, frame_idx, boxes, pa, dst, ph, pw, fmt); \
    else launch_parts<NV, 4, 1>(s, grid, frames, frame_stride, nframes, g, kc, frame_idx, boxes, pa, dst, ph, pw, fmt);    \
  } while (0)
  if (nv12) FLM_PARTS(true);
  else FLM_PARTS(false);
#undef FLM_PARTS
  FLM_LAUNCH_CHECK("warp_parts_kernel");
  return FLM_OK;
}

// Pointers, the option struct, sizes, strides and overlaps have been checked by the caller (flm_api_track.hip).
int launch_face_openness(hipStream_t s, const double* lm, size_t lm_stride, const double* wt, size_t w_stride, int n, int c,
                         const flm_open_opts* opts, const int32_t* slot, int n_slots, double* rec, double* state,
                         int32_t* reset, const double* dt_dev, double dt, const int32_t* status, int64_t frame_id) {
  OpenArgs g;
  g.lm = lm; g.lm_stride = lm_stride; g.wt = wt; g.w_stride = w_stride; g.n = n; g.c = c;
  g.o = *opts;
  g.slot = slot; g.n_slots = n_slots; g.rec = rec; g.state = state; g.reset = reset;
  g.dt_dev = dt_dev; g.dt = dt; g.status = status; g.frame_id = frame_id;
  face_openness_kernel<<<cdiv(n, 64), 64, 0, s>>>(g);
  FLM_LAUNCH_CHECK("face_openness_kernel");
  return FLM_OK;
}

}  // namespace flm
