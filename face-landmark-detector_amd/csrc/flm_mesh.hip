// Shape-normalised faces: the piecewise-affine warp over the landmark mesh (flm_mesh_map, flm_mesh_affines,
// flm_warp_mesh_frames).  include/flm.h states the contract; flm_mesh_dev.h holds the mesh arithmetic (shared with the
// host sweep of tests/native/mesh_host.cpp), flm_warp_sample_dev.h / flm_nv12_dev.h the sampling and
// flm_warp_store_dev.h the store, all three unchanged: a pixel of triangle t has the bits that
// flm_warp_affine_frames_src stores when its matrix is aff[f][t].
//
// Shape of the warp kernel: the pixel list of warp_fmt_u8_kernel / warp_nv12_kernel -- blockIdx.y is the face, a
// thread holds UNR pixels x S*S samples, a wave's 64 lanes hold 64 consecutive pixels, every gather of a thread is
// issued before the first is consumed -- with two differences.
//   * The prologue.  Thread t < T solves triangle t of the face in float64 (mesh_face_affine, up to eight divisions),
//     applies warp_inverse to the float32 result and leaves the six floats in LDS (6 KiB at T = 255).  The map bytes of
//     the workgroup's first trip are loaded before it, so that their latency lies under the solves; the first gathers
//     need an inverse and wait for the barrier.  Every workgroup of a face repeats the prologue, so the launcher gives a
//     workgroup several trips of the loop once there are enough workgroups to fill the chip without that.
//   * The matrix is per pixel: the triangle index comes from the map byte at the pixel's centre and is used for all
//     its sub-samples; the six floats come from LDS into vector registers (6 x UNR more than the per-face kernels hold).
//     A map byte >= T (255 = no triangle) stores v = 0 through the format's epilogue; its gathers go to triangle 0's
//     matrix and are discarded.  Whatever a matrix holds, warp_position clamps the source position into the frame.
#include <atomic>

#include "flm_mesh_dev.h"
#include "flm_nv12_dev.h"
#include "flm_warp_sample_dev.h"
#include "flm_warp_store_dev.h"

namespace flm {

// ---- flm_mesh_map: one thread per output pixel, the triangles in index order ----------------------------------------
__global__ __launch_bounds__(256) void mesh_map_kernel(const double* __restrict__ pts, const int32_t* __restrict__ tris,
                                                       int p, int t, int hd, int wd, uint8_t* __restrict__ map) {
  const int npix = hd * wd;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += gridDim.x * blockDim.x) {
    const int y = i / wd;
    map[i] = (uint8_t)mesh_locate(pts, tris, p, t, (double)(i - y * wd), (double)y);
  }
}

// ---- flm_mesh_affines: one thread per (face, triangle) ---------------------------------------------------------------
__global__ __launch_bounds__(256) void mesh_affines_kernel(const double* __restrict__ lm, int lm_stride,
                                                           const float* __restrict__ m, const double* __restrict__ pts,
                                                           const int32_t* __restrict__ tris, int p, int a, int t,
                                                           double min_det, float* __restrict__ aff) {
  const int f = blockIdx.y;
  const int i = threadIdx.x;
  if (i >= t) return;
  float o[6];
  mesh_face_affine(lm + (size_t)f * (p - a) * lm_stride, lm_stride, m + (size_t)f * 6, pts, tris + 3 * i, p, a, min_det, o);
  float* d = aff + ((size_t)f * t + i) * 6;
#pragma unroll
  for (int j = 0; j < 6; ++j) d[j] = o[j];
}

// ---- flm_warp_mesh_frames ----------------------------------------------------------------------------------------------
struct MeshArgs {
  const double* lm;
  int lm_stride;
  const float* m;
  const double* pts;
  const int32_t* tris;
  int p, a, t;
  const uint8_t* map;
  double min_det;
  float* aff_out;
};

template <bool NV12> struct MeshTaps { typedef WarpTapsU8 T; };
template <> struct MeshTaps<true> { typedef Nv12Taps T; };

// g.fh, g.fw: the frame, for both sources; the pitches and kc are read by the NV12 kernels alone.
template <bool NV12, int S, int UNR, int LAYOUT, int TYPE>
__global__ __launch_bounds__(256, 4) void warp_mesh_kernel(const uint8_t* __restrict__ frames, size_t frame_stride,
                                                           int nframes, Nv12Geom g, Nv12Coef kc,
                                                           const int32_t* __restrict__ frame_idx,
                                                           const int32_t* __restrict__ boxes, MeshArgs ma,
                                                           typename Pix<TYPE>::T* __restrict__ dst, int hd, int wd,
                                                           FmtArgs a) {
  typedef typename MeshTaps<NV12>::T Taps;
  constexpr int NS = S * S;
  constexpr int NQ = (NV12 && NS > 8) ? 8 : NS;  // samples gathered together (warp_nv12_kernel says why)
  __shared__ __attribute__((aligned(16))) unsigned char stage[4][192 * sizeof(typename Pix<TYPE>::T)];
  __shared__ float inv_s[kMeshMaxTris * 6];
  const int f = blockIdx.y;
  const int npix = hd * wd;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int fi = frame_idx ? frame_idx[f] : 0;
  bool zero = (unsigned)fi >= (unsigned)nframes;  // a slot outside the ring
  if (boxes) {                                    // a clipped box without pixels
    const int cx0 = min(max(boxes[4 * f + 0], 0), g.fw), cy0 = min(max(boxes[4 * f + 1], 0), g.fh);
    const int cx1 = min(max(boxes[4 * f + 2], 0), g.fw), cy1 = min(max(boxes[4 * f + 3], 0), g.fh);
    zero = zero || cx1 - cx0 <= 0 || cy1 - cy0 <= 0;
  }
  const int pend = (npix + 63) & ~63;  // whole waves run the loop together (the staging needs every lane's pixel)
  const int stride = gridDim.x * blockDim.x;
  const int pfirst = blockIdx.x * blockDim.x + threadIdx.x;
  // the map bytes of the first trip go out before the solves (a pixel past the face reads the last pixel's byte)
  int tri[UNR];
#pragma unroll
  for (int k = 0; k < UNR; ++k) tri[k] = ma.map[min(pfirst + k * stride, npix - 1)];

  // the prologue: triangle threadIdx.x of this face.  A zero face has no pixels to warp; its matrices are still owed
  // to aff_out, by the first workgroup of the face as for any other.
  const bool want_aff = ma.aff_out != nullptr && blockIdx.x == 0;
  if ((int)threadIdx.x < ma.t && (!zero || want_aff)) {
    const int t = threadIdx.x;
    float aff[6];
    mesh_face_affine(ma.lm + (size_t)f * (ma.p - ma.a) * ma.lm_stride, ma.lm_stride, ma.m + (size_t)f * 6, ma.pts,
                     ma.tris + 3 * t, ma.p, ma.a, ma.min_det, aff);
    if (want_aff) {
      float* d = ma.aff_out + ((size_t)f * ma.t + t) * 6;
#pragma unroll
      for (int j = 0; j < 6; ++j) d[j] = aff[j];
    }
    const WarpInverse w = warp_inverse(aff);
    float* o = inv_s + 6 * t;
    o[0] = w.i00; o[1] = w.i01; o[2] = w.i02; o[3] = w.i10; o[4] = w.i11; o[5] = w.i12;
  }
  if (zero) {  // (workgroup-uniform)
    store_zero_face<LAYOUT, TYPE>(dst, f, npix, a, stage[wv]);
    return;
  }
  __syncthreads();

  const uint8_t* s8 = frames + (size_t)fi * frame_stride;
  const float xmax = (float)(g.fw - 1), ymax = (float)(g.fh - 1);
  for (int p0 = pfirst; p0 < pend; p0 += UNR * stride) {
    if (p0 != pfirst) {
#pragma unroll
      for (int k = 0; k < UNR; ++k) tri[k] = ma.map[min(p0 + k * stride, npix - 1)];
    }
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
        const float* iv = inv_s + 6 * (tri[k] < ma.t ? tri[k] : 0);
        WarpInverse inv;
        inv.i00 = iv[0]; inv.i01 = iv[1]; inv.i02 = iv[2]; inv.i10 = iv[3]; inv.i11 = iv[4]; inv.i12 = iv[5];
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
      const bool hole = tri[k] >= ma.t;  // no triangle: the value of a zero face
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        if (S > 1) o3[k][c] *= 1.0f / (float)NS;
        o3[k][c] = hole ? 0.f : o3[k][c];
      }
      // (the lane index is handed over opaque for the reason warp_fmt_u8_kernel gives: the store offsets are worked out
      // here instead of being held in registers across the gathers)
      int ln = lane;
      asm volatile("" : "+v"(ln));
      store_pixel<LAYOUT, TYPE>(dst, f, npix, p - lane, ln, p < npix, o3[k], a, stage[wv]);
    }
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------------
static int check_mesh_sizes(const char* who, int p, int a, int t) {
  if (t < 1 || t > kMeshMaxTris) {
    set_error("%s: t=%d outside 1 <= t <= 255", who, t);
    return FLM_ERR_ARG;
  }
  if (p < 3 || p > kMeshMaxPoints) {
    set_error("%s: p=%d outside 3 <= p <= 256", who, p);
    return FLM_ERR_ARG;
  }
  if (a < 0 || a > p) {
    set_error("%s: a=%d outside 0 <= a <= p = %d", who, a, p);
    return FLM_ERR_ARG;
  }
  return FLM_OK;
}

static int check_mesh_solve(const char* who, int lm_stride, double min_det) {
  if (lm_stride < 2) {
    set_error("%s: lm_stride=%d, needs lm_stride >= 2", who, lm_stride);
    return FLM_ERR_ARG;
  }
  if (!(min_det >= 0.0)) {
    set_error("%s: min_det=%g, needs min_det >= 0", who, min_det);
    return FLM_ERR_ARG;
  }
  return FLM_OK;
}

int launch_mesh_map(hipStream_t s, const double* pts, const int32_t* tris, int p, int t, int hd, int wd, uint8_t* map) {
  if (const int rc = check_mesh_sizes("mesh_map", p, 0, t)) return rc;
  if (hd < 1 || wd < 1 || (long long)hd * wd * 12 >= (1ll << 31)) {
    set_error("mesh_map: aligned size %dx%d, needs hd, wd >= 1 and hd*wd*3*4 < 2^31", hd, wd);
    return FLM_ERR_SHAPE;
  }
  int bx = cdiv(hd * wd, 256);
  if (bx > 4096) bx = 4096;
  mesh_map_kernel<<<dim3(bx), 256, 0, s>>>(pts, tris, p, t, hd, wd, map);
  FLM_LAUNCH_CHECK("mesh_map_kernel");
  return FLM_OK;
}

int launch_mesh_affines(hipStream_t s, const double* lm, int lm_stride, const float* m, const double* pts,
                        const int32_t* tris, int p, int a, int t, int k, double min_det, float* aff) {
  if (const int rc = check_mesh_sizes("mesh_affines", p, a, t)) return rc;
  if (const int rc = check_mesh_solve("mesh_affines", lm_stride, min_det)) return rc;
  if (k < 1 || k > 65535) {
    set_error("mesh_affines: k=%d outside 1 <= k <= 65535", k);
    return FLM_ERR_SHAPE;
  }
  mesh_affines_kernel<<<dim3(1, k), 256, 0, s>>>(lm, lm_stride, m, pts, tris, p, a, t, min_det, aff);
  FLM_LAUNCH_CHECK("mesh_affines_kernel");
  return FLM_OK;
}

template <bool NV12, int S, int UNR>
static void launch_mesh(hipStream_t s, dim3 grid, const uint8_t* frames, size_t frame_stride, int nframes,
                        const Nv12Geom& g, const Nv12Coef& kc, const int32_t* frame_idx, const int32_t* boxes,
                        const MeshArgs& ma, void* dst, int hd, int wd, const flm_image_format* fmt) {
  const FmtArgs a = fmt_args(fmt);
#define FLM_CALL(L, P)                                                                                             \
  warp_mesh_kernel<NV12, S, UNR, L, P><<<grid, 256, 0, s>>>(frames, frame_stride, nframes, g, kc, frame_idx, boxes, \
                                                            ma, static_cast<typename Pix<P>::T*>(dst), hd, wd, a)
  FMT_DISPATCH(FLM_CALL);
#undef FLM_CALL
}

// Workgroups along a face: one per trip of the pixel loop while the launch has fewer workgroups than the chip holds at
// once -- its CUs x the four workgroups of four waves that the kernels' register bound (__launch_bounds__(256, 4)) lets
// a CU hold, 1024 on 256 CUs -- and as many trips per workgroup beyond that as keep the launch at that many: every
// workgroup of a face repeats the face's prologue, and once the chip is full a repeat buys nothing
// (profiles/mesh_workgroups_ab.json: one workgroup per face is the fastest form at 1024 faces).
constexpr int kMeshGroupsPerCu = 4;
static int mesh_fill_groups() {
  static std::atomic<int> cached{0};  // per process: the devices of one process are alike
  int v = cached.load(std::memory_order_relaxed);
  if (v > 0) return v;
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1) {
    (void)hipGetLastError();
    return 256 * kMeshGroupsPerCu;  // (not cached: asked again by the next call)
  }
  v = cus * kMeshGroupsPerCu;
  cached.store(v, std::memory_order_relaxed);
  return v;
}

// The image format (the default one for a NULL fmt) and the frame format's struct_size, pixel and matrix have been
// checked by the caller (flm_api.hip).
int launch_warp_mesh_frames(hipStream_t s, const uint8_t* frames, size_t frame_stride, int nframes, int fh, int fw,
                            const int32_t* frame_idx, const int32_t* boxes, const double* lm, int lm_stride,
                            const float* m, const double* pts, const int32_t* tris, int p, int a, int t,
                            const uint8_t* map, int k, void* dst, int hd, int wd, int samples,
                            const flm_image_format* fmt, const flm_frame_format* src, double min_det, float* aff_out) {
  const char* who = "warp_mesh_frames";
  if (samples != 1 && samples != 2 && samples != 4) {
    set_error("%s: samples=%d (must be 1, 2 or 4)", who, samples);
    return FLM_ERR_ARG;
  }
  if (const int rc = check_mesh_sizes(who, p, a, t)) return rc;
  if (const int rc = check_mesh_solve(who, lm_stride, min_det)) return rc;
  if (k < 1 || k > 65535) {
    set_error("%s: k=%d outside 1 <= k <= 65535", who, k);
    return FLM_ERR_SHAPE;
  }
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
  if (hd < 1 || wd < 1 || (long long)hd * wd * 12 >= (1ll << 31)) {
    set_error("%s: aligned size %dx%d, needs hd, wd >= 1 and hd*wd*3*4 < 2^31", who, hd, wd);
    return FLM_ERR_SHAPE;
  }
  const MeshArgs ma{lm, lm_stride, m, pts, tris, p, a, t, map, min_det, aff_out};
  const int unr = samples == 1 ? 4 : samples == 2 ? 2 : 1;  // pixels per thread and loop trip
  int bx = cdiv(hd * wd, 256 * unr);
  if (bx > 1024) bx = 1024;
  long long trips = (long long)k * bx / mesh_fill_groups();
  trips = trips < 1 ? 1 : trips > bx ? bx : trips;
  bx = cdiv(bx, (int)trips);
  const dim3 grid(bx, k);
#define FLM_MESH(NV)                                                                                                    \
  do {                                                                                                                  \
    if (samples == 1) launch_mesh<NV, 1, 4>(s, grid, frames, frame_stride, nframes, g, kc, frame_idx, boxes, ma, dst, hd, wd, fmt); \
    else if (samples == 2) launch_mesh<NV, 2, 2>(s, grid, frames, frame_stride, nframes, g, kc, frame_idx, boxes, ma, dst, hd, wd, fmt); \
    else launch_mesh<NV, 4, 1>(s, grid, frames, frame_stride, nframes, g, kc, frame_idx, boxes, ma, dst, hd, wd, fmt);  \
  } while (0)
  if (nv12) FLM_MESH(true);
  else FLM_MESH(false);
#undef FLM_MESH
  FLM_LAUNCH_CHECK("warp_mesh_kernel");
  return FLM_OK;
}

}  // namespace flm
