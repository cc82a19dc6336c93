// The alignment warps with the output format in the epilogue (flm_warp_affine_fmt, flm_warp_affine_frames_fmt): the
// value a warp writes as float32 NHWC BGR goes, while it is still in a register, through
//   t = v * scale[c];  u = t + bias[c]          (two float32 operations, two roundings: -ffp-contract=off)
// with v taken from source channel c or 2-c, is rounded to the pixel type and lands in NHWC or NCHW -- one store of a
// half or a quarter of the bytes instead of a float32 face followed by permute, flip, mul, add and cast.
// include/flm.h states the contract operation by operation; flm_warp_sample_dev.h holds the sampling.
//
// Shape of the kernels: the pixel list of warp_u8_kernel / warp_frames_kernel.  blockIdx.y is the face, a thread holds
// UNR pixels x S*S samples (4 x 1, 2 x 4, 1 x 16) and issues every gather before it consumes the first; a wave's 64
// lanes hold 64 CONSECUTIVE pixels of the face, and whole waves run the loop together.
//
// Store shapes.  Those 64 pixels are 192 consecutive elements in NHWC and 64 consecutive elements of each of the three
// planes in NCHW.  The converted elements go through a per-wave LDS line laid out as the destination is, and leave as
// non-temporal 16-byte stores (the written faces are read by a later launch, not by this one: see store_stream16 in
// flm_misc.hip):
//              bytes per wave   lanes storing 16 B        LDS line
//   f32   NHWC      768              48                   [64][3] float
//   f32   NCHW    3 x 256          3 x 16                 [3][64] float
//   16bit NHWC      384              24                   [64][3] half
//   16bit NCHW    3 x 128          3 x 8                  [3][64] half
//   u8    NHWC      192              12                   [64][3] byte
//   u8    NCHW    3 x 64           3 x 4                  [3][64] byte
// Whether a run of elements may leave as 16-byte stores is decided from its ADDRESS, per wave (NHWC) or per plane
// (NCHW): a face's base is f*npix*3*esize, a plane's (3f+c)*npix*esize, and a caller may pass a slice of a larger
// buffer, so neither the format nor the size settles it.  A run that does not start on a 16-byte boundary, and the
// ragged last wave of a face, leave as element stores from the registers.  Either way a wave writes the bytes of its
// own pixels and no others.
#include "flm_warp_sample_dev.h"
#include "flm_warp_store_dev.h"

namespace flm {

// ---- uint8 sources of two columns or more: crops (source f, or frame 0) and ring frames (source frame_idx[f]) ------
// `per_face`: without frame_idx, face f reads source f (flm_warp_affine_fmt) instead of source 0.
// Four waves per SIMD (128 registers at the most) is stated to the compiler: left alone it spends up to 156 on some
// (layout, type) pairs of the 4 x 4 grid, whose 64 gathered dwords per pixel are the bulk of that either way.
template <int S, int UNR, int LAYOUT, int TYPE>
__global__ __launch_bounds__(256, 4) void warp_fmt_u8_kernel(const uint8_t* __restrict__ src, size_t src_stride, int nsrc,
                                                          int hs, int ws, const int32_t* __restrict__ frame_idx,
                                                          int per_face, const int32_t* __restrict__ boxes,
                                                          const float* __restrict__ m,
                                                          typename Pix<TYPE>::T* __restrict__ dst, int hd, int wd,
                                                          FmtArgs a) {
  constexpr int NS = S * S;
  __shared__ __attribute__((aligned(16))) unsigned char stage[4][192 * sizeof(typename Pix<TYPE>::T)];
  const int f = blockIdx.y;
  const int npix = hd * wd;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int fi = frame_idx ? frame_idx[f] : per_face ? f : 0;
  bool zero = (unsigned)fi >= (unsigned)nsrc;  // a slot outside the ring
  if (boxes) {                                 // a clipped box without pixels
    const int cx0 = min(max(boxes[4 * f + 0], 0), ws), cy0 = min(max(boxes[4 * f + 1], 0), hs);
    const int cx1 = min(max(boxes[4 * f + 2], 0), ws), cy1 = min(max(boxes[4 * f + 3], 0), hs);
    zero = zero || cx1 - cx0 <= 0 || cy1 - cy0 <= 0;
  }
  if (zero) {  // (workgroup-uniform)
    store_zero_face<LAYOUT, TYPE>(dst, f, npix, a, stage[wv]);
    return;
  }
  const uint8_t* s8 = src + (size_t)fi * src_stride;
  const WarpInverse inv = warp_inverse(m + (size_t)f * 6);
  const int pend = (npix + 63) & ~63;  // whole waves run the loop together (the staging needs every lane's pixel)
  const int stride = gridDim.x * blockDim.x;
  for (int p0 = blockIdx.x * blockDim.x + threadIdx.x; p0 < pend; p0 += UNR * stride) {
    WarpTapsU8 taps[UNR][NS];
#pragma unroll
    for (int k = 0; k < UNR; ++k) {
      const int p = p0 + k * stride;
      const int pc = p < npix ? p : npix - 1;  // a pixel past the face is computed from the clamped index, never stored
      const int py = pc / wd;
      const float x = (float)(pc - py * wd), y = (float)py;
#pragma unroll
      for (int q = 0; q < NS; ++q) {
        float xd, yd;
        warp_subsample<S>(x, y, q, xd, yd);
        warp_gather_u8(s8, hs, ws, inv, xd, yd, taps[k][q]);
        // the 4 x 4 grid: a sample's four loads go out before the next sample's position is worked out, so that the
        // offsets of many samples are not alive at once beside the 64 dwords in flight (nothing is waited for here)
        if (S == 4) __builtin_amdgcn_sched_barrier(0);
      }
    }
    // every gather above is issued before the first is consumed below (warp_frames_kernel says what happens otherwise)
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int k = 0; k < UNR; ++k) {
      const int p = p0 + k * stride;
      float o3[3];
#pragma unroll
      for (int q = 0; q < NS; ++q) {
        float v[3];
        warp_blend_u8(taps[k][q], v);
#pragma unroll
        for (int c = 0; c < 3; ++c) o3[c] = q == 0 ? v[c] : o3[c] + v[c];
      }
      if (S > 1) {
#pragma unroll
        for (int c = 0; c < 3; ++c) o3[c] *= 1.0f / (float)NS;
      }
      // (no branch around this for a wave past the face, whose lanes are all dead: the compiler would sink the
      // gathers and the blend into it, past the barrier above)
      // The lane index is handed over opaque, so that the store offsets derived from it (LDS line, 16-byte run, element
      // run) are worked out here, a handful of integer operations, instead of being hoisted out of the loop and held in
      // registers across the gathers: with the 64 dwords of the 4 x 4 grid in flight that was a private segment.
      int ln = lane;
      asm volatile("" : "+v"(ln));
      store_pixel<LAYOUT, TYPE>(dst, f, npix, p - lane, ln, p < npix, o3, a, stage[wv]);
    }
  }
}

// ---- float32 crops, and uint8 crops of a single column: one pixel per thread and trip, as warp_kernel -------------
template <bool U8, int LAYOUT, int TYPE>
__global__ __launch_bounds__(256) void warp_fmt_any_kernel(const void* __restrict__ src, int hs, int ws,
                                                           const float* __restrict__ m,
                                                           typename Pix<TYPE>::T* __restrict__ dst, int hd, int wd,
                                                           FmtArgs a) {
  __shared__ __attribute__((aligned(16))) unsigned char stage[4][192 * sizeof(typename Pix<TYPE>::T)];
  const int f = blockIdx.y;
  const int npix = hd * wd;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const WarpInverse inv = warp_inverse(m + (size_t)f * 6);
  const void* sface = U8 ? static_cast<const void*>(static_cast<const uint8_t*>(src) + (size_t)f * hs * ws * 3)
                         : static_cast<const void*>(static_cast<const float*>(src) + (size_t)f * hs * ws * 3);
  const int pend = (npix + 63) & ~63;
  for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < pend; p += gridDim.x * blockDim.x) {
    const int pc = p < npix ? p : npix - 1;
    const int py = pc / wd;
    float o3[3];
    warp_sample_any<U8>(sface, hs, ws, inv, (float)(pc - py * wd), (float)py, o3);
    store_pixel<LAYOUT, TYPE>(dst, f, npix, p - lane, lane, p < npix, o3, a, stage[wv]);
  }
}

template <int S, int UNR>
static void launch_u8(hipStream_t s, dim3 grid, const uint8_t* src, size_t src_stride, int nsrc, int hs, int ws,
               const int32_t* frame_idx, int per_face, const int32_t* boxes, const float* m, void* dst, int hd, int wd,
               const flm_image_format* fmt) {
  const FmtArgs a = fmt_args(fmt);
#define FLM_CALL(L, P)                                                                                               \
  warp_fmt_u8_kernel<S, UNR, L, P><<<grid, 256, 0, s>>>(src, src_stride, nsrc, hs, ws, frame_idx, per_face, boxes, m, \
                                                        static_cast<typename Pix<P>::T*>(dst), hd, wd, a)
  FMT_DISPATCH(FLM_CALL);
#undef FLM_CALL
}

template <bool U8>
static void launch_any(hipStream_t s, dim3 grid, const void* src, int hs, int ws, const float* m, void* dst, int hd, int wd,
                const flm_image_format* fmt) {
  const FmtArgs a = fmt_args(fmt);
#define FLM_CALL(L, P) \
  warp_fmt_any_kernel<U8, L, P><<<grid, 256, 0, s>>>(src, hs, ws, m, static_cast<typename Pix<P>::T*>(dst), hd, wd, a)
  FMT_DISPATCH(FLM_CALL);
#undef FLM_CALL
}

// The format itself (struct_size, enums, finite scale and bias) is checked by the caller in flm_api.hip.
int launch_warp_fmt(hipStream_t s, const void* src, int src_is_u8, int n, int hs, int ws, const float* m, void* dst, int hd,
                    int wd, const flm_image_format* fmt) {
  if (n < 1 || n > 65535) {
    set_error("warp_affine_fmt: n=%d outside 1 <= n <= 65535", n);
    return FLM_ERR_SHAPE;
  }
  if (hs < 1 || ws < 1 || (long long)hs * ws * 12 >= (1ll << 31)) {
    set_error("warp_affine_fmt: source %dx%d, needs hs, ws >= 1 and hs*ws*3*4 < 2^31", hs, ws);
    return FLM_ERR_SHAPE;
  }
  if (hd < 1 || wd < 1 || (long long)hd * wd * 12 >= (1ll << 31)) {
    set_error("warp_affine_fmt: aligned size %dx%d, needs hd, wd >= 1 and hd*wd*3*4 < 2^31", hd, wd);
    return FLM_ERR_SHAPE;
  }
  if (src_is_u8 && ws >= 2) {
    int bx = cdiv(hd * wd, 256 * 4);
    if (bx > 1024) bx = 1024;
    launch_u8<1, 4>(s, dim3(bx, n), static_cast<const uint8_t*>(src), (size_t)hs * ws * 3, n, hs, ws, nullptr, 1, nullptr, m,
                    dst, hd, wd, fmt);
    FLM_LAUNCH_CHECK("warp_fmt_u8_kernel");
    return FLM_OK;
  }
  int bx = cdiv(hd * wd, 256 * 2);  // two trips per thread, as warp_kernel
  if (bx > 1024) bx = 1024;
  if (src_is_u8) launch_any<true>(s, dim3(bx, n), src, hs, ws, m, dst, hd, wd, fmt);
  else launch_any<false>(s, dim3(bx, n), src, hs, ws, m, dst, hd, wd, fmt);
  FLM_LAUNCH_CHECK("warp_fmt_any_kernel");
  return FLM_OK;
}

// The limits of a dense BGR24 ring, stated once for every launcher that reads one (here and flm_mesh.hip); `who` names
// the call in the message.
int bgr_ring_check(const char* who, size_t frame_stride, int nframes, int fh, int fw) {
  if (nframes < 1) {
    set_error("%s: nframes=%d, needs nframes >= 1", who, nframes);
    return FLM_ERR_SHAPE;
  }
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
  return FLM_OK;
}

int launch_warp_frames_fmt(hipStream_t s, const uint8_t* frames, size_t frame_stride, int nframes, int fh, int fw,
                           const int32_t* frame_idx, const int32_t* boxes, const float* m, int k, void* dst, int hd,
                           int wd, int samples, const flm_image_format* fmt) {
  if (samples != 1 && samples != 2 && samples != 4) {
    set_error("warp_affine_frames_fmt: samples=%d (must be 1, 2 or 4)", samples);
    return FLM_ERR_ARG;
  }
  if (k < 1 || k > 65535) {
    set_error("warp_affine_frames_fmt: k=%d outside 1 <= k <= 65535", k);
    return FLM_ERR_SHAPE;
  }
  if (const int rc = bgr_ring_check("warp_affine_frames_fmt", frame_stride, nframes, fh, fw)) return rc;
  if (hd < 1 || wd < 1 || (long long)hd * wd * 12 >= (1ll << 31)) {
    set_error("warp_affine_frames_fmt: aligned size %dx%d, needs hd, wd >= 1 and hd*wd*3*4 < 2^31", hd, wd);
    return FLM_ERR_SHAPE;
  }
  const int unr = samples == 1 ? 4 : samples == 2 ? 2 : 1;  // pixels per thread and loop trip
  int bx = cdiv(hd * wd, 256 * unr);
  if (bx > 1024) bx = 1024;
  const dim3 grid(bx, k);
  if (samples == 1) launch_u8<1, 4>(s, grid, frames, frame_stride, nframes, fh, fw, frame_idx, 0, boxes, m, dst, hd, wd, fmt);
  else if (samples == 2) launch_u8<2, 2>(s, grid, frames, frame_stride, nframes, fh, fw, frame_idx, 0, boxes, m, dst, hd, wd, fmt);
  else launch_u8<4, 1>(s, grid, frames, frame_stride, nframes, fh, fw, frame_idx, 0, boxes, m, dst, hd, wd, fmt);
  FLM_LAUNCH_CHECK("warp_fmt_u8_kernel");
  return FLM_OK;
}

}  // namespace flm
