// NV12 frame slots as the source of the frame-space stream: the decoder's surface (8-bit luma plane, interleaved
// half-resolution U,V plane, pitched rows) read directly by the crop / resize and by the alignment warp, and the plain
// converter to a dense BGR ring that an NV12 caller would otherwise run first.  include/flm.h states the contract
// (integer conversion, then the bits of the BGR calls on the converted frame); flm_nv12_dev.h holds the tap addressing
// and the conversion, shared with the host sweep of tests/native/nv12_taps_host.cpp.
#include "flm_nv12_dev.h"
#include "flm_resize_dev.h"
#include "flm_warp_sample_dev.h"
#include "flm_warp_store_dev.h"

namespace flm {

// ---- flm_frames_to_bgr: the plain streaming converter -----------------------------------------------------
// A thread takes 16 columns of a row PAIR, the 16 x 2 pixels under eight U,V pairs: two 16-byte luma loads, one 16-byte
// chroma load, and per row 48 output bytes as three 16-byte stores when the row segment starts on a 16-byte boundary
// of the output (always, for a 16-byte aligned ring of a width that is a multiple of 16).  A segment that ends a row
// of another width, or an unaligned output, goes pixel by pixel through nv12_tap_bgr and byte stores.  Consecutive
// threads take consecutive segments of a row pair: a wave reads 1 KiB of each plane row and writes 3 KiB per row.
__global__ __launch_bounds__(256) void frames_to_bgr_kernel(const uint8_t* __restrict__ frames, size_t frame_stride,
                                                            int nframes, Nv12Geom g, Nv12Coef kc,
                                                            uint8_t* __restrict__ out) {
  const int nseg = (g.fw + 15) >> 4, hp = g.fh >> 1;
  const long long total = (long long)nframes * hp * nseg;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int seg = (int)(i % nseg);
    const long long r = i / nseg;
    const int yp = (int)(r % hp), f = (int)(r / hp);
    const uint8_t* s = frames + (size_t)f * frame_stride;
    const int x = seg * 16, y = yp * 2;
    uint8_t* d0 = out + (((size_t)f * g.fh + y) * g.fw + x) * 3;
    uint8_t* d1 = d0 + (size_t)g.fw * 3;
    if (x + 16 <= g.fw && aligned16(d0) && aligned16(d1)) {
      uint8_t ya[16], yb[16], uv[16];
      __builtin_memcpy(ya, s + ((unsigned)y * g.y_pitch + (unsigned)x), 16);
      __builtin_memcpy(yb, s + ((unsigned)(y + 1) * g.y_pitch + (unsigned)x), 16);
      __builtin_memcpy(uv, s + (g.uv_off + (unsigned)yp * g.uv_pitch + (unsigned)x), 16);
      unsigned char o0[48], o1[48];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        int c[3], p[3];
        nv12_chroma(uv[2 * j], uv[2 * j + 1], kc, c);
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          nv12_pixel(ya[2 * j + e], c, kc, p);
          o0[6 * j + 3 * e + 0] = (unsigned char)p[0]; o0[6 * j + 3 * e + 1] = (unsigned char)p[1]; o0[6 * j + 3 * e + 2] = (unsigned char)p[2];
          nv12_pixel(yb[2 * j + e], c, kc, p);
          o1[6 * j + 3 * e + 0] = (unsigned char)p[0]; o1[6 * j + 3 * e + 1] = (unsigned char)p[1]; o1[6 * j + 3 * e + 2] = (unsigned char)p[2];
        }
      }
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        u4v v0, v1;
        __builtin_memcpy(&v0, o0 + 16 * q, 16);
        __builtin_memcpy(&v1, o1 + 16 * q, 16);
        *reinterpret_cast<u4v*>(d0 + 16 * q) = v0;
        *reinterpret_cast<u4v*>(d1 + 16 * q) = v1;
      }
    } else {
      const int n = min(16, g.fw - x);
      for (int j = 0; j < n; ++j) {
        int p[3];
        nv12_tap_bgr(s, g, kc, x + j, y, p);
        d0[3 * j + 0] = (uint8_t)p[0]; d0[3 * j + 1] = (uint8_t)p[1]; d0[3 * j + 2] = (uint8_t)p[2];
        nv12_tap_bgr(s, g, kc, x + j, y + 1, p);
        d1[3 * j + 0] = (uint8_t)p[0]; d1[3 * j + 1] = (uint8_t)p[1]; d1[3 * j + 2] = (uint8_t)p[2];
      }
    }
  }
}

// ---- crop / resize from NV12 slots ---------------------------------------------------------------------
// crop_resize_kernel (flm_misc.hip states the arithmetic operation by operation) with every tap S[r][c] read as the
// converted pixel of the slot: the same clipped region, the same 11-bit weights, the same exact-2x area path, so the
// output has the bits of flm_crop_resize_frames on the converted frame.  resize_coef / resize_coef_y (flm_resize_dev.h) are that kernel's.
__global__ __launch_bounds__(256) void crop_resize_nv12_kernel(const uint8_t* __restrict__ frames, size_t frame_stride,
                                                               int nframes, Nv12Geom g, Nv12Coef kc,
                                                               const int32_t* __restrict__ boxes,
                                                               const int32_t* __restrict__ frame_idx,
                                                               uint8_t* __restrict__ out, int oh, int ow) {
  const int k = blockIdx.y;
  const int npix = oh * ow;
  uint8_t* dst = out + (size_t)k * npix * 3;
  const int fi = frame_idx[k];
  const int cx0 = min(max(boxes[4 * k + 0], 0), g.fw), cy0 = min(max(boxes[4 * k + 1], 0), g.fh);
  const int cx1 = min(max(boxes[4 * k + 2], 0), g.fw), cy1 = min(max(boxes[4 * k + 3], 0), g.fh);
  const int cw = cx1 - cx0, ch = cy1 - cy0;
  if ((unsigned)fi >= (unsigned)nframes || cw <= 0 || ch <= 0) {  // a slot outside the ring, a box outside the frame: zeros
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < npix * 3; p += gridDim.x * blockDim.x) dst[p] = 0;
    return;
  }
  const uint8_t* s = frames + (size_t)fi * frame_stride;
  const bool area2 = (cw == 2 * ow) && (ch == 2 * oh);
  const double scale_x = 1.0 / ((double)ow / (double)cw), scale_y = 1.0 / ((double)oh / (double)ch);
  for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < npix; p += gridDim.x * blockDim.x) {
    const int x = p % ow, y = p / ow;
    uint8_t* d = dst + (size_t)p * 3;
    int x0, x1, a0, a1, y0, y1, b0, b1;
    if (area2) {
      x0 = 2 * x; x1 = x0 + 1; y0 = 2 * y; y1 = y0 + 1;
      a0 = a1 = b0 = b1 = 0;
    } else {
      resize_coef(x, scale_x, cw, x0, x1, a0, a1);
      resize_coef_y(y, scale_y, ch, y0, y1, b0, b1);
    }
    int p00[3], p01[3], p10[3], p11[3];
    nv12_tap_bgr(s, g, kc, cx0 + x0, cy0 + y0, p00);
    nv12_tap_bgr(s, g, kc, cx0 + x1, cy0 + y0, p01);
    nv12_tap_bgr(s, g, kc, cx0 + x0, cy0 + y1, p10);
    nv12_tap_bgr(s, g, kc, cx0 + x1, cy0 + y1, p11);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if (area2) {
        d[c] = (uint8_t)((p00[c] + p01[c] + p10[c] + p11[c] + 2) >> 2);
      } else {
        const int h0 = p00[c] * a0 + p01[c] * a1;
        const int h1 = p10[c] * a0 + p11[c] * a1;
        d[c] = (uint8_t)((((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2);
      }
    }
  }
}

// ---- the alignment warp from NV12 slots ----------------------------------------------------------------
// warp_fmt_u8_kernel (flm_warp_fmt.hip) with the gather and the blend of flm_nv12_dev.h: the same pixel list, the same
// zero-fill rules, warp_position and warp_subsample unchanged, every gather of a thread issued before the first is
// consumed, and the same store path.  Per sample a thread loads a luma pair and a chroma dword for each of the two rows
// (four loads, as the BGR kernel's four dwords; 12 bytes asked for instead of 16), converts the four taps to integer
// B,G,R and blends them with warp_blend_u8's three fmafs per channel.
// The 4 x 4 grid is gathered in two halves of 8 samples (32 loads in flight per thread, then the next 32), added in the
// same row-major order: the integer conversion of four taps needs about 50 registers beside the taps, and with all 16
// samples (96 registers) in flight the kernel had a private segment of 108 bytes under the 128-register bound of four
// waves per SIMD that the BGR warp runs at.  1 x 1 and 2 x 2 issue everything at once (16 and 32 loads).
template <int S, int UNR, int LAYOUT, int TYPE>
__global__ __launch_bounds__(256, 4) void warp_nv12_kernel(const uint8_t* __restrict__ frames, size_t frame_stride,
                                                           int nframes, Nv12Geom g, Nv12Coef kc,
                                                           const int32_t* __restrict__ frame_idx,
                                                           const int32_t* __restrict__ boxes,
                                                           const float* __restrict__ m,
                                                           typename Pix<TYPE>::T* __restrict__ dst, int hd, int wd,
                                                           FmtArgs a) {
  constexpr int NS = S * S;
  constexpr int NQ = NS > 8 ? 8 : NS;  // samples gathered together
  __shared__ __attribute__((aligned(16))) unsigned char stage[4][192 * sizeof(typename Pix<TYPE>::T)];
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
  if (zero) {  // (workgroup-uniform)
    store_zero_face<LAYOUT, TYPE>(dst, f, npix, a, stage[wv]);
    return;
  }
  const uint8_t* s8 = frames + (size_t)fi * frame_stride;
  const WarpInverse inv = warp_inverse(m + (size_t)f * 6);
  const float xmax = (float)(g.fw - 1), ymax = (float)(g.fh - 1);
  const int pend = (npix + 63) & ~63;  // whole waves run the loop together (the staging needs every lane's pixel)
  const int stride = gridDim.x * blockDim.x;
  for (int p0 = blockIdx.x * blockDim.x + threadIdx.x; p0 < pend; p0 += UNR * stride) {
    float o3[UNR][3];
#pragma unroll
    for (int q0 = 0; q0 < NS; q0 += NQ) {
      Nv12Taps taps[UNR][NQ];
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
          const WarpPos wp = warp_position(inv, xd, yd, xmax, ymax);
          nv12_gather(s8, g, wp.x0, wp.y0, wp.fx, wp.fy, taps[k][q]);
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
          nv12_blend(taps[k][q], kc, v);
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
      store_pixel<LAYOUT, TYPE>(dst, f, npix, p - lane, ln, p < npix, o3[k], a, stage[wv]);
    }
  }
}

// ---- host side ---------------------------------------------------------------------------------------

// The format's defaults resolved and every condition of include/flm.h checked; `who` names the call.  The format's
// struct_size, pixel and matrix have been checked by the caller (flm_api.hip).
static int nv12_geometry(const char* who, const flm_frame_format* src, int fh, int fw, Nv12Geom* g) {
  if (fh < 2 || fw < 2 || (fh & 1) || (fw & 1)) {
    set_error("%s: NV12 frame %dx%d, needs fh and fw even and >= 2", who, fh, fw);
    return FLM_ERR_SHAPE;
  }
  const unsigned long long yp = src->y_pitch ? src->y_pitch : (unsigned)fw;
  const unsigned long long up = src->uv_pitch ? src->uv_pitch : yp;
  const unsigned long long uo = src->uv_offset ? src->uv_offset : yp * (unsigned long long)fh;
  if (yp < (unsigned long long)fw) {
    set_error("%s: y_pitch=%llu, needs y_pitch >= fw = %d", who, yp, fw);
    return FLM_ERR_SHAPE;
  }
  if (up < (unsigned long long)fw) {
    set_error("%s: uv_pitch=%llu, needs uv_pitch >= fw = %d", who, up, fw);
    return FLM_ERR_SHAPE;
  }
  if (uo < yp * (unsigned long long)fh) {
    set_error("%s: uv_offset=%llu, needs uv_offset >= y_pitch*fh = %llu", who, uo, yp * (unsigned long long)fh);
    return FLM_ERR_SHAPE;
  }
  const unsigned long long bytes = uo + (unsigned long long)(fh / 2 - 1) * up + (unsigned long long)fw;
  if (uo >= (1ull << 31) || bytes >= (1ull << 31)) {
    set_error("%s: NV12 slot of %llu bytes, needs slot bytes < 2^31", who, bytes);
    return FLM_ERR_SHAPE;
  }
  g->fh = fh;
  g->fw = fw;
  g->y_pitch = (unsigned)yp;
  g->uv_pitch = (unsigned)up;
  g->uv_off = (unsigned)uo;
  return FLM_OK;
}

size_t nv12_format_bytes(const char* who, const flm_frame_format* src, int fh, int fw) {
  Nv12Geom g;
  if (nv12_geometry(who, src, fh, fw, &g) != FLM_OK) return 0;
  return (size_t)nv12_slot_bytes(g);
}

static int check_ring(const char* who, const flm_frame_format* src, size_t frame_stride, int nframes, int fh, int fw,
                      Nv12Geom* g) {
  if (nframes < 1) {
    set_error("%s: nframes=%d, needs nframes >= 1", who, nframes);
    return FLM_ERR_SHAPE;
  }
  if (const int rc = nv12_geometry(who, src, fh, fw, g)) return rc;
  if ((unsigned long long)frame_stride < nv12_slot_bytes(*g)) {
    set_error("%s: frame_stride=%zu, needs frame_stride >= flm_frame_format_bytes = %llu", who, frame_stride,
              nv12_slot_bytes(*g));
    return FLM_ERR_SHAPE;
  }
  return FLM_OK;
}

// check_ring for the launchers of other files that read NV12 slots (flm_mesh.hip)
int nv12_ring_geometry(const char* who, const flm_frame_format* src, size_t frame_stride, int nframes, int fh, int fw,
                       Nv12Geom* g) {
  return check_ring(who, src, frame_stride, nframes, fh, fw, g);
}

int launch_frames_to_bgr_nv12(hipStream_t s, const uint8_t* frames, size_t frame_stride, int nframes, int fh, int fw,
                              const flm_frame_format* src, uint8_t* out) {
  Nv12Geom g;
  if (const int rc = check_ring("frames_to_bgr", src, frame_stride, nframes, fh, fw, &g)) return rc;
  const long long total = (long long)nframes * (fh / 2) * ((fw + 15) / 16);
  long long bx = (total + 255) / 256;
  if (bx > 65536) bx = 65536;  // (a grid-stride loop takes the rest)
  frames_to_bgr_kernel<<<dim3((unsigned)bx), 256, 0, s>>>(frames, frame_stride, nframes, g, nv12_coef(src->matrix), out);
  FLM_LAUNCH_CHECK("frames_to_bgr_kernel");
  return FLM_OK;
}

int launch_crop_resize_nv12(hipStream_t s, const uint8_t* frames, size_t frame_stride, int nframes, int fh, int fw,
                            const int32_t* boxes, const int32_t* frame_idx, int k, uint8_t* out, int oh, int ow,
                            const flm_frame_format* src) {
  if (k < 1 || k > 65535) {
    set_error("crop_resize_frames_src: k=%d outside 1 <= k <= 65535", k);
    return FLM_ERR_SHAPE;
  }
  Nv12Geom g;
  if (const int rc = check_ring("crop_resize_frames_src", src, frame_stride, nframes, fh, fw, &g)) return rc;
  if (oh < 1 || ow < 1 || (long long)oh * ow * 3 >= (1ll << 31)) {
    set_error("crop_resize_frames_src: output size %dx%d, needs oh, ow >= 1 and oh*ow*3 < 2^31", oh, ow);
    return FLM_ERR_SHAPE;
  }
  int bx = cdiv(oh * ow, 256);
  if (bx > 1024) bx = 1024;
  crop_resize_nv12_kernel<<<dim3(bx, k), 256, 0, s>>>(frames, frame_stride, nframes, g, nv12_coef(src->matrix), boxes,
                                                      frame_idx, out, oh, ow);
  FLM_LAUNCH_CHECK("crop_resize_nv12_kernel");
  return FLM_OK;
}

template <int S, int UNR>
static void launch_nv12(hipStream_t s, dim3 grid, const uint8_t* frames, size_t frame_stride, int nframes,
                        const Nv12Geom& g, const Nv12Coef& kc, const int32_t* frame_idx, const int32_t* boxes,
                        const float* m, void* dst, int hd, int wd, const flm_image_format* fmt) {
  const FmtArgs a = fmt_args(fmt);
#define FLM_CALL(L, P)                                                                                          \
  warp_nv12_kernel<S, UNR, L, P><<<grid, 256, 0, s>>>(frames, frame_stride, nframes, g, kc, frame_idx, boxes, m, \
                                                      static_cast<typename Pix<P>::T*>(dst), hd, wd, a)
  FMT_DISPATCH(FLM_CALL);
#undef FLM_CALL
}

// The image format has been checked by the caller (flm_api.hip), which passes the default one for a NULL fmt.
int launch_warp_frames_nv12(hipStream_t s, const uint8_t* frames, size_t frame_stride, int nframes, int fh, int fw,
                            const int32_t* frame_idx, const int32_t* boxes, const float* m, int k, void* dst, int hd,
                            int wd, int samples, const flm_image_format* fmt, const flm_frame_format* src) {
  if (samples != 1 && samples != 2 && samples != 4) {
    set_error("warp_affine_frames_src: samples=%d (must be 1, 2 or 4)", samples);
    return FLM_ERR_ARG;
  }
  if (k < 1 || k > 65535) {
    set_error("warp_affine_frames_src: k=%d outside 1 <= k <= 65535", k);
    return FLM_ERR_SHAPE;
  }
  Nv12Geom g;
  if (const int rc = check_ring("warp_affine_frames_src", src, frame_stride, nframes, fh, fw, &g)) return rc;
  if (hd < 1 || wd < 1 || (long long)hd * wd * 12 >= (1ll << 31)) {
    set_error("warp_affine_frames_src: aligned size %dx%d, needs hd, wd >= 1 and hd*wd*3*4 < 2^31", hd, wd);
    return FLM_ERR_SHAPE;
  }
  const Nv12Coef kc = nv12_coef(src->matrix);
  const int unr = samples == 1 ? 4 : samples == 2 ? 2 : 1;  // pixels per thread and loop trip
  int bx = cdiv(hd * wd, 256 * unr);
  if (bx > 1024) bx = 1024;
  const dim3 grid(bx, k);
  if (samples == 1) launch_nv12<1, 4>(s, grid, frames, frame_stride, nframes, g, kc, frame_idx, boxes, m, dst, hd, wd, fmt);
  else if (samples == 2) launch_nv12<2, 2>(s, grid, frames, frame_stride, nframes, g, kc, frame_idx, boxes, m, dst, hd, wd, fmt);
  else launch_nv12<4, 1>(s, grid, frames, frame_stride, nframes, g, kc, frame_idx, boxes, m, dst, hd, wd, fmt);
  FLM_LAUNCH_CHECK("warp_nv12_kernel");
  return FLM_OK;
}

}  // namespace flm
