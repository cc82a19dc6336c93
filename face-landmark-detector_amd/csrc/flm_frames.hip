// Frame-space tail of the multi-face stream: decoded landmarks taken to frame pixels, and the alignment warp sampling
// the FRAME a face came from (a slot of the ring flm_crop_resize_frames reads) instead of the model-size crop.
#include "flm_common.h"

namespace flm {

// ---- landmarks: output-grid pixels -> frame pixels ------------------------------------------------------
// The box is clipped to the frame as crop_resize_kernel clips it; then, in float64 and in this order,
//   xf = (double)cx0 + x * ((double)cw / grid_w);   yf = (double)cy0 + y * ((double)ch / grid_h)
// (the pure-scale convention of predict(to_input_space=True) and of the reference's back-projection,
// prediction.py:91-94).  A point the decode rejected (a negative coordinate) stays (-1,-1); a face whose clipped box is
// empty had no pixels to find landmarks in: (-1,-1) everywhere.  One workgroup (one wave) per face, a thread per
// point: every thread reads its pair before it writes it, so out may be lm.
__global__ __launch_bounds__(64) void landmarks_to_frame_kernel(const double* __restrict__ lm,
                                                                const int32_t* __restrict__ boxes, int c, int grid_h,
                                                                int grid_w, int fh, int fw, double* __restrict__ out) {
  const int f = blockIdx.x;
  const int cx0 = min(max(boxes[4 * f + 0], 0), fw), cy0 = min(max(boxes[4 * f + 1], 0), fh);
  const int cx1 = min(max(boxes[4 * f + 2], 0), fw), cy1 = min(max(boxes[4 * f + 3], 0), fh);
  const int cw = cx1 - cx0, ch = cy1 - cy0;
  const bool empty = cw <= 0 || ch <= 0;
  const double sx = (double)cw / (double)grid_w, sy = (double)ch / (double)grid_h;
  const double* in = lm + (size_t)f * c * 2;
  double* o = out + (size_t)f * c * 2;
  for (int i = threadIdx.x; i < c; i += 64) {
    const double x = in[2 * i], y = in[2 * i + 1];
    double xf = -1.0, yf = -1.0;
    if (!empty && !(x < 0.0 || y < 0.0)) {
      xf = (double)cx0 + x * sx;
      yf = (double)cy0 + y * sy;
    }
    o[2 * i] = xf;
    o[2 * i + 1] = yf;
  }
}

int launch_landmarks_to_frame(hipStream_t s, const double* lm, const int32_t* boxes, int k, int c, int grid_h,
                              int grid_w, int fh, int fw, double* out) {
  if (k <= 0 || c <= 0 || grid_h <= 0 || grid_w <= 0 || fh <= 0 || fw <= 0) {
    set_error("landmarks_to_frame: bad sizes k=%d c=%d grid=%dx%d frame=%dx%d (all must be >= 1)", k, c, grid_h, grid_w,
              fh, fw);
    return FLM_ERR_SHAPE;
  }
  landmarks_to_frame_kernel<<<k, 64, 0, s>>>(lm, boxes, c, grid_h, grid_w, fh, fw, out);
  FLM_LAUNCH_CHECK("landmarks_to_frame_kernel");
  return FLM_OK;
}

// ---- alignment warp with a per-face source frame ------------------------------------------------------
// M maps FRAME pixels to aligned pixels.  Per sample the arithmetic is warp_kernel's (csrc/flm_misc.hip states it
// operation by operation) with the frame as the source: Ws = fw, Hs = fh.  S x S samples per output pixel: sub-sample
// (i, j), i the row, is taken at destination coordinates xd + (2j+1-S)/(2S), yd + (2i+1-S)/(2S) (float32 sums; the
// offsets are exact for S = 2, 4), the sample values are added in float32 in row-major order starting from the first,
// and the sum is multiplied by 1/(S*S).  S = 1 is the single sample at (xd, yd), the bits of flm_warp_affine on that
// frame.
//
// Shape: the pixel list of warp_u8_kernel.  Face quantities (frame base, inverse matrix, the zero-fill decision) come
// from blockIdx and stay scalar.  A thread holds UNR pixels x S*S samples (4 x 1, 2 x 4, 1 x 16) and issues the four
// unaligned dword loads of every one of them (the pixel pair of each of the two source rows, xl = min(x0, fw-2))
// before it consumes the first: 16, 32, 64 dwords in flight per thread.  x0 = fw-1 goes through the weight (fx = 1:
// fmaf(1, t1-t0, t0) = t1 exactly on small integers), as in warp_u8_rows_kernel.  Byte offsets are 32-bit (the launcher
// checks fh*fw*3 < 2^31); 24-bit multiplies for frames below 2^24 a side measured the same and were not kept.  The
// three floats of a pixel leave through the per-wave LDS line as non-temporal 16-byte stores when the face's pixel
// count is a multiple of 4 (112x112, 256x256, ...), so the written faces do not evict frame lines the neighbouring
// pixels re-read.
__device__ __forceinline__ void store_stream16(float* p, const float4& v) {
  typedef float f4v __attribute__((ext_vector_type(4)));
  const f4v vv = {v.x, v.y, v.z, v.w};
  __builtin_nontemporal_store(vv, reinterpret_cast<f4v*>(p));
}

template <int S, int UNR>
__global__ __launch_bounds__(256) void warp_frames_kernel(const uint8_t* __restrict__ frames, size_t frame_stride,
                                                          int nframes, int fh, int fw,
                                                          const int32_t* __restrict__ frame_idx,
                                                          const int32_t* __restrict__ boxes,
                                                          const float* __restrict__ m, float* __restrict__ dst, int hd,
                                                          int wd) {
  constexpr int NS = S * S;
  const int f = blockIdx.y;
  const int npix = hd * wd;
  float* dface = dst + (size_t)f * npix * 3;
  const int fi = frame_idx ? frame_idx[f] : 0;
  bool zero = (unsigned)fi >= (unsigned)nframes;   // a slot outside the ring: zeros, as flm_crop_resize_frames gives
  if (boxes) {                                     // a clipped box without pixels: zeros too
    const int cx0 = min(max(boxes[4 * f + 0], 0), fw), cy0 = min(max(boxes[4 * f + 1], 0), fh);
    const int cx1 = min(max(boxes[4 * f + 2], 0), fw), cy1 = min(max(boxes[4 * f + 3], 0), fh);
    zero = zero || cx1 - cx0 <= 0 || cy1 - cy0 <= 0;
  }
  if (zero) {  // (workgroup-uniform)
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < npix * 3; p += gridDim.x * blockDim.x) dface[p] = 0.f;
    return;
  }
  const uint8_t* s8 = frames + (size_t)fi * frame_stride;
  const float* mm = m + (size_t)f * 6;
  const float m00 = mm[0], m01 = mm[1], m02 = mm[2], m10 = mm[3], m11 = mm[4], m12 = mm[5];
  const float det = fmaf(m00, m11, -(m01 * m10));
  const float idet = 1.0f / det;
  const float i00 = m11 * idet, i01 = -m01 * idet, i10 = -m10 * idet, i11 = m00 * idet;
  const float i02 = -fmaf(i00, m02, i01 * m12), i12 = -fmaf(i10, m02, i11 * m12);
  const float xmax = (float)(fw - 1), ymax = (float)(fh - 1);
  const unsigned fw3 = (unsigned)fw * 3u;
  __shared__ float stage[4][192];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const bool wide = (npix & 3) == 0;
  const int pend = (npix + 63) & ~63;  // whole waves run the loop together (the staging needs every lane's pixel)
  const int stride = gridDim.x * blockDim.x;
  for (int p0 = blockIdx.x * blockDim.x + threadIdx.x; p0 < pend; p0 += UNR * stride) {
    float fx[UNR][NS], fy[UNR][NS];
    unsigned ta[UNR][NS], tb[UNR][NS], ba[UNR][NS], bb[UNR][NS];
#pragma unroll
    for (int k = 0; k < UNR; ++k) {
      const int p = p0 + k * stride;
      const int pc = p < npix ? p : npix - 1;
      const int py = pc / wd;
      const float xd0 = (float)(pc - py * wd), yd0 = (float)py;
#pragma unroll
      for (int q = 0; q < NS; ++q) {
        const float xd = S == 1 ? xd0 : xd0 + (float)(2 * (q % S) + 1 - S) / (float)(2 * S);
        const float yd = S == 1 ? yd0 : yd0 + (float)(2 * (q / S) + 1 - S) / (float)(2 * S);
        float xs = fmaf(i00, xd, fmaf(i01, yd, i02));
        float ys = fmaf(i10, xd, fmaf(i11, yd, i12));
        xs = fminf(fmaxf(xs, 0.f), xmax);
        ys = fminf(fmaxf(ys, 0.f), ymax);
        const float xf = floorf(xs), yf = floorf(ys);
        fy[k][q] = ys - yf;
        const int x0 = (int)xf, y0 = (int)yf;
        const int xl = min(x0, fw - 2);  // the pair (xl, xl + 1) ends inside its row
        fx[k][q] = x0 != xl ? 1.0f : xs - xf;
        const unsigned ot = ((unsigned)y0 * (unsigned)fw + (unsigned)xl) * 3u;
        const unsigned ob = ot + (y0 + 1 < fh ? fw3 : 0u);
        __builtin_memcpy(&ta[k][q], s8 + ot, 4);
        __builtin_memcpy(&tb[k][q], s8 + ot + 2, 4);
        __builtin_memcpy(&ba[k][q], s8 + ob, 4);
        __builtin_memcpy(&bb[k][q], s8 + ob + 2, 4);
      }
    }
    // every gather above is issued before the first is consumed below: left alone, the scheduler sinks the loads of
    // the 4 x 4 grid next to their uses to save registers (4 to 8 in flight instead of 64)
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int k = 0; k < UNR; ++k) {
      const int p = p0 + k * stride;  // (a pixel past the face is computed from the clamped index and never stored:
                                      // a branch around the blend would let the compiler sink the gathers into it)
      float o3[3];
#pragma unroll
      for (int q = 0; q < NS; ++q) {
        const unsigned a = ta[k][q], b = tb[k][q], c2 = ba[k][q], d = bb[k][q];
        // pixel 0 = bytes 0,1,2 of the first dword; pixel 1 = byte 3 of the first, bytes 2,3 of the second
        const float t0[3] = {(float)(a & 0xffu), (float)((a >> 8) & 0xffu), (float)((a >> 16) & 0xffu)};
        const float t1[3] = {(float)(a >> 24), (float)((b >> 16) & 0xffu), (float)(b >> 24)};
        const float b0[3] = {(float)(c2 & 0xffu), (float)((c2 >> 8) & 0xffu), (float)((c2 >> 16) & 0xffu)};
        const float b1[3] = {(float)(c2 >> 24), (float)((d >> 16) & 0xffu), (float)(d >> 24)};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const float top = fmaf(fx[k][q], t1[c] - t0[c], t0[c]);
          const float bot = fmaf(fx[k][q], b1[c] - b0[c], b0[c]);
          const float v = fmaf(fy[k][q], bot - top, top);
          o3[c] = q == 0 ? v : o3[c] + v;
        }
      }
      if (S > 1) {
#pragma unroll
        for (int c = 0; c < 3; ++c) o3[c] *= 1.0f / (float)NS;
      }
      const int pbase = p - lane;  // first pixel of the wave
      if (wide && pbase + 64 <= npix) {
        stage[wv][3 * lane + 0] = o3[0];
        stage[wv][3 * lane + 1] = o3[1];
        stage[wv][3 * lane + 2] = o3[2];
        __builtin_amdgcn_wave_barrier();
        if (lane < 48) {
          const float4 v = *reinterpret_cast<const float4*>(&stage[wv][4 * lane]);
          store_stream16(dface + pbase * 3 + 4 * lane, v);
        }
        __builtin_amdgcn_wave_barrier();
      } else if (p < npix) {
        float* d = dface + p * 3;
        d[0] = o3[0]; d[1] = o3[1]; d[2] = o3[2];
      }
    }
  }
}

int launch_warp_frames(hipStream_t s, const uint8_t* frames, size_t frame_stride, int nframes, int fh, int fw,
                       const int32_t* frame_idx, const int32_t* boxes, const float* m, int k, float* dst, int hd,
                       int wd, int samples) {
  if (samples != 1 && samples != 2 && samples != 4) {
    set_error("warp_affine_frames: samples=%d (must be 1, 2 or 4)", samples);
    return FLM_ERR_ARG;
  }
  if (k < 1 || k > 65535) {
    set_error("warp_affine_frames: k=%d outside 1 <= k <= 65535", k);
    return FLM_ERR_SHAPE;
  }
  if (nframes < 1) {
    set_error("warp_affine_frames: nframes=%d, needs nframes >= 1", nframes);
    return FLM_ERR_SHAPE;
  }
  if (fh < 1 || fw < 2) {
    set_error("warp_affine_frames: frame %dx%d, needs fh >= 1 and fw >= 2", fh, fw);
    return FLM_ERR_SHAPE;
  }
  if ((long long)fh * fw * 3 >= (1ll << 31)) {
    set_error("warp_affine_frames: frame %dx%d, needs fh*fw*3 < 2^31", fh, fw);
    return FLM_ERR_SHAPE;
  }
  if (frame_stride < (size_t)fh * fw * 3) {
    set_error("warp_affine_frames: frame_stride=%zu, needs frame_stride >= fh*fw*3 = %zu", frame_stride,
              (size_t)fh * fw * 3);
    return FLM_ERR_SHAPE;
  }
  if (hd < 1 || wd < 1 || (long long)hd * wd * 12 >= (1ll << 31)) {
    set_error("warp_affine_frames: aligned size %dx%d, needs hd, wd >= 1 and hd*wd*12 < 2^31", hd, wd);
    return FLM_ERR_SHAPE;
  }
  const int unr = samples == 1 ? 4 : samples == 2 ? 2 : 1;  // pixels per thread and loop trip
  int bx = cdiv(hd * wd, 256 * unr);
  if (bx > 1024) bx = 1024;
  const dim3 grid(bx, k);
  if (samples == 1)
    warp_frames_kernel<1, 4><<<grid, 256, 0, s>>>(frames, frame_stride, nframes, fh, fw, frame_idx, boxes, m, dst, hd, wd);
  else if (samples == 2)
    warp_frames_kernel<2, 2><<<grid, 256, 0, s>>>(frames, frame_stride, nframes, fh, fw, frame_idx, boxes, m, dst, hd, wd);
  else
    warp_frames_kernel<4, 1><<<grid, 256, 0, s>>>(frames, frame_stride, nframes, fh, fw, frame_idx, boxes, m, dst, hd, wd);
  FLM_LAUNCH_CHECK("warp_frames_kernel");
  return FLM_OK;
}

}  // namespace flm
