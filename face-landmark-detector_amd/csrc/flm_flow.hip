// flm_flow_pyramid and flm_landmark_flow (include/flm.h states every operation; flm_flow_dev.h holds them; the comments
// here only say how the work is laid out).
//
// flow_pyramid_kernel: a workgroup of 256 threads per 32x32 tile of level 0 (the tile is a multiple of 2^(levels-1), so
// every level of the tile is made from the tile alone).  Every thread reads four pixels -- one 4-byte load for a luma
// crop, three for a BGR crop -- and writes their four luma bytes with one store to level 0 and to LDS; level l+1 is then
// made from level l in LDS, (32 >> l)^2 threads at a time, so the crop is read once and level 0 never again.  A crop
// whose rows or pointers are not 4-byte aligned takes the same path with byte accesses.
//
// landmark_flow_kernel: a workgroup of one wave per point, as head_pose_kernel.  Per level the lanes sample the
// (2r+3)^2 patch of the previous image around p_l into LDS; T, Gx and Gy of the window then sit in registers, pixel k of
// the window on lane k % 64, slot k / 64 (four slots hold the 225 pixels of radius 7).  Every sum is an integer
// butterfly over the wave (__shfl_xor), so all lanes hold it and all lanes run the float64 solve redundantly: convergence
// and every branch below are wave-uniform.  The current image is read through L2 at the moving guess.  No atomics, no
// private segment; lane 0 writes the point's outputs with plain stores.
#include "flm_common.h"
#include "flm_flow_dev.h"

namespace flm {

constexpr int kPyrTile = 32;

struct PyrArgs {
  const uint8_t* src;
  uint8_t* pyr;
  int h, w, ch, levels;
  int tiles_x, tiles_y;
  size_t pyr_bytes;
  int vec;   // 4-byte accesses are aligned: w % 4 == 0, pyr_bytes % 4 == 0, both pointers on 4 bytes
};

__global__ __launch_bounds__(256) void flow_pyramid_kernel(const PyrArgs g) {
  __shared__ __attribute__((aligned(16))) uint8_t lv[2][kPyrTile * kPyrTile];
  int b = blockIdx.x;
  const int tx = b % g.tiles_x;
  b /= g.tiles_x;
  const int ty = b % g.tiles_y, img = b / g.tiles_y;
  const int t = threadIdx.x, y = t >> 3, x4 = (t & 7) * 4;
  const int gy = ty * kPyrTile + y, gx = tx * kPyrTile + x4;
  const uint8_t* s = g.src + (size_t)img * g.h * g.w * g.ch;
  uint8_t* d = g.pyr + (size_t)img * g.pyr_bytes;
  uint32_t packed = 0;
  if (gy < g.h && gx < g.w) {
    const size_t px = (size_t)gy * g.w + gx;
    if (g.vec) {
      if (g.ch == 1) {
        packed = *reinterpret_cast<const uint32_t*>(s + px);
      } else {
        const uint32_t* q = reinterpret_cast<const uint32_t*>(s + px * 3);
        const uint32_t a0 = q[0], a1 = q[1], a2 = q[2];   // b0 g0 r0 b1 | g1 r1 b2 g2 | r2 b3 g3 r3
        const int y0 = flow_luma(a0 & 255, (a0 >> 8) & 255, (a0 >> 16) & 255);
        const int y1 = flow_luma(a0 >> 24, a1 & 255, (a1 >> 8) & 255);
        const int y2 = flow_luma((a1 >> 16) & 255, a1 >> 24, a2 & 255);
        const int y3 = flow_luma((a2 >> 8) & 255, (a2 >> 16) & 255, a2 >> 24);
        packed = (uint32_t)y0 | ((uint32_t)y1 << 8) | ((uint32_t)y2 << 16) | ((uint32_t)y3 << 24);
      }
      *reinterpret_cast<uint32_t*>(d + px) = packed;
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (gx + i < g.w) {
          const uint8_t* q = s + (px + i) * g.ch;
          const int v = g.ch == 1 ? (int)q[0] : flow_luma(q[0], q[1], q[2]);
          d[px + i] = (uint8_t)v;
          packed |= (uint32_t)v << (8 * i);
        }
      }
    }
  }
  *reinterpret_cast<uint32_t*>(&lv[0][y * kPyrTile + x4]) = packed;
  __syncthreads();
  size_t off = (size_t)g.h * g.w;
  for (int l = 1; l < g.levels; ++l) {
    const int side = kPyrTile >> l, ps = side * 2, hl = g.h >> l, wl = g.w >> l;
    const uint8_t* from = lv[(l - 1) & 1];
    uint8_t* to = lv[l & 1];
    if (t < side * side) {
      const int oy = t / side, ox = t - oy * side;
      const uint8_t* q = from + (2 * oy) * ps + 2 * ox;
      const int v = flow_down(q[0], q[1], q[ps], q[ps + 1]);
      to[oy * side + ox] = (uint8_t)v;
      const int py = ty * side + oy, pxl = tx * side + ox;
      if (py < hl && pxl < wl) d[off + (size_t)py * wl + pxl] = (uint8_t)v;
    }
    __syncthreads();
    off += (size_t)hl * wl;
  }
}

int launch_flow_pyramid(hipStream_t s, const uint8_t* src, int n, int h, int w, int ch, int levels, uint8_t* pyr) {
  PyrArgs g;
  g.src = src; g.pyr = pyr; g.h = h; g.w = w; g.ch = ch; g.levels = levels;
  g.tiles_x = (w + kPyrTile - 1) / kPyrTile;
  g.tiles_y = (h + kPyrTile - 1) / kPyrTile;
  g.pyr_bytes = flow_level_offset(h, w, levels);
  g.vec = (w % 4 == 0 && g.pyr_bytes % 4 == 0 && reinterpret_cast<uintptr_t>(src) % 4 == 0 &&
           reinterpret_cast<uintptr_t>(pyr) % 4 == 0) ? 1 : 0;
  const unsigned blocks = (unsigned)g.tiles_x * (unsigned)g.tiles_y * (unsigned)n;   // < 2^31: checked by the caller
  flow_pyramid_kernel<<<blocks, 256, 0, s>>>(g);
  FLM_LAUNCH_CHECK("flow_pyramid_kernel");
  return FLM_OK;
}

struct FlowArgs {
  const uint8_t* pyr_prev;
  const uint8_t* pyr_cur;
  size_t pyr_bytes;
  int h, w, c;
  const double* lm_prev;
  const double* w_prev;   // or null
  const float* m;
  FlowParams o;
  double* lm_out;
  double* w_out;          // or null
  int32_t* err_out;       // or null
  int32_t* flags_out;
};

__device__ __forceinline__ int64_t flow_wave_sum(int64_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor((long long)v, o, 64);
  return v;
}

__device__ __forceinline__ void flow_write(const FlowArgs& g, int e, int lane, int flags, double qx, double qy, int32_t err) {
  if (lane != 0) return;
  const bool ok = flags == 0;
  g.lm_out[2 * (size_t)e] = ok ? qx : -1.0;
  g.lm_out[2 * (size_t)e + 1] = ok ? qy : -1.0;
  if (g.w_out) g.w_out[e] = ok ? (g.w_prev ? g.w_prev[e] : 1.0) : 0.0;
  if (g.err_out) g.err_out[e] = err;
  g.flags_out[e] = flags;
}

constexpr int kFlowSlots = 4;                                    // ceil(15*15 / 64)
constexpr int kFlowPatch = 2 * kFlowMaxRadius + 3;

__global__ __launch_bounds__(64) void landmark_flow_kernel(const FlowArgs g) {
  __shared__ int32_t patch[kFlowPatch * kFlowPatch];
  const int e = blockIdx.x, lane = threadIdx.x, f = e / g.c;
  double p0x, p0y;
  int flags = flow_start(g.m + 6 * (size_t)f, g.lm_prev[2 * (size_t)e], g.lm_prev[2 * (size_t)e + 1], &p0x, &p0y);
  if (flags) {   // (the same for every lane, as every branch below)
    flow_write(g, e, lane, flags, -1.0, -1.0, -1);
    return;
  }
  const int r = g.o.radius, side = 2 * r + 1, n = side * side, ps = side + 2;
  int oi[kFlowSlots], oj[kFlowSlots];
  bool on[kFlowSlots];
#pragma unroll
  for (int s = 0; s < kFlowSlots; ++s) {
    const int k = lane + 64 * s, j = k / side;
    on[s] = k < n;
    oi[s] = k - j * side - r;
    oj[s] = j - r;
  }
  const uint8_t* prev = g.pyr_prev + (size_t)f * g.pyr_bytes;
  const uint8_t* cur = g.pyr_cur + (size_t)f * g.pyr_bytes;
  double qx = 0.0, qy = 0.0;
  int32_t T[kFlowSlots];
#pragma unroll
  for (int s = 0; s < kFlowSlots; ++s) T[s] = 0;
  bool bad = false;
  for (int l = g.o.levels - 1; l >= 0 && !bad; --l) {
    const int hl = g.h >> l, wl = g.w >> l;
    const size_t off = flow_level_offset(g.h, g.w, l);
    const uint8_t* P = prev + off;
    const uint8_t* Q = cur + off;
    const double px = flow_level_coord(p0x, l), py = flow_level_coord(p0y, l);
    if (l == g.o.levels - 1) {
      qx = px;
      qy = py;
    }
    __syncthreads();   // the level above has read its patch
    for (int k = lane; k < ps * ps; k += 64) {
      const int j = k / ps, i = k - j * ps;
      patch[k] = flow_sample(P, hl, wl, px + (double)(i - r - 1), py + (double)(j - r - 1));
    }
    __syncthreads();
    int32_t Gx[kFlowSlots], Gy[kFlowSlots];
    int64_t sa = 0, sb = 0, sc = 0;
#pragma unroll
    for (int s = 0; s < kFlowSlots; ++s) {
      T[s] = 0; Gx[s] = 0; Gy[s] = 0;
      if (on[s]) {
        const int c0 = (oj[s] + r + 1) * ps + (oi[s] + r + 1);
        T[s] = patch[c0];
        Gx[s] = patch[c0 + 1] - patch[c0 - 1];
        Gy[s] = patch[c0 + ps] - patch[c0 - ps];
        sa += (int64_t)Gx[s] * Gx[s];
        sb += (int64_t)Gx[s] * Gy[s];
        sc += (int64_t)Gy[s] * Gy[s];
      }
    }
    const double A = (double)flow_wave_sum(sa), B = (double)flow_wave_sum(sb), C = (double)flow_wave_sum(sc);
    const double det = A * C - B * B;
    const double eig = flow_min_eig(A, B, C, n);
    if (!(eig >= g.o.min_eig)) {
      if (l == 0) flags |= kFlowLowTexture;
    } else {
      for (int it = 0; it < g.o.max_iter; ++it) {
        int64_t sx = 0, sy = 0;
#pragma unroll
        for (int s = 0; s < kFlowSlots; ++s) {
          if (on[s]) {
            const int64_t d = T[s] - flow_sample(Q, hl, wl, qx + (double)oi[s], qy + (double)oj[s]);
            sx += d * Gx[s];
            sy += d * Gy[s];
          }
        }
        double dx, dy;
        flow_solve(A, B, C, det, (double)flow_wave_sum(sx), (double)flow_wave_sum(sy), &dx, &dy);
        const int st = flow_update(dx, dy, g.o.eps, &qx, &qy);
        if (st == 2) bad = true;
        if (st != 0) break;
      }
    }
    if (l > 0 && !bad) {
      qx = 2.0 * qx + 0.5;
      qy = 2.0 * qy + 0.5;
    }
  }
  if (bad) {
    flow_write(g, e, lane, flags | kFlowNotFinite, -1.0, -1.0, -1);
    return;
  }
  int64_t sad = 0;   // T is the window of level 0
#pragma unroll
  for (int s = 0; s < kFlowSlots; ++s) {
    if (on[s]) {
      const int32_t d = T[s] - flow_sample(cur, g.h, g.w, qx + (double)oi[s], qy + (double)oj[s]);
      sad += d < 0 ? -d : d;
    }
  }
  const int32_t err = (int32_t)flow_wave_sum(sad);
  flags |= flow_gates(err, n, qx, qy, p0x, p0y, g.h, g.w, g.o.max_err, g.o.max_move);
  flow_write(g, e, lane, flags, qx, qy, err);
}

int launch_landmark_flow(hipStream_t s, const uint8_t* pyr_prev, const uint8_t* pyr_cur, int k, int h, int w,
                         const double* lm_prev, const double* w_prev, const float* m, int c, const flm_flow_opts* opts,
                         double* lm_out, double* w_out, int32_t* err_out, int32_t* flags_out) {
  FlowArgs g;
  g.pyr_prev = pyr_prev; g.pyr_cur = pyr_cur; g.pyr_bytes = flow_level_offset(h, w, opts->levels);
  g.h = h; g.w = w; g.c = c; g.lm_prev = lm_prev; g.w_prev = w_prev; g.m = m;
  g.o.levels = opts->levels; g.o.radius = opts->radius; g.o.max_iter = opts->max_iter;
  g.o.eps = opts->eps; g.o.min_eig = opts->min_eig; g.o.max_err = opts->max_err; g.o.max_move = opts->max_move;
  g.lm_out = lm_out; g.w_out = w_out; g.err_out = err_out; g.flags_out = flags_out;
  landmark_flow_kernel<<<(unsigned)k * (unsigned)c, 64, 0, s>>>(g);
  FLM_LAUNCH_CHECK("landmark_flow_kernel");
  return FLM_OK;
}

}  // namespace flm
