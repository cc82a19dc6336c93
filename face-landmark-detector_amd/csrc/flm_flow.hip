// flm_flow_pyramid (include/flm.h states every operation; flm_flow_dev.h holds them; the comments here only say how the
// work is laid out).  The landmark flow itself, flm_landmark_flow included, is landmark_flow_rows_kernel
// (flm_flow_rows.hip).
//
// flow_pyramid_kernel: a workgroup of 256 threads per 32x32 tile of level 0 (the tile is a multiple of 2^(levels-1), so
// every level of the tile is made from the tile alone).  Every thread reads four pixels -- one 4-byte load for a luma
// crop, three for a BGR crop -- and writes their four luma bytes with one store to level 0 and to LDS; level l+1 is then
// made from level l in LDS, (32 >> l)^2 threads at a time, so the crop is read once and level 0 never again.  A crop
// whose rows or pointers are not 4-byte aligned takes the same path with byte accesses.
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

}  // namespace flm
