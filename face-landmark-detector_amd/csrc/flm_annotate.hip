// flm_frames_annotate (include/flm.h, "frame annotation", states the contract; flm_annotate_dev.h holds the acceptance
// test, the region, the cell range, the ownership predicate, the disc and the colour conversion; the comments here only
// say how the work is laid out).  Up to four launches in stream order, a layer that is off launches nothing:
//   annotate_regions_kernel  one wave per face: lanes stride over the face's points, a butterfly of comparisons joins
//       the 64 partial extents (min and max pick one of their inputs, so the order plays no part), lane 0 writes R.
//   annotate_mosaic_kernel   grid (tile, face).  The cells that P of the face intersects are dealt over groups of L lanes
//       (L = 1, 4, 16 or 64 by the cell's size) of the face's workgroups.  Wave 0 of a workgroup first collects, 64 faces
//       per step, the faces j < f of the same frame that take part and share a cell with f (their indices, in LDS); a cell
//       is processed only when none of them holds it -- by its owner, the lowest such face.  So no cell is read by one
//       workgroup while another writes it, and every cell is replaced once, from its original bytes.
//   annotate_outline_kernel  grid (tile, face): the four bands of the outline as clipped rectangles, pixel by pixel.
//   annotate_marks_kernel    grid (tile, face): a thread per (landmark, disc offset), 32 threads per landmark, 21 in use.
// The last two store constants: where faces overlap, the stores carry the same bytes.  Nothing is allocated, nothing is
// synchronised, no workspace, no read-modify-write of memory that another workgroup touches.
#include "flm_annotate_dev.h"
#include "flm_common.h"

namespace flm {

constexpr int kAnnotThreads = 256;
constexpr int kAnnotMosaicTiles = 32;   // workgroups per face of the mosaic
constexpr int kAnnotOutlineTiles = 8;   // workgroups per face of the outline
constexpr int kAnnotMaxList = 4096;     // faces a workgroup can collect: the k <= 4096 of the header with redact

__device__ __forceinline__ AnnotBox annot_load_box(const int32_t* regions, int f) {
  return AnnotBox{regions[4 * f], regions[4 * f + 1], regions[4 * f + 2], regions[4 * f + 3]};
}

// One pixel in a layer's colour.  BGR: three bytes.  NV12: the luma byte, and the U,V pair of the pixel's 2x2 block.
__device__ __forceinline__ void annot_paint(uint8_t* s, const AnnotateArgs& g, int x, int y, const uint8_t px[3]) {
  if (g.nv12) {
    s[(unsigned)y * g.y_pitch + (unsigned)x] = px[0];
    uint8_t* c = s + (g.uv_off + (unsigned)(y >> 1) * g.uv_pitch + (unsigned)(x & ~1));
    c[0] = px[1];
    c[1] = px[2];
  } else {
    uint8_t* d = s + ((size_t)y * g.fw + x) * 3;
    d[0] = px[0];
    d[1] = px[1];
    d[2] = px[2];
  }
}

__global__ __launch_bounds__(64) void annotate_regions_kernel(const AnnotateArgs g) {
  const int f = blockIdx.x, lane = threadIdx.x;
  const double* lm = g.lm + (size_t)f * g.c * g.lm_stride;
  AnnotExtent e = annot_extent_empty();
  for (int i = lane; i < g.c; i += 64) annot_extent_add(e, lm[(size_t)i * g.lm_stride], lm[(size_t)i * g.lm_stride + 1]);
#pragma unroll
  for (int o = 32; o; o >>= 1) {
    AnnotExtent t;
    t.mnx = __shfl_xor(e.mnx, o);
    t.mny = __shfl_xor(e.mny, o);
    t.mxx = __shfl_xor(e.mxx, o);
    t.mxy = __shfl_xor(e.mxy, o);
    t.any = __shfl_xor(e.any, o);
    annot_extent_merge(e, t);
  }
  if (lane == 0) {
    const AnnotBox r = annot_region(e, g.margin);
    int32_t* out = g.regions + 4 * (size_t)f;
    out[0] = r.x0; out[1] = r.y0; out[2] = r.x1; out[3] = r.y1;
  }
}

// lanes_log2: log2 of the lanes that share a cell (0, 2, 4 or 6).
__global__ __launch_bounds__(kAnnotThreads) void annotate_mosaic_kernel(const AnnotateArgs g, int lanes_log2) {
  __shared__ unsigned short s_list[kAnnotMaxList];
  __shared__ int s_count;
  const int f = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
  const int s = g.redact;
  const int fi = g.frame_idx ? g.frame_idx[f] : 0;
  const AnnotBox pf = annot_clip(annot_load_box(g.regions, f), g.fw, g.fh);
  if (!annot_takes_part(pf, fi, g.nframes)) return;  // (workgroup-uniform)
  const AnnotBox cf = annot_cells(pf, s);
  const int ncx = cf.x1 - cf.x0, ncell = ncx * (cf.y1 - cf.y0);
  const int L = 1 << lanes_log2, groups = kAnnotThreads >> lanes_log2;
  if (blockIdx.x * groups >= ncell) return;          // no cell left for this workgroup
  if (tid < 64) {
    int cnt = 0;
    // four steps of 64 faces per trip: their loads are independent and go out together, the ballots follow in order
    for (int j0 = 0; j0 < f; j0 += 256) {
      bool hit[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int j = j0 + 64 * u + lane;
        hit[u] = false;
        if (j < f) {
          AnnotBox cj;
          hit[u] = annot_competes(annot_load_box(g.regions, j), g.frame_idx ? g.frame_idx[j] : 0, cf, fi, g.nframes, g.fw,
                                  g.fh, s, &cj);
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const unsigned long long mask = __ballot(hit[u]);
        if (hit[u])  // (the index is below the faces scanned so far: < f <= 4095)
          s_list[cnt + __popcll(mask & ((1ull << lane) - 1ull))] = (unsigned short)(j0 + 64 * u + lane);
        cnt += __popcll(mask);
      }
    }
    if (lane == 0) s_count = cnt;
  }
  __syncthreads();
  const int count = s_count;
  uint8_t* slot = g.frames + (size_t)fi * g.frame_stride;
  const int sub = tid & (L - 1);
  const int gg = blockIdx.x * groups + (tid >> lanes_log2), total = gridDim.x * groups;
  // every lane of a wave walks the loop the same number of times: the shuffles below need them all
  for (int base = 0; base < ncell; base += total) {
    const int cell = base + gg;
    bool mine = cell < ncell;
    int cx = 0, cy = 0;
    if (mine) {
      cy = cell / ncx;
      cx = cf.x0 + (cell - cy * ncx);
      cy += cf.y0;
      for (int q = 0; q < count && mine; ++q) {
        const int j = s_list[q];
        const AnnotBox cj = annot_cells(annot_clip(annot_load_box(g.regions, j), g.fw, g.fh), s);
        mine = !annot_cell_in(cj, cx, cy);
      }
    }
    const int x0 = cx * s, y0 = cy * s;
    const int cw = min(x0 + s, g.fw) - x0, ch = min(y0 + s, g.fh) - y0;
    const int n = cw * ch;
    int s0 = 0, s1 = 0, s2 = 0;
    if (mine) {
      if (g.nv12) {
        for (int p = sub; p < n; p += L) {
          const int r = p / cw, c = p - r * cw;
          s0 += slot[(unsigned)(y0 + r) * g.y_pitch + (unsigned)(x0 + c)];
        }
        const int hw = cw >> 1;
        for (int p = sub; p < (n >> 2); p += L) {
          const int r = p / hw, c = p - r * hw;
          const uint8_t* uv = slot + (g.uv_off + (unsigned)((y0 >> 1) + r) * g.uv_pitch + (unsigned)(x0 + 2 * c));
          s1 += uv[0];
          s2 += uv[1];
        }
      } else {
        for (int p = sub; p < n; p += L) {
          const int r = p / cw, c = p - r * cw;
          const uint8_t* d = slot + ((size_t)(y0 + r) * g.fw + (x0 + c)) * 3;
          s0 += d[0];
          s1 += d[1];
          s2 += d[2];
        }
      }
    }
    for (int o = L >> 1; o; o >>= 1) {  // (wave-uniform: L is a launch constant)
      s0 += __shfl_xor(s0, o);
      s1 += __shfl_xor(s1, o);
      s2 += __shfl_xor(s2, o);
    }
    if (!mine) continue;
    if (g.nv12) {
      const int m = n >> 2;
      const uint8_t a0 = (uint8_t)((s0 + (n >> 1)) / n), a1 = (uint8_t)((s1 + (m >> 1)) / m), a2 = (uint8_t)((s2 + (m >> 1)) / m);
      for (int p = sub; p < n; p += L) {
        const int r = p / cw, c = p - r * cw;
        slot[(unsigned)(y0 + r) * g.y_pitch + (unsigned)(x0 + c)] = a0;
      }
      const int hw = cw >> 1;
      for (int p = sub; p < m; p += L) {
        const int r = p / hw, c = p - r * hw;
        uint8_t* uv = slot + (g.uv_off + (unsigned)((y0 >> 1) + r) * g.uv_pitch + (unsigned)(x0 + 2 * c));
        uv[0] = a1;
        uv[1] = a2;
      }
    } else {
      const uint8_t a0 = (uint8_t)((s0 + (n >> 1)) / n), a1 = (uint8_t)((s1 + (n >> 1)) / n), a2 = (uint8_t)((s2 + (n >> 1)) / n);
      for (int p = sub; p < n; p += L) {
        const int r = p / cw, c = p - r * cw;
        uint8_t* d = slot + ((size_t)(y0 + r) * g.fw + (x0 + c)) * 3;
        d[0] = a0;
        d[1] = a1;
        d[2] = a2;
      }
    }
  }
}

// The pixels of a clipped rectangle, dealt over the face's workgroups.
__device__ __forceinline__ void annot_paint_rect(uint8_t* slot, const AnnotateArgs& g, int x0, int y0, int x1, int y1,
                                                 const uint8_t px[3]) {
  if (x1 <= x0 || y1 <= y0) return;
  const int w = x1 - x0;
  const long long n = (long long)w * (y1 - y0);
  for (long long p = (long long)blockIdx.x * kAnnotThreads + threadIdx.x; p < n; p += (long long)gridDim.x * kAnnotThreads) {
    const int r = (int)(p / w), c = (int)(p - (long long)r * w);
    annot_paint(slot, g, x0 + c, y0 + r, px);
  }
}

__global__ __launch_bounds__(kAnnotThreads) void annotate_outline_kernel(const AnnotateArgs g) {
  const int f = blockIdx.y, t = g.box;
  const int fi = g.frame_idx ? g.frame_idx[f] : 0;
  const AnnotBox r = annot_load_box(g.regions, f);
  const AnnotBox p = annot_clip(r, g.fw, g.fh);
  if (!annot_takes_part(p, fi, g.nframes)) return;
  uint8_t* slot = g.frames + (size_t)fi * g.frame_stride;
  // (|R| <= 2^30 and t <= 16: the sums stay inside int32)
  annot_paint_rect(slot, g, p.x0, p.y0, p.x1, min(p.y1, r.y0 + t), g.box_px);  // y <  R.y0 + t
  annot_paint_rect(slot, g, p.x0, max(p.y0, r.y1 - t), p.x1, p.y1, g.box_px);  // y >= R.y1 - t
  annot_paint_rect(slot, g, p.x0, p.y0, min(p.x1, r.x0 + t), p.y1, g.box_px);  // x <  R.x0 + t
  annot_paint_rect(slot, g, max(p.x0, r.x1 - t), p.y0, p.x1, p.y1, g.box_px);  // x >= R.x1 - t
}

__global__ __launch_bounds__(kAnnotThreads) void annotate_marks_kernel(const AnnotateArgs g) {
  const int f = blockIdx.y;
  const int t = blockIdx.x * kAnnotThreads + threadIdx.x;
  const int i = t >> 5, o = t & 31;
  if (i >= g.c || o >= kAnnotDisc) return;
  const int fi = g.frame_idx ? g.frame_idx[f] : 0;
  const AnnotBox p = annot_clip(annot_load_box(g.regions, f), g.fw, g.fh);
  if (!annot_takes_part(p, fi, g.nframes)) return;
  const double* pt = g.lm + ((size_t)f * g.c + i) * g.lm_stride;
  const double x = pt[0], y = pt[1];
  if (!annot_accepted(x, y)) return;
  int dx, dy;
  annot_disc_offset(o, &dx, &dy);
  const int px = (int)x + dx, py = (int)y + dy;  // (x, y <= 2^30)
  if (px < 0 || py < 0 || px >= g.fw || py >= g.fh) return;
  annot_paint(g.frames + (size_t)fi * g.frame_stride, g, px, py, g.mark_px);
}

int launch_frames_annotate(hipStream_t s, const AnnotateArgs& g) {
  annotate_regions_kernel<<<g.k, 64, 0, s>>>(g);
  FLM_LAUNCH_CHECK("annotate_regions_kernel");
  if (g.redact) {
    const int lanes_log2 = g.redact <= 2 ? 0 : g.redact <= 4 ? 2 : g.redact <= 8 ? 4 : 6;
    annotate_mosaic_kernel<<<dim3(kAnnotMosaicTiles, g.k), kAnnotThreads, 0, s>>>(g, lanes_log2);
    FLM_LAUNCH_CHECK("annotate_mosaic_kernel");
  }
  if (g.box) {
    annotate_outline_kernel<<<dim3(kAnnotOutlineTiles, g.k), kAnnotThreads, 0, s>>>(g);
    FLM_LAUNCH_CHECK("annotate_outline_kernel");
  }
  if (g.marks) {
    annotate_marks_kernel<<<dim3(cdiv(g.c * 32, kAnnotThreads), g.k), kAnnotThreads, 0, s>>>(g);
    FLM_LAUNCH_CHECK("annotate_marks_kernel");
  }
  return FLM_OK;
}

}  // namespace flm
