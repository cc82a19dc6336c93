// The mesh of the piecewise-affine warp: which template triangle a point lies in, where a mesh vertex lies in the frame,
// and the affine of one (face, triangle).  Stated once, as __host__ __device__ code, for the kernels of flm_mesh.hip
// and for the host sweep of tests/native/mesh_host.cpp, which runs these same functions against a long-double
// restatement.  include/flm.h states the contract; this header is its arithmetic.  Everything is float64, one IEEE
// operation per written operator in the written order: the build's -ffp-contract=off keeps every product and sum apart.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace flm {

constexpr int kMeshMaxPoints = 256;
constexpr int kMeshMaxTris = 255;
constexpr int kMeshNoTri = 255;  // the map's "no triangle"

// E_ab(q) = (bx-ax)*(qy-ay) - (by-ay)*(qx-ax): two products and one subtraction, in that order.  >= 0 on the inner side
// of edge a->b of a positively oriented triangle, and exactly 0 for q = a or q = b.
__host__ __device__ __forceinline__ double mesh_edge(double ax, double ay, double bx, double by, double qx, double qy) {
  const double u = (bx - ax) * (qy - ay);
  const double v = (by - ay) * (qx - ax);
  return u - v;
}

// Are i0, i1, i2 three indices into [0, p)?  (A triangle that names a point outside the mesh is never dereferenced:
// the map skips it and the affine takes the face's M.)
__host__ __device__ __forceinline__ bool mesh_tri_ok(const int32_t* __restrict__ tri, int p) {
  return (unsigned)tri[0] < (unsigned)p && (unsigned)tri[1] < (unsigned)p && (unsigned)tri[2] < (unsigned)p;
}

// The lowest t whose three edge functions at (qx, qy) are all >= 0; kMeshNoTri if none is.
__host__ __device__ inline int mesh_locate(const double* __restrict__ pts, const int32_t* __restrict__ tris, int p, int t,
                                           double qx, double qy) {
  for (int i = 0; i < t; ++i) {
    const int32_t* tri = tris + 3 * i;
    if (!mesh_tri_ok(tri, p)) continue;
    const double ax = pts[2 * tri[0]], ay = pts[2 * tri[0] + 1];
    const double bx = pts[2 * tri[1]], by = pts[2 * tri[1] + 1];
    const double cx = pts[2 * tri[2]], cy = pts[2 * tri[2] + 1];
    if (mesh_edge(ax, ay, bx, by, qx, qy) >= 0.0 && mesh_edge(bx, by, cx, cy, qx, qy) >= 0.0 &&
        mesh_edge(cx, cy, ax, ay, qx, qy) >= 0.0)
      return i;
  }
  return kMeshNoTri;
}

// An anchor's place in the frame: M^-1 d in float64 from the float32 M (frame px -> aligned px).
//   det = m00*m11 - m01*m10;  i00 = m11/det, i01 = -m01/det, i10 = -m10/det, i11 = m00/det
//   sx = i00*(dx-m02) + i01*(dy-m12);  sy = i10*(dx-m02) + i11*(dy-m12)
__host__ __device__ __forceinline__ void mesh_anchor_source(const float* __restrict__ m, double dx, double dy, double& sx,
                                                            double& sy) {
  const double m00 = (double)m[0], m01 = (double)m[1], m02 = (double)m[2];
  const double m10 = (double)m[3], m11 = (double)m[4], m12 = (double)m[5];
  const double det = m00 * m11 - m01 * m10;
  const double i00 = m11 / det, i01 = -m01 / det, i10 = -m10 / det, i11 = m00 / det;
  const double tx = dx - m02, ty = dy - m12;
  sx = i00 * tx + i01 * ty;
  sy = i10 * tx + i11 * ty;
}

// The frame position of mesh vertex v of a face: its landmark for v < c (lm_face: the face's first landmark,
// lm_stride float64 elements between points), the anchor's M^-1 image of its template position otherwise.
__host__ __device__ __forceinline__ void mesh_vertex_source(const double* __restrict__ lm_face, int lm_stride,
                                                            const float* __restrict__ m, const double* __restrict__ pts,
                                                            int c, int v, double& sx, double& sy) {
  if (v < c) {
    sx = lm_face[(size_t)v * lm_stride];
    sy = lm_face[(size_t)v * lm_stride + 1];
  } else {
    mesh_anchor_source(m, pts[2 * v], pts[2 * v + 1], sx, sy);
  }
}

// The forward matrix frame px -> aligned px that takes s0, s1, s2 (frame) onto d0, d1, d2 (template):
//   e1 = s1-s0, e2 = s2-s0, g1 = d1-d0, g2 = d2-d0, det = e1x*e2y - e1y*e2x
//   a00 = (g1x*e2y - g2x*e1y)/det   a01 = (g2x*e1x - g1x*e2x)/det   a02 = d0x - (a00*s0x + a01*s0y)
//   a10 = (g1y*e2y - g2y*e1y)/det   a11 = (g2y*e1x - g1y*e2x)/det   a12 = d0y - (a10*s0x + a11*s0y)
// each of the six rounded to float32.  !(fabs(det) >= min_det) -- collapsed, collinear or NaN sources -- gives M.
__host__ __device__ __forceinline__ void mesh_affine(const double s[3][2], const double d[3][2],
                                                     const float* __restrict__ m, double min_det, float out[6]) {
  const double e1x = s[1][0] - s[0][0], e1y = s[1][1] - s[0][1];
  const double e2x = s[2][0] - s[0][0], e2y = s[2][1] - s[0][1];
  const double g1x = d[1][0] - d[0][0], g1y = d[1][1] - d[0][1];
  const double g2x = d[2][0] - d[0][0], g2y = d[2][1] - d[0][1];
  const double det = e1x * e2y - e1y * e2x;
  if (!(fabs(det) >= min_det)) {
#pragma unroll
    for (int i = 0; i < 6; ++i) out[i] = m[i];
    return;
  }
  const double a00 = (g1x * e2y - g2x * e1y) / det;
  const double a01 = (g2x * e1x - g1x * e2x) / det;
  const double a10 = (g1y * e2y - g2y * e1y) / det;
  const double a11 = (g2y * e1x - g1y * e2x) / det;
  const double a02 = d[0][0] - (a00 * s[0][0] + a01 * s[0][1]);
  const double a12 = d[0][1] - (a10 * s[0][0] + a11 * s[0][1]);
  out[0] = (float)a00; out[1] = (float)a01; out[2] = (float)a02;
  out[3] = (float)a10; out[4] = (float)a11; out[5] = (float)a12;
}

// Triangle `tri` of one face, start to end: the three sources, the three template points, the solve.
__host__ __device__ __forceinline__ void mesh_face_affine(const double* __restrict__ lm_face, int lm_stride,
                                                          const float* __restrict__ m, const double* __restrict__ pts,
                                                          const int32_t* __restrict__ tri, int p, int a, double min_det,
                                                          float out[6]) {
  if (!mesh_tri_ok(tri, p)) {
#pragma unroll
    for (int i = 0; i < 6; ++i) out[i] = m[i];
    return;
  }
  double s[3][2], d[3][2];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int v = tri[j];
    d[j][0] = pts[2 * v];
    d[j][1] = pts[2 * v + 1];
    mesh_vertex_source(lm_face, lm_stride, m, pts, p - a, v, s[j][0], s[j][1]);
  }
  mesh_affine(s, d, m, min_det, out);
}

}  // namespace flm
