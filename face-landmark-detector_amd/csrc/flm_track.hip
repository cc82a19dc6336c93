// Tracking: the crop of the next frame from the landmarks of this one (include/flm.h states every operation; the
// comments here only say how the work is laid out).  float64 throughout, -ffp-contract=off: nothing fuses.
#include "flm_common.h"
#include "flm_track_seed_dev.h"

namespace flm {

__device__ __forceinline__ bool box_empty(int x0, int y0, int x1, int y1, int fh, int fw) {
  const int cx0 = min(max(x0, 0), fw), cy0 = min(max(y0, 0), fh);
  const int cx1 = min(max(x1, 0), fw), cy1 = min(max(y1, 0), fh);
  return cx1 - cx0 <= 0 || cy1 - cy0 <= 0;
}

// A 2x3 matrix widened to double, and the back-projection through it.
struct Affine {
  double m00, m01, m02, m10, m11, m12, det;
  bool ok;  // det finite and not zero
};
__device__ __forceinline__ Affine make_affine(float f00, float f01, float f02, float f10, float f11, float f12) {
  Affine a;
  a.m00 = (double)f00; a.m01 = (double)f01; a.m02 = (double)f02;
  a.m10 = (double)f10; a.m11 = (double)f11; a.m12 = (double)f12;
  a.det = a.m00 * a.m11 - a.m01 * a.m10;
  a.ok = __builtin_isfinite(a.det) && a.det != 0.0;
  return a;
}
__device__ __forceinline__ void affine_back(const Affine& a, double x, double y, double& xf, double& yf) {
  const double u = x - a.m02, v = y - a.m12;
  xf = (a.m11 * u - a.m01 * v) / a.det;
  yf = (a.m00 * v - a.m10 * u) / a.det;
}
// One landmark on the output grid -> frame px, (-1,-1) for every reason the header lists.
__device__ __forceinline__ void landmark_back(const Affine& a, double x, double y, double sx, double sy, double& xf,
                                              double& yf) {
  xf = -1.0;
  yf = -1.0;
  if (!a.ok || x < 0.0 || y < 0.0) return;
  double tx, ty;
  affine_back(a, x * sx, y * sy, tx, ty);
  if (tx < 0.0 || ty < 0.0 || !__builtin_isfinite(tx) || !__builtin_isfinite(ty)) return;
  xf = tx;
  yf = ty;
}

// ---- flm_track_seed: a thread per face (the arithmetic: flm_track_seed_dev.h) --------------------------------
__global__ __launch_bounds__(64) void track_seed_kernel(const int32_t* __restrict__ boxes, int k, int in_h, int in_w,
                                                        int fh, int fw, float* __restrict__ m,
                                                        int32_t* __restrict__ status) {
  const int f = blockIdx.x * 64 + threadIdx.x;
  if (f >= k) return;
  const int x0 = boxes[4 * f + 0], y0 = boxes[4 * f + 1], x1 = boxes[4 * f + 2], y1 = boxes[4 * f + 3];
  const TrackSeed sd = track_seed_one(x0, y0, x1, y1, box_empty(x0, y0, x1, y1, fh, fw), in_h, in_w);
  track_seed_store(sd, m + (size_t)f * 6);
  status[f] = sd.status;
}

// ---- flm_landmarks_from_crop: a workgroup (one wave) per face, a thread per point ----------------------------
__global__ __launch_bounds__(64) void landmarks_from_crop_kernel(const double* __restrict__ lm, size_t lm_stride,
                                                                 const float* __restrict__ m, int c, double sx, double sy,
                                                                 double* __restrict__ out) {
  const int f = blockIdx.x;
  const float* mm = m + (size_t)f * 6;
  const Affine a = make_affine(mm[0], mm[1], mm[2], mm[3], mm[4], mm[5]);
  for (int i = threadIdx.x; i < c; i += 64) {
    const double* p = lm + ((size_t)f * c + i) * lm_stride;
    double xf, yf;
    landmark_back(a, p[0], p[1], sx, sy, xf, yf);
    out[((size_t)f * c + i) * 2] = xf;
    out[((size_t)f * c + i) * 2 + 1] = yf;
  }
}

// ---- flm_track_step ---------------------------------------------------------------------------------------
// The shape of similarity_weighted_kernel (csrc/flm_misc.hip): one wave per face stages the face in LDS -- here the
// points already back-projected to frame px, a thread each -- and the sequential sums of the fit run in landmark order
// on LDS latency.  The two fits (onto tmpl_crop and onto tmpl_align) walk the same participating set, so lanes 0 and 1
// run them in lockstep, a template each: one pass of the serial loops for both matrices.  Lane 0 then owns the status
// tests and the box, lane 1 the aligned matrix.  m_next / boxes_next may be m_crop / boxes: every lane has read both
// before the barrier, the writes come after it.
struct TrackStepArgs {
  const double* lm;
  size_t lm_stride;
  const double* wt;
  size_t w_stride;
  const float* m_crop;
  const int32_t* boxes;
  int c;
  double sx, sy;
  int in_h, in_w, fh, fw;
  const double* tmpl_crop;
  const double* tmpl_align;
  int min_points;
  double min_score, min_side, max_side;
  double* lm_frame;
  float* m_align;
  float* m_next;
  int32_t* boxes_next;
  int32_t* status;
  // the One-Euro filter of flm_track_step_filtered; read by the filtered instantiation alone
  double min_cutoff, beta, d_cutoff, dt;
  double* state;   // [K,C,6]
  double* lm_raw;  // [K,C,2] or null
};

__device__ __forceinline__ int box_coord(double t) {
  const double lim = 1073741824.0;  // 2^30
  return (int)fmin(fmax(t, -lim), lim);
}

// One point's six doubles of filter state (flm_track_step_filtered), in registers.
struct EuroState {
  double xh, yh, vx, vy, xr, yr;
};
// One point through the One-Euro filter of the header: (x, y) is the raw point in frame px, s its state as read; (x, y)
// leaves as what the fits and lm_frame get, s as the state to write back.  dt is the row's time step; !dt_ok (a row of
// flm_track_step_rows whose dt is not > 0 and finite) takes the point's history away.
__device__ __forceinline__ void one_euro_point(const TrackStepArgs& g, double side, double dt, bool dt_ok, double& x,
                                               double& y, EuroState& s) {
  const double TWO_PI = 6.283185307179586;
  const double xraw = x, yraw = y;
  if (xraw < 0.0) {  // rejected (landmark_back writes exactly (-1,-1)): the point's history ends
    s.xh = -1.0; s.yh = -1.0; s.vx = 0.0; s.vy = 0.0; s.xr = -1.0; s.yr = -1.0;
    return;
  }
  const bool hist = dt_ok && s.xh >= 0.0 && s.yh >= 0.0 && __builtin_isfinite(s.xh) && __builtin_isfinite(s.yh) &&
                    __builtin_isfinite(s.vx) && __builtin_isfinite(s.vy) && __builtin_isfinite(s.xr) &&
                    __builtin_isfinite(s.yr);
  double nvx = 0.0, nvy = 0.0;
  if (hist) {
    const double rx = (xraw - s.xr) / dt, ry = (yraw - s.yr) / dt;
    const double ad = 1.0 / (1.0 + (1.0 / (TWO_PI * g.d_cutoff)) / dt);
    const double vx1 = ad * rx + (1.0 - ad) * s.vx, vy1 = ad * ry + (1.0 - ad) * s.vy;
    const double fc = g.min_cutoff + g.beta * (sqrt(vx1 * vx1 + vy1 * vy1) / side);
    const double a = 1.0 / (1.0 + (1.0 / (TWO_PI * fc)) / dt);
    const double xh1 = a * xraw + (1.0 - a) * s.xh, yh1 = a * yraw + (1.0 - a) * s.yh;
    if (__builtin_isfinite(xh1) && __builtin_isfinite(yh1) && __builtin_isfinite(vx1) && __builtin_isfinite(vy1)) {
      x = xh1; y = yh1; nvx = vx1; nvy = vy1;
    }
  }
  s.xh = x; s.yh = y; s.vx = nvx; s.vy = nvy; s.xr = xraw; s.yr = yraw;
}

// FILT: the staging loop passes every point through the filter before it reaches LDS (flm_track_step_filtered); all
// that follows the barrier is the same code on the filtered points.
// The body is shared by track_step_kernel and track_step_rows_kernel, the way track_assoc_body is shared between its two
// kernels: the arithmetic is stated once.  f is the face's ROW -- where its landmarks, weights, matrix and box are read and
// lm_frame, m_align and lm_raw written --, gs its SLOT -- where the state is read and written and m_next, boxes_next and
// status are written.  track_step_kernel passes f == gs, its scalar dt and dt_ok = true; status_rows is null there.
template <bool FILT>
__device__ __forceinline__ void track_step_body(const TrackStepArgs& g, int f, size_t gs, double dt, bool dt_ok,
                                                int32_t* status_rows) {
  extern __shared__ __attribute__((aligned(16))) double trk_s[];  // [c][2] frame px, [c][2] x 2 templates, [c] weights
  const int c = g.c;
  double* p = trk_s;
  double* tc = trk_s + 2 * c;   // tmpl_crop, then tmpl_align: lane l of the fit reads tc + l*2c
  double* w = trk_s + 6 * c;
  const int32_t* bx = g.boxes + 4 * (size_t)f;
  const bool dead = box_empty(bx[0], bx[1], bx[2], bx[3], g.fh, g.fw);
  const float* mm = g.m_crop + (size_t)f * 6;
  const Affine crop = make_affine(mm[0], mm[1], mm[2], mm[3], mm[4], mm[5]);
  double crop_side = 0.0;  // this frame's crop side in frame px: what the filter measures speed in
  if constexpr (FILT) crop_side = (double)g.in_w / sqrt(crop.m00 * crop.m00 + crop.m10 * crop.m10);
  for (int i = threadIdx.x; i < c; i += 64) {
    const double* q = g.lm + ((size_t)f * c + i) * g.lm_stride;
    double xf = -1.0, yf = -1.0;
    if (!dead) landmark_back(crop, q[0], q[1], g.sx, g.sy, xf, yf);
    const double xraw = xf, yraw = yf;
    double* sp = nullptr;
    EuroState es;
    if constexpr (FILT) {
      sp = g.state + (gs * c + i) * 6;
      es.xh = sp[0]; es.yh = sp[1]; es.vx = sp[2]; es.vy = sp[3]; es.xr = sp[4]; es.yr = sp[5];
      one_euro_point(g, crop_side, dt, dt_ok, xf, yf, es);
    }
    p[2 * i] = xf;
    p[2 * i + 1] = yf;
    g.lm_frame[((size_t)f * c + i) * 2] = xf;
    g.lm_frame[((size_t)f * c + i) * 2 + 1] = yf;
    if constexpr (FILT) {
      sp[0] = es.xh; sp[1] = es.yh; sp[2] = es.vx; sp[3] = es.vy; sp[4] = es.xr; sp[5] = es.yr;
      if (g.lm_raw) {
        g.lm_raw[((size_t)f * c + i) * 2] = xraw;
        g.lm_raw[((size_t)f * c + i) * 2 + 1] = yraw;
      }
    }
    w[i] = g.wt ? g.wt[((size_t)f * c + i) * g.w_stride] : 1.0;
    tc[2 * i] = g.tmpl_crop[2 * i];
    tc[2 * i + 1] = g.tmpl_crop[2 * i + 1];
    if (g.tmpl_align) {
      tc[2 * c + 2 * i] = g.tmpl_align[2 * i];
      tc[2 * c + 2 * i + 1] = g.tmpl_align[2 * i + 1];
    }
  }
  __syncthreads();
  const int lane = threadIdx.x;
  if (lane > (g.tmpl_align ? 1 : 0)) return;
  // the weighted fit of similarity_weighted_kernel with sx = sy = 1 (p * 1 is p), operation for operation
  const double* t = tc + (size_t)lane * 2 * c;
  double mpx = 0, mpy = 0, mqx = 0, mqy = 0, wsum = 0;
  int cnt = 0;
  for (int i = 0; i < c; ++i) {
    if (!(p[2 * i] >= 0.0 && p[2 * i + 1] >= 0.0 && w[i] > 0.0)) continue;
    mpx += w[i] * p[2 * i]; mpy += w[i] * p[2 * i + 1];
    mqx += w[i] * t[2 * i]; mqy += w[i] * t[2 * i + 1];
    wsum += w[i];
    ++cnt;
  }
  double a = 1.0, b = 0.0, tx = 0.0, ty = 0.0;
  if (cnt >= 2) {
    mpx /= wsum; mpy /= wsum; mqx /= wsum; mqy /= wsum;
    double sa = 0, sb = 0, var = 0;
    for (int i = 0; i < c; ++i) {
      if (!(p[2 * i] >= 0.0 && p[2 * i + 1] >= 0.0 && w[i] > 0.0)) continue;
      const double px = p[2 * i] - mpx, py = p[2 * i + 1] - mpy;
      const double qx = t[2 * i] - mqx, qy = t[2 * i + 1] - mqy;
      sa += w[i] * (px * qx + py * qy);
      sb += w[i] * (px * qy - py * qx);
      var += w[i] * (px * px + py * py);
    }
    if (var > 0.0) {
      a = sa / var;
      b = sb / var;
      tx = mqx - (a * mpx - b * mpy);
      ty = mqy - (b * mpx + a * mpy);
    }
  }
  const float f00 = (float)a, f01 = (float)(-b), f02 = (float)tx, f10 = (float)b, f11 = (float)a, f12 = (float)ty;
  if (lane == 1) {
    float* o = g.m_align + (size_t)f * 6;
    o[0] = f00; o[1] = f01; o[2] = f02;
    o[3] = f10; o[4] = f11; o[5] = f12;
    return;
  }
  int st = dead ? FLM_TRACK_DEAD : 0;
  if (cnt < g.min_points) st |= FLM_TRACK_FEW_POINTS;
  if (g.wt && !(wsum / (double)cnt >= g.min_score)) st |= FLM_TRACK_LOW_SCORE;
  const double da = (double)f00, db = (double)f10;
  const double side = (double)g.in_w / sqrt(da * da + db * db);
  if (!(side >= g.min_side && side <= g.max_side)) st |= FLM_TRACK_SCALE;
  const Affine nx = make_affine(f00, f01, f02, f10, f11, f12);
  const double ex = (double)(g.in_w - 1), ey = (double)(g.in_h - 1);
  double cx, cy;
  affine_back(nx, ex / 2.0, ey / 2.0, cx, cy);
  if (!(nx.ok && cx >= 0.0 && cx <= (double)(g.fw - 1) && cy >= 0.0 && cy <= (double)(g.fh - 1))) st |= FLM_TRACK_OUTSIDE;
  int b0 = 0, b1 = 0, b2 = 0, b3 = 0;
  float o0 = 1.f, o1 = 0.f, o2 = 0.f, o3 = 0.f, o4 = 1.f, o5 = 0.f;
  if (st == 0) {
    double mnx, mny, mxx, mxy, x, y;
    affine_back(nx, 0.0, 0.0, mnx, mny);
    mxx = mnx;
    mxy = mny;
    affine_back(nx, ex, 0.0, x, y);
    mnx = x < mnx ? x : mnx; mny = y < mny ? y : mny; mxx = x > mxx ? x : mxx; mxy = y > mxy ? y : mxy;
    affine_back(nx, 0.0, ey, x, y);
    mnx = x < mnx ? x : mnx; mny = y < mny ? y : mny; mxx = x > mxx ? x : mxx; mxy = y > mxy ? y : mxy;
    affine_back(nx, ex, ey, x, y);
    mnx = x < mnx ? x : mnx; mny = y < mny ? y : mny; mxx = x > mxx ? x : mxx; mxy = y > mxy ? y : mxy;
    b0 = box_coord(floor(mnx));
    b1 = box_coord(floor(mny));
    b2 = box_coord(ceil(mxx) + 1.0);
    b3 = box_coord(ceil(mxy) + 1.0);
    o0 = f00; o1 = f01; o2 = f02; o3 = f10; o4 = f11; o5 = f12;
  }
  float* o = g.m_next + gs * 6;
  o[0] = o0; o[1] = o1; o[2] = o2;
  o[3] = o3; o[4] = o4; o[5] = o5;
  int32_t* bo = g.boxes_next + 4 * gs;
  bo[0] = b0; bo[1] = b1; bo[2] = b2; bo[3] = b3;
  g.status[gs] = st;
  if (status_rows) status_rows[f] = st;
}

template <bool FILT>
__global__ __launch_bounds__(64) void track_step_kernel(const TrackStepArgs g) {
  track_step_body<FILT>(g, blockIdx.x, blockIdx.x, g.dt, true, nullptr);
}

// ---- flm_track_step_rows: the body above on the rows of a compacted batch -------------------------------------------
// A workgroup of one wave per row, as track_step_kernel.  The row map is read once; an inert row writes its compact
// outputs and leaves before anything global is touched (the whole wave leaves: the body's barrier is never reached).
struct TrackRowArgs {
  const int32_t* slot;    // [N] the global slot of every row
  int n_slots;
  const double* dt;       // [N] or null: the scalar dt of TrackStepArgs
  int32_t* status_rows;   // [N]
};

template <bool FILT>
__global__ __launch_bounds__(64) void track_step_rows_kernel(const TrackStepArgs g, const TrackRowArgs r) {
  const int f = blockIdx.x;
  const int gs = r.slot[f];
  if (gs < 0 || gs >= r.n_slots) {
    for (int i = threadIdx.x; i < 2 * g.c; i += 64) {
      g.lm_frame[(size_t)f * g.c * 2 + i] = -1.0;
      if constexpr (FILT) {
        if (g.lm_raw) g.lm_raw[(size_t)f * g.c * 2 + i] = -1.0;
      }
    }
    if (g.m_align && threadIdx.x < 6) g.m_align[(size_t)f * 6 + threadIdx.x] = (threadIdx.x == 0 || threadIdx.x == 4) ? 1.f : 0.f;
    if (threadIdx.x == 0) r.status_rows[f] = FLM_TRACK_DEAD;
    return;
  }
  double dt = g.dt;
  bool dt_ok = true;
  if constexpr (FILT) {
    if (r.dt) {
      dt = r.dt[f];
      dt_ok = dt > 0.0 && __builtin_isfinite(dt);
    }
  }
  track_step_body<FILT>(g, f, (size_t)gs, dt, dt_ok, r.status_rows);
}

// ---- flm_track_gather_streams: a thread per row, a copy ---------------------------------------------------------------
struct TrackGatherArgs {
  const int32_t* active;   // [A]
  int n_rows, s, k;        // n_rows = A*k
  const int32_t* frame_idx_stream;  // [S] or null
  const double* dt_stream;          // [S] or null
  const float* m_crop;     // [S*K,2,3]
  const int32_t* boxes;    // [S*K,4]
  const double* best_q;    // [S*K] or null
  int32_t* reset;          // [S*K] or null, in/out
  int32_t* slot_c;
  float* m_c;
  int32_t* boxes_c;
  int32_t* frame_idx_c;
  double* dt_c;
  double* best_q_c;
  int32_t* reset_c;
};

__global__ __launch_bounds__(64) void track_gather_streams_kernel(const TrackGatherArgs g) {
  const int r = blockIdx.x * 64 + threadIdx.x;
  if (r >= g.n_rows) return;
  const int a = r / g.k, j = r - a * g.k;
  const int sid = g.active[a];
  const bool valid = sid >= 0 && sid < g.s;
  const size_t gs = valid ? (size_t)sid * g.k + j : 0;
  float m0 = 1.f, m1 = 0.f, m2 = 0.f, m3 = 0.f, m4 = 1.f, m5 = 0.f;
  int b0 = 0, b1 = 0, b2 = 0, b3 = 0, fi = 0, rs = 0;
  double dt = 0.0, bq = -1.0;
  if (valid) {
    const float* mm = g.m_crop + gs * 6;
    m0 = mm[0]; m1 = mm[1]; m2 = mm[2]; m3 = mm[3]; m4 = mm[4]; m5 = mm[5];
    const int32_t* bx = g.boxes + gs * 4;
    b0 = bx[0]; b1 = bx[1]; b2 = bx[2]; b3 = bx[3];
    if (g.frame_idx_stream) fi = g.frame_idx_stream[sid];
    if (g.dt_stream) dt = g.dt_stream[sid];
    if (g.best_q) bq = g.best_q[gs];
    if (g.reset) {
      rs = g.reset[gs];
      g.reset[gs] = 0;
    }
  }
  g.slot_c[r] = valid ? (int)gs : -1;
  float* mo = g.m_c + (size_t)r * 6;
  mo[0] = m0; mo[1] = m1; mo[2] = m2; mo[3] = m3; mo[4] = m4; mo[5] = m5;
  int32_t* bo = g.boxes_c + (size_t)r * 4;
  bo[0] = b0; bo[1] = b1; bo[2] = b2; bo[3] = b3;
  g.frame_idx_c[r] = fi;
  if (g.dt_c) g.dt_c[r] = dt;
  if (g.best_q_c) g.best_q_c[r] = bq;
  if (g.reset_c) g.reset_c[r] = rs;
}

// ---- flm_track_gather_live: flm_track_gather_streams with the row map computed from the slots' liveness ----------------
// ONE workgroup walks the slots in the cyclic order of the contract -- position p is slot (c0 + p) mod S*K -- a chunk of
// blockDim.x positions at a time, so an eligible slot's exclusive prefix count IS its rank and no second pass is needed:
// a ballot and mbcnt give the prefix within the wave, the waves' totals meet in LDS, and a carry every thread keeps for
// itself (the same sum in all of them) runs from chunk to chunk.  No atomics: the order is a function of the inputs.  A
// thread owns its slot: it copies the row when the rank fits the budget and settles reset and age either way.  E is known
// after the last chunk; the inert rows, the counts and the cursor are written then.  The cursor is read by every thread
// before the first barrier and written by thread 0 after the last.
__global__ __launch_bounds__(1024) void track_gather_live_kernel(const TrackLiveArgs g) {
  __shared__ int wave_total[16];
  __shared__ int last_served;
  const int n_slots = g.s * g.k, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n_waves = blockDim.x >> 6;
  int c0 = g.cursor ? g.cursor[0] : 0;
  if (c0 < 0 || c0 >= n_slots) c0 = 0;
  int carry = 0;   // eligible slots at the positions before this chunk
  for (int base = 0; base < n_slots; base += blockDim.x) {
    const int p = base + tid;
    int gs = c0 + p;
    if (gs >= n_slots) gs -= n_slots;
    bool on = false, elig = false;
    int sid = 0, b0 = 0, b1 = 0, b2 = 0, b3 = 0;
    if (p < n_slots) {
      sid = gs / g.k;
      on = !g.stream_on || g.stream_on[sid] != 0;
      if (on) {
        const int32_t* bx = g.boxes + (size_t)gs * 4;
        b0 = bx[0]; b1 = bx[1]; b2 = bx[2]; b3 = bx[3];
        elig = !box_empty(b0, b1, b2, b3, g.fh, g.fw);
      }
    }
    const unsigned long long mask = __ballot(elig);
    const int below = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
    if (lane == 0) wave_total[wave] = __popcll(mask);
    __syncthreads();
    int before = 0, total = 0;
    for (int w = 0; w < n_waves; ++w) {
      const int t = wave_total[w];
      before += w < wave ? t : 0;
      total += t;
    }
    const int rank = carry + before + below;
    carry += total;
    if (on) {
      const bool served = elig && rank < g.n;
      double d = 0.0;
      bool good = false;
      if (g.age) {
        d = g.dt_stream ? g.dt_stream[sid] : g.dt;
        good = d > 0.0 && __builtin_isfinite(d);
      }
      if (served) {
        const int r = rank;
        g.slot_c[r] = gs;
        const float* mm = g.m_crop + (size_t)gs * 6;
        float* mo = g.m_c + (size_t)r * 6;
        mo[0] = mm[0]; mo[1] = mm[1]; mo[2] = mm[2]; mo[3] = mm[3]; mo[4] = mm[4]; mo[5] = mm[5];
        int32_t* bo = g.boxes_c + (size_t)r * 4;
        bo[0] = b0; bo[1] = b1; bo[2] = b2; bo[3] = b3;
        g.frame_idx_c[r] = g.frame_idx_stream ? g.frame_idx_stream[sid] : 0;
        if (g.best_q) g.best_q_c[r] = g.best_q[gs];
        if (g.reset) {
          g.reset_c[r] = g.reset[gs];
          g.reset[gs] = 0;
        }
        if (g.age) {
          g.dt_c[r] = good ? d + g.age[gs] : d;
          g.age[gs] = 0.0;
        }
        if (rank == g.n - 1) last_served = gs;
      } else if (g.age) {
        g.age[gs] = !elig ? 0.0 : good ? g.age[gs] + d : __builtin_nan("");
      }
    }
    __syncthreads();   // wave_total is rewritten by the next chunk; last_served is read below
  }
  const int served = min(carry, g.n);
  for (int r = served + tid; r < g.n; r += blockDim.x) {
    g.slot_c[r] = -1;
    float* mo = g.m_c + (size_t)r * 6;
    mo[0] = 1.f; mo[1] = 0.f; mo[2] = 0.f; mo[3] = 0.f; mo[4] = 1.f; mo[5] = 0.f;
    int32_t* bo = g.boxes_c + (size_t)r * 4;
    bo[0] = 0; bo[1] = 0; bo[2] = 0; bo[3] = 0;
    g.frame_idx_c[r] = 0;
    if (g.dt_c) g.dt_c[r] = 0.0;
    if (g.best_q_c) g.best_q_c[r] = -1.0;
    if (g.reset_c) g.reset_c[r] = 0;
  }
  if (tid == 0) {
    int next = c0;
    if (carry > g.n) next = last_served + 1 == n_slots ? 0 : last_served + 1;
    g.counts[0] = carry; g.counts[1] = served; g.counts[2] = carry - served; g.counts[3] = next;
    if (g.cursor) g.cursor[0] = next;
  }
}

// ---- launchers: the sizes every entry point shares ----------------------------------------------------------
static int check_track_sizes(const char* who, int k, int c, int in_h, int in_w, int fh, int fw) {
  if (k < 1 || k > 65535) {
    set_error("%s: k=%d, needs 1 <= k <= 65535", who, k);
    return FLM_ERR_SHAPE;
  }
  if (c < 1 || c > 1024) {
    set_error("%s: c=%d, needs 1 <= c <= 1024", who, c);
    return FLM_ERR_SHAPE;
  }
  if (in_h < 1 || in_w < 1 || fh < 1 || fw < 1) {
    set_error("%s: input %dx%d, frame %dx%d, needs in_h, in_w, fh, fw >= 1", who, in_h, in_w, fh, fw);
    return FLM_ERR_SHAPE;
  }
  return FLM_OK;
}

static int check_track_points(const char* who, size_t lm_stride, size_t w_stride, double sx, double sy) {
  if (lm_stride < 2 || w_stride < 1) {
    set_error("%s: needs lm_stride >= 2 and w_stride >= 1 (got %zu, %zu)", who, lm_stride, w_stride);
    return FLM_ERR_SHAPE;
  }
  if (!(sx > 0.0 && sy > 0.0)) {
    set_error("%s: needs sx, sy > 0 (got %g, %g)", who, sx, sy);
    return FLM_ERR_SHAPE;
  }
  return FLM_OK;
}

int launch_track_seed(hipStream_t s, const int32_t* boxes, int k, int in_h, int in_w, int fh, int fw, float* m,
                      int32_t* status) {
  if (const int rc = check_track_sizes("flm_track_seed", k, 1, in_h, in_w, fh, fw)) return rc;
  track_seed_kernel<<<cdiv(k, 64), 64, 0, s>>>(boxes, k, in_h, in_w, fh, fw, m, status);
  FLM_LAUNCH_CHECK("track_seed_kernel");
  return FLM_OK;
}

int launch_landmarks_from_crop(hipStream_t s, const double* lm, size_t lm_stride, const float* m, int k, int c, double sx,
                               double sy, double* out) {
  if (const int rc = check_track_sizes("flm_landmarks_from_crop", k, c, 1, 1, 1, 1)) return rc;
  if (const int rc = check_track_points("flm_landmarks_from_crop", lm_stride, 1, sx, sy)) return rc;
  landmarks_from_crop_kernel<<<k, 64, 0, s>>>(lm, lm_stride, m, c, sx, sy, out);
  FLM_LAUNCH_CHECK("landmarks_from_crop_kernel");
  return FLM_OK;
}

// slot == null: flm_track_step / flm_track_step_filtered (k slots, row == slot); else flm_track_step_rows (k rows).
int launch_track_step(hipStream_t s, const char* who, const double* lm, size_t lm_stride, const double* wt, size_t w_stride,
                      const float* m_crop, const int32_t* boxes, int k, int c, double sx, double sy, int in_h, int in_w,
                      int fh, int fw, const double* tmpl_crop, const double* tmpl_align, const flm_track_opts* opts,
                      double* lm_frame, float* m_align, float* m_next, int32_t* boxes_next, int32_t* status,
                      const flm_track_filter* filt, double dt, double* state, double* lm_raw, const int32_t* slot,
                      int n_slots, const double* dt_rows, int32_t* status_rows) {
  if (slot) {
    if (k < 1 || k > 65535) {
      set_error("%s: n=%d, needs 1 <= n <= 65535", who, k);
      return FLM_ERR_SHAPE;
    }
    if (n_slots < 1 || n_slots > 65535) {
      set_error("%s: n_slots=%d, needs 1 <= n_slots <= 65535", who, n_slots);
      return FLM_ERR_SHAPE;
    }
  }
  if (const int rc = check_track_sizes(who, k, c, in_h, in_w, fh, fw)) return rc;
  if (const int rc = check_track_points(who, lm_stride, w_stride, sx, sy)) return rc;
  TrackStepArgs g;
  g.lm = lm; g.lm_stride = lm_stride; g.wt = wt; g.w_stride = w_stride;
  g.m_crop = m_crop; g.boxes = boxes; g.c = c; g.sx = sx; g.sy = sy;
  g.in_h = in_h; g.in_w = in_w; g.fh = fh; g.fw = fw;
  g.tmpl_crop = tmpl_crop; g.tmpl_align = tmpl_align;
  g.min_points = opts->min_points; g.min_score = opts->min_score; g.min_side = opts->min_side; g.max_side = opts->max_side;
  g.lm_frame = lm_frame; g.m_align = m_align; g.m_next = m_next; g.boxes_next = boxes_next; g.status = status;
  g.min_cutoff = g.beta = g.d_cutoff = g.dt = 0.0;
  g.state = nullptr; g.lm_raw = nullptr;
  if (filt) {
    g.min_cutoff = filt->min_cutoff; g.beta = filt->beta; g.d_cutoff = filt->d_cutoff; g.dt = dt;
    g.state = state; g.lm_raw = lm_raw;
  }
  const size_t lds = sizeof(double) * 7 * c;   // (at most 56 KiB: c <= 1024)
  if (!slot) {
    if (filt)
      track_step_kernel<true><<<k, 64, lds, s>>>(g);
    else
      track_step_kernel<false><<<k, 64, lds, s>>>(g);
    FLM_LAUNCH_CHECK("track_step_kernel");
    return FLM_OK;
  }
  TrackRowArgs r;
  r.slot = slot; r.n_slots = n_slots; r.dt = filt ? dt_rows : nullptr; r.status_rows = status_rows;
  if (filt)
    track_step_rows_kernel<true><<<k, 64, lds, s>>>(g, r);
  else
    track_step_rows_kernel<false><<<k, 64, lds, s>>>(g, r);
  FLM_LAUNCH_CHECK("track_step_rows_kernel");
  return FLM_OK;
}

// Pointers and their pairing have been checked by the caller in flm_api.hip.
int launch_track_gather_streams(hipStream_t s, const int32_t* active, int a, int n_streams, int k,
                                const int32_t* frame_idx_stream, const double* dt_stream, const float* m_crop,
                                const int32_t* boxes, const double* best_q, int32_t* reset, int32_t* slot_c, float* m_c,
                                int32_t* boxes_c, int32_t* frame_idx_c, double* dt_c, double* best_q_c, int32_t* reset_c) {
  const char* who = "flm_track_gather_streams";
  if (a < 1 || n_streams < 1 || k < 1) {
    set_error("%s: a=%d, s=%d, k=%d, needs 1 <= a, 1 <= s and 1 <= k", who, a, n_streams, k);
    return FLM_ERR_SHAPE;
  }
  if ((long long)a * k > 65535 || (long long)n_streams * k > 65535) {
    set_error("%s: a=%d, s=%d streams of k=%d slots, needs a*k <= 65535 and s*k <= 65535", who, a, n_streams, k);
    return FLM_ERR_SHAPE;
  }
  TrackGatherArgs g;
  g.active = active; g.n_rows = a * k; g.s = n_streams; g.k = k;
  g.frame_idx_stream = frame_idx_stream; g.dt_stream = dt_stream; g.m_crop = m_crop; g.boxes = boxes;
  g.best_q = best_q; g.reset = reset;
  g.slot_c = slot_c; g.m_c = m_c; g.boxes_c = boxes_c; g.frame_idx_c = frame_idx_c;
  g.dt_c = dt_c; g.best_q_c = best_q_c; g.reset_c = reset_c;
  track_gather_streams_kernel<<<cdiv(g.n_rows, 64), 64, 0, s>>>(g);
  FLM_LAUNCH_CHECK("track_gather_streams_kernel");
  return FLM_OK;
}

// Pointers, their pairing and the scalar dt have been checked by the caller in flm_api.hip.
int launch_track_gather_live(hipStream_t s, const TrackLiveArgs& g) {
  const char* who = "flm_track_gather_live";
  if (g.n < 1 || g.n > 65535) {
    set_error("%s: n=%d, needs 1 <= n <= 65535", who, g.n);
    return FLM_ERR_SHAPE;
  }
  if (g.s < 1 || g.k < 1 || (long long)g.s * g.k > 65535) {
    set_error("%s: s=%d streams of k=%d slots, needs 1 <= s, 1 <= k and s*k <= 65535", who, g.s, g.k);
    return FLM_ERR_SHAPE;
  }
  if (g.fh < 1 || g.fw < 1) {
    set_error("%s: frame %dx%d, needs fh, fw >= 1", who, g.fh, g.fw);
    return FLM_ERR_SHAPE;
  }
  const int waves = cdiv(g.s * g.k, 64);   // whole waves, 16 at the most: the kernel walks the rest in chunks
  const int threads = 64 * (waves < 16 ? waves : 16);
  track_gather_live_kernel<<<1, threads, 0, s>>>(g);
  FLM_LAUNCH_CHECK("track_gather_live_kernel");
  return FLM_OK;
}

}  // namespace flm
