// flm_track_gather_flow, flm_landmark_flow_rows, flm_landmark_flow and flm_track_flow_history_put (include/flm.h states
// every rule; flm_flow_rows_dev.h holds them; the comments here only say how the work is laid out).
//
// track_gather_flow_kernel: the layout of track_gather_live_kernel (flm_track.hip) -- ONE workgroup walks the slots in the
// cyclic order of the contract a chunk of blockDim.x positions at a time; a ballot and mbcnt give the prefix count of
// the eligible slots within the wave, the waves' totals meet in LDS and a carry runs from chunk to chunk, so an eligible
// slot's exclusive prefix count IS its rank.  The live slots are counted by the same ballots.  A thread owns its slot:
// it reads flow_ready before it clears it.  No atomics: the order is a function of the inputs.
//
// landmark_flow_rows_kernel, the one landmark-flow kernel body: a workgroup of one wave per landmark of a row, as
// head_pose_kernel; instantiated once for flm_landmark_flow_rows and once for flm_landmark_flow (slot[r] = r, no check,
// no fb, one pass).  The pyramid walk is ONE device function, flow_walk_wave: per level the lanes sample the (2r+3)^2
// patch of the first image around p_l into LDS; T, Gx, Gy of the window then sit in registers, pixel k on lane k % 64,
// slot k / 64 (four slots hold the 225 pixels of radius 7); every sum is an integer butterfly over the wave
// (__shfl_xor), so all lanes hold it, all lanes run the float64 solve and every branch is wave-uniform.  The second
// image is read through L2 at the moving guess.  The forward pass calls the walk with (prev, cur) from p0, the backward
// pass with (cur, prev) from q: a loop of two trips around one call site, so the kernel holds the walk once.  No
// atomics, no private segment; lane 0 writes with plain stores.
//
// flow_history_put_kernel: a workgroup of one wave per row; the lanes share the row's landmarks.
#include "flm_common.h"
#include "flm_flow_rows_dev.h"

namespace flm {

__global__ __launch_bounds__(1024) void track_gather_flow_kernel(const TrackFlowArgs g) {
  __shared__ int wave_elig[16], wave_live[16];
  __shared__ int last_served;
  const int n_slots = g.s * g.k, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n_waves = blockDim.x >> 6;
  const int c0 = flow_gather_cursor(g.cursor, n_slots);
  int carry = 0, carry_live = 0;   // eligible and live slots at the positions before this chunk
  for (int base = 0; base < n_slots; base += blockDim.x) {
    const int p = base + tid;
    int gs = c0 + p;
    if (gs >= n_slots) gs -= n_slots;
    bool on = false, live = false, elig = false;
    if (p < n_slots) {
      on = !g.stream_on || g.stream_on[gs / g.k] != 0;
      if (on) flow_gather_classify(g, gs, &live, &elig);
    }
    const unsigned long long mask = __ballot(elig), lmask = __ballot(live);
    const int below = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
    if (lane == 0) {
      wave_elig[wave] = __popcll(mask);
      wave_live[wave] = __popcll(lmask);
    }
    __syncthreads();
    int before = 0, total = 0;
    for (int w = 0; w < n_waves; ++w) {
      const int t = wave_elig[w];
      before += w < wave ? t : 0;
      total += t;
      carry_live += wave_live[w];
    }
    const int rank = carry + before + below;
    carry += total;
    if (on) {
      if (elig && rank == g.n - 1) last_served = gs;
      flow_gather_settle(g, gs, live, elig, rank);
    }
    __syncthreads();   // the totals are rewritten by the next chunk; last_served is read below
  }
  const int served = min(carry, g.n);
  for (int r = served + tid; r < g.n; r += blockDim.x) flow_gather_inert(g, r);
  if (tid == 0) flow_gather_finish(g, c0, carry_live, carry, carry > g.n ? last_served : 0);
}

// Pointers, their pairing and the scalar dt have been checked by the caller in flm_api.hip.
int launch_track_gather_flow(hipStream_t s, const TrackFlowArgs& g) {
  const char* who = "flm_track_gather_flow";
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
  track_gather_flow_kernel<<<1, threads, 0, s>>>(g);
  FLM_LAUNCH_CHECK("track_gather_flow_kernel");
  return FLM_OK;
}

// ---- flm_landmark_flow_rows and flm_landmark_flow -----------------------------------------------------------------------
struct FlowRowsArgs {
  const uint8_t* pyr_prev;
  const uint8_t* pyr_cur;
  size_t pyr_bytes;
  int h, w, c, n_slots;
  const int32_t* slot;    // [N], or null: slot[r] = r (n_slots = N)
  const double* lm_prev;  // [n_slots,C,2], read at the slot
  const double* w_prev;   // [n_slots,C] or null, read at the slot
  const float* m;         // [N,2,3]
  FlowParams o;
  double max_fb;          // 0: no backward pass
  double* lm_out;
  double* w_out;          // or null
  int32_t* err_out;       // or null
  double* fb_out;         // or null
  int32_t* flags_out;
};

__device__ __forceinline__ int64_t flow_rows_wave_sum(int64_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor((long long)v, o, 64);
  return v;
}

constexpr int kFlowRowsSlots = 4;                                // ceil(15*15 / 64)
constexpr int kFlowRowsPatch = 2 * kFlowMaxRadius + 3;

// flow_walk (flm_flow_dev.h) by one wave: the window of image `a` at p0 is looked for in image `b`.  Returns LOW_TEXTURE,
// NOT_FINITE or both; qx, qy: where the walk stopped; sad: the residual sum of the end, -1 after NOT_FINITE.  All lanes
// return the same values.
__device__ __forceinline__ int flow_walk_wave(int32_t* patch, const uint8_t* a, const uint8_t* b, int h, int w,
                                              const FlowParams& o, double p0x, double p0y, int lane, double& qx_out,
                                              double& qy_out, int32_t& sad_out) {
  const int r = o.radius, side = 2 * r + 1, n = side * side, ps = side + 2;
  int oi[kFlowRowsSlots], oj[kFlowRowsSlots];
  bool on[kFlowRowsSlots];
#pragma unroll
  for (int s = 0; s < kFlowRowsSlots; ++s) {
    const int k = lane + 64 * s, j = k / side;
    on[s] = k < n;
    oi[s] = k - j * side - r;
    oj[s] = j - r;
  }
  int flags = 0;
  double qx = 0.0, qy = 0.0;
  int32_t T[kFlowRowsSlots];
#pragma unroll
  for (int s = 0; s < kFlowRowsSlots; ++s) T[s] = 0;
  bool bad = false;
  for (int l = o.levels - 1; l >= 0 && !bad; --l) {
    const int hl = h >> l, wl = w >> l;
    const size_t off = flow_level_offset(h, w, l);
    const uint8_t* P = a + off;
    const uint8_t* Q = b + off;
    const double px = flow_level_coord(p0x, l), py = flow_level_coord(p0y, l);
    if (l == o.levels - 1) {
      qx = px;
      qy = py;
    }
    __syncthreads();   // the level above (or the pass before) has read its patch
    for (int k = lane; k < ps * ps; k += 64) {
      const int j = k / ps, i = k - j * ps;
      patch[k] = flow_sample(P, hl, wl, px + (double)(i - r - 1), py + (double)(j - r - 1));
    }
    __syncthreads();
    int32_t Gx[kFlowRowsSlots], Gy[kFlowRowsSlots];
    int64_t sa = 0, sb = 0, sc = 0;
#pragma unroll
    for (int s = 0; s < kFlowRowsSlots; ++s) {
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
    const double A = (double)flow_rows_wave_sum(sa), B = (double)flow_rows_wave_sum(sb), C = (double)flow_rows_wave_sum(sc);
    const double det = A * C - B * B;
    const double eig = flow_min_eig(A, B, C, n);
    if (!(eig >= o.min_eig)) {
      if (l == 0) flags |= kFlowLowTexture;
    } else {
      for (int it = 0; it < o.max_iter; ++it) {
        int64_t sx = 0, sy = 0;
#pragma unroll
        for (int s = 0; s < kFlowRowsSlots; ++s) {
          if (on[s]) {
            const int64_t d = T[s] - flow_sample(Q, hl, wl, qx + (double)oi[s], qy + (double)oj[s]);
            sx += d * Gx[s];
            sy += d * Gy[s];
          }
        }
        double dx, dy;
        flow_solve(A, B, C, det, (double)flow_rows_wave_sum(sx), (double)flow_rows_wave_sum(sy), &dx, &dy);
        const int st = flow_update(dx, dy, o.eps, &qx, &qy);
        if (st == 2) bad = true;
        if (st != 0) break;
      }
    }
    if (l > 0 && !bad) {
      qx = 2.0 * qx + 0.5;
      qy = 2.0 * qy + 0.5;
    }
  }
  qx_out = qx;
  qy_out = qy;
  sad_out = -1;
  if (bad) return flags | kFlowNotFinite;
  int64_t sad = 0;   // T is the window of level 0
#pragma unroll
  for (int s = 0; s < kFlowRowsSlots; ++s) {
    if (on[s]) {
      const int32_t d = T[s] - flow_sample(b, h, w, qx + (double)oi[s], qy + (double)oj[s]);
      sad += d < 0 ? -d : d;
    }
  }
  sad_out = (int32_t)flow_rows_wave_sum(sad);
  return flags;
}

template <bool kRows>
__device__ __forceinline__ void flow_rows_write(const FlowRowsArgs& g, size_t e, int lane, const FlowRowsOut& o) {
  if (lane != 0) return;
  g.lm_out[2 * e] = o.x;
  g.lm_out[2 * e + 1] = o.y;
  if (g.w_out) g.w_out[e] = o.w;
  if (g.err_out) g.err_out[e] = o.err;
  if (kRows) g.fb_out[e] = o.fb;
  g.flags_out[e] = o.flags;
}

// The (2r+3)^2 window patch in LDS, every workgroup its own; declared once for both instantiations of the kernel below
// (declared in each, it makes the compiler schedule the rows form differently than it does alone).
__shared__ int32_t patch[kFlowRowsPatch * kFlowRowsPatch];

// kRows: flm_landmark_flow_rows (slot, fb, the backward pass where max_fb > 0); without it: flm_landmark_flow (row r
// reads slot r, no fb, one pass).  One body, two instantiations.
template <bool kRows>
__global__ __launch_bounds__(64) void landmark_flow_rows_kernel(const FlowRowsArgs g) {
  const int lane = threadIdx.x, f = blockIdx.x / g.c, i = blockIdx.x - f * g.c;
  const size_t e = blockIdx.x;
  const int gs = kRows ? g.slot[f] : f;
  if (kRows && flow_row_inert(gs, g.n_slots)) {   // reads nothing more (the same for every lane, as every branch below)
    flow_rows_write<kRows>(g, e, lane, flow_rows_inert_out());
    return;
  }
  const size_t he = (size_t)gs * g.c + i;
  double p0x, p0y;
  int flags = flow_start(g.m + 6 * (size_t)f, g.lm_prev[2 * he], g.lm_prev[2 * he + 1], &p0x, &p0y);
  if (flags) {
    flow_rows_write<kRows>(g, e, lane, flow_rows_out(flags, -1.0, -1.0, 0.0, -1, -1.0));
    return;
  }
  const uint8_t* prev = g.pyr_prev + (size_t)f * g.pyr_bytes;
  const uint8_t* cur = g.pyr_cur + (size_t)f * g.pyr_bytes;
  const int side = 2 * g.o.radius + 1;
  double qx = 0.0, qy = 0.0, fb2 = -1.0;
  int32_t err = -1;
  const int passes = kRows && g.max_fb > 0.0 ? 2 : 1;
  for (int pass = 0; pass < passes; ++pass) {
    double wx, wy;
    int32_t sad;
    const int wf = flow_walk_wave(patch, pass ? cur : prev, pass ? prev : cur, g.h, g.w, g.o, pass ? qx : p0x,
                                  pass ? qy : p0y, lane, wx, wy, sad);
    if (pass == 0) {
      qx = wx;
      qy = wy;
      err = sad;
      flags = wf;
      if (!(wf & kFlowNotFinite))
        flags |= flow_gates(sad, side * side, wx, wy, p0x, p0y, g.h, g.w, g.o.max_err, g.o.max_move);
      if (flags) break;
    } else {
      flags = flow_fb_gate(wf, wx, wy, p0x, p0y, g.max_fb, &fb2);
    }
  }
  const double wp = (flags == 0 && g.w_prev) ? g.w_prev[he] : 1.0;
  flow_rows_write<kRows>(g, e, lane, flow_rows_out(flags, qx, qy, wp, err, fb2));
}

// slot null (flm_landmark_flow): row r reads slot r, n_slots is n, and neither fb nor the backward pass is run.
int launch_landmark_flow_rows(hipStream_t s, const uint8_t* pyr_prev, const uint8_t* pyr_cur, int n, int h, int w,
                              const int32_t* slot, int n_slots, const double* lm_prev, const double* w_prev, const float* m,
                              int c, const flm_flow_opts* opts, double max_fb, double* lm_out, double* w_out,
                              int32_t* err_out, double* fb_out, int32_t* flags_out) {
  FlowRowsArgs g;
  g.pyr_prev = pyr_prev; g.pyr_cur = pyr_cur; g.pyr_bytes = flow_level_offset(h, w, opts->levels);
  g.h = h; g.w = w; g.c = c; g.n_slots = slot ? n_slots : n; g.slot = slot;
  g.lm_prev = lm_prev; g.w_prev = w_prev; g.m = m;
  g.o.levels = opts->levels; g.o.radius = opts->radius; g.o.max_iter = opts->max_iter;
  g.o.eps = opts->eps; g.o.min_eig = opts->min_eig; g.o.max_err = opts->max_err; g.o.max_move = opts->max_move;
  g.max_fb = max_fb;
  g.lm_out = lm_out; g.w_out = w_out; g.err_out = err_out; g.fb_out = fb_out; g.flags_out = flags_out;
  const unsigned blocks = (unsigned)n * (unsigned)c;
  if (slot)
    landmark_flow_rows_kernel<true><<<blocks, 64, 0, s>>>(g);
  else
    landmark_flow_rows_kernel<false><<<blocks, 64, 0, s>>>(g);
  FLM_LAUNCH_CHECK("landmark_flow_rows_kernel");
  return FLM_OK;
}

// ---- flm_track_flow_history_put -----------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void flow_history_put_kernel(const FlowPutArgs g) {
  flow_history_put_row(g, blockIdx.x, threadIdx.x, 64);
}

int launch_flow_history_put(hipStream_t s, const FlowPutArgs& g) {
  flow_history_put_kernel<<<g.n, 64, 0, s>>>(g);
  FLM_LAUNCH_CHECK("flow_history_put_kernel");
  return FLM_OK;
}

}  // namespace flm
