// The arithmetic and the slot rules of flm_track_gather_flow, flm_landmark_flow_rows and flm_track_flow_history_put
// (include/flm.h states the contracts), as __host__ __device__ functions: the kernels of flm_flow_rows.hip and a host
// program (tests/native/flow_rows_host.cpp) run this text.  As flm_flow_dev.h: every float64 line is one IEEE operation
// per written operator, in the written order; the file must be compiled without contraction.
//
// THE HISTORY RULE.  flow_ready[g] == 1 exactly when slot g was served with status 0 by the last tick of its stream, key
// or flow, and nothing has written its crop matrix since.  hist_lm[g] (and hist_w[g]) are then the raw landmarks of that
// tick in frame px and flow_frame[g] the ring slot they were found in.
#ifndef FLM_FLOW_ROWS_DEV_H_
#define FLM_FLOW_ROWS_DEV_H_

#include "flm_flow_dev.h"

namespace flm {

constexpr int kFlowFb = 64;   // FLM_FLOW_FB

// The verdict of the forward-backward check.  bflags: what the backward walk returned; (bx, by): where it stopped.
// *fb2: the squared distance of the round trip, or -1.0 where the backward walk did not finish.  Returns FB or 0.
FLM_FLOW_HD int flow_fb_gate(int bflags, double bx, double by, double p0x, double p0y, double max_fb, double* fb2) {
  if (bflags & kFlowNotFinite) {
    *fb2 = -1.0;
    return kFlowFb;
  }
  const double ex = bx - p0x, ey = by - p0y;
  *fb2 = ex * ex + ey * ey;
  if (bflags & kFlowLowTexture) return kFlowFb;
  return !(*fb2 <= max_fb * max_fb) ? kFlowFb : 0;
}

// The whole flow of one point of flm_landmark_flow_rows, serially: what a host program calls.  The kernel runs the same
// functions with the window spread over the lanes of a wave.  The forward pass is flow_point; returns the flags; *qx,
// *qy: the forward guess where it stopped; *err: the forward SAD or -1; *fb2 as flow_fb_gate, -1.0 where the backward
// pass did not run.
FLM_FLOW_HD int flow_rows_point(const uint8_t* prev, const uint8_t* cur, int h, int w, const float* m, double x, double y,
                                const FlowParams& o, double max_fb, double* qx, double* qy, int32_t* err, double* fb2) {
  *fb2 = -1.0;
  const int flags = flow_point(prev, cur, h, w, m, x, y, o, qx, qy, err);
  if (flags || !(max_fb > 0.0)) return flags;
  double p0x, p0y, bx, by;
  int32_t berr;
  flow_start(m, x, y, &p0x, &p0y);   // (0: the forward pass started from this p0)
  const int bflags = flow_walk(cur, prev, h, w, *qx, *qy, o, &bx, &by, &berr);
  return flow_fb_gate(bflags, bx, by, p0x, p0y, max_fb, fb2);
}

// A row whose slot lies outside the store is inert: it reads nothing.
FLM_FLOW_HD bool flow_row_inert(int gs, int n_slots) { return gs < 0 || gs >= n_slots; }

// What a point writes: "Outputs" of flm_landmark_flow, plus fb.  wp: the point's previous weight (1.0 without weights).
struct FlowRowsOut {
  double x, y, w, fb;
  int32_t err, flags;
};
FLM_FLOW_HD FlowRowsOut flow_rows_out(int flags, double qx, double qy, double wp, int32_t err, double fb2) {
  const bool ok = flags == 0;
  FlowRowsOut o;
  o.x = ok ? qx : -1.0;
  o.y = ok ? qy : -1.0;
  o.w = ok ? wp : 0.0;
  o.fb = fb2;
  o.err = err;
  o.flags = flags;
  return o;
}
FLM_FLOW_HD FlowRowsOut flow_rows_inert_out() { return flow_rows_out(kFlowNoHistory, -1.0, -1.0, 0.0, -1, -1.0); }

// ---- flm_track_gather_flow --------------------------------------------------------------------------------------------
// The arguments under the names of include/flm.h (the kernel takes the struct as it is).
struct TrackFlowArgs {
  const int32_t* boxes;             // [S*K,4]
  const float* m_crop;              // [S*K,2,3]
  int s, k, fh, fw, n;              // n: the budget, the number of rows
  const int32_t* stream_on;         // [S] or null
  const int32_t* frame_idx_stream;  // [S] or null
  const double* dt_stream;          // [S] or null
  double dt;
  const double* best_q;             // [S*K] or null
  int32_t* reset;                   // [S*K] or null, in/out
  double* age;                      // [S*K] or null, in/out
  int32_t* cursor;                  // [1] or null, in/out
  const int32_t* flow_frame;        // [S*K]
  int32_t* flow_ready;              // [S*K] in/out
  int32_t* slot_c;
  float* m_c;
  int32_t* boxes_c;
  int32_t* frame_idx_c;
  int32_t* prev_frame_idx_c;
  double* dt_c;
  double* best_q_c;
  int32_t* reset_c;
  int32_t* counts;                  // [6]
};

FLM_FLOW_HD bool flow_box_empty(int x0, int y0, int x1, int y1, int fh, int fw) {   // the clip of flm_landmarks_to_frame
  const int cx0 = flow_clampi(x0, fw), cy0 = flow_clampi(y0, fh);
  const int cx1 = flow_clampi(x1, fw), cy1 = flow_clampi(y1, fh);
  return cx1 - cx0 <= 0 || cy1 - cy0 <= 0;
}

FLM_FLOW_HD int flow_gather_cursor(const int32_t* cursor, int n_slots) {
  const int c0 = cursor ? cursor[0] : 0;
  return (c0 < 0 || c0 >= n_slots) ? 0 : c0;
}

// What one slot of a stream that is on is: *live by rule 1 of flm_track_gather_live, *elig = live with a history.
FLM_FLOW_HD void flow_gather_classify(const TrackFlowArgs& g, int gs, bool* live, bool* elig) {
  const int32_t* bx = g.boxes + (size_t)gs * 4;
  *live = !flow_box_empty(bx[0], bx[1], bx[2], bx[3], g.fh, g.fw);
  *elig = *live && g.flow_ready[gs] != 0;
}

// Everything one slot of a stream that is on reads and writes once its rank among the eligible slots is known.
FLM_FLOW_HD void flow_gather_settle(const TrackFlowArgs& g, int gs, bool live, bool elig, int rank) {
  const int sid = gs / g.k;
  const bool served = elig && rank < g.n;
  double d = 0.0;
  bool good = false;
  if (g.age) {
    d = g.dt_stream ? g.dt_stream[sid] : g.dt;
    good = d > 0.0 && flow_fin(d);
  }
  if (served) {
    const int r = rank;
    g.slot_c[r] = gs;
    const float* mm = g.m_crop + (size_t)gs * 6;
    float* mo = g.m_c + (size_t)r * 6;
    mo[0] = mm[0]; mo[1] = mm[1]; mo[2] = mm[2]; mo[3] = mm[3]; mo[4] = mm[4]; mo[5] = mm[5];
    const int32_t* bx = g.boxes + (size_t)gs * 4;
    int32_t* bo = g.boxes_c + (size_t)r * 4;
    bo[0] = bx[0]; bo[1] = bx[1]; bo[2] = bx[2]; bo[3] = bx[3];
    g.frame_idx_c[r] = g.frame_idx_stream ? g.frame_idx_stream[sid] : 0;
    g.prev_frame_idx_c[r] = g.flow_frame[gs];
    if (g.best_q) g.best_q_c[r] = g.best_q[gs];
    if (g.reset) {
      g.reset_c[r] = g.reset[gs];
      g.reset[gs] = 0;
    }
    if (g.age) {
      g.dt_c[r] = good ? d + g.age[gs] : d;
      g.age[gs] = 0.0;
    }
  } else if (g.age) {
    g.age[gs] = !live ? 0.0 : good ? g.age[gs] + d : __builtin_nan("");
  }
  g.flow_ready[gs] = 0;   // the put of this tick sets it again for the rows served alive
}

FLM_FLOW_HD void flow_gather_inert(const TrackFlowArgs& g, int r) {
  g.slot_c[r] = -1;
  float* mo = g.m_c + (size_t)r * 6;
  mo[0] = 1.f; mo[1] = 0.f; mo[2] = 0.f; mo[3] = 0.f; mo[4] = 1.f; mo[5] = 0.f;
  int32_t* bo = g.boxes_c + (size_t)r * 4;
  bo[0] = 0; bo[1] = 0; bo[2] = 0; bo[3] = 0;
  g.frame_idx_c[r] = 0;
  g.prev_frame_idx_c[r] = 0;
  if (g.dt_c) g.dt_c[r] = 0.0;
  if (g.best_q_c) g.best_q_c[r] = -1.0;
  if (g.reset_c) g.reset_c[r] = 0;
}

// live, elig: the totals; last_served: the slot of row n-1 (read only when elig > n).
FLM_FLOW_HD void flow_gather_finish(const TrackFlowArgs& g, int c0, int live, int elig, int last_served) {
  const int n_slots = g.s * g.k, served = elig < g.n ? elig : g.n;
  int next = c0;
  if (elig > g.n) next = last_served + 1 == n_slots ? 0 : last_served + 1;
  g.counts[0] = live; g.counts[1] = elig; g.counts[2] = served; g.counts[3] = elig - served;
  g.counts[4] = live - elig; g.counts[5] = next;
  if (g.cursor) g.cursor[0] = next;
}

// The whole call, serially: what a host program runs.  The kernel ranks with a prefix count over one workgroup instead
// of this loop's running count, and calls the same functions.
FLM_FLOW_HD void flow_gather_serial(const TrackFlowArgs& g) {
  const int n_slots = g.s * g.k, c0 = flow_gather_cursor(g.cursor, n_slots);
  int n_live = 0, n_elig = 0, last_served = 0;
  for (int p = 0; p < n_slots; ++p) {
    const int gs = c0 + p >= n_slots ? c0 + p - n_slots : c0 + p;
    if (g.stream_on && g.stream_on[gs / g.k] == 0) continue;
    bool live, elig;
    flow_gather_classify(g, gs, &live, &elig);
    if (elig && n_elig == g.n - 1) last_served = gs;
    flow_gather_settle(g, gs, live, elig, n_elig);
    n_live += live ? 1 : 0;
    n_elig += elig ? 1 : 0;
  }
  for (int r = n_elig < g.n ? n_elig : g.n; r < g.n; ++r) flow_gather_inert(g, r);
  flow_gather_finish(g, c0, n_live, n_elig, last_served);
}

// ---- flm_track_flow_history_put ---------------------------------------------------------------------------------------
struct FlowPutArgs {
  const int32_t* slot;         // [N]
  const int32_t* status_rows;  // [N]
  const int32_t* frame_idx_c;  // [N]
  const double* lm_rows;       // [N,C,2] or null
  const double* w_rows;        // [N,C] or null
  int n, n_slots, c;
  double* hist_lm;             // [n_slots,C,2] or null, with lm_rows
  double* hist_w;              // [n_slots,C] or null, with w_rows
  int32_t* flow_frame;         // [n_slots]
  int32_t* flow_ready;         // [n_slots]
};

// Row r, by `lanes` workers of which this is worker `lane` (a host program: one worker).
FLM_FLOW_HD void flow_history_put_row(const FlowPutArgs& g, int r, int lane, int lanes) {
  const int gs = g.slot[r];
  if (gs < 0 || gs >= g.n_slots) return;
  if (g.status_rows[r] != 0) {
    if (lane == 0) g.flow_ready[gs] = 0;
    return;
  }
  if (g.lm_rows) {
    const double* src = g.lm_rows + (size_t)r * g.c * 2;
    double* dst = g.hist_lm + (size_t)gs * g.c * 2;
    for (int i = lane; i < 2 * g.c; i += lanes) dst[i] = src[i];
    if (g.w_rows) {
      const double* ws = g.w_rows + (size_t)r * g.c;
      double* wd = g.hist_w + (size_t)gs * g.c;
      for (int i = lane; i < g.c; i += lanes) wd[i] = ws[i];
    }
  }
  if (lane == 0) {
    g.flow_frame[gs] = g.frame_idx_c[r];
    g.flow_ready[gs] = 1;
  }
}

}  // namespace flm
#endif  // FLM_FLOW_ROWS_DEV_H_
