// The __host__ __device__ text of csrc/flm_flow_rows_dev.h -- the point of flm_landmark_flow_rows with its backward pass,
// the slot rules of flm_track_gather_flow, the row of flm_track_flow_history_put -- run on the host over cases a test
// writes (tests/test_flow_rows_native_host.py), which compares every byte of the answer with tests/flow_rows_ref.py.
// Built without contraction, as the library is, and with the host's address and undefined-behaviour sanitizers.
//
//   flow_rows_host IN OUT
// IN:  int32 n_records; per record int32 kind, then
//   kind 1 (flow):   int32 {h, w, ch, levels, radius, max_iter, c, n, n_slots, has_w}, double {eps, min_eig, max_err,
//                    max_move, max_fb}, float m[n*6], int32 slot[n], double lm[n_slots*c*2], double w[n_slots*c] if has_w,
//                    uint8 prev[n*h*w*ch], uint8 cur[n*h*w*ch]
//   kind 2 (gather): int32 {s, k, fh, fw, n, has_on, has_fi, has_dts, has_bq, has_reset, has_age, has_cursor}, double dt,
//                    then, each if it is there, int32 on[s], int32 fi[s], double dts[s]; float m_crop[s*k*6],
//                    int32 boxes[s*k*4]; double best_q[s*k], int32 reset[s*k], double age[s*k], int32 cursor[1];
//                    int32 flow_frame[s*k], int32 flow_ready[s*k]
//   kind 3 (put):    int32 {n, n_slots, c, has_lm, has_w}, int32 slot[n], status[n], frame_idx[n]; double lm_rows[n*c*2],
//                    hist_lm[n_slots*c*2] if has_lm; double w_rows[n*c], hist_w[n_slots*c] if has_w; int32
//                    flow_frame[n_slots], flow_ready[n_slots]
// OUT: per record
//   kind 1: per row and point double {x, y, w, fb}, int32 {err, flags}
//   kind 2: reset, age, cursor (each if there), flow_ready, slot_c, m_c, boxes_c, frame_idx_c, prev_frame_idx_c, dt_c,
//           best_q_c, reset_c (each if there), counts[6]
//   kind 3: hist_lm, hist_w (each if there), flow_frame, flow_ready
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "flm_flow_rows_dev.h"

using namespace flm;

static void must(bool ok, const char* what) {
  if (!ok) {
    std::fprintf(stderr, "flow_rows_host: %s\n", what);
    std::exit(2);
  }
}

template <class T>
static void rd(FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  must(n == 0 || std::fread(v.data(), sizeof(T), n, f) == n, "short read");
}
template <class T>
static void wr(FILE* f, const std::vector<T>& v) {
  must(v.empty() || std::fwrite(v.data(), sizeof(T), v.size(), f) == v.size(), "short write");
}
template <class T>
static T* ptr(std::vector<T>& v) { return v.empty() ? nullptr : v.data(); }

static std::vector<uint8_t> pyramid(const uint8_t* src, int h, int w, int ch, int levels) {
  std::vector<uint8_t> p(flow_level_offset(h, w, levels));
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x) {
      const uint8_t* q = src + ((size_t)y * w + x) * ch;
      p[(size_t)y * w + x] = (uint8_t)(ch == 1 ? q[0] : flow_luma(q[0], q[1], q[2]));
    }
  for (int l = 1; l < levels; ++l) {
    const uint8_t* a = p.data() + flow_level_offset(h, w, l - 1);
    uint8_t* b = p.data() + flow_level_offset(h, w, l);
    const int wa = w >> (l - 1), hb = h >> l, wb = w >> l;
    for (int y = 0; y < hb; ++y)
      for (int x = 0; x < wb; ++x) {
        const uint8_t* q = a + (size_t)(2 * y) * wa + 2 * x;
        b[(size_t)y * wb + x] = (uint8_t)flow_down(q[0], q[1], q[wa], q[wa + 1]);
      }
  }
  return p;
}

static long flow_record(FILE* in, FILE* out) {
  std::vector<int32_t> hd, slot;
  std::vector<double> od, lm, wt;
  std::vector<float> m;
  std::vector<uint8_t> prev, cur;
  rd(in, hd, 10);
  rd(in, od, 5);
  const int h = hd[0], w = hd[1], ch = hd[2], c = hd[6], n = hd[7], n_slots = hd[8];
  FlowParams o;
  o.levels = hd[3]; o.radius = hd[4]; o.max_iter = hd[5];
  o.eps = od[0]; o.min_eig = od[1]; o.max_err = od[2]; o.max_move = od[3];
  must(h >= 1 && w >= 1 && (ch == 1 || ch == 3) && o.levels >= 1 && o.levels <= kFlowMaxLevels && o.radius >= 1 &&
           o.radius <= kFlowMaxRadius && c >= 1 && n >= 1 && n_slots >= 1, "bad flow header");
  rd(in, m, (size_t)n * 6);
  rd(in, slot, (size_t)n);
  rd(in, lm, (size_t)n_slots * c * 2);
  rd(in, wt, hd[9] ? (size_t)n_slots * c : 0);
  const size_t img = (size_t)h * w * ch;
  rd(in, prev, img * n);
  rd(in, cur, img * n);
  for (int r = 0; r < n; ++r) {
    const int gs = slot[r];
    std::vector<uint8_t> pp, pc;
    if (!flow_row_inert(gs, n_slots)) {
      pp = pyramid(prev.data() + img * r, h, w, ch, o.levels);
      pc = pyramid(cur.data() + img * r, h, w, ch, o.levels);
    }
    for (int i = 0; i < c; ++i) {
      FlowRowsOut res = flow_rows_inert_out();
      if (!flow_row_inert(gs, n_slots)) {
        const size_t he = (size_t)gs * c + i;
        double qx, qy, fb2;
        int32_t err;
        const int flags = flow_rows_point(pp.data(), pc.data(), h, w, m.data() + 6 * (size_t)r, lm[2 * he], lm[2 * he + 1], o,
                                          od[4], &qx, &qy, &err, &fb2);
        res = flow_rows_out(flags, qx, qy, (flags == 0 && hd[9]) ? wt[he] : 1.0, err, fb2);
      }
      const double d[4] = {res.x, res.y, res.w, res.fb};
      const int32_t e[2] = {res.err, res.flags};
      must(std::fwrite(d, sizeof(double), 4, out) == 4 && std::fwrite(e, sizeof(int32_t), 2, out) == 2, "short write");
    }
  }
  return (long)n * c;
}

static void gather_record(FILE* in, FILE* out) {
  std::vector<int32_t> hd, on, fi, boxes, reset, cursor, frame, ready;
  std::vector<double> dt, dts, bq, age;
  std::vector<float> m_crop;
  rd(in, hd, 12);
  rd(in, dt, 1);
  const int s = hd[0], k = hd[1], n = hd[4];
  must(s >= 1 && k >= 1 && n >= 1 && hd[2] >= 1 && hd[3] >= 1, "bad gather header");
  const size_t ns = (size_t)s * k;
  rd(in, on, hd[5] ? s : 0);
  rd(in, fi, hd[6] ? s : 0);
  rd(in, dts, hd[7] ? s : 0);
  rd(in, m_crop, ns * 6);
  rd(in, boxes, ns * 4);
  rd(in, bq, hd[8] ? ns : 0);
  rd(in, reset, hd[9] ? ns : 0);
  rd(in, age, hd[10] ? ns : 0);
  rd(in, cursor, hd[11] ? 1 : 0);
  rd(in, frame, ns);
  rd(in, ready, ns);
  // the compact outputs start from a pattern the call must overwrite everywhere
  std::vector<int32_t> slot_c(n, 0x5a5a5a5a), boxes_c((size_t)n * 4, 0x5a5a5a5a), fi_c(n, 0x5a5a5a5a), prev_c(n, 0x5a5a5a5a);
  std::vector<int32_t> reset_c(hd[9] ? n : 0, 0x5a5a5a5a), counts(6, 0x5a5a5a5a);
  std::vector<float> m_c((size_t)n * 6, -7.f);
  std::vector<double> dt_c(hd[10] ? n : 0, -7.0), bq_c(hd[8] ? n : 0, -7.0);
  TrackFlowArgs g;
  g.boxes = boxes.data(); g.m_crop = m_crop.data(); g.s = s; g.k = k; g.fh = hd[2]; g.fw = hd[3]; g.n = n;
  g.stream_on = ptr(on); g.frame_idx_stream = ptr(fi); g.dt_stream = ptr(dts); g.dt = dt[0];
  g.best_q = ptr(bq); g.reset = ptr(reset); g.age = ptr(age); g.cursor = ptr(cursor);
  g.flow_frame = frame.data(); g.flow_ready = ready.data();
  g.slot_c = slot_c.data(); g.m_c = m_c.data(); g.boxes_c = boxes_c.data(); g.frame_idx_c = fi_c.data();
  g.prev_frame_idx_c = prev_c.data(); g.dt_c = ptr(dt_c); g.best_q_c = ptr(bq_c); g.reset_c = ptr(reset_c);
  g.counts = counts.data();
  flow_gather_serial(g);
  wr(out, reset); wr(out, age); wr(out, cursor); wr(out, ready);
  wr(out, slot_c); wr(out, m_c); wr(out, boxes_c); wr(out, fi_c); wr(out, prev_c); wr(out, dt_c); wr(out, bq_c);
  wr(out, reset_c); wr(out, counts);
}

static void put_record(FILE* in, FILE* out) {
  std::vector<int32_t> hd, slot, status, fi, frame, ready;
  std::vector<double> lm_rows, hist_lm, w_rows, hist_w;
  rd(in, hd, 5);
  const int n = hd[0], n_slots = hd[1], c = hd[2];
  must(n >= 1 && n_slots >= 1 && c >= 1, "bad put header");
  rd(in, slot, n);
  rd(in, status, n);
  rd(in, fi, n);
  rd(in, lm_rows, hd[3] ? (size_t)n * c * 2 : 0);
  rd(in, hist_lm, hd[3] ? (size_t)n_slots * c * 2 : 0);
  rd(in, w_rows, hd[4] ? (size_t)n * c : 0);
  rd(in, hist_w, hd[4] ? (size_t)n_slots * c : 0);
  rd(in, frame, n_slots);
  rd(in, ready, n_slots);
  FlowPutArgs g;
  g.slot = slot.data(); g.status_rows = status.data(); g.frame_idx_c = fi.data(); g.lm_rows = ptr(lm_rows);
  g.w_rows = ptr(w_rows); g.n = n; g.n_slots = n_slots; g.c = c; g.hist_lm = ptr(hist_lm); g.hist_w = ptr(hist_w);
  g.flow_frame = frame.data(); g.flow_ready = ready.data();
  for (int r = 0; r < n; ++r) flow_history_put_row(g, r, 0, 1);
  wr(out, hist_lm); wr(out, hist_w); wr(out, frame); wr(out, ready);
}

int main(int argc, char** argv) {
  must(argc == 3, "usage: flow_rows_host IN OUT");
  FILE* in = std::fopen(argv[1], "rb");
  FILE* out = std::fopen(argv[2], "wb");
  must(in && out, "cannot open the files");
  std::vector<int32_t> head, kind;
  rd(in, head, 1);
  long points = 0;
  for (int t = 0; t < head[0]; ++t) {
    rd(in, kind, 1);
    must(kind[0] >= 1 && kind[0] <= 3, "bad record kind");
    if (kind[0] == 1) points += flow_record(in, out);
    if (kind[0] == 2) gather_record(in, out);
    if (kind[0] == 3) put_record(in, out);
  }
  std::fclose(in);
  must(std::fclose(out) == 0, "close failed");
  std::printf("flow_rows_host: %d records, %ld points, 0 failures\n", head[0], points);
  return 0;
}
