// flm_track_associate: detector boxes against the live tracks of a tracker, in one launch of ONE workgroup (include/flm.h
// states every operation; flm_track_assoc_dev.h holds the integer pieces; the comments here only say how the work is
// laid out).  The problem is small and latency-bound -- at most 1024 x 1024 pairs -- so nothing leaves the CU:
// thread i owns slot i and detection i (the workgroup has max(k, d) threads, rounded up to whole waves), the clipped
// boxes of both sides sit in LDS (2 x 16 KiB) beside five int32 arrays of flags and choices (20 KiB), and every pair is
// evaluated from those boxes whenever it is needed; there is no workspace.
//
// Matching.  The greedy rule of the header (take the first pair of the strict order, remove its slot and its detection,
// repeat) is run in rounds: every free slot knows the first pair of its row, every free detection the first pair of its
// column, and a pair that is first in both is in the greedy solution whatever else happens (nothing before it in the
// order shares its slot or its detection), so all such pairs of a round are taken at once.  The first pair overall is
// always among them: a round without a match means no pair is left.  A row's choice stays right until its detection is
// taken (rows and columns only lose members), so a thread rescans only then, and a thread that finds nothing is done
// for good.  A box that has left the matching (a void detection, a dead or duplicate slot, either side of a match) is
// overwritten in LDS by the empty box, which intersects nothing: a scan reads one 16-byte box per pair and no flag,
// four pairs' boxes before it evaluates the first, so the LDS latency is paid once per four pairs.  The number of
// rounds depends on the data (one round per match at worst: every box the same), the number of launches does not.
//
// flm_track_associate_streams runs the same body once per stream, one workgroup each, in one launch of S workgroups,
// on LDS arrays of 64, 256 or 1024 items -- the smallest that holds max(k, d).
#include "flm_common.h"
#include "flm_track_assoc_dev.h"
#include "flm_track_seed_dev.h"

namespace flm {

struct TrackAssocArgs {
  const int32_t* det;
  const int32_t* n_det;
  int d, k, c, in_h, in_w, fh, fw;
  int max_misses, square;
  double match_iou, dup_iou, refresh_iou;
  float* m_crop;
  int32_t* boxes;
  int32_t* status;
  int32_t* misses;
  double* state;
  int32_t* det_slot;
  int32_t* slot_det;
  int32_t* counts;
};
enum { CNT_MATCHED, CNT_BORN, CNT_REFRESHED, CNT_DUPLICATE, CNT_UNCONFIRMED, CNT_DROPPED, CNT_VOID, CNT_ZERO };

// Detection j as the matching sees it: through the box maths when the call asks for it.  Only for rows in range.
__device__ __forceinline__ AssocBox assoc_detection(const TrackAssocArgs& g, const AssocBox& raw) {
  return g.square ? assoc_square(raw) : raw;
}

// Slot `slot` starts from detection j as flm_track_seed would start it.
__device__ __forceinline__ void assoc_restart(const TrackAssocArgs& g, int slot, int j) {
  const int32_t* r = g.det + 4 * (size_t)j;
  const AssocBox q = assoc_detection(g, AssocBox{r[0], r[1], r[2], r[3]});
  const TrackSeed sd = track_seed_one(q.x0, q.y0, q.x1, q.y1, assoc_empty(assoc_clip(q, g.fh, g.fw)), g.in_h, g.in_w);
  track_seed_store(sd, g.m_crop + (size_t)slot * 6);
  int32_t* bo = g.boxes + 4 * (size_t)slot;
  bo[0] = q.x0; bo[1] = q.y0; bo[2] = q.x1; bo[3] = q.y1;
  g.status[slot] = sd.status;
  g.misses[slot] = 0;
}

// Slot `slot` is given up for the reason `bit`.
__device__ __forceinline__ void assoc_kill(const TrackAssocArgs& g, int slot, int bit) {
  float* o = g.m_crop + (size_t)slot * 6;
  o[0] = 1.f; o[1] = 0.f; o[2] = 0.f;
  o[3] = 0.f; o[4] = 1.f; o[5] = 0.f;
  int32_t* bo = g.boxes + 4 * (size_t)slot;
  bo[0] = 0; bo[1] = 0; bo[2] = 0; bo[3] = 0;
  g.status[slot] |= bit;
  g.misses[slot] = 0;
}

// The first pair, in the order of the header, among (mine, others[0..n)) with IoU >= match_iou; MINE_IS_SLOT says which
// side `self` indexes.  -> the other side's index, or -2; its inter and uni in bi, bu.
template <bool MINE_IS_SLOT>
__device__ __forceinline__ int assoc_scan(const AssocBox& mine, int64_t my_area, int self, const AssocBox* others, int n,
                                          double match_iou, int64_t& bi, int64_t& bu) {
  int best = -2;
  bi = 0;
  bu = 1;
  auto consider = [&](const AssocBox& o, int idx) {
    const int64_t in = assoc_inter(mine, o);
    if (in == 0) return;
    const int64_t un = assoc_union(my_area, assoc_area(o), in);
    if (!assoc_iou_ge(in, un, match_iou)) return;
    const bool first = MINE_IS_SLOT ? assoc_before(in, un, self, idx, bi, bu, self, best)
                                    : assoc_before(in, un, idx, self, bi, bu, best, self);
    if (best < 0 || first) {
      bi = in; bu = un; best = idx;
    }
  };
  int j = 0;
  for (; j + 4 <= n; j += 4) {
    const AssocBox o0 = others[j], o1 = others[j + 1], o2 = others[j + 2], o3 = others[j + 3];
    consider(o0, j);
    consider(o1, j + 1);
    consider(o2, j + 2);
    consider(o3, j + 3);
  }
  for (; j < n; ++j) consider(others[j], j);
  return best;
}

// One association, by one workgroup of max(k, d) threads rounded up to whole waves, on LDS arrays of CAP >= max(k, d)
// items: the body of both kernels below.  g names the K slots, the D detection rows and the outputs of THIS association;
// slot_base is what det_slot adds to a slot's index (the slot's place in a tracker that holds several associations'
// slots; slot_det and everything else stay local).  Integers and fixed float64 products only, and no loop bound but
// the wave-count loop depends on CAP: every CAP gives the same bits.
template <int CAP>
__device__ __forceinline__ void track_assoc_body(const TrackAssocArgs& g, const int slot_base) {
  __shared__ AssocBox tb[CAP], db[CAP];    // clipped boxes: slots, detections
  __shared__ int s_free[CAP], d_free[CAP];  // still to be matched
  __shared__ int s_best[CAP], d_best[CAP];  // a round's choices; later: born-from, the dead list
  __shared__ int fill[CAP];                 // the slot's state rows are to be reset
  __shared__ int wave_cnt[2][CAP / 64];
  __shared__ int cnt[8];
  const int i = threadIdx.x, k = g.k, d = g.d;
  const int lane = i & 63, wave = i >> 6;
  if (i < 8) cnt[i] = 0;
  if (i < 2 * (CAP / 64)) (&wave_cnt[0][0])[i] = 0;
  int nd = d;
  if (g.n_det) {
    const int v = *g.n_det;
    nd = v < 0 ? 0 : v > d ? d : v;
  }

  // ---- the boxes of both sides, clipped ----
  AssocBox tc{0, 0, 0, 0}, dc{0, 0, 0, 0};
  bool live = false, dvalid = false;
  if (i < k) {
    const int32_t* b = g.boxes + 4 * (size_t)i;
    tc = assoc_clip(AssocBox{b[0], b[1], b[2], b[3]}, g.fh, g.fw);
    live = !assoc_empty(tc);
  }
  if (i < nd) {
    const int32_t* r = g.det + 4 * (size_t)i;
    const AssocBox raw{r[0], r[1], r[2], r[3]};
    if (assoc_in_range(raw)) {
      dc = assoc_clip(assoc_detection(g, raw), g.fh, g.fw);
      dvalid = !assoc_empty(dc);
    }
  }
  tb[i] = tc;
  db[i] = dc;
  s_free[i] = live;
  d_free[i] = dvalid;
  fill[i] = 0;
  __syncthreads();

  // ---- duplicates: a live slot below covers the same face (s counts whether or not it is a duplicate itself) ----
  const int64_t ta = live ? assoc_area(tc) : 0, da = dvalid ? assoc_area(dc) : 0;
  bool dup = false;
  if (live) {
    for (int s = 0; s < i && !dup; ++s) {  // (a slot that is not live has an empty box: it intersects nothing)
      const AssocBox o = tb[s];
      const int64_t in = assoc_inter(tc, o);
      if (in == 0) continue;
      dup = assoc_iou_ge(in, assoc_union(ta, assoc_area(o), in), g.dup_iou);
    }
  }
  __syncthreads();
  const bool surv = live && !dup;
  s_free[i] = surv;
  if (!surv) tb[i] = AssocBox{0, 0, 0, 0};
  __syncthreads();

  // ---- matching in rounds ----
  int sb = surv ? -1 : -2, dbst = dvalid ? -1 : -2;  // -1: to be scanned, -2: nothing left, >= 0: the row's / column's first pair
  int my_det = -1;
  int64_t sbi = 0, sbu = 1, dbi = 0, dbu = 1, m_in = 0, m_un = 1;  // inter and uni of the choices, and of the match
  for (;;) {
    if (dbst != -2 && !d_free[i]) dbst = -2;  // (taken in the round before)
    if (sb == -1 || (sb >= 0 && !d_free[sb])) sb = assoc_scan<true>(tc, ta, i, db, nd, g.match_iou, sbi, sbu);
    if (dbst == -1 || (dbst >= 0 && !s_free[dbst])) dbst = assoc_scan<false>(dc, da, i, tb, k, g.match_iou, dbi, dbu);
    s_best[i] = sb;
    d_best[i] = dbst;
    __syncthreads();
    const bool m = sb >= 0 && d_best[sb] == i;
    const int any = __syncthreads_or(m);
    if (m) {
      s_free[i] = 0;
      d_free[sb] = 0;
      tb[i] = AssocBox{0, 0, 0, 0};
      db[sb] = AssocBox{0, 0, 0, 0};
      my_det = sb;
      m_in = sbi;
      m_un = sbu;
      g.det_slot[sb] = slot_base + i;
      sb = -2;
    }
    if (!any) break;
    __syncthreads();
  }

  // ---- births: unmatched detections, ascending, into the slots that were dead at entry, ascending ----
  const bool was_dead = i < k && !live;
  const bool unmatched = dvalid && d_free[i];
  const unsigned long long bal_dead = __ballot(was_dead), bal_unm = __ballot(unmatched);
  const unsigned long long below = (1ull << lane) - 1ull;
  int r_dead = __popcll(bal_dead & below), r_unm = __popcll(bal_unm & below);
  if (lane == 0) {
    wave_cnt[0][wave] = __popcll(bal_dead);
    wave_cnt[1][wave] = __popcll(bal_unm);
  }
  s_best[i] = -1;  // from here: the detection a slot is born from
  __syncthreads();
  int n_dead = 0;
  for (int w = 0; w < CAP / 64; ++w) {
    const int a = wave_cnt[0][w], b = wave_cnt[1][w];
    n_dead += a;
    if (w < wave) {
      r_dead += a;
      r_unm += b;
    }
  }
  if (was_dead) d_best[r_dead] = i;  // from here: the slots dead at entry, in order
  __syncthreads();
  if (unmatched) {
    if (r_unm < n_dead) {
      const int slot = d_best[r_unm];
      s_best[slot] = i;
      g.det_slot[i] = slot_base + slot;
      atomicAdd(&cnt[CNT_BORN], 1);
    } else {
      g.det_slot[i] = -2;
      atomicAdd(&cnt[CNT_DROPPED], 1);
    }
  } else if (i < d && !dvalid) {
    g.det_slot[i] = -1;
    if (i < nd) atomicAdd(&cnt[CNT_VOID], 1);
  }
  __syncthreads();

  // ---- what becomes of every slot ----
  if (i < k) {
    int sd = -1;
    if (dup) {
      assoc_kill(g, i, FLM_TRACK_DUPLICATE);
      atomicAdd(&cnt[CNT_DUPLICATE], 1);
    } else if (my_det >= 0) {
      sd = my_det;
      atomicAdd(&cnt[CNT_MATCHED], 1);
      if (g.refresh_iou > 0.0 && !assoc_iou_ge(m_in, m_un, g.refresh_iou)) {
        assoc_restart(g, i, my_det);
        fill[i] = 1;
        atomicAdd(&cnt[CNT_REFRESHED], 1);
      } else {
        g.misses[i] = 0;
      }
    } else if (surv) {
      const int mis = (int)((unsigned)g.misses[i] + 1u);
      if (g.max_misses > 0 && mis >= g.max_misses) {
        assoc_kill(g, i, FLM_TRACK_UNCONFIRMED);
        atomicAdd(&cnt[CNT_UNCONFIRMED], 1);
      } else {
        g.misses[i] = mis;
      }
    } else if (s_best[i] >= 0) {  // dead at entry, born now
      sd = s_best[i];
      assoc_restart(g, i, sd);
      fill[i] = 1;
    }
    g.slot_det[i] = sd;
  }
  __syncthreads();
  if (i < 8) g.counts[i] = cnt[i];

  // ---- the filter state of every restarted slot: no landmark has a history ----
  if (g.state) {
    const int c6 = g.c * 6, nt = blockDim.x;
    for (int s = 0; s < k; ++s) {
      if (!fill[s]) continue;
      double* p = g.state + (size_t)s * c6;
      for (int e = i; e < c6; e += nt) p[e] = -1.0;
    }
  }
}

// flm_track_associate: one workgroup, the arrays of the largest problem.
__global__ __launch_bounds__(kAssocMaxItems) void track_assoc_kernel(const TrackAssocArgs g) {
  track_assoc_body<kAssocMaxItems>(g, 0);
}

// flm_track_associate_streams: workgroup s is the association of stream s on its own slices -- slots [s*k, (s+1)*k),
// the rows det[s], n_det[s], det_slot[s], counts[s] -- so no pair of two streams exists.  LDS is dimensioned by CAP
// (3.4 KB at 64, 13 KB at 256), which is what lets many streams of a camera-sized tracker share a CU.  A stream whose
// n_det is negative is skipped: its workgroup writes the three outputs and returns before the first barrier, having
// read and written nothing of the stream's state; the test is uniform over the workgroup.
template <int CAP>
__global__ __launch_bounds__(CAP) void track_assoc_streams_kernel(const TrackAssocArgs g) {
  const int s = blockIdx.x, i = threadIdx.x, k = g.k, d = g.d;
  const size_t slot0 = (size_t)s * k, det0 = (size_t)s * d;
  if (g.n_det && g.n_det[s] < 0) {
    if (i < d) g.det_slot[det0 + i] = -1;
    if (i < k) g.slot_det[slot0 + i] = -1;
    if (i < 8) g.counts[(size_t)s * 8 + i] = 0;
    return;
  }
  TrackAssocArgs h = g;
  h.det = g.det + 4 * det0;
  h.n_det = g.n_det ? g.n_det + s : nullptr;
  h.m_crop = g.m_crop + 6 * slot0;
  h.boxes = g.boxes + 4 * slot0;
  h.status = g.status + slot0;
  h.misses = g.misses + slot0;
  h.state = g.state ? g.state + slot0 * (size_t)g.c * 6 : nullptr;
  h.det_slot = g.det_slot + det0;
  h.slot_det = g.slot_det + slot0;
  h.counts = g.counts + (size_t)s * 8;
  track_assoc_body<CAP>(h, (int)slot0);
}

static TrackAssocArgs track_assoc_args(const int32_t* det, const int32_t* n_det, int d, int k, int c, int in_h, int in_w,
                                       int fh, int fw, const flm_track_assoc_opts* opts, float* m_crop, int32_t* boxes,
                                       int32_t* status, int32_t* misses, double* state, int32_t* det_slot,
                                       int32_t* slot_det, int32_t* counts) {
  TrackAssocArgs g;
  g.det = det; g.n_det = n_det; g.d = d; g.k = k; g.c = c;
  g.in_h = in_h; g.in_w = in_w; g.fh = fh; g.fw = fw;
  g.max_misses = opts->max_misses; g.square = opts->square != 0;
  g.match_iou = opts->match_iou; g.dup_iou = opts->dup_iou; g.refresh_iou = opts->refresh_iou;
  g.m_crop = m_crop; g.boxes = boxes; g.status = status; g.misses = misses; g.state = state;
  g.det_slot = det_slot; g.slot_det = slot_det; g.counts = counts;
  return g;
}

int launch_track_associate(hipStream_t s, const int32_t* det, const int32_t* n_det, int d, int k, int c, int in_h, int in_w,
                           int fh, int fw, const flm_track_assoc_opts* opts, float* m_crop, int32_t* boxes, int32_t* status,
                           int32_t* misses, double* state, int32_t* det_slot, int32_t* slot_det, int32_t* counts) {
  const TrackAssocArgs g = track_assoc_args(det, n_det, d, k, c, in_h, in_w, fh, fw, opts, m_crop, boxes, status, misses,
                                            state, det_slot, slot_det, counts);
  const int n = k > d ? k : d;
  track_assoc_kernel<<<1, cdiv(n, 64) * 64, 0, s>>>(g);
  FLM_LAUNCH_CHECK("track_assoc_kernel");
  return FLM_OK;
}

// The smallest item capacity that holds max(k, d); the workgroup has max(k, d) threads rounded up to whole waves.
int launch_track_associate_streams(hipStream_t s, const int32_t* det, const int32_t* n_det, int n_streams, int d, int k,
                                   int c, int in_h, int in_w, int fh, int fw, const flm_track_assoc_opts* opts,
                                   float* m_crop, int32_t* boxes, int32_t* status, int32_t* misses, double* state,
                                   int32_t* det_slot, int32_t* slot_det, int32_t* counts) {
  const TrackAssocArgs g = track_assoc_args(det, n_det, d, k, c, in_h, in_w, fh, fw, opts, m_crop, boxes, status, misses,
                                            state, det_slot, slot_det, counts);
  const int n = k > d ? k : d;
  const dim3 grid(n_streams), block(cdiv(n, 64) * 64);
  if (n <= 64)
    track_assoc_streams_kernel<64><<<grid, block, 0, s>>>(g);
  else if (n <= 256)
    track_assoc_streams_kernel<256><<<grid, block, 0, s>>>(g);
  else
    track_assoc_streams_kernel<kAssocMaxItems><<<grid, block, 0, s>>>(g);
  FLM_LAUNCH_CHECK("track_assoc_streams_kernel");
  return FLM_OK;
}

}  // namespace flm
