// extern "C" entry points of the tracker (see include/flm.h): seed, step, gathers, association, quality and best shots,
// exits, head pose, pose-binned views, landmark flow and the flow tick on rows.
#include <cmath>
#include <cstring>

#include "flm_api_checks.h"
#include "flm_flow_rows_dev.h"

using namespace flm;

// Two sizes the best-shot, exit, pose and view calls share.
static int check_face_bytes(const char* who, size_t face_bytes) {
  if (face_bytes >= 1) return FLM_OK;
  set_error("%s: face_bytes=0, needs face_bytes >= 1", who);
  return FLM_ERR_SHAPE;
}
static int check_lm_strides(const char* who, size_t lm_stride, const double* wt, size_t w_stride) {
  if (lm_stride >= 2 && !(wt && w_stride < 1)) return FLM_OK;
  set_error("%s: lm_stride=%zu, w_stride=%zu, needs lm_stride >= 2 and w_stride >= 1", who, lm_stride, w_stride);
  return FLM_ERR_SHAPE;
}

extern "C" {

// ---- tracking (flm_track.hip) ------------------------------------------------------------------------------------

void flm_track_opts_init(flm_track_opts* opts) {
  if (!opts) return;
  opts->struct_size = (uint32_t)sizeof(flm_track_opts);
  opts->min_points = 2;
  opts->min_score = 0.0;
  opts->min_side = 0.0;
  opts->max_side = HUGE_VAL;
}

int flm_track_seed(flm_stream_t stream, const int32_t* boxes, int k, int in_h, int in_w, int fh, int fw, float* m,
                   int32_t* status) {
  if (!boxes || !m || !status) return null_argument("flm_track_seed");
  return launch_track_seed(static_cast<hipStream_t>(stream), boxes, k, in_h, in_w, fh, fw, m, status);
}

int flm_landmarks_from_crop(flm_stream_t stream, const double* lm, size_t lm_stride, const float* m, int k, int c,
                            double sx, double sy, double* out) {
  if (!lm || !m || !out) return null_argument("flm_landmarks_from_crop");
  return launch_landmarks_from_crop(static_cast<hipStream_t>(stream), lm, lm_stride, m, k, c, sx, sy, out);
}

// The pointer and option checks of the three step entry points; *opts is replaced by `defaults` when null.
static int check_track_step_args(const char* who, const double* lm, const float* m_crop, const int32_t* boxes,
                                 const double* tmpl_crop, const double* tmpl_align, const flm_track_opts** opts,
                                 flm_track_opts* defaults, const double* lm_frame, const float* m_align,
                                 const float* m_next, const int32_t* boxes_next, const int32_t* status) {
  // (wt is optional)
  if (!lm || !m_crop || !boxes || !tmpl_crop || !lm_frame || !m_next || !boxes_next || !status) return null_argument(who);
  if ((tmpl_align == nullptr) != (m_align == nullptr)) {
    set_error("%s: tmpl_align_dev and m_align_dev go together (both or neither)", who);
    return FLM_ERR_ARG;
  }
  if (const int rc = check_opts<false>(who, FLM_OPTS(flm_track_opts), opts, defaults)) return rc;
  const flm_track_opts* o = *opts;
  if (o->min_points < 2) {
    set_error("%s: min_points=%d, needs min_points >= 2 (a similarity takes two points)", who, o->min_points);
    return FLM_ERR_ARG;
  }
  if (std::isnan(o->min_score) || std::isnan(o->min_side) || std::isnan(o->max_side)) {
    set_error("%s: min_score, min_side and max_side must not be NaN (got %g, %g, %g)", who, o->min_score, o->min_side,
              o->max_side);
    return FLM_ERR_ARG;
  }
  return FLM_OK;
}

void flm_track_filter_init(flm_track_filter* filt) {
  if (!filt) return;
  filt->struct_size = (uint32_t)sizeof(flm_track_filter);
  filt->reserved = 0;
  filt->min_cutoff = 1.0;
  filt->beta = 15.0;
  filt->d_cutoff = 1.0;
}

// The checks of a flm_track_filter.
static int check_track_filter(const char* who, const flm_track_filter* filt) {
  if (const int rc = check_opts_head<true>(who, "flm_track_filter", filt)) return rc;
  if (!(filt->min_cutoff > 0.0)) {
    set_error("%s: min_cutoff=%g, needs min_cutoff > 0 (+inf switches the smoothing off)", who, filt->min_cutoff);
    return FLM_ERR_ARG;
  }
  if (!(filt->beta >= 0.0 && std::isfinite(filt->beta))) {
    set_error("%s: beta=%g, needs a finite beta >= 0", who, filt->beta);
    return FLM_ERR_ARG;
  }
  if (!(filt->d_cutoff > 0.0 && std::isfinite(filt->d_cutoff))) {
    set_error("%s: d_cutoff=%g, needs a finite d_cutoff > 0", who, filt->d_cutoff);
    return FLM_ERR_ARG;
  }
  return FLM_OK;
}

// The three step entry points, stated once.  need_filt: filt must be given (flm_track_step_filtered; flm_track_step has
// none to give, flm_track_step_rows may or may not).  rows: the call is flm_track_step_rows -- slot and status_rows
// must be given, dt_rows may replace the scalar dt, and the compact inputs must not overlap what is written at the slots.
static int track_step(const char* who, bool need_filt, bool rows, flm_stream_t stream, const double* lm, size_t lm_stride,
                      const double* wt, size_t w_stride, const float* m_crop, const int32_t* boxes, int k, int c, double sx,
                      double sy, int in_h, int in_w, int fh, int fw, const double* tmpl_crop, const double* tmpl_align,
                      const flm_track_opts* opts, double* lm_frame, float* m_align, float* m_next, int32_t* boxes_next,
                      int32_t* status, const flm_track_filter* filt, double dt, double* state, double* lm_raw,
                      const int32_t* slot, int n_slots, const double* dt_rows, int32_t* status_rows) {
  flm_track_opts defaults;
  if (const int rc = check_track_step_args(who, lm, m_crop, boxes, tmpl_crop, tmpl_align, &opts, &defaults, lm_frame, m_align,
                                           m_next, boxes_next, status))
    return rc;
  if (rows && (!slot || !status_rows)) {
    set_error("%s: null %s", who, !slot ? "slot_dev" : "status_rows_dev");
    return FLM_ERR_ARG;
  }
  if (filt || need_filt) {
    if (!filt || !state) {  // (lm_raw is optional)
      set_error("%s: null %s", who, !filt ? "filt" : "state_dev");
      return FLM_ERR_ARG;
    }
    if (const int rc = check_track_filter(who, filt)) return rc;
    if (!dt_rows && !(dt > 0.0 && std::isfinite(dt))) {
      set_error("%s: dt=%g, needs a finite dt > 0 (seconds since the previous step)%s", who, dt, rows ? " or dt_dev" : "");
      return FLM_ERR_ARG;
    }
  } else if (state || lm_raw || dt_rows) {
    set_error("%s: state_dev, lm_raw_dev and dt_dev go with filt", who);
    return FLM_ERR_ARG;
  }
  // the compact inputs must not be the tensors the step writes at the slots (the snapshot exists to keep them apart)
  if (rows && k >= 1 && k <= 65535 && n_slots >= 1 && n_slots <= 65535 &&
      (ranges_overlap(m_crop, (size_t)k * 24, m_next, (size_t)n_slots * 24) ||
       ranges_overlap(boxes, (size_t)k * 16, boxes_next, (size_t)n_slots * 16) ||
       ranges_overlap(status_rows, (size_t)k * 4, status, (size_t)n_slots * 4))) {
    set_error("%s: m_crop_c/m_next, boxes_c/boxes_next or status_rows/status overlap (rows are read while slots are "
              "written: gather a snapshot first)", who);
    return FLM_ERR_ARG;
  }
  return launch_track_step(static_cast<hipStream_t>(stream), who, lm, lm_stride, wt, w_stride, m_crop, boxes, k, c, sx, sy, in_h,
                           in_w, fh, fw, tmpl_crop, tmpl_align, opts, lm_frame, m_align, m_next, boxes_next, status, filt, dt,
                           state, lm_raw, slot, n_slots, dt_rows, status_rows);
}

int flm_track_step(flm_stream_t stream, const double* lm, size_t lm_stride, const double* wt, size_t w_stride,
                   const float* m_crop, const int32_t* boxes, int k, int c, double sx, double sy, int in_h, int in_w,
                   int fh, int fw, const double* tmpl_crop, const double* tmpl_align, const flm_track_opts* opts,
                   double* lm_frame, float* m_align, float* m_next, int32_t* boxes_next, int32_t* status) {
  return track_step("flm_track_step", false, false, stream, lm, lm_stride, wt, w_stride, m_crop, boxes, k, c, sx, sy, in_h,
                    in_w, fh, fw, tmpl_crop, tmpl_align, opts, lm_frame, m_align, m_next, boxes_next, status, nullptr, 0.0,
                    nullptr, nullptr, nullptr, 0, nullptr, nullptr);
}

int flm_track_step_filtered(flm_stream_t stream, const double* lm, size_t lm_stride, const double* wt, size_t w_stride,
                            const float* m_crop, const int32_t* boxes, int k, int c, double sx, double sy, int in_h,
                            int in_w, int fh, int fw, const double* tmpl_crop, const double* tmpl_align,
                            const flm_track_opts* opts, double* lm_frame, float* m_align, float* m_next,
                            int32_t* boxes_next, int32_t* status, const flm_track_filter* filt, double dt, double* state,
                            double* lm_raw) {
  return track_step("flm_track_step_filtered", true, false, stream, lm, lm_stride, wt, w_stride, m_crop, boxes, k, c, sx, sy,
                    in_h, in_w, fh, fw, tmpl_crop, tmpl_align, opts, lm_frame, m_align, m_next, boxes_next, status, filt, dt,
                    state, lm_raw, nullptr, 0, nullptr, nullptr);
}

int flm_track_step_rows(flm_stream_t stream, const double* lm, size_t lm_stride, const double* wt, size_t w_stride,
                        const float* m_crop_c, const int32_t* boxes_c, int n, int c, double sx, double sy, int in_h,
                        int in_w, int fh, int fw, const double* tmpl_crop, const double* tmpl_align,
                        const flm_track_opts* opts, double* lm_frame, float* m_align, float* m_next, int32_t* boxes_next,
                        int32_t* status, const flm_track_filter* filt, double dt, double* state, double* lm_raw,
                        const int32_t* slot, int n_slots, const double* dt_rows, int32_t* status_rows) {
  return track_step("flm_track_step_rows", false, true, stream, lm, lm_stride, wt, w_stride, m_crop_c, boxes_c, n, c, sx, sy,
                    in_h, in_w, fh, fw, tmpl_crop, tmpl_align, opts, lm_frame, m_align, m_next, boxes_next, status, filt, dt,
                    state, lm_raw, slot, n_slots, dt_rows, status_rows);
}

int flm_track_gather_streams(flm_stream_t stream, const int32_t* active, int a, int s, int k,
                             const int32_t* frame_idx_stream, const double* dt_stream, const float* m_crop,
                             const int32_t* boxes, const double* best_q, int32_t* reset, int32_t* slot_c, float* m_c,
                             int32_t* boxes_c, int32_t* frame_idx_c, double* dt_c, double* best_q_c, int32_t* reset_c) {
  const char* who = "flm_track_gather_streams";
  // (frame_idx_stream and the three optional groups may be null)
  if (!active || !m_crop || !boxes || !slot_c || !m_c || !boxes_c || !frame_idx_c) return null_argument(who);
  if ((dt_stream == nullptr) != (dt_c == nullptr) || (best_q == nullptr) != (best_q_c == nullptr) ||
      (reset == nullptr) != (reset_c == nullptr)) {
    set_error("%s: dt_stream_dev/dt_c, best_q_dev/best_q_c and reset_dev/reset_c go together (both or neither)", who);
    return FLM_ERR_ARG;
  }
  return launch_track_gather_streams(static_cast<hipStream_t>(stream), active, a, s, k, frame_idx_stream, dt_stream, m_crop,
                                     boxes, best_q, reset, slot_c, m_c, boxes_c, frame_idx_c, dt_c, best_q_c, reset_c);
}

// The three optional groups of flm_track_gather_live and flm_track_gather_flow and the clock that goes with the ages.
static int check_gather_groups(const char* who, const double* dt_stream, double dt, const double* best_q,
                               const int32_t* reset, const double* age, const double* dt_c, const double* best_q_c,
                               const int32_t* reset_c) {
  if ((age == nullptr) != (dt_c == nullptr) || (best_q == nullptr) != (best_q_c == nullptr) ||
      (reset == nullptr) != (reset_c == nullptr)) {
    set_error("%s: age_dev/dt_c, best_q_dev/best_q_c and reset_dev/reset_c go together (both or neither)", who);
    return FLM_ERR_ARG;
  }
  if (dt_stream && !age) {
    set_error("%s: dt_stream_dev goes with age_dev", who);
    return FLM_ERR_ARG;
  }
  if (age && !dt_stream && !(dt > 0.0 && std::isfinite(dt))) {
    set_error("%s: dt=%g, needs a finite dt > 0 (seconds since the previous step) or dt_stream_dev", who, dt);
    return FLM_ERR_ARG;
  }
  return FLM_OK;
}

int flm_track_gather_live(flm_stream_t stream, const int32_t* stream_on, int s, int k, int fh, int fw, int n,
                          const int32_t* frame_idx_stream, const double* dt_stream, double dt, const float* m_crop,
                          const int32_t* boxes, const double* best_q, int32_t* reset, double* age, int32_t* cursor,
                          int32_t* slot_c, float* m_c, int32_t* boxes_c, int32_t* frame_idx_c, double* dt_c,
                          double* best_q_c, int32_t* reset_c, int32_t* counts) {
  const char* who = "flm_track_gather_live";
  // (stream_on, frame_idx_stream, cursor and the three optional groups may be null)
  if (!m_crop || !boxes || !slot_c || !m_c || !boxes_c || !frame_idx_c || !counts) return null_argument(who);
  if (const int rc = check_gather_groups(who, dt_stream, dt, best_q, reset, age, dt_c, best_q_c, reset_c)) return rc;
  TrackLiveArgs g;
  g.boxes = boxes; g.m_crop = m_crop; g.s = s; g.k = k; g.fh = fh; g.fw = fw; g.n = n;
  g.stream_on = stream_on; g.frame_idx_stream = frame_idx_stream; g.dt_stream = dt_stream; g.dt = dt;
  g.best_q = best_q; g.reset = reset; g.age = age; g.cursor = cursor;
  g.slot_c = slot_c; g.m_c = m_c; g.boxes_c = boxes_c; g.frame_idx_c = frame_idx_c;
  g.dt_c = dt_c; g.best_q_c = best_q_c; g.reset_c = reset_c; g.counts = counts;
  return launch_track_gather_live(static_cast<hipStream_t>(stream), g);
}

// ---- association (flm_track_assoc.hip) ------------------------------------------------------------------------------

void flm_track_assoc_opts_init(flm_track_assoc_opts* opts) {
  if (!opts) return;
  opts->struct_size = (uint32_t)sizeof(flm_track_assoc_opts);
  opts->max_misses = 0;
  opts->square = 1;
  opts->reserved = 0;
  opts->match_iou = 0.3;
  opts->dup_iou = 0.7;
  opts->refresh_iou = 0.0;
}

// The checks flm_track_associate and flm_track_associate_streams share; *opts is replaced by `defaults` when null.
static int track_assoc_check(const char* who, const void* det, const void* m_crop, const void* boxes, const void* status,
                             const void* misses, const void* det_slot, const void* slot_det, const void* counts,
                             const flm_track_assoc_opts** opts, flm_track_assoc_opts* defaults) {
  // (n_det_dev, state_dev and opts are optional)
  if (!det || !m_crop || !boxes || !status || !misses || !det_slot || !slot_det || !counts) return null_argument(who);
  return check_opts<true>(who, FLM_OPTS(flm_track_assoc_opts), opts, defaults);
}

static int track_assoc_check_sizes(const char* who, int d, int k, int c, bool has_state, int in_h, int in_w, int fh, int fw,
                                   const flm_track_assoc_opts* opts) {
  if (const int rc = check_range(who, "k", k, 1, 1024)) return rc;
  if (const int rc = check_range(who, "d", d, 1, 1024)) return rc;
  if (has_state)
    if (const int rc = check_range(who, "c", c, 1, 1024)) return rc;
  if (in_h < 1 || in_w < 1 || fh < 1 || fw < 1) {
    set_error("%s: input %dx%d, frame %dx%d, needs in_h, in_w, fh, fw >= 1", who, in_h, in_w, fh, fw);
    return FLM_ERR_SHAPE;
  }
  if ((int64_t)fh * (int64_t)fw > (int64_t(1) << 30)) {
    set_error("%s: frame %dx%d, needs fh*fw <= 2^30 (the pair order is exact in int64 up to there)", who, fh, fw);
    return FLM_ERR_SHAPE;
  }
  if (opts->max_misses < 0) {
    set_error("%s: max_misses=%d, needs max_misses >= 0 (0 = never)", who, opts->max_misses);
    return FLM_ERR_SHAPE;
  }
  if (std::isnan(opts->match_iou) || std::isnan(opts->dup_iou) || std::isnan(opts->refresh_iou)) {
    set_error("%s: match_iou, dup_iou and refresh_iou must not be NaN (got %g, %g, %g)", who, opts->match_iou,
              opts->dup_iou, opts->refresh_iou);
    return FLM_ERR_SHAPE;
  }
  return FLM_OK;
}

int flm_track_associate(flm_stream_t stream, const int32_t* det, const int32_t* n_det, int d, int k, int c, int in_h,
                        int in_w, int fh, int fw, const flm_track_assoc_opts* opts, float* m_crop, int32_t* boxes,
                        int32_t* status, int32_t* misses, double* state, int32_t* det_slot, int32_t* slot_det,
                        int32_t* counts) {
  const char* who = "flm_track_associate";
  flm_track_assoc_opts defaults;
  int rc = track_assoc_check(who, det, m_crop, boxes, status, misses, det_slot, slot_det, counts, &opts, &defaults);
  if (rc != FLM_OK) return rc;
  rc = track_assoc_check_sizes(who, d, k, c, state != nullptr, in_h, in_w, fh, fw, opts);
  if (rc != FLM_OK) return rc;
  return launch_track_associate(static_cast<hipStream_t>(stream), det, n_det, d, k, c, in_h, in_w, fh, fw, opts, m_crop,
                                boxes, status, misses, state, det_slot, slot_det, counts);
}

int flm_track_associate_streams(flm_stream_t stream, const int32_t* det, const int32_t* n_det, int s, int d, int k, int c,
                                int in_h, int in_w, int fh, int fw, const flm_track_assoc_opts* opts, float* m_crop,
                                int32_t* boxes, int32_t* status, int32_t* misses, double* state, int32_t* det_slot,
                                int32_t* slot_det, int32_t* counts) {
  const char* who = "flm_track_associate_streams";
  flm_track_assoc_opts defaults;
  int rc = track_assoc_check(who, det, m_crop, boxes, status, misses, det_slot, slot_det, counts, &opts, &defaults);
  if (rc != FLM_OK) return rc;
  if (s < 1) {
    set_error("%s: s=%d, needs 1 <= s", who, s);
    return FLM_ERR_SHAPE;
  }
  if (k >= 1 && (int64_t)s * (int64_t)k > 65535) {
    set_error("%s: s=%d streams of k=%d slots, needs s*k <= 65535 (the capacity of the warps and the tracker)", who, s, k);
    return FLM_ERR_SHAPE;
  }
  rc = track_assoc_check_sizes(who, d, k, c, state != nullptr, in_h, in_w, fh, fw, opts);
  if (rc != FLM_OK) return rc;
  return launch_track_associate_streams(static_cast<hipStream_t>(stream), det, n_det, s, d, k, c, in_h, in_w, fh, fw, opts,
                                        m_crop, boxes, status, misses, state, det_slot, slot_det, counts);
}

// ---- best shot (flm_quality.hip) ------------------------------------------------------------------------------------

void flm_quality_opts_init(flm_quality_opts* opts) {
  if (!opts) return;
  opts->struct_size = (uint32_t)sizeof(flm_quality_opts);
  opts->dark = 16;
  opts->bright = 239;
}

int flm_face_quality(flm_stream_t stream, const void* faces, int k, int h, int w, const flm_image_format* fmt,
                     const flm_quality_opts* opts, int64_t* rec) {
  const char* who = "flm_face_quality";
  if (!faces || !rec) return null_argument(who);  // (fmt and opts are optional)
  flm_image_format plain;
  flm_image_format_init(&plain);
  if (!fmt) fmt = &plain;
  if (const int rc = check_image_format(who, fmt)) return rc;
  if (const int rc = check_image_aligned(who, "faces", faces, fmt)) return rc;
  for (int c = 0; c < 3; ++c) {
    if (fmt->scale[c] == 0.0f) {
      set_error("%s: scale[%d] is 0, needs a scale that can be undone (scale != 0)", who, c);
      return FLM_ERR_ARG;
    }
  }
  flm_quality_opts defaults;
  if (const int rc = check_opts<false>(who, FLM_OPTS(flm_quality_opts), &opts, &defaults)) return rc;
  if (opts->dark < 0 || opts->dark > 255 || opts->bright < 0 || opts->bright > 255) {
    set_error("%s: dark=%d, bright=%d, needs both in [0, 255]", who, opts->dark, opts->bright);
    return FLM_ERR_ARG;
  }
  return launch_face_quality(static_cast<hipStream_t>(stream), faces, k, h, w, fmt, opts, rec);
}

void flm_best_opts_init(flm_best_opts* opts) {
  if (!opts) return;
  opts->struct_size = (uint32_t)sizeof(flm_best_opts);
  opts->reserved = 0;
  opts->sharp_ref = 100.0;
  opts->min_exposed = 0.5;
}

// The option and size checks flm_track_best_update and flm_track_best_update_rows share; *popts is replaced by `defaults`
// when null.  kname: what the call names its number of faces.
static int check_best_args(const char* who, const flm_best_opts** popts, flm_best_opts* defaults, const char* kname, int k,
                           int c, size_t face_bytes, size_t lm_stride, const double* wt, size_t w_stride) {
  if (const int rc = check_opts<true>(who, FLM_OPTS(flm_best_opts), popts, defaults)) return rc;
  const flm_best_opts* opts = *popts;
  if (!(opts->sharp_ref > 0.0)) {
    set_error("%s: sharp_ref=%g, needs sharp_ref > 0", who, opts->sharp_ref);
    return FLM_ERR_ARG;
  }
  if (std::isnan(opts->min_exposed)) {
    set_error("%s: min_exposed must not be NaN", who);
    return FLM_ERR_ARG;
  }
  if (const int rc = check_range(who, kname, k, 1, 65535)) return rc;
  if (c < 1) {
    set_error("%s: c=%d, needs c >= 1", who, c);
    return FLM_ERR_SHAPE;
  }
  if (const int rc = check_face_bytes(who, face_bytes)) return rc;
  return check_lm_strides(who, lm_stride, wt, w_stride);
}

int flm_track_best_update(flm_stream_t stream, const void* faces, size_t face_bytes, int k, const int64_t* rec,
                          const int32_t* status, const int32_t* reset, const double* lm, size_t lm_stride,
                          const double* wt, size_t w_stride, int c, const double* factor, const float* m,
                          int64_t frame_id, const flm_best_opts* opts, const double* best_q_in, double* best_q_out,
                          void* gallery, int64_t* best_frame, float* best_m, double* best_lm, int64_t* best_rec) {
  const char* who = "flm_track_best_update";
  // (status, reset, w, factor, m, opts and the last three outputs are optional)
  if (!faces || !rec || !lm || !best_q_in || !best_q_out || !gallery || !best_frame) return null_argument(who);
  if (best_m && !m) {
    set_error("%s: best_m_dev needs m_dev", who);
    return FLM_ERR_ARG;
  }
  flm_best_opts defaults;
  if (const int rc = check_best_args(who, &opts, &defaults, "k", k, c, face_bytes, lm_stride, wt, w_stride)) return rc;
  if (ranges_overlap(best_q_in, (size_t)k * sizeof(double), best_q_out, (size_t)k * sizeof(double))) {
    set_error("%s: best_q_in and best_q_out overlap (every workgroup of a slot reads best_q_in: swap two buffers)", who);
    return FLM_ERR_ARG;
  }
  if (ranges_overlap(faces, (size_t)k * face_bytes, gallery, (size_t)k * face_bytes)) {
    set_error("%s: faces_dev and gallery_dev overlap", who);
    return FLM_ERR_ARG;
  }
  return launch_track_best_update(static_cast<hipStream_t>(stream), faces, face_bytes, k, rec, status, reset, lm, lm_stride,
                                  wt, w_stride, c, factor, m, frame_id, opts, nullptr, 0, best_q_in, best_q_out, gallery,
                                  best_frame, best_m, best_lm, best_rec);
}

int flm_track_best_update_rows(flm_stream_t stream, const void* faces, size_t face_bytes, int n, const int64_t* rec,
                               const int32_t* status_rows, const int32_t* reset_c, const double* lm, size_t lm_stride,
                               const double* wt, size_t w_stride, int c, const double* factor, const float* m,
                               int64_t frame_id, const flm_best_opts* opts, const int32_t* slot, int n_slots,
                               const double* best_q_c, double* best_q, void* gallery, int64_t* best_frame, float* best_m,
                               double* best_lm, int64_t* best_rec) {
  const char* who = "flm_track_best_update_rows";
  // (status, reset, w, factor, m, opts and the last three outputs are optional)
  if (!faces || !rec || !lm || !slot || !best_q_c || !best_q || !gallery || !best_frame) return null_argument(who);
  if (best_m && !m) {
    set_error("%s: best_m_dev needs m_dev", who);
    return FLM_ERR_ARG;
  }
  flm_best_opts defaults;
  if (const int rc = check_best_args(who, &opts, &defaults, "n", n, c, face_bytes, lm_stride, wt, w_stride)) return rc;
  if (const int rc = check_range(who, "n_slots", n_slots, 1, 65535)) return rc;
  if (ranges_overlap(best_q_c, (size_t)n * sizeof(double), best_q, (size_t)n_slots * sizeof(double))) {
    set_error("%s: best_q_c and best_q overlap (every workgroup of a row reads best_q_c: it is the snapshot)", who);
    return FLM_ERR_ARG;
  }
  if (ranges_overlap(faces, (size_t)n * face_bytes, gallery, (size_t)n_slots * face_bytes)) {
    set_error("%s: faces_dev and gallery_dev overlap", who);
    return FLM_ERR_ARG;
  }
  return launch_track_best_update(static_cast<hipStream_t>(stream), faces, face_bytes, n, rec, status_rows, reset_c, lm,
                                  lm_stride, wt, w_stride, c, factor, m, frame_id, opts, slot, n_slots, best_q_c, best_q,
                                  gallery, best_frame, best_m, best_lm, best_rec);
}

// ---- finished tracks (flm_track_exit.hip) -----------------------------------------------------------------------------

void flm_exit_opts_init(flm_exit_opts* opts) {
  if (!opts) return;
  opts->struct_size = (uint32_t)sizeof(flm_exit_opts);
  opts->reserved = 0;
  opts->min_q = 0.0;
}

int flm_track_retire(flm_stream_t stream, const int32_t* boxes, const int32_t* status, int k, int fh, int fw,
                     const double* best_q, const void* gallery, size_t face_bytes, const int64_t* best_frame,
                     const float* best_m, const double* best_lm, int c, const int64_t* best_rec, int64_t frame_id,
                     int flush, const flm_exit_opts* opts, int32_t* born, int64_t* track_id, int64_t* born_frame,
                     int64_t* head, int q, void* x_gallery, int64_t* x_meta, double* x_q, float* x_m, double* x_lm,
                     int64_t* x_rec, int32_t* exit_row) {
  const char* who = "flm_track_retire";
  if (!boxes || !status || !best_q || !gallery || !best_frame || !born || !track_id || !born_frame || !head ||
      !x_gallery || !x_meta || !x_q || !exit_row)
    return null_argument(who);  // (opts and the three pairs best_m/x_m, best_lm/x_lm, best_rec/x_rec are optional)
  if (!best_m != !x_m || !best_lm != !x_lm || !best_rec != !x_rec) {
    set_error("%s: best_m_dev goes with x_m, best_lm_dev with x_lm and best_rec_dev with x_rec: both or neither", who);
    return FLM_ERR_ARG;
  }
  flm_exit_opts defaults;
  if (const int rc = check_opts<true>(who, FLM_OPTS(flm_exit_opts), &opts, &defaults)) return rc;
  if (!(opts->min_q >= 0.0)) {
    set_error("%s: min_q=%g, needs min_q >= 0", who, opts->min_q);
    return FLM_ERR_ARG;
  }
  if (const int rc = check_range(who, "k", k, 1, 65535)) return rc;
  if (const int rc = check_range(who, "q", q, 1, 65535)) return rc;
  if (const int rc = check_range(who, "c", c, 1, 1024)) return rc;
  if (const int rc = check_face_bytes(who, face_bytes)) return rc;
  if (fh < 1 || fw < 1) {
    set_error("%s: frame %dx%d, needs fh, fw >= 1", who, fh, fw);
    return FLM_ERR_SHAPE;
  }
  const size_t sk = (size_t)k, sq = (size_t)q, sc = (size_t)c;
  const NamedRange bufs[] = {
      {boxes, sk * 16, "boxes_dev"}, {status, sk * 4, "status_dev"}, {best_q, sk * 8, "best_q_dev"},
      {gallery, sk * face_bytes, "gallery_dev"}, {best_frame, sk * 8, "best_frame_dev"}, {best_m, sk * 24, "best_m_dev"},
      {best_lm, sk * sc * 16, "best_lm_dev"}, {best_rec, sk * FLM_QUALITY_REC * 8, "best_rec_dev"},
      {born, sk * 4, "born_dev"}, {track_id, sk * 8, "track_id_dev"}, {born_frame, sk * 8, "born_frame_dev"},
      {head, 4 * 8, "head_dev"}, {x_gallery, sq * face_bytes, "x_gallery"}, {x_meta, sq * FLM_EXIT_META * 8, "x_meta"},
      {x_q, sq * 8, "x_q"}, {x_m, sq * 24, "x_m"}, {x_lm, sq * sc * 16, "x_lm"},
      {x_rec, sq * FLM_QUALITY_REC * 8, "x_rec"}, {exit_row, sk * 4, "exit_row_dev"}};
  if (const int rc = check_apart(who, bufs, "%s: %s and %s overlap (no two arguments may)")) return rc;
  TrackExitArgs g;
  g.boxes = boxes; g.status = status; g.k = k; g.fh = fh; g.fw = fw; g.c = c; g.q = q;
  g.face_bytes = face_bytes;
  g.best_q = best_q; g.gallery = static_cast<const unsigned char*>(gallery); g.best_frame = best_frame;
  g.best_m = best_m; g.best_lm = best_lm; g.best_rec = best_rec;
  g.frame_id = frame_id; g.flush = flush; g.min_q = opts->min_q;
  g.born = born; g.track_id = track_id; g.born_frame = born_frame; g.head = head;
  g.x_gallery = static_cast<unsigned char*>(x_gallery); g.x_meta = x_meta; g.x_q = x_q;
  g.x_m = x_m; g.x_lm = x_lm; g.x_rec = x_rec; g.exit_row = exit_row;
  return launch_track_retire(static_cast<hipStream_t>(stream), g);
}

// ---- head pose (flm_pose.hip) ---------------------------------------------------------------------------------------

void flm_pose_opts_init(flm_pose_opts* opts) {
  if (!opts) return;
  opts->struct_size = (uint32_t)sizeof(flm_pose_opts);
  opts->reserved = 0;
  opts->min_volume = 1e-6;
  opts->min_frontal = 0.0;
}

int flm_head_pose(flm_stream_t stream, const double* lm, size_t lm_stride, const double* wt, size_t w_stride, int n, int c,
                  const int32_t* idx, const double* xyz, int p, const flm_pose_opts* opts, const int32_t* slot,
                  int n_slots, double* pose, double* factor) {
  const char* who = "flm_head_pose";
  if (!lm || !idx || !xyz || !pose) return null_argument(who);  // (w, opts, slot and factor_out are optional)
  flm_pose_opts defaults;
  if (const int rc = check_opts<true>(who, FLM_OPTS(flm_pose_opts), &opts, &defaults)) return rc;
  if (!(opts->min_volume >= 0.0)) {
    set_error("%s: min_volume=%g, needs min_volume >= 0", who, opts->min_volume);
    return FLM_ERR_ARG;
  }
  if (!(opts->min_frontal >= 0.0 && opts->min_frontal <= 1.0)) {
    set_error("%s: min_frontal=%g, needs 0 <= min_frontal <= 1", who, opts->min_frontal);
    return FLM_ERR_ARG;
  }
  if (const int rc = check_range(who, "n", n, 1, 65535)) return rc;
  if (const int rc = check_range(who, "c", c, 1, 1024)) return rc;
  if (const int rc = check_range(who, "p", p, 4, 256)) return rc;
  if (const int rc = check_lm_strides(who, lm_stride, wt, w_stride)) return rc;
  if (slot)
    if (const int rc = check_range(who, "n_slots", n_slots, 1, 65535)) return rc;
  const size_t last = (size_t)n * c - 1;  // the last landmark read
  const NamedRange in[] = {
      {lm, (last * lm_stride + 2) * sizeof(double), "lm_dev"},
      {wt, wt ? (last * w_stride + 1) * sizeof(double) : 0, "w_dev"},
      {idx, (size_t)p * sizeof(int32_t), "idx_dev"},
      {xyz, (size_t)p * 3 * sizeof(double), "xyz_dev"},
      {slot, slot ? (size_t)n * sizeof(int32_t) : 0, "slot_dev"}};
  const size_t pose_bytes = (size_t)(slot ? n_slots : n) * FLM_POSE_REC * sizeof(double);
  const size_t factor_bytes = factor ? (size_t)n * sizeof(double) : 0;
  // (one message for both outputs, input by input: the pair is named by hand, not through check_outputs_apart)
  for (const NamedRange& a : in) {
    if (!a.p) continue;
    if (ranges_overlap(pose, pose_bytes, a.p, a.bytes) || (factor && ranges_overlap(factor, factor_bytes, a.p, a.bytes))) {
      set_error("%s: pose_dev or factor_out overlaps %s", who, a.name);
      return FLM_ERR_ARG;
    }
  }
  if (factor && ranges_overlap(pose, pose_bytes, factor, factor_bytes)) {
    set_error("%s: pose_dev and factor_out overlap", who);
    return FLM_ERR_ARG;
  }
  return launch_head_pose(static_cast<hipStream_t>(stream), lm, lm_stride, wt, w_stride, n, c, idx, xyz, p, opts, slot,
                          n_slots, pose, factor);
}

// ---- openness and blink state (flm_parts.hip) -----------------------------------------------------------------------

void flm_open_opts_init(flm_open_opts* opts) {
  if (!opts) return;
  memset(opts, 0, sizeof(*opts));
  opts->struct_size = (uint32_t)sizeof(flm_open_opts);
  opts->n_measures = 3;
  static const int32_t width[3][2] = {{36, 39}, {42, 45}, {60, 64}};
  static const int32_t upper[3][4] = {{37, 38, 0, 0}, {43, 44, 0, 0}, {61, 62, 63, 0}};
  static const int32_t lower[3][4] = {{41, 40, 0, 0}, {47, 46, 0, 0}, {67, 66, 65, 0}};
  for (int g = 0; g < 3; ++g) {
    opts->n_pairs[g] = g < 2 ? 2 : 3;
    for (int j = 0; j < 2; ++j) opts->width[g][j] = width[g][j];
    for (int j = 0; j < 4; ++j) {
      opts->upper[g][j] = upper[g][j];
      opts->lower[g][j] = lower[g][j];
    }
  }
  opts->close_below = 0.18;
  opts->open_above = 0.22;
  opts->min_closed = 0.03;
  opts->max_closed = 0.5;
  opts->min_width = 4.0;
}

int flm_face_openness(flm_stream_t stream, const double* lm, size_t lm_stride, const double* wt, size_t w_stride, int n, int c,
                      const flm_open_opts* opts, const int32_t* slot, int n_slots, double* rec, double* state,
                      int32_t* reset, const double* dt_dev, double dt, const int32_t* status, int64_t frame_id) {
  const char* who = "flm_face_openness";
  if (!lm || !rec) return null_argument(who);  // (w, opts, slot, state, dt_dev and status_rows are optional)
  if (state && !reset) {
    set_error("%s: state_dev needs reset_dev", who);
    return FLM_ERR_ARG;
  }
  flm_open_opts defaults;
  if (const int rc = check_opts<true>(who, FLM_OPTS(flm_open_opts), &opts, &defaults)) return rc;
  if (opts->n_measures < 1 || opts->n_measures > FLM_OPEN_MAX_MEASURES) {
    set_error("%s: n_measures=%d outside 1 <= n_measures <= %d", who, opts->n_measures, FLM_OPEN_MAX_MEASURES);
    return FLM_ERR_ARG;
  }
  for (int g = 0; g < opts->n_measures; ++g)
    if (opts->n_pairs[g] < 1 || opts->n_pairs[g] > FLM_OPEN_MAX_PAIRS) {
      set_error("%s: n_pairs[%d]=%d outside 1 <= n_pairs <= %d", who, g, opts->n_pairs[g], FLM_OPEN_MAX_PAIRS);
      return FLM_ERR_ARG;
    }
  if (!(opts->close_below < opts->open_above)) {
    set_error("%s: close_below=%g, open_above=%g, needs close_below < open_above", who, opts->close_below, opts->open_above);
    return FLM_ERR_ARG;
  }
  if (!(opts->min_closed >= 0.0) || !(opts->max_closed >= 0.0) || !(opts->min_width >= 0.0)) {
    set_error("%s: min_closed=%g, max_closed=%g, min_width=%g, each needs to be >= 0", who, opts->min_closed,
              opts->max_closed, opts->min_width);
    return FLM_ERR_ARG;
  }
  if (opts->max_closed < opts->min_closed) {
    set_error("%s: max_closed=%g is below min_closed=%g", who, opts->max_closed, opts->min_closed);
    return FLM_ERR_ARG;
  }
  if (state && !dt_dev && !(dt > 0.0 && std::isfinite(dt))) {
    set_error("%s: dt=%g, needs dt finite and > 0", who, dt);
    return FLM_ERR_ARG;
  }
  if (const int rc = check_range(who, "n", n, 1, 65535)) return rc;
  if (const int rc = check_range(who, "c", c, 1, 1024)) return rc;
  if (const int rc = check_lm_strides(who, lm_stride, wt, w_stride)) return rc;
  if (slot)
    if (const int rc = check_range(who, "n_slots", n_slots, 1, 65535)) return rc;
  const size_t last = (size_t)n * c - 1;  // the last landmark read
  const size_t rows = (size_t)(slot ? n_slots : n), gm = (size_t)opts->n_measures;
  const NamedRange in[] = {
      {lm, (last * lm_stride + 2) * sizeof(double), "lm_dev"},
      {wt, wt ? (last * w_stride + 1) * sizeof(double) : 0, "w_dev"},
      {slot, slot ? (size_t)n * sizeof(int32_t) : 0, "slot_dev"},
      {dt_dev, dt_dev ? (size_t)n * sizeof(double) : 0, "dt_dev"},
      {status, status ? (size_t)n * sizeof(int32_t) : 0, "status_rows_dev"}};
  const NamedRange out[] = {
      {rec, rows * gm * FLM_OPEN_REC * sizeof(double), "rec_dev"},
      {state, state ? rows * gm * FLM_OPEN_STATE * sizeof(double) : 0, "state_dev"},
      {state ? reset : nullptr, rows * sizeof(int32_t), "reset_dev"}};
  if (const int rc = check_outputs_apart(who, in, out, "%s: %s overlaps %s", "%s: %s and %s overlap")) return rc;
  return launch_face_openness(static_cast<hipStream_t>(stream), lm, lm_stride, wt, w_stride, n, c, opts, slot, n_slots, rec,
                              state, state ? reset : nullptr, state ? dt_dev : nullptr, dt, state ? status : nullptr,
                              frame_id);
}

// ---- pose-binned best shots (flm_track_views.hip) -------------------------------------------------------------------

void flm_views_opts_init(flm_views_opts* opts) {
  if (!opts) return;
  memset(opts, 0, sizeof(*opts));
  opts->struct_size = (uint32_t)sizeof(flm_views_opts);
  opts->sharp_ref = 100.0;
  opts->min_exposed = 0.5;
  opts->n_u = 2;
  opts->u_edge[0] = -0.3420201433256687;  // -+sin(20 degrees): right, frontal, left
  opts->u_edge[1] = 0.3420201433256687;
  opts->n_v = 0;
}

static int check_view_edges(const char* who, const char* axis, int n, const double* edge) {
  if (n < 0 || n > FLM_VIEWS_MAX_EDGES) {
    set_error("%s: n_%s=%d, needs 0 <= n_%s <= %d", who, axis, n, axis, FLM_VIEWS_MAX_EDGES);
    return FLM_ERR_ARG;
  }
  for (int i = 0; i < n; ++i) {
    if (!(edge[i] > -1.0 && edge[i] < 1.0)) {  // (false for a NaN and for an infinity)
      set_error("%s: %s_edge[%d]=%g, needs a finite edge inside (-1, 1)", who, axis, i, edge[i]);
      return FLM_ERR_ARG;
    }
    if (i > 0 && !(edge[i] > edge[i - 1])) {
      set_error("%s: %s_edge[%d]=%g after %g, needs strictly ascending edges", who, axis, i, edge[i], edge[i - 1]);
      return FLM_ERR_ARG;
    }
  }
  return FLM_OK;
}

int flm_track_views_update(flm_stream_t stream, const void* faces, size_t face_bytes, int n, const int64_t* rec,
                           const int32_t* status_rows, const int32_t* reset, const double* lm, size_t lm_stride,
                           const double* wt, size_t w_stride, int c, const float* m, int64_t frame_id,
                           const flm_views_opts* opts, const int32_t* slot, int n_slots, const double* pose, double* view_q,
                           int64_t* view_frame, void* view_gallery, float* view_m, double* view_lm, double* view_pose,
                           int32_t* take) {
  const char* who = "flm_track_views_update";
  // (status, reset, w, m, opts, slot and the three view_m/lm/pose are optional)
  if (!faces || !rec || !lm || !pose || !view_q || !view_frame || !view_gallery || !take) return null_argument(who);
  if (view_m && !m) {
    set_error("%s: view_m needs m_dev", who);
    return FLM_ERR_ARG;
  }
  flm_views_opts defaults;
  if (const int rc = check_opts<true>(who, FLM_OPTS(flm_views_opts), &opts, &defaults)) return rc;
  if (!(opts->sharp_ref > 0.0)) {
    set_error("%s: sharp_ref=%g, needs sharp_ref > 0", who, opts->sharp_ref);
    return FLM_ERR_ARG;
  }
  if (std::isnan(opts->min_exposed)) {
    set_error("%s: min_exposed must not be NaN", who);
    return FLM_ERR_ARG;
  }
  if (const int rc = check_view_edges(who, "u", opts->n_u, opts->u_edge)) return rc;
  if (const int rc = check_view_edges(who, "v", opts->n_v, opts->v_edge)) return rc;
  if (const int rc = check_range(who, "n", n, 1, 65535)) return rc;
  if (slot)
    if (const int rc = check_range(who, "n_slots", n_slots, 1, 65535)) return rc;
  if (!slot) n_slots = n;
  if (const int rc = check_range(who, "c", c, 1, 1024)) return rc;
  if (const int rc = check_face_bytes(who, face_bytes)) return rc;
  if (const int rc = check_lm_strides(who, lm_stride, wt, w_stride)) return rc;
  const int bins = (opts->n_u + 1) * (opts->n_v + 1);
  const size_t sn = (size_t)n, ss = (size_t)n_slots * bins, sc = (size_t)c;
  const size_t last = sn * sc - 1;  // the last landmark read
  const NamedRange in[] = {
      {faces, sn * face_bytes, "faces_dev"}, {rec, sn * FLM_QUALITY_REC * 8, "rec_dev"},
      {status_rows, sn * 4, "status_rows_dev"}, {reset, sn * 4, "reset_dev"},
      {lm, (last * lm_stride + 2) * sizeof(double), "lm_dev"}, {wt, (last * w_stride + 1) * sizeof(double), "w_dev"},
      {m, sn * 24, "m_dev"}, {slot, sn * 4, "slot_dev"}, {pose, (size_t)n_slots * FLM_POSE_REC * 8, "pose_dev"}};
  const NamedRange out[] = {
      {view_q, ss * 8, "view_q"}, {view_frame, ss * 8, "view_frame"}, {view_gallery, ss * face_bytes, "view_gallery"},
      {view_m, ss * 24, "view_m"}, {view_lm, ss * sc * 16, "view_lm"}, {view_pose, ss * FLM_POSE_REC * 8, "view_pose"},
      {take, sn * 4, "take_dev"}};
  if (const int rc = check_outputs_apart(who, in, out, "%s: %s and %s overlap (no output may overlap an input)",
                                         "%s: %s and %s overlap (no two outputs may)"))
    return rc;
  TrackViewsArgs g;
  g.faces = static_cast<const unsigned char*>(faces);
  g.face_bytes = face_bytes;
  g.n = n; g.n_slots = n_slots; g.c = c; g.bins = bins;
  g.rec = rec; g.status = status_rows; g.reset = reset;
  g.lm = lm; g.lm_stride = lm_stride; g.wt = wt; g.w_stride = w_stride; g.m = m; g.frame_id = frame_id;
  g.sharp_ref = opts->sharp_ref; g.min_exposed = opts->min_exposed;
  g.n_u = opts->n_u; g.n_v = opts->n_v;
  for (int i = 0; i < FLM_VIEWS_MAX_EDGES; ++i) {  // (the edges not in use are never compared: zeros keep the struct defined)
    g.u_edge[i] = i < opts->n_u ? opts->u_edge[i] : 0.0;
    g.v_edge[i] = i < opts->n_v ? opts->v_edge[i] : 0.0;
  }
  g.slot = slot; g.pose = pose;
  g.view_q = view_q; g.view_frame = view_frame; g.view_gallery = static_cast<unsigned char*>(view_gallery);
  g.view_m = view_m; g.view_lm = view_lm; g.view_pose = view_pose; g.take = take;
  return launch_track_views_update(static_cast<hipStream_t>(stream), g);
}

int flm_track_exit_views(flm_stream_t stream, const int32_t* exit_row, int k, int q, int bins, size_t face_bytes, int c,
                         const double* view_q, const int64_t* view_frame, const void* view_gallery, const float* view_m,
                         const double* view_lm, const double* view_pose, double* x_view_q, int64_t* x_view_frame,
                         void* x_view_gallery, float* x_view_m, double* x_view_lm, double* x_view_pose) {
  const char* who = "flm_track_exit_views";
  // (the three pairs view_m/x_view_m, view_lm/x_view_lm, view_pose/x_view_pose are optional)
  if (!exit_row || !view_q || !view_frame || !view_gallery || !x_view_q || !x_view_frame || !x_view_gallery)
    return null_argument(who);
  if (!view_m != !x_view_m || !view_lm != !x_view_lm || !view_pose != !x_view_pose) {
    set_error("%s: view_m goes with x_view_m, view_lm with x_view_lm and view_pose with x_view_pose: both or neither", who);
    return FLM_ERR_ARG;
  }
  if (const int rc = check_range(who, "k", k, 1, 65535)) return rc;
  if (const int rc = check_range(who, "q", q, 1, 65535)) return rc;
  if (const int rc = check_range(who, "bins", bins, 1, 64)) return rc;
  if (const int rc = check_range(who, "c", c, 1, 1024)) return rc;
  if (const int rc = check_face_bytes(who, face_bytes)) return rc;
  const size_t sk = (size_t)k * bins, sq = (size_t)q * bins, sc = (size_t)c;
  const NamedRange bufs[] = {
      {exit_row, (size_t)k * 4, "exit_row_dev"}, {view_q, sk * 8, "view_q"}, {view_frame, sk * 8, "view_frame"},
      {view_gallery, sk * face_bytes, "view_gallery"}, {view_m, sk * 24, "view_m"}, {view_lm, sk * sc * 16, "view_lm"},
      {view_pose, sk * FLM_POSE_REC * 8, "view_pose"}, {x_view_q, sq * 8, "x_view_q"},
      {x_view_frame, sq * 8, "x_view_frame"}, {x_view_gallery, sq * face_bytes, "x_view_gallery"},
      {x_view_m, sq * 24, "x_view_m"}, {x_view_lm, sq * sc * 16, "x_view_lm"},
      {x_view_pose, sq * FLM_POSE_REC * 8, "x_view_pose"}};
  if (const int rc = check_apart(who, bufs, "%s: %s and %s overlap (no two arguments may)")) return rc;
  TrackExitViewsArgs g;
  g.exit_row = exit_row; g.k = k; g.q = q; g.bins = bins; g.c = c; g.face_bytes = face_bytes;
  g.view_q = view_q; g.view_frame = view_frame; g.view_gallery = static_cast<const unsigned char*>(view_gallery);
  g.view_m = view_m; g.view_lm = view_lm; g.view_pose = view_pose;
  g.x_view_q = x_view_q; g.x_view_frame = x_view_frame; g.x_view_gallery = static_cast<unsigned char*>(x_view_gallery);
  g.x_view_m = x_view_m; g.x_view_lm = x_view_lm; g.x_view_pose = x_view_pose;
  return launch_track_exit_views(static_cast<hipStream_t>(stream), g);
}

// ---- landmark flow (flm_flow.hip; the flow launch of both calls is in flm_flow_rows.hip) ----------------------------

size_t flm_flow_pyramid_bytes(int h, int w, int levels) {
  if (h < 1 || w < 1 || levels < 1 || levels > 6) return 0;
  size_t bytes = 0;
  for (int l = 0; l < levels; ++l) bytes += (size_t)(h >> l) * (size_t)(w >> l);
  return bytes;
}

// The geometry both flow calls share.
static int check_flow_geometry(const char* who, int h, int w, int levels) {
  if (const int rc = check_range(who, "levels", levels, 1, 6)) return rc;
  const int t = 1 << (levels - 1);
  if (h < 1 || w < 1 || h > 32768 || w > 32768 || h % t || w % t || (h >> (levels - 1)) < 2 || (w >> (levels - 1)) < 2) {
    set_error("%s: crop %dx%d with %d levels, needs h and w <= 32768, multiples of 2^(levels-1) = %d and at least %d",
              who, h, w, levels, t, 2 * t);
    return FLM_ERR_SHAPE;
  }
  return FLM_OK;
}

int flm_flow_pyramid(flm_stream_t stream, const uint8_t* src, int n, int h, int w, int ch, int levels, uint8_t* pyr) {
  const char* who = "flm_flow_pyramid";
  if (!src || !pyr) return null_argument(who);
  if (const int rc = check_range(who, "n", n, 1, 131070)) return rc;
  if (ch != 1 && ch != 3) {
    set_error("%s: ch=%d, needs ch 1 (luma) or 3 (BGR)", who, ch);
    return FLM_ERR_SHAPE;
  }
  if (int rc = check_flow_geometry(who, h, w, levels)) return rc;
  const long long tiles = (long long)((h + 31) / 32) * ((w + 31) / 32) * n;
  if (tiles >= (1ll << 31)) {
    set_error("%s: %d crops of %dx%d are %lld tiles of 32x32, needs fewer than 2^31", who, n, h, w, tiles);
    return FLM_ERR_SHAPE;
  }
  if (ranges_overlap(src, (size_t)n * h * w * ch, pyr, (size_t)n * flm_flow_pyramid_bytes(h, w, levels))) {
    set_error("%s: pyr_dev overlaps src_dev", who);
    return FLM_ERR_ARG;
  }
  return launch_flow_pyramid(static_cast<hipStream_t>(stream), src, n, h, w, ch, levels, pyr);
}

void flm_flow_opts_init(flm_flow_opts* opts) {
  if (!opts) return;
  opts->struct_size = (uint32_t)sizeof(flm_flow_opts);
  opts->reserved = 0;
  opts->levels = 4;
  opts->radius = 7;
  opts->max_iter = 10;
  opts->pad = 0;
  opts->eps = 0.03;
  opts->min_eig = 0.5;
  opts->max_err = 12.0;
  opts->max_move = 64.0;
}

// The options every flow call takes: the struct's header and the four numbers; *popts is replaced by `defaults` when
// null.  (reserved and pad share one message here, so the header check leaves reserved to it.)
static int check_flow_opts(const char* who, const flm_flow_opts** popts, flm_flow_opts* defaults) {
  if (const int rc = check_opts<false>(who, FLM_OPTS(flm_flow_opts), popts, defaults)) return rc;
  const flm_flow_opts* opts = *popts;
  if (opts->reserved != 0 || opts->pad != 0) {
    set_error("%s: flm_flow_opts reserved=%u, pad=%d, both must be 0", who, opts->reserved, opts->pad);
    return FLM_ERR_ARG;
  }
  if (!(opts->eps > 0.0)) {
    set_error("%s: eps=%g, needs eps > 0", who, opts->eps);
    return FLM_ERR_ARG;
  }
  if (!(opts->min_eig >= 0.0)) {
    set_error("%s: min_eig=%g, needs min_eig >= 0", who, opts->min_eig);
    return FLM_ERR_ARG;
  }
  if (!(opts->max_err >= 0.0)) {
    set_error("%s: max_err=%g, needs max_err >= 0", who, opts->max_err);
    return FLM_ERR_ARG;
  }
  if (!(opts->max_move > 0.0)) {
    set_error("%s: max_move=%g, needs max_move > 0", who, opts->max_move);
    return FLM_ERR_ARG;
  }
  return FLM_OK;
}

// The window of every flow call: radius and max_iter (after the call's own sizes, the order flm_landmark_flow had).
static int check_flow_window(const char* who, const flm_flow_opts* opts) {
  if (const int rc = check_range(who, "radius", opts->radius, 1, 7)) return rc;
  if (const int rc = check_range(who, "max_iter", opts->max_iter, 1, 64)) return rc;
  return FLM_OK;
}

// How the flow family words an output that overlaps an input or another output (check_outputs_apart).
static const char kOverlaps[] = "%s: %s overlaps %s";

int flm_landmark_flow(flm_stream_t stream, const uint8_t* pyr_prev, const uint8_t* pyr_cur, int k, int h, int w,
                      const double* lm_prev, const double* w_prev, const float* m, int c, const flm_flow_opts* opts,
                      double* lm_out, double* w_out, int32_t* err_out, int32_t* flags_out) {
  const char* who = "flm_landmark_flow";
  // (w_prev, opts, w_out and err_out are optional)
  if (!pyr_prev || !pyr_cur || !lm_prev || !m || !lm_out || !flags_out) return null_argument(who);
  flm_flow_opts defaults;
  if (int rc = check_flow_opts(who, &opts, &defaults)) return rc;
  if (const int rc = check_range(who, "k", k, 1, 65535)) return rc;
  if (const int rc = check_range(who, "c", c, 1, 1024)) return rc;
  if (int rc = check_flow_window(who, opts)) return rc;
  if (int rc = check_flow_geometry(who, h, w, opts->levels)) return rc;
  const size_t pyr = (size_t)k * flm_flow_pyramid_bytes(h, w, opts->levels), kc = (size_t)k * c;
  const NamedRange in[] = {{pyr_prev, pyr, "pyr_prev_dev"}, {pyr_cur, pyr, "pyr_cur_dev"},
                           {lm_prev, kc * 16, "lm_prev_dev"}, {w_prev, w_prev ? kc * 8 : 0, "w_prev_dev"},
                           {m, (size_t)k * 24, "m_dev"}};
  const NamedRange out[] = {{lm_out, kc * 16, "lm_out_dev"}, {w_out, kc * 8, "w_out_dev"},
                            {err_out, kc * 4, "err_out_dev"}, {flags_out, kc * 4, "flags_out_dev"}};
  if (int rc = check_outputs_apart(who, in, out, kOverlaps, kOverlaps)) return rc;
  return launch_landmark_flow_rows(static_cast<hipStream_t>(stream), pyr_prev, pyr_cur, k, h, w, nullptr, k, lm_prev,
                                   w_prev, m, c, opts, 0.0, lm_out, w_out, err_out, nullptr, flags_out);
}

// ---- the flow tick on rows (flm_flow_rows.hip) ------------------------------------------------------------------------

int flm_track_gather_flow(flm_stream_t stream, const int32_t* stream_on, int s, int k, int fh, int fw, int n,
                          const int32_t* frame_idx_stream, const double* dt_stream, double dt, const float* m_crop,
                          const int32_t* boxes, const double* best_q, int32_t* reset, double* age, int32_t* cursor,
                          const int32_t* flow_frame, int32_t* flow_ready, int32_t* slot_c, float* m_c, int32_t* boxes_c,
                          int32_t* frame_idx_c, int32_t* prev_frame_idx_c, double* dt_c, double* best_q_c, int32_t* reset_c,
                          int32_t* counts) {
  const char* who = "flm_track_gather_flow";
  if (!m_crop || !boxes || !flow_frame || !flow_ready || !slot_c || !m_c || !boxes_c || !frame_idx_c || !prev_frame_idx_c ||
      !counts)
    return null_argument(who);  // (stream_on, frame_idx_stream, cursor and the three optional groups may be null)
  if (const int rc = check_gather_groups(who, dt_stream, dt, best_q, reset, age, dt_c, best_q_c, reset_c)) return rc;
  TrackFlowArgs g;
  g.boxes = boxes; g.m_crop = m_crop; g.s = s; g.k = k; g.fh = fh; g.fw = fw; g.n = n;
  g.stream_on = stream_on; g.frame_idx_stream = frame_idx_stream; g.dt_stream = dt_stream; g.dt = dt;
  g.best_q = best_q; g.reset = reset; g.age = age; g.cursor = cursor; g.flow_frame = flow_frame; g.flow_ready = flow_ready;
  g.slot_c = slot_c; g.m_c = m_c; g.boxes_c = boxes_c; g.frame_idx_c = frame_idx_c; g.prev_frame_idx_c = prev_frame_idx_c;
  g.dt_c = dt_c; g.best_q_c = best_q_c; g.reset_c = reset_c; g.counts = counts;
  if (n >= 1 && n <= 65535 && s >= 1 && k >= 1 && (long long)s * k <= 65535) {   // (the launcher names a size outside)
    const size_t ns = (size_t)s * k, nr = (size_t)n;
    const NamedRange in[] = {{stream_on, stream_on ? (size_t)s * 4 : 0, "stream_on_dev"},
                             {frame_idx_stream, frame_idx_stream ? (size_t)s * 4 : 0, "frame_idx_stream_dev"},
                             {dt_stream, dt_stream ? (size_t)s * 8 : 0, "dt_stream_dev"}, {m_crop, ns * 24, "m_crop_dev"},
                             {boxes, ns * 16, "boxes_dev"}, {best_q, best_q ? ns * 8 : 0, "best_q_dev"},
                             {flow_frame, ns * 4, "flow_frame_dev"}};
    const NamedRange out[] = {{reset, ns * 4, "reset_dev"}, {age, ns * 8, "age_dev"}, {cursor, 4, "cursor_dev"},
                              {flow_ready, ns * 4, "flow_ready_dev"}, {slot_c, nr * 4, "slot_c"}, {m_c, nr * 24, "m_c"},
                              {boxes_c, nr * 16, "boxes_c"}, {frame_idx_c, nr * 4, "frame_idx_c"},
                              {prev_frame_idx_c, nr * 4, "prev_frame_idx_c"}, {dt_c, nr * 8, "dt_c"},
                              {best_q_c, nr * 8, "best_q_c"}, {reset_c, nr * 4, "reset_c"}, {counts, 24, "counts_dev"}};
    if (int rc = check_outputs_apart(who, in, out, kOverlaps, kOverlaps)) return rc;
  }
  return launch_track_gather_flow(static_cast<hipStream_t>(stream), g);
}

int flm_landmark_flow_rows(flm_stream_t stream, const uint8_t* pyr_prev, const uint8_t* pyr_cur, int n, int h, int w,
                           const int32_t* slot, int n_slots, const double* lm_prev, const double* w_prev, const float* m,
                           int c, const flm_flow_opts* opts, double max_fb, double* lm_out, double* w_out,
                           int32_t* err_out, double* fb_out, int32_t* flags_out) {
  const char* who = "flm_landmark_flow_rows";
  // (w_prev, opts, w_out and err_out are optional)
  if (!pyr_prev || !pyr_cur || !slot || !lm_prev || !m || !lm_out || !fb_out || !flags_out) return null_argument(who);
  flm_flow_opts defaults;
  if (int rc = check_flow_opts(who, &opts, &defaults)) return rc;
  if (!(max_fb >= 0.0 && std::isfinite(max_fb))) {
    set_error("%s: max_fb=%g, needs a finite max_fb >= 0 (0: no forward-backward check)", who, max_fb);
    return FLM_ERR_ARG;
  }
  if (const int rc = check_range(who, "n", n, 1, 65535)) return rc;
  if (const int rc = check_range(who, "n_slots", n_slots, 1, 65535)) return rc;
  if (const int rc = check_range(who, "c", c, 1, 1024)) return rc;
  if (int rc = check_flow_window(who, opts)) return rc;
  if (int rc = check_flow_geometry(who, h, w, opts->levels)) return rc;
  const size_t pyr = (size_t)n * flm_flow_pyramid_bytes(h, w, opts->levels), nc = (size_t)n * c, sc = (size_t)n_slots * c;
  const NamedRange in[] = {{pyr_prev, pyr, "pyr_prev_dev"}, {pyr_cur, pyr, "pyr_cur_dev"}, {slot, (size_t)n * 4, "slot_dev"},
                           {lm_prev, sc * 16, "lm_prev_dev"}, {w_prev, w_prev ? sc * 8 : 0, "w_prev_dev"},
                           {m, (size_t)n * 24, "m_dev"}};
  const NamedRange out[] = {{lm_out, nc * 16, "lm_out_dev"}, {w_out, nc * 8, "w_out_dev"}, {err_out, nc * 4, "err_out_dev"},
                            {fb_out, nc * 8, "fb_out_dev"}, {flags_out, nc * 4, "flags_out_dev"}};
  if (int rc = check_outputs_apart(who, in, out, kOverlaps, kOverlaps)) return rc;
  return launch_landmark_flow_rows(static_cast<hipStream_t>(stream), pyr_prev, pyr_cur, n, h, w, slot, n_slots, lm_prev,
                                   w_prev, m, c, opts, max_fb, lm_out, w_out, err_out, fb_out, flags_out);
}

int flm_track_flow_history_put(flm_stream_t stream, const int32_t* slot, const int32_t* status_rows,
                               const int32_t* frame_idx_c, const double* lm_rows, const double* w_rows, int n, int n_slots,
                               int c, double* hist_lm, double* hist_w, int32_t* flow_frame, int32_t* flow_ready) {
  const char* who = "flm_track_flow_history_put";
  // (lm_rows/hist_lm_dev and w_rows/hist_w_dev are optional)
  if (!slot || !status_rows || !frame_idx_c || !flow_frame || !flow_ready) return null_argument(who);
  if ((lm_rows == nullptr) != (hist_lm == nullptr) || (w_rows == nullptr) != (hist_w == nullptr)) {
    set_error("%s: lm_rows_dev/hist_lm_dev and w_rows_dev/hist_w_dev go together (both or neither)", who);
    return FLM_ERR_ARG;
  }
  if (w_rows && !lm_rows) {
    set_error("%s: w_rows_dev goes with lm_rows_dev", who);
    return FLM_ERR_ARG;
  }
  if (const int rc = check_range(who, "n", n, 1, 65535)) return rc;
  if (const int rc = check_range(who, "n_slots", n_slots, 1, 65535)) return rc;
  if (const int rc = check_range(who, "c", c, 1, 1024)) return rc;
  const size_t nc = (size_t)n * c, sc = (size_t)n_slots * c;
  const NamedRange in[] = {{slot, (size_t)n * 4, "slot_dev"}, {status_rows, (size_t)n * 4, "status_rows_dev"},
                           {frame_idx_c, (size_t)n * 4, "frame_idx_c"}, {lm_rows, nc * 16, "lm_rows_dev"},
                           {w_rows, nc * 8, "w_rows_dev"}};
  const NamedRange out[] = {{hist_lm, sc * 16, "hist_lm_dev"}, {hist_w, sc * 8, "hist_w_dev"},
                            {flow_frame, (size_t)n_slots * 4, "flow_frame_dev"},
                            {flow_ready, (size_t)n_slots * 4, "flow_ready_dev"}};
  if (int rc = check_outputs_apart(who, in, out, kOverlaps, kOverlaps)) return rc;
  FlowPutArgs g;
  g.slot = slot; g.status_rows = status_rows; g.frame_idx_c = frame_idx_c; g.lm_rows = lm_rows; g.w_rows = w_rows;
  g.n = n; g.n_slots = n_slots; g.c = c; g.hist_lm = hist_lm; g.hist_w = hist_w; g.flow_frame = flow_frame;
  g.flow_ready = flow_ready;
  return launch_flow_history_put(static_cast<hipStream_t>(stream), g);
}

}  // extern "C"
