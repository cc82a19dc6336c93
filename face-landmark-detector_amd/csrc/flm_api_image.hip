// extern "C" entry points of the image side (see include/flm.h): similarity fits, warps, crops, frame-space landmarks,
// image and frame formats, NV12 rings, the mesh warp, frame annotation.
#include <cstring>

#include "flm_annotate_dev.h"
#include "flm_api_checks.h"

using namespace flm;

extern "C" {

int flm_similarity_from_landmarks(flm_stream_t stream, const double* lm, const double* tmpl, int n, int k,
                                  float* m) {
  if (!lm || !tmpl || !m) return null_argument("flm_similarity_from_landmarks");
  return launch_similarity(static_cast<hipStream_t>(stream), lm, tmpl, n, k, 1.0, 1.0, m);
}

int flm_similarity_from_landmarks_scaled(flm_stream_t stream, const double* lm, const double* tmpl, int n, int k,
                                         double sx, double sy, float* m) {
  if (!lm || !tmpl || !m) return null_argument("flm_similarity_from_landmarks_scaled");
  return launch_similarity(static_cast<hipStream_t>(stream), lm, tmpl, n, k, sx, sy, m);
}

int flm_similarity_from_landmarks_weighted(flm_stream_t stream, const double* lm, size_t lm_stride, const double* wt,
                                           size_t w_stride, const double* tmpl, int n, int k, double sx, double sy,
                                           float* m) {
  if (!lm || !tmpl || !m) return null_argument("flm_similarity_from_landmarks_weighted");  // (wt is optional)
  return launch_similarity_weighted(static_cast<hipStream_t>(stream), lm, lm_stride, wt, w_stride, tmpl, n, k, sx, sy, m);
}

int flm_warp_affine(flm_stream_t stream, const void* src, int src_is_u8, int n, int hs, int ws, const float* m,
                    float* dst, int hd, int wd) {
  if (!src || !m || !dst) return null_argument("flm_warp_affine");
  return launch_warp(static_cast<hipStream_t>(stream), src, src_is_u8, n, hs, ws, m, dst, hd, wd);
}

int flm_crop_resize(flm_stream_t stream, const uint8_t* frame, int fh, int fw, const int32_t* boxes, int k,
                    uint8_t* out, int oh, int ow) {
  if (!frame || !boxes || !out) return null_argument("flm_crop_resize");
  return launch_crop_resize(static_cast<hipStream_t>(stream), frame, fh, fw, boxes, k, out, oh, ow);
}

int flm_crop_resize_frames(flm_stream_t stream, const uint8_t* frames, size_t frame_stride, int nframes, int fh, int fw,
                           const int32_t* boxes, const int32_t* frame_idx, int k, uint8_t* out, int oh, int ow) {
  if (!frames || !boxes || !frame_idx || !out) return null_argument("flm_crop_resize_frames");
  return launch_crop_resize(static_cast<hipStream_t>(stream), frames, fh, fw, boxes, k, out, oh, ow, frame_idx,
                            frame_stride, nframes);
}

int flm_landmarks_to_frame(flm_stream_t stream, const double* lm, const int32_t* boxes, int k, int c, int grid_h,
                           int grid_w, int fh, int fw, double* out) {
  if (!lm || !boxes || !out) return null_argument("flm_landmarks_to_frame");
  return launch_landmarks_to_frame(static_cast<hipStream_t>(stream), lm, boxes, k, c, grid_h, grid_w, fh, fw, out);
}

int flm_warp_affine_frames(flm_stream_t stream, const uint8_t* frames, size_t frame_stride, int nframes, int fh, int fw,
                           const int32_t* frame_idx, const int32_t* boxes, const float* m, int k, float* dst, int hd,
                           int wd, int samples) {
  if (!frames || !m || !dst) return null_argument("flm_warp_affine_frames");  // frame_idx and boxes are optional
  return launch_warp_frames(static_cast<hipStream_t>(stream), frames, frame_stride, nframes, fh, fw, frame_idx, boxes, m,
                            k, dst, hd, wd, samples);
}

void flm_image_format_init(flm_image_format* fmt) {
  if (!fmt) return;
  fmt->struct_size = (uint32_t)sizeof(flm_image_format);
  fmt->layout = FLM_LAYOUT_NHWC;
  fmt->type = FLM_PIX_F32;
  fmt->reverse_channels = 0;
  for (int c = 0; c < 3; ++c) {
    fmt->scale[c] = 1.0f;
    fmt->bias[c] = 0.0f;
  }
}

size_t flm_image_format_bytes(const flm_image_format* fmt, int n, int h, int w) {
  if (check_image_format("flm_image_format_bytes", fmt) != FLM_OK) return 0;
  if (n < 1 || h < 1 || w < 1) {
    set_error("flm_image_format_bytes: n, h, w must be >= 1 (got %d, %d, %d)", n, h, w);
    return 0;
  }
  return (size_t)n * (size_t)h * (size_t)w * 3 * image_element_bytes(fmt);
}

int flm_warp_affine_fmt(flm_stream_t stream, const void* src, int src_is_u8, int n, int hs, int ws, const float* m,
                        void* dst, int hd, int wd, const flm_image_format* fmt) {
  if (!src || !m || !dst) return null_argument("flm_warp_affine_fmt");
  if (const int rc = check_image_format("flm_warp_affine_fmt", fmt)) return rc;
  if (const int rc = check_image_dst("flm_warp_affine_fmt", dst, fmt)) return rc;
  return launch_warp_fmt(static_cast<hipStream_t>(stream), src, src_is_u8, n, hs, ws, m, dst, hd, wd, fmt);
}

int flm_warp_affine_frames_fmt(flm_stream_t stream, const uint8_t* frames, size_t frame_stride, int nframes, int fh,
                               int fw, const int32_t* frame_idx, const int32_t* boxes, const float* m, int k, void* dst,
                               int hd, int wd, int samples, const flm_image_format* fmt) {
  if (!frames || !m || !dst) return null_argument("flm_warp_affine_frames_fmt");  // frame_idx and boxes are optional
  if (const int rc = check_image_format("flm_warp_affine_frames_fmt", fmt)) return rc;
  if (const int rc = check_image_dst("flm_warp_affine_frames_fmt", dst, fmt)) return rc;
  return launch_warp_frames_fmt(static_cast<hipStream_t>(stream), frames, frame_stride, nframes, fh, fw, frame_idx, boxes,
                                m, k, dst, hd, wd, samples, fmt);
}

// ---- frame formats: the ring as the decoder hands it out (flm_frames_nv12.hip) -------------------------------

void flm_frame_format_init(flm_frame_format* src) {
  if (!src) return;
  src->struct_size = (uint32_t)sizeof(flm_frame_format);
  src->pixel = FLM_FRAME_BGR24;
  src->matrix = FLM_YUV_BT601_LIMITED;
  src->y_pitch = 0;
  src->uv_pitch = 0;
  src->uv_offset = 0;
}

size_t flm_frame_format_bytes(const flm_frame_format* src, int fh, int fw) {
  if (check_frame_format("flm_frame_format_bytes", src) != FLM_OK) return 0;
  if (src->pixel == FLM_FRAME_NV12) return nv12_format_bytes("flm_frame_format_bytes", src, fh, fw);
  if (fh < 1 || fw < 1) {
    set_error("flm_frame_format_bytes: frame %dx%d, needs fh, fw >= 1", fh, fw);
    return 0;
  }
  return (size_t)fh * (size_t)fw * 3;
}

int flm_frames_to_bgr(flm_stream_t stream, const uint8_t* frames, size_t frame_stride, int nframes, int fh, int fw,
                      const flm_frame_format* src, uint8_t* out) {
  if (!frames || !out) return null_argument("flm_frames_to_bgr");
  if (const int rc = check_frame_format("flm_frames_to_bgr", src)) return rc;
  if (src->pixel != FLM_FRAME_NV12) {
    set_error("flm_frames_to_bgr: the source is BGR24 already (pixel must be FLM_FRAME_NV12)");
    return FLM_ERR_ARG;
  }
  return launch_frames_to_bgr_nv12(static_cast<hipStream_t>(stream), frames, frame_stride, nframes, fh, fw, src, out);
}

int flm_crop_resize_frames_src(flm_stream_t stream, const uint8_t* frames, size_t frame_stride, int nframes, int fh,
                               int fw, const int32_t* boxes, const int32_t* frame_idx, int k, uint8_t* out, int oh,
                               int ow, const flm_frame_format* src) {
  if (!frames || !boxes || !frame_idx || !out) return null_argument("flm_crop_resize_frames_src");
  if (const int rc = check_frame_format("flm_crop_resize_frames_src", src)) return rc;
  if (src->pixel == FLM_FRAME_BGR24)
    return launch_crop_resize(static_cast<hipStream_t>(stream), frames, fh, fw, boxes, k, out, oh, ow, frame_idx,
                              frame_stride, nframes);
  return launch_crop_resize_nv12(static_cast<hipStream_t>(stream), frames, frame_stride, nframes, fh, fw, boxes,
                                 frame_idx, k, out, oh, ow, src);
}

int flm_warp_affine_frames_src(flm_stream_t stream, const uint8_t* frames, size_t frame_stride, int nframes, int fh,
                               int fw, const int32_t* frame_idx, const int32_t* boxes, const float* m, int k, void* dst,
                               int hd, int wd, int samples, const flm_image_format* fmt, const flm_frame_format* src) {
  if (!frames || !m || !dst) return null_argument("flm_warp_affine_frames_src");  // frame_idx and boxes are optional
  if (const int rc = check_frame_format("flm_warp_affine_frames_src", src)) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (src->pixel == FLM_FRAME_BGR24 && !fmt)  // flm_warp_affine_frames, its checks and no others
    return launch_warp_frames(s, frames, frame_stride, nframes, fh, fw, frame_idx, boxes, m, k, static_cast<float*>(dst), hd,
                              wd, samples);
  flm_image_format plain;  // fmt NULL: float32 NHWC BGR, scale 1, bias 0
  flm_image_format_init(&plain);
  if (fmt) {
    if (const int rc = check_image_format("flm_warp_affine_frames_src", fmt)) return rc;
  }
  if (const int rc = check_image_dst("flm_warp_affine_frames_src", dst, fmt ? fmt : &plain)) return rc;
  if (src->pixel == FLM_FRAME_BGR24)
    return launch_warp_frames_fmt(s, frames, frame_stride, nframes, fh, fw, frame_idx, boxes, m, k, dst, hd, wd, samples,
                                  fmt);
  return launch_warp_frames_nv12(s, frames, frame_stride, nframes, fh, fw, frame_idx, boxes, m, k, dst, hd, wd, samples,
                                 fmt ? fmt : &plain, src);
}

// ---- the piecewise-affine warp over the landmark mesh (flm_mesh.hip) -------------------------------------------------

int flm_mesh_map(flm_stream_t stream, const double* pts, const int32_t* tris, int p, int t, int hd, int wd,
                 uint8_t* map) {
  if (!pts || !tris || !map) return null_argument("flm_mesh_map");
  return launch_mesh_map(static_cast<hipStream_t>(stream), pts, tris, p, t, hd, wd, map);
}

int flm_mesh_affines(flm_stream_t stream, const double* lm, int lm_stride, const float* m, const double* pts,
                     const int32_t* tris, int p, int a, int t, int k, double min_det, float* aff) {
  if (!lm || !m || !pts || !tris || !aff) return null_argument("flm_mesh_affines");
  return launch_mesh_affines(static_cast<hipStream_t>(stream), lm, lm_stride, m, pts, tris, p, a, t, k, min_det, aff);
}

int flm_warp_mesh_frames(flm_stream_t stream, const uint8_t* frames, size_t frame_stride, int nframes, int fh, int fw,
                         const int32_t* frame_idx, const int32_t* boxes, const double* lm, int lm_stride, const float* m,
                         const double* pts, const int32_t* tris, int p, int a, int t, const uint8_t* map, int k,
                         void* dst, int hd, int wd, int samples, const flm_image_format* fmt,
                         const flm_frame_format* src, double min_det, float* aff_out) {
  if (!frames || !lm || !m || !pts || !tris || !map || !dst) return null_argument("flm_warp_mesh_frames");  // frame_idx, boxes, fmt, src and aff_out are optional
  flm_frame_format bgr;  // src NULL: the dense BGR ring
  flm_frame_format_init(&bgr);
  if (src) {
    if (const int rc = check_frame_format("flm_warp_mesh_frames", src)) return rc;
  }
  flm_image_format plain;  // fmt NULL: float32 NHWC BGR, scale 1, bias 0
  flm_image_format_init(&plain);
  if (fmt) {
    if (const int rc = check_image_format("flm_warp_mesh_frames", fmt)) return rc;
  }
  if (const int rc = check_image_dst("flm_warp_mesh_frames", dst, fmt ? fmt : &plain)) return rc;
  return launch_warp_mesh_frames(static_cast<hipStream_t>(stream), frames, frame_stride, nframes, fh, fw, frame_idx, boxes,
                                 lm, lm_stride, m, pts, tris, p, a, t, map, k, dst, hd, wd, samples, fmt ? fmt : &plain,
                                 src ? src : &bgr, min_det, aff_out);
}

// ---- face parts (flm_parts.hip) -----------------------------------------------------------------------------------------

int flm_part_affines(flm_stream_t stream, const double* lm, size_t lm_stride, const double* wt, size_t w_stride, int k, int c,
                     const int32_t* part_idx, const double* part_tmpl, const int32_t* part_n, int r, float* aff,
                     int32_t* part_ok) {
  if (!lm || !part_idx || !part_tmpl || !part_n || !aff || !part_ok) return null_argument("flm_part_affines");  // (w is optional)
  return launch_part_affines(static_cast<hipStream_t>(stream), lm, lm_stride, wt, w_stride, k, c, part_idx, part_tmpl,
                             part_n, r, aff, part_ok);
}

int flm_warp_parts_frames(flm_stream_t stream, const uint8_t* frames, size_t frame_stride, int nframes, int fh, int fw,
                          const int32_t* frame_idx, const int32_t* boxes, const double* lm, size_t lm_stride,
                          const double* wt, size_t w_stride, int c, const int32_t* part_idx, const double* part_tmpl,
                          const int32_t* part_n, int r, int k, void* dst, int ph, int pw, int samples,
                          const flm_image_format* fmt, const flm_frame_format* src, float* aff_out, int32_t* part_ok_out) {
  // frame_idx, boxes, w, fmt, src and the last two outputs are optional
  if (!frames || !lm || !part_idx || !part_tmpl || !part_n || !dst) return null_argument("flm_warp_parts_frames");
  flm_frame_format bgr;  // src NULL: the dense BGR ring
  flm_frame_format_init(&bgr);
  if (src) {
    if (const int rc = check_frame_format("flm_warp_parts_frames", src)) return rc;
  }
  flm_image_format plain;  // fmt NULL: float32 NHWC BGR, scale 1, bias 0
  flm_image_format_init(&plain);
  if (fmt) {
    if (const int rc = check_image_format("flm_warp_parts_frames", fmt)) return rc;
  }
  if (const int rc = check_image_dst("flm_warp_parts_frames", dst, fmt ? fmt : &plain)) return rc;
  return launch_warp_parts_frames(static_cast<hipStream_t>(stream), frames, frame_stride, nframes, fh, fw, frame_idx, boxes,
                                  lm, lm_stride, wt, w_stride, c, part_idx, part_tmpl, part_n, r, k, dst, ph, pw, samples,
                                  fmt ? fmt : &plain, src ? src : &bgr, aff_out, part_ok_out);
}

// ---- frame annotation (flm_annotate.hip) ------------------------------------------------------------------------------

void flm_annotate_opts_init(flm_annotate_opts* opts) {
  if (!opts) return;
  memset(opts, 0, sizeof(*opts));
  opts->struct_size = (uint32_t)sizeof(flm_annotate_opts);
  opts->marks = 1;
  opts->box = 0;
  opts->redact = 0;
  opts->margin[0] = 0.1; opts->margin[1] = 0.35; opts->margin[2] = 0.1; opts->margin[3] = 0.1;
  opts->mark_bgr[0] = 0; opts->mark_bgr[1] = 255; opts->mark_bgr[2] = 0;
  opts->box_bgr[0] = 0; opts->box_bgr[1] = 255; opts->box_bgr[2] = 0;
}

int flm_bgr_to_yuv(int matrix, const uint8_t bgr[3], uint8_t yuv[3]) {
  if (!bgr || !yuv) return null_argument("flm_bgr_to_yuv");
  if (matrix != FLM_YUV_BT601_LIMITED && matrix != FLM_YUV_BT709_LIMITED) {
    set_error("flm_bgr_to_yuv: unknown YUV matrix %d", matrix);
    return FLM_ERR_ARG;
  }
  annot_bgr_to_yuv(matrix, bgr, yuv);
  return FLM_OK;
}

int flm_frames_annotate(flm_stream_t stream, uint8_t* frames, size_t frame_stride, int nframes, int fh, int fw,
                        const flm_frame_format* src, const int32_t* frame_idx, const double* lm, size_t lm_stride, int k,
                        int c, const flm_annotate_opts* opts, int32_t* regions) {
  const char* who = "flm_frames_annotate";
  if (!frames || !lm || !regions) return null_argument(who);  // src, frame_idx and opts are optional
  flm_frame_format bgr;
  flm_frame_format_init(&bgr);
  if (!src) src = &bgr;
  const int rc_fmt = check_frame_format(who, src);
  if (rc_fmt == FLM_ERR_ARG) return rc_fmt;  // (a BGR24 format with a pitch is a shape error: after the options)
  flm_annotate_opts defaults;
  if (const int rc = check_opts<false>(who, FLM_OPTS(flm_annotate_opts), &opts, &defaults)) return rc;
  if (opts->marks != 0 && opts->marks != 1) {
    set_error("%s: marks=%d (must be 0 or 1)", who, opts->marks);
    return FLM_ERR_ARG;
  }
  if (opts->box < 0 || opts->box > 16) {
    set_error("%s: box=%d outside 0 <= box <= 16", who, opts->box);
    return FLM_ERR_ARG;
  }
  if (opts->redact != 0 && (opts->redact < 2 || opts->redact > 64 || (opts->redact & 1))) {
    set_error("%s: redact=%d (must be 0, or even and 2 <= redact <= 64)", who, opts->redact);
    return FLM_ERR_ARG;
  }
  for (int i = 0; i < 4; ++i)
    if (!(opts->margin[i] >= 0.0 && opts->margin[i] <= 4.0)) {  // (NaN fails the test)
      set_error("%s: margin[%d]=%g outside 0 <= margin <= 4", who, i, opts->margin[i]);
      return FLM_ERR_ARG;
    }
  if (k < 1 || k > 65535) {
    set_error("%s: k=%d outside 1 <= k <= 65535", who, k);
    return FLM_ERR_SHAPE;
  }
  if (opts->redact && k > 4096) {
    set_error("%s: k=%d with redact, needs k <= 4096 (every workgroup of the mosaic scans the faces before its own)", who,
              k);
    return FLM_ERR_SHAPE;
  }
  if (c < 1 || c > 1024) {
    set_error("%s: c=%d outside 1 <= c <= 1024", who, c);
    return FLM_ERR_SHAPE;
  }
  if (lm_stride < 2) {
    set_error("%s: lm_stride=%zu, needs lm_stride >= 2", who, lm_stride);
    return FLM_ERR_SHAPE;
  }
  if (rc_fmt) return check_frame_format(who, src);  // (sets the message again)
  if (nframes < 1) {
    set_error("%s: nframes=%d, needs nframes >= 1", who, nframes);
    return FLM_ERR_SHAPE;
  }
  AnnotateArgs g;
  memset(&g, 0, sizeof(g));
  if (src->pixel == FLM_FRAME_NV12) {
    const size_t bytes = nv12_format_bytes(who, src, fh, fw);  // fh, fw even and >= 2, the pitches, slot bytes < 2^31
    if (!bytes) return FLM_ERR_SHAPE;
    if (frame_stride < bytes) {
      set_error("%s: frame_stride=%zu, needs frame_stride >= flm_frame_format_bytes = %zu", who, frame_stride, bytes);
      return FLM_ERR_SHAPE;
    }
    g.nv12 = 1;
    g.y_pitch = src->y_pitch ? src->y_pitch : (unsigned)fw;
    g.uv_pitch = src->uv_pitch ? src->uv_pitch : g.y_pitch;
    g.uv_off = src->uv_offset ? (unsigned)src->uv_offset : g.y_pitch * (unsigned)fh;
    annot_bgr_to_yuv(src->matrix, opts->mark_bgr, g.mark_px);
    annot_bgr_to_yuv(src->matrix, opts->box_bgr, g.box_px);
  } else {
    if (fh < 1 || fw < 2) {
      set_error("%s: frame %dx%d, needs fh >= 1 and fw >= 2", who, fh, fw);
      return FLM_ERR_SHAPE;
    }
    if ((long long)fh * fw * 3 >= (1ll << 31)) {
      set_error("%s: frame %dx%d, needs fh*fw*3 < 2^31", who, fh, fw);
      return FLM_ERR_SHAPE;
    }
    if (frame_stride < (size_t)fh * fw * 3) {
      set_error("%s: frame_stride=%zu, needs frame_stride >= fh*fw*3 = %zu", who, frame_stride, (size_t)fh * fw * 3);
      return FLM_ERR_SHAPE;
    }
    for (int i = 0; i < 3; ++i) {
      g.mark_px[i] = opts->mark_bgr[i];
      g.box_px[i] = opts->box_bgr[i];
    }
  }
  g.frames = frames; g.frame_stride = frame_stride; g.nframes = nframes; g.fh = fh; g.fw = fw;
  g.frame_idx = frame_idx; g.lm = lm; g.lm_stride = lm_stride; g.k = k; g.c = c;
  g.marks = opts->marks; g.box = opts->box; g.redact = opts->redact;
  for (int i = 0; i < 4; ++i) g.margin[i] = opts->margin[i];
  g.regions = regions;
  return launch_frames_annotate(static_cast<hipStream_t>(stream), g);
}

}  // extern "C"
