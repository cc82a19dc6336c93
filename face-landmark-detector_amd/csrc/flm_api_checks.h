// The argument checks of the extern "C" entry points, each stated once.  Host only: included by the flm_api*.hip files,
// never by a kernel file.  Every helper is a pure function of its arguments that reports through set_error (the calling
// thread's error string): none allocates, takes a lock or touches any other process state.  A helper returns FLM_OK or
// the error code of the rejection with the message set; `who` names the entry point in the message.
#pragma once

#include <cmath>

#include "flm_common.h"

namespace flm {

static inline int null_argument(const char* who) {
  set_error("%s: null argument", who);
  return FLM_ERR_ARG;
}

// "<who>: <name>=<v>, needs <lo> <= <name> <= <hi>", FLM_ERR_SHAPE.
static inline int check_range(const char* who, const char* name, int v, int lo, int hi) {
  if (v >= lo && v <= hi) return FLM_OK;
  set_error("%s: %s=%d, needs %d <= %s <= %d", who, name, v, lo, name, hi);
  return FLM_ERR_SHAPE;
}

// ---- option structs ----------------------------------------------------------------------------------------------------
static inline int check_struct_size(const char* who, const char* type, uint32_t struct_size, size_t need) {
  if (struct_size >= need) return FLM_OK;
  set_error("%s: %s struct_size %u is smaller than this library's %zu (initialise with %s_init)", who, type, struct_size,
            need, type);
  return FLM_ERR_ARG;
}

// The head of an option struct that is given: struct_size and, with kReserved, the reserved field.
template <bool kReserved, class T>
static inline int check_opts_head(const char* who, const char* type, const T* opts) {
  if (const int rc = check_struct_size(who, type, opts->struct_size, sizeof(T))) return rc;
  if constexpr (kReserved) {
    if (opts->reserved != 0) {
      set_error("%s: %s reserved=%lld, must be 0", who, type, (long long)opts->reserved);
      return FLM_ERR_ARG;
    }
  }
  return FLM_OK;
}

// An optional option struct: a null *opts becomes `defaults`, filled by the struct's _init; then the head.  The value
// checks stay with the call.  FLM_OPTS(T) spells the two middle arguments.
template <bool kReserved, class T>
static inline int check_opts(const char* who, const char* type, void (*init)(T*), const T** opts, T* defaults) {
  if (!*opts) {
    init(defaults);
    *opts = defaults;
  }
  return check_opts_head<kReserved>(who, type, *opts);
}
#define FLM_OPTS(T) #T, T##_init

// ---- overlaps ----------------------------------------------------------------------------------------------------------
static inline bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
  return a0 < b0 + nb && b0 < a0 + na;
}

struct NamedRange {
  const void* p;  // null: the argument was not given, the entry is skipped
  size_t bytes;
  const char* name;
};

// No two of these may overlap.  `fmt` takes who and the two names, the earlier entry first; the first pair in array order
// is the one named.
template <size_t N>
static inline int check_apart(const char* who, const NamedRange (&r)[N], const char* fmt) {
  for (size_t i = 0; i < N; ++i)
    for (size_t j = i + 1; j < N; ++j)
      if (r[i].p && r[j].p && ranges_overlap(r[i].p, r[i].bytes, r[j].p, r[j].bytes)) {
        set_error(fmt, who, r[i].name, r[j].name);
        return FLM_ERR_ARG;
      }
  return FLM_OK;
}

// No output may overlap an input or another output: output by output, its inputs first, then the outputs after it.
// `fmt_in` and `fmt_out` take who, the output's name and the name of what it overlaps.
template <size_t NI, size_t NO>
static inline int check_outputs_apart(const char* who, const NamedRange (&in)[NI], const NamedRange (&out)[NO],
                                      const char* fmt_in, const char* fmt_out) {
  for (size_t a = 0; a < NO; ++a) {
    if (!out[a].p) continue;
    for (size_t b = 0; b < NI; ++b)
      if (in[b].p && ranges_overlap(out[a].p, out[a].bytes, in[b].p, in[b].bytes)) {
        set_error(fmt_in, who, out[a].name, in[b].name);
        return FLM_ERR_ARG;
      }
    for (size_t b = a + 1; b < NO; ++b)
      if (out[b].p && ranges_overlap(out[a].p, out[a].bytes, out[b].p, out[b].bytes)) {
        set_error(fmt_out, who, out[a].name, out[b].name);
        return FLM_ERR_ARG;
      }
  }
  return FLM_OK;
}

// ---- image and frame formats (the warps, flm_face_quality, the annotation) ---------------------------------------------
static inline size_t image_element_bytes(const flm_image_format* fmt) {
  return fmt->type == FLM_PIX_F32 ? 4 : fmt->type == FLM_PIX_U8 ? 1 : 2;
}

// FLM_OK, or FLM_ERR_ARG with the reason in the message.
static inline int check_image_format(const char* who, const flm_image_format* fmt) {
  if (!fmt) {
    set_error("%s: null format", who);
    return FLM_ERR_ARG;
  }
  if (const int rc = check_struct_size(who, "flm_image_format", fmt->struct_size, sizeof(flm_image_format))) return rc;
  if (fmt->layout != FLM_LAYOUT_NHWC && fmt->layout != FLM_LAYOUT_NCHW) {
    set_error("%s: unknown layout %d", who, fmt->layout);
    return FLM_ERR_ARG;
  }
  if (fmt->type != FLM_PIX_F32 && fmt->type != FLM_PIX_F16 && fmt->type != FLM_PIX_BF16 && fmt->type != FLM_PIX_U8) {
    set_error("%s: unknown pixel type %d", who, fmt->type);
    return FLM_ERR_ARG;
  }
  if (fmt->reverse_channels != 0 && fmt->reverse_channels != 1) {
    set_error("%s: reverse_channels=%d (must be 0 or 1)", who, fmt->reverse_channels);
    return FLM_ERR_ARG;
  }
  for (int c = 0; c < 3; ++c) {
    if (!std::isfinite(fmt->scale[c]) || !std::isfinite(fmt->bias[c])) {
      set_error("%s: scale and bias must be finite (channel %d: %g, %g)", who, c, (double)fmt->scale[c],
                (double)fmt->bias[c]);
      return FLM_ERR_ARG;
    }
  }
  return FLM_OK;
}

// an image needs the alignment of its element type, no more (a slice of a larger buffer is fine); `name`: the argument
static inline int check_image_aligned(const char* who, const char* name, const void* img, const flm_image_format* fmt) {
  const uintptr_t esize = image_element_bytes(fmt);
  if (reinterpret_cast<uintptr_t>(img) % esize) {
    set_error("%s: %s is not aligned to its %d-byte element", who, name, (int)esize);
    return FLM_ERR_ARG;
  }
  return FLM_OK;
}
static inline int check_image_dst(const char* who, const void* dst, const flm_image_format* fmt) {
  return check_image_aligned(who, "dst", dst, fmt);
}

// FLM_OK, FLM_ERR_ARG (null, struct_size, unknown pixel or matrix) or FLM_ERR_SHAPE (a BGR24 format that is not the
// dense ring); the sizes of an NV12 format are checked against the frame by the launchers.
static inline int check_frame_format(const char* who, const flm_frame_format* src) {
  if (!src) {
    set_error("%s: null frame format", who);
    return FLM_ERR_ARG;
  }
  if (const int rc = check_struct_size(who, "flm_frame_format", src->struct_size, sizeof(flm_frame_format))) return rc;
  if (src->pixel != FLM_FRAME_BGR24 && src->pixel != FLM_FRAME_NV12) {
    set_error("%s: unknown frame pixel format %d", who, src->pixel);
    return FLM_ERR_ARG;
  }
  if (src->matrix != FLM_YUV_BT601_LIMITED && src->matrix != FLM_YUV_BT709_LIMITED) {
    set_error("%s: unknown YUV matrix %d", who, src->matrix);
    return FLM_ERR_ARG;
  }
  if (src->pixel == FLM_FRAME_BGR24 && (src->y_pitch || src->uv_pitch || src->uv_offset)) {
    set_error("%s: a BGR24 ring is dense: y_pitch, uv_pitch and uv_offset must be 0 (got %u, %u, %llu)", who,
              src->y_pitch, src->uv_pitch, (unsigned long long)src->uv_offset);
    return FLM_ERR_SHAPE;
  }
  return FLM_OK;
}

}  // namespace flm
