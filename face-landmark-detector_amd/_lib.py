"""ctypes binding of libflm_hip.so (C ABI: include/flm.h).

There is no CPU fallback: if the library is missing or a call fails, the op raises.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libflm_hip.so")

# enums of include/flm.h
FLM_F32, FLM_BF16 = 0, 1
IN_U8_BGR, IN_F32_RGB = 0, 1
OUT_PROBS, OUT_CLASSMAP, OUT_LANDMARKS, OUT_LOGITS, OUT_LANDMARKS_STATS = 0, 1, 2, 3, 4
LANDMARK_REC = 6  # FLM_LANDMARK_REC: x, y, score, var_x, var_y, cov_xy
QUALITY_REC = 8   # FLM_QUALITY_REC: n_pix, sum Y, sum Y*Y, n_lap, sum L, sum L*L, dark, bright
POSE_REC = 18     # FLM_POSE_REC: R row by row, s, mx, my, rms, cnt, ok, yaw, pitch, roll
PARTS_MAX, PART_MAX_POINTS, PART_MAX_SIDE = 8, 32, 256   # FLM_PARTS_MAX, FLM_PART_MAX_POINTS, FLM_PART_MAX_SIDE
OPEN_REC, OPEN_STATE = 4, 8                              # FLM_OPEN_REC: o, dw, ok, sum; FLM_OPEN_STATE
OPEN_MAX_MEASURES, OPEN_MAX_PAIRS = 8, 4                 # FLM_OPEN_MAX_MEASURES, FLM_OPEN_MAX_PAIRS
DECODE_ALL, DECODE_TOPN = 0, 1
NORM_SUB_MEAN, NORM_SUB_AND_DIVIDE, NORM_DIVIDE = 0, 1, 2
ABI_VERSION = 2
SWEEP_MAX_MODES = 16  # FLM_SWEEP_MAX_MODES
LAYOUT_NHWC, LAYOUT_NCHW = 0, 1                      # flm_pixel_layout
PIX_F32, PIX_F16, PIX_BF16, PIX_U8 = 0, 1, 2, 3      # flm_pixel_type
FRAME_BGR24, FRAME_NV12 = 0, 1                       # flm_frame_pixel
YUV_BT601_LIMITED, YUV_BT709_LIMITED = 0, 1          # flm_yuv_matrix
TRACK_DEAD, TRACK_FEW_POINTS, TRACK_LOW_SCORE, TRACK_SCALE, TRACK_OUTSIDE = 1, 2, 4, 8, 16   # flm_track_status
TRACK_DUPLICATE, TRACK_UNCONFIRMED = 32, 64          # flm_track_status, set by flm_track_associate alone
FLOW_NO_HISTORY, FLOW_LOW_TEXTURE, FLOW_RESIDUAL, FLOW_OUTSIDE, FLOW_MOVED, FLOW_NOT_FINITE = 1, 2, 4, 8, 16, 32  # FLM_FLOW_*
FLOW_FB = 64               # FLM_FLOW_FB: the forward-backward check of flm_landmark_flow_rows

EXPORTS = [
    "flm_abi_version", "flm_last_error",
    "flm_fcn8_packed_bytes", "flm_fcn8_pack",
    "flm_fcn32_packed_bytes", "flm_fcn32_pack", "flm_fcn32_workspace_bytes", "flm_fcn32_forward",
    "flm_fcn_packed_bytes", "flm_fcn_pack", "flm_fcn_workspace_bytes", "flm_fcn_forward",
    "flm_forward_opts_init", "flm_fcn_workspace_bytes_opts", "flm_fcn_forward_opts", "flm_fcn8_workspace_offset_opts",
    "flm_fcn_workspace_offset_opts", "flm_fcn_encoder_layers", "flm_fcn_encoder_layer",
    "flm_fallback_opts_init", "flm_fcn_workspace_bytes_fb", "flm_fcn_workspace_offset_fb", "flm_fcn_forward_fb",
    "flm_fcn8_workspace_bytes", "flm_fcn8_forward", "flm_fcn8_workspace_offset", "flm_fcn8_run_layer",
    "flm_set_tuning", "flm_get_tuning", "flm_debug_query", "flm_profile_enable", "flm_profile_filter", "flm_profile_reset", "flm_profile_read", "flm_profile_disable",
    "flm_preprocess",
    "flm_decode_workspace_bytes", "flm_decode", "flm_decode_sweep_workspace_bytes", "flm_decode_sweep",
    "flm_decode_stats_workspace_bytes", "flm_decode_stats", "flm_similarity_from_landmarks_weighted",
    "flm_gaussian_heatmaps",
    "flm_similarity_from_landmarks", "flm_similarity_from_landmarks_scaled", "flm_warp_affine", "flm_crop_resize", "flm_crop_resize_frames",
    "flm_landmarks_to_frame", "flm_warp_affine_frames",
    "flm_image_format_init", "flm_image_format_bytes", "flm_warp_affine_fmt", "flm_warp_affine_frames_fmt",
    "flm_frame_format_init", "flm_frame_format_bytes", "flm_frames_to_bgr", "flm_crop_resize_frames_src",
    "flm_warp_affine_frames_src",
    "flm_mesh_map", "flm_mesh_affines", "flm_warp_mesh_frames",
    "flm_track_opts_init", "flm_track_seed", "flm_landmarks_from_crop", "flm_track_step",
    "flm_track_filter_init", "flm_track_step_filtered",
    "flm_track_assoc_opts_init", "flm_track_associate", "flm_track_associate_streams",
    "flm_quality_opts_init", "flm_face_quality", "flm_best_opts_init", "flm_track_best_update",
    "flm_track_gather_streams", "flm_track_step_rows", "flm_track_best_update_rows", "flm_track_gather_live",
    "flm_pose_opts_init", "flm_head_pose",
    "flm_part_affines", "flm_warp_parts_frames", "flm_open_opts_init", "flm_face_openness",
    "flm_exit_opts_init", "flm_track_retire",
    "flm_views_opts_init", "flm_track_views_update", "flm_track_exit_views",
    "flm_annotate_opts_init", "flm_bgr_to_yuv", "flm_frames_annotate",
    "flm_flow_pyramid_bytes", "flm_flow_pyramid", "flm_flow_opts_init", "flm_landmark_flow",
    "flm_track_gather_flow", "flm_landmark_flow_rows", "flm_track_flow_history_put",
]


class FlmError(RuntimeError):
    """A call into libflm_hip.so returned a negative status."""


class ConvParams(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("kernel", "bias", "gamma", "beta", "mean", "var")]


class Fcn8Params(C.Structure):
    _fields_ = [("enc", ConvParams * 5), ("fc6", ConvParams), ("fc7", ConvParams),
                ("score5", ConvParams), ("score4", ConvParams), ("score3", ConvParams),
                ("up5", C.c_void_p), ("up4", C.c_void_p), ("up3", C.c_void_p)]


class ForwardOpts(C.Structure):
    """flm_forward_opts: per-call options that change the workspace layout (include/flm.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("landmark_candidates", C.c_int32), ("candidate_sub_phases", C.c_int32),
                ("candidate_cap_div", C.c_int32)]

    @classmethod
    def make(cls, landmark_candidates=1, candidate_sub_phases=0, candidate_cap_div=1):
        o = cls()
        load().flm_forward_opts_init(C.byref(o))
        o.landmark_candidates = int(landmark_candidates)
        o.candidate_sub_phases = int(candidate_sub_phases)
        o.candidate_cap_div = int(candidate_cap_div)
        return o

    def key(self):
        return (self.landmark_candidates, self.candidate_sub_phases, self.candidate_cap_div)


class FallbackOpts(C.Structure):
    """flm_fallback_opts: the row budget of the candidate path's per-face fallback (include/flm.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("faces", C.c_int32)]

    @classmethod
    def make(cls, faces=0):
        o = cls()
        load().flm_fallback_opts_init(C.byref(o))
        o.faces = int(faces)
        return o


class EncLayerInfo(C.Structure):
    """flm_enc_layer_info: one encoder layer of an architecture and its grids for an h x w input (include/flm.h)."""
    _fields_ = [(n, C.c_int32) for n in ("kind", "cin", "cout", "kernel", "stride", "activation", "pool", "src", "res",
                                         "in_h", "in_w", "out_h", "out_w")]


ENC_FIRST3, ENC_CONV3, ENC_MB_CONV1, ENC_MB_DW, ENC_MB_PW, ENC_RN_CONV1, ENC_MAXPOOL3, ENC_CONV = range(8)  # flm_enc_kind


class ImageFormat(C.Structure):
    """flm_image_format: layout, type, channel order, scale and bias of the aligned faces (include/flm.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("layout", C.c_int32), ("type", C.c_int32), ("reverse_channels", C.c_int32),
                ("scale", C.c_float * 3), ("bias", C.c_float * 3)]


class FrameFormat(C.Structure):
    """flm_frame_format: how a ring slot holds its pixels -- dense BGR, or the NV12 surface of a decoder (include/flm.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("pixel", C.c_int32), ("matrix", C.c_int32), ("y_pitch", C.c_uint32),
                ("uv_pitch", C.c_uint32), ("uv_offset", C.c_uint64)]


class TrackOpts(C.Structure):
    """flm_track_opts: when flm_track_step gives a track up (include/flm.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("min_points", C.c_int32), ("min_score", C.c_double),
                ("min_side", C.c_double), ("max_side", C.c_double)]

    @classmethod
    def make(cls, min_points=2, min_score=0.0, min_side=0.0, max_side=float("inf")):
        o = cls()
        load().flm_track_opts_init(C.byref(o))
        o.min_points = int(min_points)
        o.min_score = float(min_score)
        o.min_side = float(min_side)
        o.max_side = float(max_side)
        return o


class TrackFilter(C.Structure):
    """flm_track_filter: the One-Euro filter of flm_track_step_filtered (include/flm.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32), ("min_cutoff", C.c_double), ("beta", C.c_double),
                ("d_cutoff", C.c_double)]

    @classmethod
    def make(cls, min_cutoff=1.0, beta=15.0, d_cutoff=1.0):
        o = cls()
        load().flm_track_filter_init(C.byref(o))
        o.min_cutoff = float(min_cutoff)
        o.beta = float(beta)
        o.d_cutoff = float(d_cutoff)
        return o


class TrackAssocOpts(C.Structure):
    """flm_track_assoc_opts: how flm_track_associate pairs detections with tracks (include/flm.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("max_misses", C.c_int32), ("square", C.c_int32), ("reserved", C.c_int32),
                ("match_iou", C.c_double), ("dup_iou", C.c_double), ("refresh_iou", C.c_double)]

    @classmethod
    def make(cls, match_iou=0.3, dup_iou=0.7, refresh_iou=0.0, max_misses=0, square=True):
        o = cls()
        load().flm_track_assoc_opts_init(C.byref(o))
        o.match_iou = float(match_iou)
        o.dup_iou = float(dup_iou)
        o.refresh_iou = float(refresh_iou)
        o.max_misses = int(max_misses)
        o.square = 1 if square else 0
        return o


class QualityOpts(C.Structure):
    """flm_quality_opts: the exposure levels of flm_face_quality (include/flm.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("dark", C.c_int32), ("bright", C.c_int32)]

    @classmethod
    def make(cls, dark=16, bright=239):
        o = cls()
        load().flm_quality_opts_init(C.byref(o))
        o.dark = int(dark)
        o.bright = int(bright)
        return o


class BestOpts(C.Structure):
    """flm_best_opts: how flm_track_best_update scores a face (include/flm.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_int32), ("sharp_ref", C.c_double),
                ("min_exposed", C.c_double)]

    @classmethod
    def make(cls, sharp_ref=100.0, min_exposed=0.5):
        o = cls()
        load().flm_best_opts_init(C.byref(o))
        o.sharp_ref = float(sharp_ref)
        o.min_exposed = float(min_exposed)
        return o


class PoseOpts(C.Structure):
    """flm_pose_opts: when flm_head_pose accepts a fit and when a face counts as frontal (include/flm.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32), ("min_volume", C.c_double),
                ("min_frontal", C.c_double)]

    @classmethod
    def make(cls, min_volume=1e-6, min_frontal=0.0):
        o = cls()
        load().flm_pose_opts_init(C.byref(o))
        o.min_volume = float(min_volume)
        o.min_frontal = float(min_frontal)
        return o


class OpenOpts(C.Structure):
    """flm_open_opts: the measures and thresholds of flm_face_openness (include/flm.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32), ("n_measures", C.c_int32),
                ("n_pairs", C.c_int32 * OPEN_MAX_MEASURES), ("width", (C.c_int32 * 2) * OPEN_MAX_MEASURES),
                ("upper", (C.c_int32 * OPEN_MAX_PAIRS) * OPEN_MAX_MEASURES),
                ("lower", (C.c_int32 * OPEN_MAX_PAIRS) * OPEN_MAX_MEASURES),
                ("close_below", C.c_double), ("open_above", C.c_double), ("min_closed", C.c_double),
                ("max_closed", C.c_double), ("min_width", C.c_double)]

    @classmethod
    def make(cls, measures=None, **numbers):
        """measures: None (the library's defaults) or a sequence of ((a, b), ((u, l), ...)); numbers: the five doubles."""
        o = cls()
        load().flm_open_opts_init(C.byref(o))
        if measures is not None:
            o.n_measures = len(measures)
            for g in range(OPEN_MAX_MEASURES):
                (a, b), pairs = measures[g] if g < len(measures) else ((0, 0), ())
                o.n_pairs[g] = len(pairs)
                o.width[g][0], o.width[g][1] = int(a), int(b)
                for v in range(OPEN_MAX_PAIRS):
                    o.upper[g][v], o.lower[g][v] = [int(x) for x in pairs[v]] if v < len(pairs) else (0, 0)
        for name, v in numbers.items():
            setattr(o, name, float(v))
        return o


class ExitOpts(C.Structure):
    """flm_exit_opts: which finished tracks flm_track_retire queues (include/flm.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32), ("min_q", C.c_double)]

    @classmethod
    def make(cls, min_q=0.0):
        o = cls()
        load().flm_exit_opts_init(C.byref(o))
        o.min_q = float(min_q)
        return o


VIEWS_MAX_EDGES = 7   # FLM_VIEWS_MAX_EDGES


class ViewsOpts(C.Structure):
    """flm_views_opts: how flm_track_views_update scores a face and which pose bin it falls into (include/flm.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32), ("sharp_ref", C.c_double),
                ("min_exposed", C.c_double), ("n_u", C.c_int32), ("n_v", C.c_int32),
                ("u_edge", C.c_double * VIEWS_MAX_EDGES), ("v_edge", C.c_double * VIEWS_MAX_EDGES)]

    @classmethod
    def make(cls, u_edges=None, v_edges=(), sharp_ref=100.0, min_exposed=0.5):
        """u_edges None: the library's default edges."""
        o = cls()
        load().flm_views_opts_init(C.byref(o))
        o.sharp_ref = float(sharp_ref)
        o.min_exposed = float(min_exposed)
        for count, arr, edges in (("n_u", o.u_edge, u_edges), ("n_v", o.v_edge, v_edges)):
            if edges is None:
                continue
            setattr(o, count, len(edges))
            for i in range(VIEWS_MAX_EDGES):
                arr[i] = float(edges[i]) if i < min(len(edges), VIEWS_MAX_EDGES) else 0.0
        return o


class AnnotateOpts(C.Structure):
    """flm_annotate_opts: which layers flm_frames_annotate writes into the ring, and how (include/flm.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("marks", C.c_int32), ("box", C.c_int32), ("redact", C.c_int32),
                ("margin", C.c_double * 4), ("mark_bgr", C.c_uint8 * 3), ("box_bgr", C.c_uint8 * 3),
                ("reserved", C.c_uint8 * 2)]

    @classmethod
    def make(cls, marks=1, box=0, redact=0, margin=None, mark_bgr=None, box_bgr=None):
        """margin, mark_bgr, box_bgr None: the library's defaults."""
        o = cls()
        load().flm_annotate_opts_init(C.byref(o))
        o.marks, o.box, o.redact = int(marks), int(box), int(redact)
        for arr, values, conv in ((o.margin, margin, float), (o.mark_bgr, mark_bgr, int), (o.box_bgr, box_bgr, int)):
            if values is not None:
                for i, v in enumerate(values):
                    arr[i] = conv(v)
        return o


class FlowOpts(C.Structure):
    """flm_flow_opts: the pyramid, the window and the gates of flm_landmark_flow (include/flm.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32), ("levels", C.c_int32), ("radius", C.c_int32),
                ("max_iter", C.c_int32), ("pad", C.c_int32), ("eps", C.c_double), ("min_eig", C.c_double),
                ("max_err", C.c_double), ("max_move", C.c_double)]

    @classmethod
    def make(cls, levels=4, radius=7, max_iter=10, eps=0.03, min_eig=0.5, max_err=12.0, max_move=64.0):
        o = cls()
        load().flm_flow_opts_init(C.byref(o))
        o.levels, o.radius, o.max_iter = int(levels), int(radius), int(max_iter)
        o.eps, o.min_eig, o.max_err, o.max_move = float(eps), float(min_eig), float(max_err), float(max_move)
        return o


class FcnParams(C.Structure):
    _fields_ = [("enc", C.POINTER(ConvParams)), ("n_enc", C.c_int), ("fc6", ConvParams), ("fc7", ConvParams),
                ("score5", ConvParams), ("score4", ConvParams), ("score3", ConvParams),
                ("up5", C.c_void_p), ("up4", C.c_void_p), ("up3", C.c_void_p)]


ARCH_FCN8, ARCH_FCN32, ARCH_FCN8_VGG, ARCH_FCN32_VGG, ARCH_FCN8_MOBILENET, ARCH_FCN32_MOBILENET = 0, 1, 2, 3, 4, 5
ARCH_FCN8_RESNET50, ARCH_FCN32_RESNET50 = 6, 7

_lib = None


def _declare(lib):
    vp, i, f, sz = C.c_void_p, C.c_int, C.c_float, C.c_size_t
    lib.flm_abi_version.restype = i
    lib.flm_abi_version.argtypes = []
    lib.flm_last_error.restype = C.c_char_p
    lib.flm_last_error.argtypes = []
    lib.flm_fcn8_packed_bytes.restype = sz
    lib.flm_fcn8_packed_bytes.argtypes = [i, i]
    lib.flm_fcn8_pack.restype = i
    lib.flm_fcn8_pack.argtypes = [vp, C.POINTER(Fcn8Params), i, i, vp, sz]
    lib.flm_fcn8_workspace_bytes.restype = sz
    lib.flm_fcn8_workspace_bytes.argtypes = [i] * 8
    lib.flm_fcn8_forward.restype = i
    lib.flm_fcn8_forward.argtypes = [vp, vp, vp, i, i, i, i, i, i, i, i, i, f, vp, vp, sz]
    lib.flm_fcn32_packed_bytes.restype = sz
    lib.flm_fcn32_packed_bytes.argtypes = [i, i]
    lib.flm_fcn32_pack.restype = i
    lib.flm_fcn32_pack.argtypes = [vp, C.POINTER(Fcn8Params), i, i, vp, sz]
    lib.flm_fcn32_workspace_bytes.restype = sz
    lib.flm_fcn32_workspace_bytes.argtypes = [i] * 8
    lib.flm_fcn32_forward.restype = i
    lib.flm_fcn32_forward.argtypes = [vp, vp, vp, i, i, i, i, i, i, i, i, i, f, vp, vp, sz]
    lib.flm_fcn_packed_bytes.restype = sz
    lib.flm_fcn_packed_bytes.argtypes = [i, i, i]
    lib.flm_fcn_pack.restype = i
    lib.flm_fcn_pack.argtypes = [vp, i, C.POINTER(FcnParams), i, i, vp, sz]
    lib.flm_fcn_workspace_bytes.restype = sz
    lib.flm_fcn_workspace_bytes.argtypes = [i] * 9
    lib.flm_fcn_forward.restype = i
    lib.flm_fcn_forward.argtypes = [vp, i, vp, vp, i, i, i, i, i, i, i, i, i, f, vp, vp, sz]
    lib.flm_forward_opts_init.restype = None
    lib.flm_forward_opts_init.argtypes = [C.POINTER(ForwardOpts)]
    lib.flm_fcn_workspace_bytes_opts.restype = sz
    lib.flm_fcn_workspace_bytes_opts.argtypes = [i] * 9 + [C.POINTER(ForwardOpts)]
    lib.flm_fcn_forward_opts.restype = i
    lib.flm_fcn_forward_opts.argtypes = [vp, i, vp, vp, i, i, i, i, i, i, i, i, i, f, vp, vp, sz, C.POINTER(ForwardOpts)]
    lib.flm_fcn8_workspace_offset_opts.restype = C.c_int64
    lib.flm_fcn8_workspace_offset_opts.argtypes = [C.c_char_p] + [i] * 8 + [C.POINTER(ForwardOpts)]
    lib.flm_fcn8_workspace_offset.restype = C.c_int64
    lib.flm_fcn8_workspace_offset.argtypes = [C.c_char_p] + [i] * 8
    lib.flm_fcn_workspace_offset_opts.restype = C.c_int64
    lib.flm_fcn_workspace_offset_opts.argtypes = [i, C.c_char_p] + [i] * 8 + [C.POINTER(ForwardOpts)]
    lib.flm_fallback_opts_init.restype = None
    lib.flm_fallback_opts_init.argtypes = [C.POINTER(FallbackOpts)]
    lib.flm_fcn_workspace_bytes_fb.restype = sz
    lib.flm_fcn_workspace_bytes_fb.argtypes = [i] * 9 + [C.POINTER(ForwardOpts), C.POINTER(FallbackOpts)]
    lib.flm_fcn_workspace_offset_fb.restype = C.c_int64
    lib.flm_fcn_workspace_offset_fb.argtypes = [i, C.c_char_p] + [i] * 8 + [C.POINTER(ForwardOpts), C.POINTER(FallbackOpts)]
    lib.flm_fcn_forward_fb.restype = i
    lib.flm_fcn_forward_fb.argtypes = [vp, i, vp, vp, i, i, i, i, i, i, i, i, i, f, vp, vp, sz, C.POINTER(ForwardOpts),
                                       C.POINTER(FallbackOpts)]
    lib.flm_fcn_encoder_layers.restype = i
    lib.flm_fcn_encoder_layers.argtypes = [i]
    lib.flm_fcn_encoder_layer.restype = i
    lib.flm_fcn_encoder_layer.argtypes = [i, i, i, i, C.POINTER(EncLayerInfo)]
    lib.flm_fcn8_run_layer.restype = i
    lib.flm_fcn8_run_layer.argtypes = [vp, vp, C.c_char_p, vp, vp, i, i, i, i, i]
    lib.flm_profile_filter.restype = i
    lib.flm_profile_filter.argtypes = [C.c_char_p]
    lib.flm_set_tuning.restype = i
    lib.flm_set_tuning.argtypes = [C.c_char_p, i]
    lib.flm_get_tuning.restype = i
    lib.flm_get_tuning.argtypes = [C.c_char_p, C.POINTER(i)]
    lib.flm_debug_query.restype = i
    lib.flm_debug_query.argtypes = [C.c_char_p, i]
    lib.flm_profile_enable.restype = i
    lib.flm_profile_enable.argtypes = [i]
    lib.flm_profile_reset.restype = i
    lib.flm_profile_reset.argtypes = []
    lib.flm_profile_read.restype = i
    lib.flm_profile_read.argtypes = [i, C.c_char_p, i, C.POINTER(C.c_float)]
    lib.flm_profile_disable.restype = i
    lib.flm_profile_disable.argtypes = []
    lib.flm_preprocess.restype = i
    lib.flm_preprocess.argtypes = [vp, vp, i, i, i, i, vp]
    lib.flm_decode_workspace_bytes.restype = sz
    lib.flm_decode_workspace_bytes.argtypes = [i] * 6
    lib.flm_decode.restype = i
    lib.flm_decode.argtypes = [vp, vp, i, i, i, i, i, i, f, vp, vp, sz]
    lib.flm_decode_stats_workspace_bytes.restype = sz
    lib.flm_decode_stats_workspace_bytes.argtypes = [i] * 6
    lib.flm_decode_stats.restype = i
    lib.flm_decode_stats.argtypes = [vp, vp, i, i, i, i, i, i, f, vp, vp, sz]
    lib.flm_similarity_from_landmarks_weighted.restype = i
    lib.flm_similarity_from_landmarks_weighted.argtypes = [vp, vp, sz, vp, sz, vp, i, i, C.c_double, C.c_double, vp]
    ip = C.POINTER(C.c_int)
    lib.flm_decode_sweep_workspace_bytes.restype = sz
    lib.flm_decode_sweep_workspace_bytes.argtypes = [i, i, i, i, ip, i]
    lib.flm_decode_sweep.restype = i
    lib.flm_decode_sweep.argtypes = [vp, vp, i, i, i, i, ip, i, f, vp, vp, sz]
    lib.flm_gaussian_heatmaps.restype = i
    lib.flm_gaussian_heatmaps.argtypes = [vp, vp, i, i, i, i, C.c_double, vp]
    lib.flm_similarity_from_landmarks.restype = i
    lib.flm_similarity_from_landmarks.argtypes = [vp, vp, vp, i, i, vp]
    lib.flm_similarity_from_landmarks_scaled.restype = i
    lib.flm_similarity_from_landmarks_scaled.argtypes = [vp, vp, vp, i, i, C.c_double, C.c_double, vp]
    lib.flm_warp_affine.restype = i
    lib.flm_warp_affine.argtypes = [vp, vp, i, i, i, i, vp, vp, i, i]
    lib.flm_crop_resize.restype = i
    lib.flm_crop_resize.argtypes = [vp, vp, i, i, vp, i, vp, i, i]
    lib.flm_crop_resize_frames.restype = i
    lib.flm_crop_resize_frames.argtypes = [vp, vp, C.c_size_t, i, i, i, vp, vp, i, vp, i, i]
    lib.flm_landmarks_to_frame.restype = i
    lib.flm_landmarks_to_frame.argtypes = [vp, vp, vp, i, i, i, i, i, i, vp]
    lib.flm_warp_affine_frames.restype = i
    lib.flm_warp_affine_frames.argtypes = [vp, vp, C.c_size_t, i, i, i, vp, vp, vp, i, vp, i, i, i]
    lib.flm_image_format_init.restype = None
    lib.flm_image_format_init.argtypes = [C.POINTER(ImageFormat)]
    lib.flm_image_format_bytes.restype = sz
    lib.flm_image_format_bytes.argtypes = [C.POINTER(ImageFormat), i, i, i]
    lib.flm_warp_affine_fmt.restype = i
    lib.flm_warp_affine_fmt.argtypes = [vp, vp, i, i, i, i, vp, vp, i, i, C.POINTER(ImageFormat)]
    lib.flm_warp_affine_frames_fmt.restype = i
    lib.flm_warp_affine_frames_fmt.argtypes = [vp, vp, C.c_size_t, i, i, i, vp, vp, vp, i, vp, i, i, i,
                                               C.POINTER(ImageFormat)]
    lib.flm_frame_format_init.restype = None
    lib.flm_frame_format_init.argtypes = [C.POINTER(FrameFormat)]
    lib.flm_frame_format_bytes.restype = sz
    lib.flm_frame_format_bytes.argtypes = [C.POINTER(FrameFormat), i, i]
    lib.flm_frames_to_bgr.restype = i
    lib.flm_frames_to_bgr.argtypes = [vp, vp, C.c_size_t, i, i, i, C.POINTER(FrameFormat), vp]
    lib.flm_crop_resize_frames_src.restype = i
    lib.flm_crop_resize_frames_src.argtypes = [vp, vp, C.c_size_t, i, i, i, vp, vp, i, vp, i, i, C.POINTER(FrameFormat)]
    lib.flm_warp_affine_frames_src.restype = i
    lib.flm_warp_affine_frames_src.argtypes = [vp, vp, C.c_size_t, i, i, i, vp, vp, vp, i, vp, i, i, i,
                                               C.POINTER(ImageFormat), C.POINTER(FrameFormat)]
    d = C.c_double
    lib.flm_mesh_map.restype = i
    lib.flm_mesh_map.argtypes = [vp, vp, vp, i, i, i, i, vp]
    lib.flm_mesh_affines.restype = i
    lib.flm_mesh_affines.argtypes = [vp, vp, i, vp, vp, vp, i, i, i, i, d, vp]
    lib.flm_warp_mesh_frames.restype = i
    lib.flm_warp_mesh_frames.argtypes = [vp, vp, C.c_size_t, i, i, i, vp, vp, vp, i, vp, vp, vp, i, i, i, vp, i, vp, i, i, i,
                                         C.POINTER(ImageFormat), C.POINTER(FrameFormat), d, vp]
    lib.flm_track_opts_init.restype = None
    lib.flm_track_opts_init.argtypes = [C.POINTER(TrackOpts)]
    lib.flm_track_seed.restype = i
    lib.flm_track_seed.argtypes = [vp, vp, i, i, i, i, i, vp, vp]
    lib.flm_landmarks_from_crop.restype = i
    lib.flm_landmarks_from_crop.argtypes = [vp, vp, sz, vp, i, i, d, d, vp]
    lib.flm_track_step.restype = i
    lib.flm_track_step.argtypes = [vp, vp, sz, vp, sz, vp, vp, i, i, d, d, i, i, i, i, vp, vp, C.POINTER(TrackOpts),
                                   vp, vp, vp, vp, vp]
    lib.flm_track_filter_init.restype = None
    lib.flm_track_filter_init.argtypes = [C.POINTER(TrackFilter)]
    lib.flm_track_step_filtered.restype = i
    lib.flm_track_step_filtered.argtypes = lib.flm_track_step.argtypes + [C.POINTER(TrackFilter), d, vp, vp]
    lib.flm_track_assoc_opts_init.restype = None
    lib.flm_track_assoc_opts_init.argtypes = [C.POINTER(TrackAssocOpts)]
    lib.flm_track_associate.restype = i
    lib.flm_track_associate.argtypes = [vp, vp, vp, i, i, i, i, i, i, i, C.POINTER(TrackAssocOpts), vp, vp, vp, vp, vp, vp,
                                        vp, vp]
    lib.flm_track_associate_streams.restype = i
    lib.flm_track_associate_streams.argtypes = [vp, vp, vp, i, i, i, i, i, i, i, i, C.POINTER(TrackAssocOpts), vp, vp, vp,
                                                vp, vp, vp, vp, vp]
    lib.flm_quality_opts_init.restype = None
    lib.flm_quality_opts_init.argtypes = [C.POINTER(QualityOpts)]
    lib.flm_face_quality.restype = i
    lib.flm_face_quality.argtypes = [vp, vp, i, i, i, C.POINTER(ImageFormat), C.POINTER(QualityOpts), vp]
    lib.flm_best_opts_init.restype = None
    lib.flm_best_opts_init.argtypes = [C.POINTER(BestOpts)]
    lib.flm_track_best_update.restype = i
    lib.flm_track_best_update.argtypes = [vp, vp, sz, i, vp, vp, vp, vp, sz, vp, sz, i, vp, vp, C.c_int64,
                                          C.POINTER(BestOpts), vp, vp, vp, vp, vp, vp, vp]
    lib.flm_track_gather_streams.restype = i
    lib.flm_track_gather_streams.argtypes = [vp, vp, i, i, i] + [vp] * 13
    lib.flm_track_step_rows.restype = i
    lib.flm_track_step_rows.argtypes = lib.flm_track_step_filtered.argtypes + [vp, i, vp, vp]
    lib.flm_track_best_update_rows.restype = i
    lib.flm_track_best_update_rows.argtypes = [vp, vp, sz, i, vp, vp, vp, vp, sz, vp, sz, i, vp, vp, C.c_int64,
                                               C.POINTER(BestOpts), vp, i, vp, vp, vp, vp, vp, vp, vp]
    lib.flm_track_gather_live.restype = i
    lib.flm_track_gather_live.argtypes = [vp, vp, i, i, i, i, i, vp, vp, d] + [vp] * 14
    lib.flm_pose_opts_init.restype = None
    lib.flm_pose_opts_init.argtypes = [C.POINTER(PoseOpts)]
    lib.flm_head_pose.restype = i
    lib.flm_head_pose.argtypes = [vp, vp, sz, vp, sz, i, i, vp, vp, i, C.POINTER(PoseOpts), vp, i, vp, vp]
    lib.flm_part_affines.restype = i
    lib.flm_part_affines.argtypes = [vp, vp, sz, vp, sz, i, i, vp, vp, C.POINTER(C.c_int32), i, vp, vp]
    lib.flm_warp_parts_frames.restype = i
    lib.flm_warp_parts_frames.argtypes = [vp, vp, sz, i, i, i, vp, vp, vp, sz, vp, sz, i, vp, vp, C.POINTER(C.c_int32), i, i,
                                          vp, i, i, i, C.POINTER(ImageFormat), C.POINTER(FrameFormat), vp, vp]
    lib.flm_open_opts_init.restype = None
    lib.flm_open_opts_init.argtypes = [C.POINTER(OpenOpts)]
    lib.flm_face_openness.restype = i
    lib.flm_face_openness.argtypes = [vp, vp, sz, vp, sz, i, i, C.POINTER(OpenOpts), vp, i, vp, vp, vp, vp, d, vp, C.c_int64]
    lib.flm_exit_opts_init.restype = None
    lib.flm_exit_opts_init.argtypes = [C.POINTER(ExitOpts)]
    lib.flm_track_retire.restype = i
    lib.flm_track_retire.argtypes = [vp, vp, vp, i, i, i, vp, vp, sz, vp, vp, vp, i, vp, C.c_int64, i, C.POINTER(ExitOpts),
                                     vp, vp, vp, vp, i, vp, vp, vp, vp, vp, vp, vp]
    lib.flm_views_opts_init.restype = None
    lib.flm_views_opts_init.argtypes = [C.POINTER(ViewsOpts)]
    lib.flm_track_views_update.restype = i
    lib.flm_track_views_update.argtypes = [vp, vp, sz, i, vp, vp, vp, vp, sz, vp, sz, i, vp, C.c_int64, C.POINTER(ViewsOpts),
                                           vp, i, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.flm_track_exit_views.restype = i
    lib.flm_track_exit_views.argtypes = [vp, vp, i, i, i, sz, i, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.flm_annotate_opts_init.restype = None
    lib.flm_annotate_opts_init.argtypes = [C.POINTER(AnnotateOpts)]
    lib.flm_bgr_to_yuv.restype = i
    lib.flm_bgr_to_yuv.argtypes = [i, vp, vp]
    lib.flm_frames_annotate.restype = i
    lib.flm_frames_annotate.argtypes = [vp, vp, sz, i, i, i, C.POINTER(FrameFormat), vp, vp, sz, i, i,
                                        C.POINTER(AnnotateOpts), vp]
    lib.flm_flow_pyramid_bytes.restype = sz
    lib.flm_flow_pyramid_bytes.argtypes = [i, i, i]
    lib.flm_flow_pyramid.restype = i
    lib.flm_flow_pyramid.argtypes = [vp, vp, i, i, i, i, i, vp]
    lib.flm_flow_opts_init.restype = None
    lib.flm_flow_opts_init.argtypes = [C.POINTER(FlowOpts)]
    lib.flm_landmark_flow.restype = i
    lib.flm_landmark_flow.argtypes = [vp, vp, vp, i, i, i, vp, vp, vp, i, C.POINTER(FlowOpts), vp, vp, vp, vp]
    lib.flm_track_gather_flow.restype = i
    lib.flm_track_gather_flow.argtypes = [vp, vp, i, i, i, i, i, vp, vp, d] + [vp] * 17
    lib.flm_landmark_flow_rows.restype = i
    lib.flm_landmark_flow_rows.argtypes = [vp, vp, vp, i, i, i, vp, i, vp, vp, vp, i, C.POINTER(FlowOpts), d] + [vp] * 5
    lib.flm_track_flow_history_put.restype = i
    lib.flm_track_flow_history_put.argtypes = [vp, vp, vp, vp, vp, vp, i, i, i, vp, vp, vp, vp]


def load():
    """Load the HIP library or raise: the product path has no fallback."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.isfile(LIB_PATH):
        raise FlmError(
            "libflm_hip.so is not built (%s). Build it with `python face-landmark-detector_amd/build.py`; "
            "this package has no CPU fallback." % LIB_PATH)
    # PyTorch-ROCm bundles its own libamdhip64.so.7 / libhsa-runtime64.so.1.  Import torch FIRST so the
    # dynamic linker binds this library to that same runtime (same SONAME) -- loading ours first would
    # pull /opt/rocm's copy in beside torch's: two HIP runtimes in one process, and launches on torch's
    # streams / pointers fail with "no ROCm-capable device".
    import torch  # noqa: F401
    lib = C.CDLL(LIB_PATH)
    for name in EXPORTS:
        if not hasattr(lib, name):
            raise FlmError("libflm_hip.so lacks symbol %s (stale build?)" % name)
    _declare(lib)
    if lib.flm_abi_version() != ABI_VERSION:
        raise FlmError("libflm_hip.so ABI %d != expected %d" % (lib.flm_abi_version(), ABI_VERSION))
    _lib = lib
    return lib


def check(rc: int, what: str = ""):
    if rc != 0:
        msg = load().flm_last_error()
        raise FlmError("%s failed (%d): %s" % (what or "flm call", rc, msg.decode() if msg else "?"))


@contextlib.contextmanager
def tuning(*keys, **knobs):
    """The A/B knobs of flm_set_tuning for the length of a `with` block: tuning(up3_wreg=1) sets a knob, tuning("warp_rows")
    only names one the block sets itself.  On exit, also by exception, every named knob returns to the value it had on
    entry (read with flm_get_tuning); blocks nest."""
    lib = load()
    saved = {}
    try:
        for key in (*keys, *knobs):
            old = C.c_int()
            check(lib.flm_get_tuning(key.encode(), C.byref(old)), "get_tuning")
            saved[key] = old.value
            if key in knobs:
                check(lib.flm_set_tuning(key.encode(), int(knobs[key])), "set_tuning")
        yield
    finally:
        for key, old in saved.items():
            check(lib.flm_set_tuning(key.encode(), old), "set_tuning")


def require_gpu():
    """The torch device used for HBM allocations and streams; raises without a GPU."""
    import torch
    if not torch.cuda.is_available():
        raise FlmError("no AMD GPU visible to PyTorch-ROCm: the landmark path runs on MI355X only "
                       "(there is no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device())


def stream_ptr():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def int_array(values):
    """A host int32 array for the `const int*` arguments (flm_decode_sweep's mode list)."""
    values = [int(v) for v in values]
    return (C.c_int * max(1, len(values)))(*values)


def ptr(t):
    return C.c_void_p(t.data_ptr())
