"""Inference workflows: mirror of reference keypoints_detector/prediction.py on the HIP path.

Same function names, argument order and error behaviour as the reference
(`keypts_predict` :158-196, `_prediction` :199-222, `detect_marks` :16-96,
`model_from_checkpoint_path` :116-133), with the defects of SURVEY.md section 3.4 routed
around rather than reproduced (`keypts_predict` returns the class map instead of dropping it;
`os.path.isdir` is only asked about strings), plus the batch entry points `predict()` and
`align()` that BASELINE.json names.
"""
from __future__ import annotations

import glob
import json
import os

import numpy as np
import six

from . import _lib, alignment
from .data.generator import get_image_array, imread_bgr, resize_u8_device
from .networks.config import IMAGE_ORDERING


# ---- checkpoint discovery (reference training.py:41-71, prediction.py:116-133) ---------------------
def find_latest_checkpoint(checkpoints_path, fail_safe=True):
    """Newest `<checkpoints_path>.<epoch>[.npz]` by numeric suffix (training.py:41-71; the
    reference strips TensorFlow's `.index`, this build's container suffix is `.npz`)."""
    def epoch_of(path):
        tail = path.replace(checkpoints_path, "").strip(".")
        for suf in (".npz", ".index"):
            if tail.endswith(suf):
                tail = tail[: -len(suf)]
        return tail

    files = [f for f in glob.glob(checkpoints_path + ".*") if epoch_of(f).isdigit()]
    if not files:
        if not fail_safe:
            raise ValueError("Checkpoint path {0} invalid".format(checkpoints_path))
        return None
    return max(files, key=lambda f: int(epoch_of(f)))


def model_from_checkpoint_path(checkpoints_path):
    """prediction.py:116-133.  The sidecar `<ckpt>_config.json` holds model_class, n_classes,
    input_height, input_width (the trainer omits the last two, training.py:195-200: they then
    default to output_height-8 / output_width-8, the vanilla FCN-8 relation)."""
    from .networks.basic_models import LANDMARKS_MODELS
    assert (os.path.isfile(checkpoints_path + "_config.json")), "Checkpoint not found."
    model_config = json.loads(open(checkpoints_path + "_config.json", "r").read())
    latest_weights = find_latest_checkpoint(checkpoints_path)
    assert (latest_weights is not None), "Checkpoint not found."
    ih = model_config.get("input_height", model_config.get("output_height", 264) - 8)
    iw = model_config.get("input_width", model_config.get("output_width", 264) - 8)
    model = LANDMARKS_MODELS[model_config["model_class"]](model_config["n_classes"], input_height=ih,
                                                          input_width=iw)
    print("loaded weights ", latest_weights)
    status = model.load_weights(latest_weights)
    if status is not None:
        status.expect_partial()
    return model


# ---- FCN class-map prediction ------------------------------------------------------------------------
def _prediction(model, inp, input_width, input_height, output_height, output_width, n_classes,
                colors=None, show_legends=False, class_names=None, pred_dim=None, overlay_img=False,
                out_fname=None):
    """prediction.py:199-222: preprocess -> model.predict -> per-pixel argmax, int64 [H',W'].

    The preprocess (get_image_array sub_mean, :207), the forward (:208) and the argmax (:209)
    run as one launch sequence on the device; only the class map returns to the host.
    """
    import torch
    dev = _lib.require_gpu()
    if not isinstance(inp, np.ndarray) or inp.ndim != 3 or inp.shape[2] != 3 or inp.dtype != np.uint8:
        # non-uint8 arrays take the reference's host route (float images are only mean-shifted)
        x = get_image_array(inp, input_width, input_height, ordering=IMAGE_ORDERING)
        xd = torch.from_numpy(np.ascontiguousarray(x[None])).to(dev)
    else:
        d = resize_u8_device(torch.from_numpy(np.ascontiguousarray(inp)).to(dev), input_height, input_width)
        xd = d[None].contiguous()
    pr = model.forward_device(xd, "classmap")[0].to(torch.int64).cpu().numpy()
    assert pr.shape == (output_height, output_width)
    if out_fname is not None:
        from .utils.plots import visualize_keypoints
        seg_img = visualize_keypoints(pr, inp, n_classes=n_classes, colors=colors, overlay_img=overlay_img,
                                      show_legends=show_legends, class_names=class_names, pred_dim=pred_dim)
        from PIL import Image
        Image.fromarray(np.ascontiguousarray(seg_img[:, :, ::-1].astype(np.uint8))).save(out_fname)
    return pr


def keypts_predict(model=None, inp=None, out_fname=None, checkpoints_path=None, overlay_img=False,
                   class_names=None, show_legends=False, colors=None, pred_dim=None, read_image_type=1):
    """prediction.py:158-196, returning the class map (the reference drops it)."""
    if model is None and checkpoints_path is None:
        raise ValueError("Both model and checkpoint_path cannot be empty")
    if model is None and (checkpoints_path is not None):
        model = model_from_checkpoint_path(checkpoints_path)
    assert (inp is not None), "Invalid input, should be either directory, ndarray or image path"
    assert ((type(inp) is np.ndarray) or isinstance(inp, six.string_types)), \
        "Input should be the CV image or the input file name"
    if isinstance(inp, six.string_types):
        inp = imread_bgr(inp, read_image_type)
    assert (len(inp.shape) == 3 or len(inp.shape) == 1 or len(inp.shape) == 4), "Image should be h,w,3 "
    return _prediction(model, inp, model.input_width, model.input_height, model.output_height,
                       model.output_width, model.n_classes, colors, show_legends, class_names, pred_dim,
                       overlay_img, out_fname)


# ---- batch entry points --------------------------------------------------------------------------------
def _fit_weights(weights, landmarks_given):
    """The `weights` argument of align / align_frames: None, "score" or an [N,C] array / tensor; anything else is a
    ValueError raised before any device work."""
    if weights is None:
        return
    if isinstance(weights, str):
        if weights != "score":
            raise ValueError("weights must be None, \"score\" or an [N,C] tensor (got %r)" % (weights,))
        if landmarks_given:
            raise ValueError("weights=\"score\" needs the model's own forward: pass the weights as a tensor with `landmarks`")
    elif getattr(weights, "ndim", None) != 2:
        raise ValueError("weights must be None, \"score\" or an [N,C] tensor")


def _weights_on_device(weights, n, c, dev):
    import torch
    w = torch.as_tensor(weights).to(device=dev, dtype=torch.float64)
    if tuple(w.shape) != (n, c):
        raise ValueError("weights must be [%d,%d], got %s" % (n, c, tuple(w.shape)))
    return w


def _aligned_format(aligned_format, numpy_io):
    """The `aligned_format` argument of align / align_frames, checked before any device work."""
    if aligned_format is None:
        return
    if not isinstance(aligned_format, alignment.AlignedFormat):
        raise ValueError("aligned_format must be an alignment.AlignedFormat or None (got %r)" % (aligned_format,))
    if numpy_io and aligned_format.numpy_dtype is None:
        raise ValueError("numpy has no %s: pass the crops as a CUDA tensor to get aligned faces of that type"
                         % aligned_format.dtype)


def predict(crops, model, n_points=4, thresh=0.0, to_input_space=False, return_stats=False, fallback_faces=0):
    """Batched landmarks: crops [N,H,W,3] (numpy or CUDA tensor; uint8 BGR or float32
    preprocessed) -> float64 [N,C,2] (x,y).

    `return_stats=True` returns (landmarks [N,C,2], score [N,C], cov [N,C,3]) instead: three views of ONE landmark
    record tensor [N,C,6] (forward_device "landmark_stats"; include/flm.h).  score is the mean selected probability the
    reject test of utils/metrics.py:78-79 compares -- the reference computes it and keeps only the verdict, which with
    the shipped thresh = 0 never rejects; cov = (var_x, var_y, cov_xy) of the selected pixels about (x, y), in
    output-grid px^2, (-1, -1, 0) for a rejected landmark.  `to_input_space` scales the COORDINATES only: score has no
    unit and cov stays in output-grid px^2.

    Coordinates are in output-grid pixels (0..W'-1), as the reference's decode leaves them
    (utils/metrics.py:80); `to_input_space=True` rescales to input-crop pixels
    (x * W / W').  n_points < 1 selects the all-pixel centroid, else top-n (utils/metrics.py:58,66);
    the reference as shipped always runs n_points=4, thresh=0.
    `fallback_faces` = B > 0 (here, in `align`, in `align_frames` and in `FaceTracker`): the forward redoes only the
    faces whose candidate lists fail, at most B of them, instead of the whole batch (forward_device; same landmarks).
    Returns the type it was given (numpy -> numpy, CUDA tensor -> CUDA tensor).
    """
    import torch
    if return_stats not in (False, True):
        raise ValueError("return_stats must be a bool")
    if return_stats and (getattr(crops, "ndim", None) != 4 or crops.shape[3] != 3):
        raise ValueError("crops must be [N,H,W,3]")
    was_np = not isinstance(crops, torch.Tensor)
    xd = torch.from_numpy(np.ascontiguousarray(crops)).to(_lib.require_gpu()) if was_np else crops
    rec = model.forward_device(xd, "landmark_stats" if return_stats else "landmarks", n_points=n_points, thresh=thresh,
                               fallback_faces=fallback_faces)
    if was_np and return_stats:
        rec = rec.cpu()
    lm = rec[..., :2] if return_stats else rec
    if to_input_space:
        scale = torch.tensor([model.input_width / model.output_width, model.input_height / model.output_height],
                             dtype=torch.float64, device=lm.device)
        if return_stats:
            lm.copy_(torch.where(lm < 0, lm, lm * scale))   # in place: the three results stay views of one tensor
        else:
            lm = torch.where(lm < 0, lm, lm * scale)
    if return_stats:
        out = (lm, rec[..., 2], rec[..., 3:])
        return tuple(t.numpy() for t in out) if was_np else out
    return lm.cpu().numpy() if was_np else lm


def align(crops, model=None, landmarks=None, template=None, out_size=None, n_points=4, thresh=0.0, weights=None,
          aligned_format=None, fallback_faces=0):
    """Align face crops by the similarity transform that maps their landmarks onto a template.

    crops [N,H,W,3] uint8/float32; `landmarks` float64 [N,C,2] in output-grid pixels (predicted
    with `model` when omitted); `template` float64 [C,2] in aligned-image pixels (default
    `alignment.canonical_template`); out_size (h, w) defaults to the crop size.
    Returns (aligned float32 [N,h,w,3], M float32 [N,2,3], landmarks).

    `weights` weighs the landmarks of the fit (flm_similarity_from_landmarks_weighted): None, the unweighted fit on every
    landmark the decode kept -- with the shipped thresh = 0 that is all of them, occluded ones included; "score", the
    model's own per-landmark score: the forward runs in its "landmark_stats" mode and the fit reads coordinates and
    scores from that record tensor in place, no launch in between; or a float64 [N,C] array / tensor (weight <= 0 or
    NaN: the landmark is left out).  With weights the call returns a fourth value, the [N,C] weights it used.

    `aligned_format`: an `alignment.AlignedFormat` -- the aligned crops leave the warp in that layout, type, channel
    order and normalisation (`AlignedFormat.matcher()`: float16 [N,3,h,w], RGB, in [-1,1]) instead of float32
    [N,h,w,3]; every other returned value is what the call returns without it.  numpy callers get numpy arrays
    (float32, float16, uint8; bfloat16 needs tensors: ValueError).
    """
    import torch
    _fit_weights(weights, landmarks is not None)
    was_np = not isinstance(crops, torch.Tensor)
    _aligned_format(aligned_format, was_np)
    dev = _lib.require_gpu()
    xd = torch.from_numpy(np.ascontiguousarray(crops)).to(dev) if was_np else crops
    if landmarks is None:
        if model is None:
            raise ValueError("align needs either landmarks or a model")
        if isinstance(weights, str):   # "score"
            rec = model.forward_device(xd, "landmark_stats", n_points=n_points, thresh=thresh,
                                       fallback_faces=fallback_faces)
            lm, wd = rec[..., :2], rec[..., 2]
        else:
            lm = model.forward_device(xd, "landmarks", n_points=n_points, thresh=thresh, fallback_faces=fallback_faces)
    else:
        lm = torch.as_tensor(landmarks, dtype=torch.float64).to(dev)
    if weights is not None and not isinstance(weights, str):
        wd = _weights_on_device(weights, int(lm.shape[0]), int(lm.shape[1]), dev)
    h, w = int(xd.shape[1]), int(xd.shape[2])
    oh, ow = out_size if out_size is not None else (h, w)
    k = int(lm.shape[1])
    tm = alignment.canonical_template(k, oh, ow) if template is None else np.asarray(template, np.float64)
    tmd = torch.from_numpy(np.ascontiguousarray(tm)).to(dev)
    # landmarks live on the model's output grid (W' = W + 8): bring them to crop pixels
    sc = (1.0, 1.0)
    if model is not None:
        sc = (model.input_width / model.output_width, model.input_height / model.output_height)
    if weights is not None:
        aligned, m = alignment.align_device(xd, lm, tmd, oh, ow, sc, weights=wd, fmt=aligned_format)
        if was_np:
            return aligned.cpu().numpy(), m.cpu().numpy(), lm.cpu().numpy(), wd.cpu().numpy()
        return aligned, m, lm, wd
    aligned, m = alignment.align_device(xd, lm, tmd, oh, ow, sc, fmt=aligned_format)
    if was_np:
        return aligned.cpu().numpy(), m.cpu().numpy(), lm.cpu().numpy()
    return aligned, m, lm


# ---- multi-face stream: detect_marks (prediction.py:16-96) ---------------------------------------------
def get_square_box(box):
    """prediction.py:36-65, integer box squaring by symmetric expansion."""
    left_x, top_y, right_x, bottom_y = box
    box_width = right_x - left_x
    box_height = bottom_y - top_y
    diff = box_height - box_width
    delta = int(abs(diff) / 2)
    if diff == 0:
        return box
    elif diff > 0:
        left_x -= delta
        right_x += delta
        if diff % 2 == 1:
            right_x += 1
    else:
        top_y -= delta
        bottom_y += delta
        if diff % 2 == 1:
            bottom_y += 1
    assert ((right_x - left_x) == (bottom_y - top_y)), 'Box is not square.'
    return [left_x, top_y, right_x, bottom_y]


def move_box(box, offset):
    """prediction.py:67-74."""
    return [box[0] + offset[0], box[1] + offset[1], box[2] + offset[0], box[3] + offset[1]]


def face_boxes(faces):
    """The box maths of detect_marks for a list of faces (prediction.py:76-78)."""
    out = []
    for face in faces:
        offset_y = int(abs((face[3] - face[1]) * 0.1))
        out.append(get_square_box(move_box(list(face), [0, offset_y])))
    return out


def crop_faces_device(frame, boxes, out_h, out_w, out=None, boxes_dev=None):
    """frame: CUDA uint8 [H,W,3]; boxes: list of (x0,y0,x1,y1) -> CUDA uint8 [K,out_h,out_w,3]
    (crop + bilinear resize, prediction.py:80-82; BGR kept, the FCN loader handles the order).
    `out`: write into this contiguous [K,out_h,out_w,3] uint8 tensor (a slice of a larger batch) instead of a new one;
    `boxes_dev`: the boxes already on the device (int32 [K,4]), e.g. a slice of one upload for several frames."""
    import torch
    lib = _lib.load()
    k = len(boxes) if boxes_dev is None else int(boxes_dev.shape[0])
    if boxes_dev is None:
        boxes_dev = torch.tensor(np.asarray(boxes, np.int32).reshape(k, 4), dtype=torch.int32, device=frame.device)
    elif boxes_dev.dtype != torch.int32 or not boxes_dev.is_cuda or not boxes_dev.is_contiguous() or boxes_dev.shape[1:] != (4,):
        raise ValueError("boxes_dev must be a contiguous CUDA int32 [K,4] tensor")
    if out is None:
        out = torch.empty((k, out_h, out_w, 3), dtype=torch.uint8, device=frame.device)
    elif (tuple(out.shape) != (k, out_h, out_w, 3) or out.dtype != torch.uint8 or not out.is_cuda
          or not out.is_contiguous()):
        raise ValueError("out must be a contiguous CUDA uint8 [%d,%d,%d,3] tensor" % (k, out_h, out_w))
    if k:
        _lib.check(lib.flm_crop_resize(_lib.stream_ptr(), _lib.ptr(frame.contiguous()), int(frame.shape[0]),
                                       int(frame.shape[1]), _lib.ptr(boxes_dev), k, _lib.ptr(out), out_h, out_w),
                   "flm_crop_resize")
    return out


def _frame_format(frame_format):
    if frame_format is not None and not isinstance(frame_format, alignment.FrameFormat):
        raise ValueError("frame_format must be an alignment.FrameFormat or None (got %r)" % (frame_format,))


def frames_to_bgr_device(frames, frame_format, out=None):
    """An NV12 ring as a dense BGR ring: frames CUDA uint8 [F,rows,pitch] in `frame_format`
    (alignment.FrameFormat.nv12(...)) -> CUDA uint8 [F,H,W,3] (flm_frames_to_bgr: the integer conversion include/flm.h
    states).  The frame-reading calls take the NV12 ring directly (`frame_format=`); this is the frame they compute
    on, for a consumer that needs the BGR pixels themselves."""
    import torch
    _frame_format(frame_format)
    if frame_format is None or frame_format.pixel != "nv12":
        raise ValueError("frames_to_bgr_device converts an NV12 ring: frame_format must be FrameFormat.nv12(...)")
    nf, fh, fw, stride = frame_format.ring(frames)
    if out is None:
        out = torch.empty((nf, fh, fw, 3), dtype=torch.uint8, device=frames.device)
    elif (not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or tuple(out.shape) != (nf, fh, fw, 3)
          or not out.is_cuda or not out.is_contiguous()):
        raise ValueError("out must be a contiguous CUDA uint8 [%d,%d,%d,3] tensor" % (nf, fh, fw))
    if nf:
        cs = frame_format.struct(frames)
        _lib.check(_lib.load().flm_frames_to_bgr(_lib.stream_ptr(), _lib.ptr(frames), stride, nf, fh, fw, _lib.C.byref(cs),
                                                 _lib.ptr(out)), "flm_frames_to_bgr")
    return out


def crop_frames_device(frames, faces_per_frame, out_h, out_w, frame_index=None, return_device=False, frame_format=None):
    """The faces of several frames as ONE batch: faces_per_frame: per frame a list of detector boxes (x0,y0,x1,y1) ->
    (CUDA uint8 [K_total,out_h,out_w,3], squared boxes per frame).  One upload of all boxes; no per-frame allocation,
    no concatenation: the shape a multi-face stream feeds the landmark model with (prediction.py:99-113 loops per face).
    frames: either a list of CUDA uint8 [H,W,3] tensors (one crop / resize launch per frame straight into its slice of
    the batch) or ONE CUDA uint8 [F,H,W,3] tensor -- a ring of stream frames in one allocation -- with `frame_index`
    naming the ring slot of every entry of faces_per_frame (default 0, 1, ...): then all faces are cut in one launch.
    `return_device=True` also returns the CUDA int32 tensors of the squared boxes [K_total,4] and of every face's frame
    (ring slot, or position in the list) [K_total], views of the one upload: what the frame-space tail
    (`align_frames`) reads.
    `frame_format`: an alignment.FrameFormat -- how the ring holds its pixels (flm_crop_resize_frames_src; then `frames`
    must be the one ring tensor).  FrameFormat.nv12(H, W, ...): the decoder's CUDA uint8 [F,rows,pitch] ring, the crops
    bit for bit those of the converted BGR ring.  None: as ever."""
    import torch
    _frame_format(frame_format)
    geom = None if frame_format is None else frame_format.ring(frames)   # (before anything is allocated or uploaded)
    boxes = [face_boxes(f) for f in faces_per_frame]
    total = sum(len(b) for b in boxes)
    ring = isinstance(frames, torch.Tensor)
    if geom is None and ring and (frames.dim() != 4 or frames.dtype != torch.uint8 or not frames.is_cuda or not frames.is_contiguous()
                 or frames.shape[3] != 3):
        raise ValueError("frames must be a list of CUDA uint8 [H,W,3] tensors or one contiguous CUDA uint8 [F,H,W,3] tensor")
    dev = frames.device if ring else (frames[0].device if len(frames) else _lib.require_gpu())
    out = torch.empty((total, out_h, out_w, 3), dtype=torch.uint8, device=dev)
    if total == 0:
        if return_device:
            return (out, boxes, torch.empty((0, 4), dtype=torch.int32, device=dev),
                    torch.empty((0,), dtype=torch.int32, device=dev))
        return out, boxes
    flat = np.concatenate([np.asarray(b, np.int32).reshape(len(b), 4) for b in boxes if len(b)], 0)
    if ring:
        slots = list(range(len(boxes))) if frame_index is None else [int(v) for v in frame_index]
        if len(slots) != len(boxes) or any(not (0 <= v < frames.shape[0]) for v in slots):
            raise ValueError("frame_index must name a ring slot in [0, %d) for every frame" % frames.shape[0])
        idx = np.concatenate([np.full(len(b), v, np.int32) for b, v in zip(boxes, slots) if len(b)])
        both = torch.from_numpy(np.concatenate([flat.reshape(-1), idx])).to(dev)   # one upload: boxes, then slots
        lib = _lib.load()
        if geom is not None:
            nf, fh, fw, stride = geom
            cs = frame_format.struct(frames)
            _lib.check(lib.flm_crop_resize_frames_src(_lib.stream_ptr(), _lib.ptr(frames), stride, nf, fh, fw,
                                                      _lib.ptr(both), _lib.ptr(both[4 * total:]), total, _lib.ptr(out),
                                                      out_h, out_w, _lib.C.byref(cs)), "flm_crop_resize_frames_src")
            if return_device:
                return out, boxes, both[:4 * total].view(total, 4), both[4 * total:]
            return out, boxes
        fh, fw = int(frames.shape[1]), int(frames.shape[2])
        _lib.check(lib.flm_crop_resize_frames(_lib.stream_ptr(), _lib.ptr(frames), fh * fw * 3, int(frames.shape[0]), fh, fw,
                                              _lib.ptr(both), _lib.ptr(both[4 * total:]), total, _lib.ptr(out), out_h, out_w),
                   "flm_crop_resize_frames")
        if return_device:
            return out, boxes, both[:4 * total].view(total, 4), both[4 * total:]
        return out, boxes
    if return_device:
        idx = np.concatenate([np.full(len(b), v, np.int32) for v, b in enumerate(boxes) if len(b)])
        both = torch.from_numpy(np.concatenate([flat.reshape(-1), idx])).to(dev)   # one upload: boxes, then frames
        bdev = both[:4 * total].view(total, 4)
    else:
        bdev = torch.from_numpy(flat).to(dev)
    o = 0
    for frame, b in zip(frames, boxes):
        if len(b):
            crop_faces_device(frame, None, out_h, out_w, out=out[o:o + len(b)], boxes_dev=bdev[o:o + len(b)])
            o += len(b)
    if return_device:
        return out, boxes, bdev, both[4 * total:]
    return out, boxes


_TEMPLATES = {}   # (landmarks, out_h, out_w, device) -> canonical template on the device, uploaded once


def align_frames(frames, faces_per_frame, model, template=None, out_size=(112, 112), n_points=4, thresh=0.0,
                 frame_index=None, samples=1, weights=None, aligned_format=None, frame_format=None, fallback_faces=0):
    """The multi-face stream end to end in FRAME coordinates: detector boxes of a group of frames -> aligned faces
    sampled from the frames themselves.

    frames: the CUDA uint8 [F,H,W,3] ring (or a list of same-size CUDA uint8 [H,W,3] frames, stacked once);
    faces_per_frame: per entry a list of detector boxes (x0,y0,x1,y1); `frame_index` names the ring slot of every entry
    (default 0, 1, ...).  Sequence: crop_frames_device -> model.forward_device(crops, "landmarks") ->
    alignment.landmarks_to_frame_device -> alignment.similarity_device -> alignment.warp_frames_device: one upload (the
    boxes), no download, no host synchronisation.  `template` float64 [C,2] in aligned pixels (numpy or CUDA; default
    `alignment.canonical_template`); `samples` 1, 2 or 4 bilinear samples per axis and aligned pixel (for faces much
    larger than out_size).  `weights`: None, "score" or a float64 [K,C] tensor, as `align` takes it -- "score" runs the
    forward in its "landmark_stats" mode, hands a contiguous copy of the record's xy columns (16 bytes per landmark) to
    flm_landmarks_to_frame and feeds the score column to the weighted fit in place; the call then returns the [K,C]
    weights it used as a fifth value.  `aligned_format`: an `alignment.AlignedFormat` for the aligned faces, written by
    the warp itself -- `AlignedFormat.matcher()` gives float16 [K,3,oh,ow], RGB, in [-1,1], what a face-embedding network
    reads -- instead of float32 [K,oh,ow,3]; the other returned values do not depend on it.  `frame_format`: an
    `alignment.FrameFormat` -- `FrameFormat.nv12(H, W, matrix="bt709")` takes the decoder's CUDA uint8 [F,rows,pitch]
    ring as it is: the crop and the warp convert their taps, nothing between them changes, and all returned tensors
    equal those of the call on `frames_to_bgr_device(frames, frame_format)`.
    Returns CUDA tensors (aligned float32 [K,oh,ow,3], M float32 [K,2,3] frame px -> aligned px, landmarks float64
    [K,C,2] in frame px with (-1,-1) for rejected points, squared boxes int32 [K,4]); K == 0 launches nothing."""
    import torch
    _fit_weights(weights, False)
    _aligned_format(aligned_format, False)
    _frame_format(frame_format)
    if frame_format is not None:
        nf, fh, fw, _ = frame_format.ring(frames)
    else:
        if isinstance(frames, (list, tuple)):
            if not len(frames) or any(not isinstance(f, torch.Tensor) or f.dim() != 3 or f.dtype != torch.uint8
                                      or tuple(f.shape) != tuple(frames[0].shape) for f in frames):
                raise ValueError("frames must be a non-empty list of same-size uint8 [H,W,3] tensors")
            frames = torch.stack(list(frames), 0)
        if not isinstance(frames, torch.Tensor) or frames.dim() != 4 or frames.dtype != torch.uint8 or frames.shape[3] != 3:
            raise ValueError("frames must be one uint8 [F,H,W,3] tensor or a list of uint8 [H,W,3] tensors")
        nf, fh, fw = [int(v) for v in frames.shape[:3]]
    if fw < 2 or fh < 1 or fh * fw * 3 >= 2 ** 31:
        raise ValueError("frames of %dx%d are outside the warp's reach (width >= 2, H*W*3 < 2^31)" % (fh, fw))
    slots = list(range(len(faces_per_frame))) if frame_index is None else [int(v) for v in frame_index]
    if len(slots) != len(faces_per_frame) or any(not (0 <= v < nf) for v in slots):
        raise ValueError("frame_index must name a ring slot in [0, %d) for every entry of faces_per_frame" % nf)
    if samples not in (1, 2, 4):
        raise ValueError("samples must be 1, 2 or 4")
    oh, ow = [int(v) for v in out_size]
    if oh < 1 or ow < 1:
        raise ValueError("out_size must be positive")
    if not frames.is_cuda:
        raise ValueError("frames must live on the GPU")
    frames = frames.contiguous()
    dev = frames.device
    c = int(model.n_classes)
    crops, _, boxes_dev, idx_dev = crop_frames_device(frames, faces_per_frame, model.input_height, model.input_width,
                                                      frame_index=slots, return_device=True,
                                                      frame_format=frame_format)
    k = int(crops.shape[0])
    if k == 0:
        empty = (torch.empty((0, oh, ow, 3), dtype=torch.float32, device=dev) if aligned_format is None else
                 torch.empty(aligned_format.shape(0, oh, ow), dtype=aligned_format.torch_dtype, device=dev),
                 torch.empty((0, 2, 3), dtype=torch.float32, device=dev),
                 torch.empty((0, c, 2), dtype=torch.float64, device=dev), boxes_dev)
        return empty if weights is None else empty + (torch.empty((0, c), dtype=torch.float64, device=dev),)
    if template is None:
        key = (c, oh, ow, str(dev))
        if key not in _TEMPLATES:
            _TEMPLATES[key] = torch.from_numpy(alignment.canonical_template(c, oh, ow)).to(dev)
        tmd = _TEMPLATES[key]
    elif isinstance(template, torch.Tensor):
        tmd = template.to(device=dev, dtype=torch.float64)
    else:
        tmd = torch.from_numpy(np.ascontiguousarray(np.asarray(template, np.float64))).to(dev)
    if tuple(tmd.shape) != (c, 2):
        raise ValueError("template must be [%d,2]" % c)
    wd = None
    if isinstance(weights, str):   # "score"
        rec = model.forward_device(crops, "landmark_stats", n_points=n_points, thresh=thresh,
                                   fallback_faces=fallback_faces)
        lm, wd = rec[..., :2].contiguous(), rec[..., 2]
    else:
        lm = model.forward_device(crops, "landmarks", n_points=n_points, thresh=thresh, fallback_faces=fallback_faces)
        if weights is not None:
            wd = _weights_on_device(weights, k, c, dev)
    lm = alignment.landmarks_to_frame_device(lm, boxes_dev, (model.output_height, model.output_width), (fh, fw))
    m = alignment.similarity_device(lm, tmd, weights=wd)
    aligned = alignment.warp_frames_device(frames, m, oh, ow, frame_index_dev=idx_dev, boxes_dev=boxes_dev,
                                           samples=samples, fmt=aligned_format, src=frame_format)
    if weights is not None:
        return aligned, m, lm, boxes_dev, wd
    return aligned, m, lm, boxes_dev


_MESHES = {}


def _default_mesh(n_landmarks, oh, ow):
    key = (int(n_landmarks), int(oh), int(ow))
    if key not in _MESHES:
        _MESHES[key] = alignment.FaceMesh.default(*key)
    return _MESHES[key]


def normalize_frames(ring, landmarks, m, mesh=None, out_size=(112, 112), frame_index=None, samples=1, aligned_format=None,
                     frame_format=None):
    """Shape-normalised faces for landmarks and matrices that `align_frames` returned: every face is warped piecewise
    affinely over the landmark mesh, so that each landmark's texture lands on its template pixel -- what
    `skimage.transform.PiecewiseAffineTransform` + `warp` do on the host, in one launch from the ring
    (alignment.warp_mesh_frames_device).

    ring, frame_format: as `align_frames` takes them; landmarks: CUDA float64 [K,C,2] in frame pixels (third value of
    `align_frames`); m: CUDA float32 [K,2,3] frame px -> aligned px (its second); mesh: an `alignment.FaceMesh` whose
    landmark points are the template the matrices were fitted to, None for `FaceMesh.default(C, *out_size)` (the mesh of
    `align_frames`' default template); frame_index: None (every face lies in slot 0), a host sequence of K ring slots
    (one upload) or a CUDA int32 [K] tensor, what `crop_frames_device` returns last; samples, aligned_format: as
    `align_frames` takes them.  Returns the faces, float32 [K,oh,ow,3] or the format's tensor."""
    import torch
    _aligned_format(aligned_format, False)
    _frame_format(frame_format)
    if mesh is not None and not isinstance(mesh, alignment.FaceMesh):
        raise ValueError("mesh must be None or an alignment.FaceMesh (got %r)" % (mesh,))
    if samples not in (1, 2, 4):
        raise ValueError("samples must be 1, 2 or 4")
    oh, ow = [int(v) for v in out_size]
    if not isinstance(landmarks, torch.Tensor) or landmarks.dim() != 3 or not landmarks.is_cuda:
        raise ValueError("landmarks must be a CUDA float64 [K,C,2] tensor")
    k, c = int(landmarks.shape[0]), int(landmarks.shape[1])
    if mesh is None:
        mesh = _default_mesh(c, oh, ow)
    if frame_index is not None and not isinstance(frame_index, torch.Tensor):
        idx = [int(v) for v in frame_index]
        if len(idx) != k:
            raise ValueError("frame_index must name a ring slot for each of the %d faces" % k)
        frame_index = torch.tensor(idx, dtype=torch.int32).to(landmarks.device)
    return alignment.warp_mesh_frames_device(ring, landmarks, m, mesh, oh, ow, frame_index_dev=frame_index,
                                             samples=samples, fmt=aligned_format, src=frame_format)


def annotate_frames(ring, landmarks, frame_index=None, frame_format=None, **options):
    """`draw_marks(img, marks)`, the last line of the reference's frame loop (prediction.py:99-113), for the faces of a
    ring that stays on the device -- and an outline and a mosaic of every face beside the marks.

    ring: the frame ring as `align_frames` takes it (`frame_format`: an alignment.FrameFormat, None for the CUDA uint8
    [F,H,W,3] ring); landmarks: CUDA float64 [K,C,2] in frame pixels, what `align_frames` returns third; frame_index:
    None (every face lies in slot 0), a host sequence of K ring slots (one upload) or a CUDA int32 [K] tensor (used where
    it lies), what `crop_frames_device` returns last.  options: the arguments of `alignment.FrameAnnotation` -- marks,
    box, redact, margin, mark_color, box_color.  The ring slots are WRITTEN: run it after the calls that read the frame.
    Returns the regions, CUDA int32 [K,4]."""
    import torch
    _frame_format(frame_format)
    opts = alignment.FrameAnnotation(**options)
    if frame_index is not None and not isinstance(frame_index, torch.Tensor):
        if not isinstance(landmarks, torch.Tensor) or not landmarks.is_cuda:
            raise ValueError("landmarks must be a CUDA float64 [K,C,2] tensor")
        idx = [int(v) for v in frame_index]
        if len(idx) != int(landmarks.shape[0]):
            raise ValueError("frame_index must name a ring slot for each of the %d faces" % int(landmarks.shape[0]))
        frame_index = torch.tensor(idx, dtype=torch.int32).to(landmarks.device)
    return alignment.annotate_frames_device(ring, landmarks, frame_index_dev=frame_index, opts=opts, src=frame_format)


def detect_marks_batch(img, model, faces, n_points=4, thresh=0.0):
    """All faces of one frame in one batch: crop -> FCN -> decode -> back-projection
    (prediction.py:76-94).  Returns uint [K,C,2] image coordinates."""
    import torch
    if len(faces) == 0:   # a frame without faces: the reference's per-face loop (prediction.py:105-107) does nothing
        return np.zeros((0, model.n_classes, 2), np.uint)
    dev = _lib.require_gpu()
    frame = torch.from_numpy(np.ascontiguousarray(img)).to(dev) if not isinstance(img, torch.Tensor) else img
    boxes = face_boxes(faces)
    crops = crop_faces_device(frame, boxes, model.input_height, model.input_width)
    lm = model.forward_device(crops, "landmarks", n_points=n_points, thresh=thresh).cpu().numpy()
    out = []
    for k, fb in enumerate(boxes):
        # marks in [0,1] of the crop, then prediction.py:91-94
        marks = (lm[k] / np.array([model.output_width, model.output_height], np.float64)).astype(np.float32)
        marks *= (fb[2] - fb[0])
        marks[:, 0] += fb[0]
        marks[:, 1] += fb[1]
        out.append(np.maximum(marks, 0).astype(np.uint))
    return np.stack(out)


def detect_marks(img, model, face):
    """prediction.py:16-96 for one face; `model` is this package's FCN-8 model object."""
    return detect_marks_batch(img, model, [face])[0]


def video_predict(facedetector_fn, landmark_model, frames=None, on_frame=None, n_points=4, thresh=0.0):
    """prediction.py:99-113: per frame `rects = facedetector_fn(img)`, landmarks of every face, `draw_marks(img, marks)`.

    The reference reads camera 0 through cv2.VideoCapture and shows each frame with cv2.imshow until 'q' is pressed;
    neither exists here, so the frame source and the sink are arguments: `frames` is any iterable of uint8 BGR
    [H,W,3] arrays, `on_frame(img, marks)` receives the annotated frame (marks: uint [K,C,2], K may be 0) and ends
    the loop by returning False -- the 'q' key.  All faces of a frame go through ONE batched launch sequence
    (`detect_marks_batch`) instead of the reference's per-face model calls.  Returns the number of frames processed."""
    from .utils.plots import draw_marks
    if frames is None:
        raise ValueError("video_predict needs `frames` (an iterable of BGR uint8 images): there is no camera capture "
                         "without cv2 (prediction.py:100)")
    count = 0
    for img in frames:
        rects = facedetector_fn(img)
        marks = detect_marks_batch(img, landmark_model, list(rects), n_points=n_points, thresh=thresh)
        for k in range(marks.shape[0]):
            draw_marks(img, marks[k])
        count += 1
        if on_frame is not None and on_frame(img, marks) is False:
            break
    return count


def face_quality(faces, aligned_format=None):
    """The exact quality record of aligned faces and its customary scalars.  faces: K aligned faces as `align` /
    `align_frames` return them under `aligned_format` (None: float32 [K,h,w,3] BGR), a numpy array (one upload, two
    downloads) or a CUDA tensor (nothing leaves the device) -> (rec int64 [K,8] as `alignment.face_quality_device`
    describes it, scalars float64 [K,4]: sharpness, mean luma, luma standard deviation, exposed share), of the kind of
    `faces`."""
    import torch
    numpy_io = not isinstance(faces, torch.Tensor)
    _aligned_format(aligned_format, numpy_io)
    if numpy_io:
        faces = torch.from_numpy(np.ascontiguousarray(faces)).to(_lib.require_gpu())
    rec = alignment.face_quality_device(faces.contiguous(), aligned_format)
    sc = alignment.quality_scalars(rec)
    return (rec.cpu().numpy(), sc.cpu().numpy()) if numpy_io else (rec, sc)


def head_pose(landmarks, weights=None, pose=None):
    """Where every face looks, from its landmarks (alignment.head_pose_device: a scaled-orthographic fit of a rigid 3-D
    face model, one launch).  landmarks: float64 [N,C,2] in any pixel unit, (-1,-1) for a rejected point; weights: None
    or float64 [N,C]; both numpy arrays (one upload, one download) or CUDA tensors (nothing leaves the device; views of a
    landmark record tensor are read in place).  pose: None or an `alignment.HeadPose`; without a model of its own the
    default one is used, which exists for 68 landmarks.  Returns a dict of the kind of `landmarks`, every entry a view
    of "record" float64 [N,18]: "R" [N,3,3] (model frame -> camera frame; the identity for a face that looks straight
    into the camera), "scale" [N] (pixels per model unit), "centre" [N,2] (the weighted mean of the landmarks used),
    "rms" [N] (the fit's residual in pixels), "count" [N], "ok" [N] (1.0 or 0.0) and "angles" [N,3] (yaw, pitch, roll in
    radians, R = Rz(roll) Rx(pitch) Ry(yaw)).  A face whose fit is not ok -- fewer than four usable model points, or
    coplanar ones -- has the identity, scale 0, centre (-1,-1) and angles 0."""
    import torch
    if pose is None:
        pose = alignment.HeadPose()
    elif not isinstance(pose, alignment.HeadPose):
        raise ValueError("pose must be None or an alignment.HeadPose (got %r)" % (pose,))
    numpy_io = not isinstance(landmarks, torch.Tensor)
    if numpy_io:
        lm_np = np.ascontiguousarray(landmarks, np.float64)
        if lm_np.ndim != 3 or lm_np.shape[2] != 2:
            raise ValueError("landmarks must be float64 [N,C,2]")
        if weights is not None:
            weights = np.ascontiguousarray(weights, np.float64)
            if weights.shape != lm_np.shape[:2]:
                raise ValueError("weights must be float64 [%d,%d]" % lm_np.shape[:2])
    elif landmarks.dim() != 3:
        raise ValueError("landmarks must be float64 [N,C,2]")
    model = pose.model_for(int(landmarks.shape[1]))
    if numpy_io:
        dev = _lib.require_gpu()
        landmarks = torch.from_numpy(lm_np).to(dev)
        weights = None if weights is None else torch.from_numpy(weights).to(dev)
    rec = alignment.head_pose_device(landmarks, model, weights=weights, opts=pose)
    if numpy_io:
        rec = rec.cpu().numpy()
    n = int(rec.shape[0])
    return dict(record=rec, R=rec[:, :9].reshape(n, 3, 3), scale=rec[:, 9], centre=rec[:, 10:12], rms=rec[:, 12],
                count=rec[:, 13], ok=rec[:, 14], angles=rec[:, 15:18])


def _parts_for(parts, n_landmarks):
    """parts None or True -> `FaceParts.default` of the landmark count; a FaceParts is used as it is (an index beyond
    the landmark count takes no part in its fit)."""
    if parts is None or parts is True:
        return alignment.FaceParts.default(n_landmarks)
    if not isinstance(parts, alignment.FaceParts):
        raise ValueError("parts must be None, True or an alignment.FaceParts (got %r)" % (parts,))
    return parts


def _openness_for(openness, n_landmarks):
    if openness is None or openness is True:
        return alignment.Openness.default(n_landmarks)
    if not isinstance(openness, alignment.Openness):
        raise ValueError("openness must be None, True or an alignment.Openness (got %r)" % (openness,))
    return openness


def face_parts(ring, landmarks, parts=None, weights=None, frame_index=None, samples=1, aligned_format=None,
               frame_format=None):
    """Eye and mouth patches for landmarks that `align_frames` returned, cut from the ring in one launch
    (alignment.warp_parts_frames_device): every part under a similarity fitted to its own landmarks.

    ring, frame_format, samples, aligned_format: as `align_frames` takes them; landmarks: CUDA float64 [K,C,2] in frame
    pixels; parts: None (`alignment.FaceParts.default(C)`: right eye, left eye, mouth at 32x48, for 68 landmarks) or an
    `alignment.FaceParts`; weights: None or CUDA float64 [K,C]; frame_index: None (every face lies in slot 0), a host
    sequence of K ring slots (one upload) or a CUDA int32 [K] tensor.  Returns CUDA tensors (patches [K,R,ph,pw,3] float32
    or [K,R] faces of the format, M float32 [K,R,2,3] frame px -> patch px, ok int32 [K,R]); a part that is not ok -- fewer
    than two usable points, or coincident ones -- is a zero patch under the identity."""
    import torch
    _aligned_format(aligned_format, False)
    _frame_format(frame_format)
    if not isinstance(landmarks, torch.Tensor) or landmarks.dim() != 3 or not landmarks.is_cuda:
        raise ValueError("landmarks must be a CUDA float64 [K,C,2] tensor")
    k, c = int(landmarks.shape[0]), int(landmarks.shape[1])
    parts = _parts_for(parts, c)
    if frame_index is not None and not isinstance(frame_index, torch.Tensor):
        idx = [int(v) for v in frame_index]
        if len(idx) != k:
            raise ValueError("frame_index must name a ring slot for each of the %d faces" % k)
        frame_index = torch.tensor(idx, dtype=torch.int32).to(landmarks.device)
    aff = torch.empty((k, len(parts), 2, 3), dtype=torch.float32, device=landmarks.device)
    ok = torch.empty((k, len(parts)), dtype=torch.int32, device=landmarks.device)
    out = alignment.warp_parts_frames_device(ring, landmarks, parts, weights=weights, frame_index_dev=frame_index,
                                             samples=samples, fmt=aligned_format, src=frame_format, affines_out=aff,
                                             ok_out=ok)
    return out, aff, ok


def face_openness(landmarks, weights=None, openness=None):
    """How open the eyes and the mouth of every face are (alignment.face_openness_device, one launch).  landmarks:
    float64 [N,C,2] in frame pixels, (-1,-1) for a rejected point; weights: None or float64 [N,C]; both numpy arrays (one
    upload, one download) or CUDA tensors (nothing leaves the device).  openness: None (`alignment.Openness.default(C)`:
    both eyes and the inner mouth, for 68 landmarks) or an `alignment.Openness`.  Returns a dict of the kind of
    `landmarks`, every entry a view of "record" float64 [N,G,4]: "openness" [N,G] (for the eyes the eye aspect ratio; -1
    where the measure is not ok), "width" [N,G] in pixels, "ok" [N,G] (1.0 or 0.0) and "sum" [N,G].  The blink state
    needs a history and lives in `FaceTracker(openness=...)` or `alignment.face_openness_device(state=...)`."""
    import torch
    numpy_io = not isinstance(landmarks, torch.Tensor)
    if numpy_io:
        lm_np = np.ascontiguousarray(landmarks, np.float64)
        if lm_np.ndim != 3 or lm_np.shape[2] != 2:
            raise ValueError("landmarks must be float64 [N,C,2]")
        if weights is not None:
            weights = np.ascontiguousarray(weights, np.float64)
            if weights.shape != lm_np.shape[:2]:
                raise ValueError("weights must be float64 [%d,%d]" % lm_np.shape[:2])
    elif landmarks.dim() != 3:
        raise ValueError("landmarks must be float64 [N,C,2]")
    openness = _openness_for(openness, int(landmarks.shape[1]))
    if numpy_io:
        dev = _lib.require_gpu()
        landmarks = torch.from_numpy(lm_np).to(dev)
        weights = None if weights is None else torch.from_numpy(weights).to(dev)
    rec = alignment.face_openness_device(landmarks, openness, weights=weights)
    if numpy_io:
        rec = rec.cpu().numpy()
    return dict(record=rec, openness=rec[..., 0], width=rec[..., 1], ok=rec[..., 2], sum=rec[..., 3])


def landmark_flow(prev_crops, cur_crops, points, flow=None):
    """Points carried from one crop to the next by sparse optical flow (alignment.flow_pyramid_device and
    alignment.landmark_flow_device: a pyramidal, translation-only Lucas-Kanade step per point, two launches), numpy in and
    numpy out.  prev_crops, cur_crops: uint8 [K,H,W,3] (B,G,R) or [K,H,W] (luma) of one size, H and W multiples of
    2^(flow.levels-1); points: float64 [K,C,2] in crop px of prev_crops, a negative or non-finite point is left out;
    flow: None or an `alignment.LandmarkFlow`.  Returns (points float64 [K,C,2] in cur_crops, (-1,-1) for a rejected
    point; err int32 [K,C], the window's sum of absolute differences in 1/1024 grey levels, -1 where it was not reached;
    flags int32 [K,C], 0 or the alignment.FLOW_* bits that rejected the point)."""
    import torch
    if flow is None:
        flow = alignment.LandmarkFlow()
    elif not isinstance(flow, alignment.LandmarkFlow):
        raise ValueError("flow must be None or an alignment.LandmarkFlow (got %r)" % (flow,))
    prev_crops, cur_crops = np.ascontiguousarray(prev_crops), np.ascontiguousarray(cur_crops)
    if (prev_crops.dtype != np.uint8 or prev_crops.shape != cur_crops.shape or cur_crops.dtype != np.uint8
            or prev_crops.ndim not in (3, 4) or (prev_crops.ndim == 4 and prev_crops.shape[3] != 3)):
        raise ValueError("prev_crops and cur_crops must be uint8 [K,H,W,3] or [K,H,W] arrays of one shape")
    points = np.ascontiguousarray(points, np.float64)
    k, h, w = prev_crops.shape[:3]
    if points.ndim != 3 or points.shape[0] != k or points.shape[2] != 2:
        raise ValueError("points must be float64 [%d,C,2]" % k)
    flow.check_crop(h, w)
    dev = _lib.require_gpu()
    both = torch.from_numpy(np.concatenate([prev_crops, cur_crops])).to(dev)
    pyr = alignment.flow_pyramid_device(both, flow.levels)
    m = torch.eye(2, 3, dtype=torch.float32, device=dev).repeat(k, 1, 1).contiguous()
    lm, _, err, flags = alignment.landmark_flow_device(pyr[:k], pyr[k:], torch.from_numpy(points).to(dev), m, (h, w), flow)
    return lm.cpu().numpy(), err.cpu().numpy(), flags.cpu().numpy()


# ---- tracking: faces followed across frames from their own landmarks ---------------------------------------------------
class FaceTracker:
    """Faces followed across the frames of a stream on the device: the landmarks of frame t place the crop of frame t+1.

    The detector seeds a track and re-seeds one that was lost; between those the per-frame step makes no host transfer
    and no synchronisation.  The tracker owns the device state of `capacity` slots: the crop matrix of every slot (frame
    px -> network-input px), its box (the frame region the crop covers; empty = no face), the ring slot its frame lies
    in, and its status (0 or `_lib.TRACK_*` bits); it is allocated by the first seed, step or lost.

    model: a landmark model of this package; frame_hw: (H, W) of the frames; out_size, template, samples,
    aligned_format, frame_format, n_points, thresh, fallback_faces: as `align_frames` takes them (every forward the
    tracker runs gets the budget; empty slots are zero crops, the faces most likely to need it); weights: None or "score" (the forward
    runs in its "landmark_stats" mode and both fits read the record tensor in place); crop_template float64 [C,2] in
    network-input px: where the landmarks sit in the next crop -- upright, centred, at a fixed scale (default
    `alignment.canonical_template(C, in_h, in_w)`); crop_samples: 1, 2 or 4 samples per axis and crop pixel, for faces
    much larger than the network input; min_points, min_score, min_side, max_side: when a track is given up
    (flm_track_opts; the defaults leave that to the geometric tests); smooth: None, True (the defaults) or an
    `alignment.LandmarkFilter`: every landmark passes through a One-Euro filter inside the step's own launch, and the
    returned landmarks, the aligned fit and the next crop are those of the smoothed points.  The tracker then also owns
    `filter_state` float64 [capacity,C,6]; a seed clears the history of its slots.  associate: None (the defaults) or an
    `alignment.TrackAssociation`: how `update` pairs the boxes of a detector with the live tracks; the tracker owns
    `misses` int32 [capacity], the updates in a row that found no detection for a slot.  best_shot: None, True (the
    defaults) or an `alignment.BestShot`: after the aligned warp every step scores the aligned faces on the device
    (flm_face_quality, flm_track_best_update; with weights="score" the landmark scores take part) and keeps, per slot,
    the best one of its track: the tracker then owns `gallery` [capacity,...] in the aligned format, `best_q` float64
    [capacity] (-1: none yet), `best_frame` int64, `best_M` float32 [capacity,2,3], `best_landmarks` float64
    [capacity,C,2] and `best_rec` int64 [capacity,8]; `best()` hands them out.  A seed, and a birth in `update`, make
    the slot forget its best with the next step; a track that ends keeps its best readable until then.  streams: how
    many streams (cameras) share the tracker, an integer in [1, capacity] that divides capacity: slot t belongs to
    stream t // slots_per_stream, `step` takes one ring slot per stream and `update` one list of detections per stream
    (alignment.track_associate_streams_device: no pair of two streams is ever evaluated); every tensor the tracker
    owns or returns stays flat over the `capacity` global slots.  With streams=1 every method is the single-stream
    code, launch for launch.  `step_active` steps only the streams that delivered a frame, each on its own `dt`, and
    leaves every other stream's state untouched; `step_live` steps only the slots that hold a face, at most a `budget`
    of them, and leaves every other slot untouched (the tracker then also owns `live_counts`, `live_cursor` and, with
    `smooth`, `slot_age`).  pose: None, True (the defaults) or an `alignment.HeadPose`: after the step call every step
    fits the head pose of its faces (alignment.head_pose_device, one more launch) to the landmarks the step returns --
    the smoothed ones with `smooth` -- weighted by the scores with weights="score"; the tracker then owns `pose` float64
    [capacity,18], one record per slot ({R row by row, s, mx, my, rms, count, ok, yaw, pitch, roll}; the not-ok record
    of an empty face until a step writes it).  `step` writes every slot, `step_active` and `step_live` the slots they
    serve; every other slot keeps its bits.  With `best_shot` as well, the frontality of the pose (R[2][2], or 0 below
    the `min_frontal` of the HeadPose, or for a fit that is not ok) multiplies the quality of the face.  The pose of a
    kept best shot is not stored: it is `head_pose(best_landmarks)`.  A model with other than 68 landmarks needs a
    HeadPose with a model of its own.  exits: None, a ring size Q or an `alignment.TrackExits`, for a tracker with
    `best_shot`: the tracker then says who a slot is and that a track is over (alignment.track_retire_device, two more
    launches first thing in `step`, `step_active` and `step_live`, over all slots whichever of them the tick serves).  It
    owns `track_id` int64 [capacity] (-1: the slot holds no track; ids count up from 0 in the order the tracks began, by
    ascending slot within a tick), `born_frame` int64 [capacity], `exit_row` int32 [capacity] (what the last retire did
    with the slot: -1 nothing, -2 discarded, -3 overrun, else the ring row) and the exit ring of Q rows, one per finished
    track and each delivered once: `exit_faces` in the aligned format, `exit_meta` int64 [Q,8] (track_id, slot,
    born_frame, the frame_id of the tick that saw the end, best_frame, end, seq, 0; end = the status that lost the track,
    -1 for a slot restarted before its end was seen, -2 for a flush), `exit_q`, `exit_M`, `exit_landmarks`, `exit_rec`,
    and `exit_head` int64 [4] = (exits queued so far, ids given so far, tracks discarded for having no best shot of at
    least min_q, exits overrun within one tick).  `exits()` hands them out, `alignment.exit_rows` turns a downloaded
    `exit_head[0]` and the consumer's own cursor into the ring rows to read, and `retire(flush=True)` ends every held
    track at the end of a video.  A track ends when its slot is found empty, or restarted, at the start of the next tick.
    A reborn slot's `best()` row is the previous track's until that slot's first step (true without `exits` too); with
    `exits` the previous track has been queued by then, and a track that ends before its slot was ever stepped has no
    best shot of its own and is discarded (the retire call reads a best_q of -1 for such a slot).  Without `exits` the tracker makes no additional launch and no additional
    allocation.  views: None, True (the defaults: right, frontal and left at a yaw of 20 degrees) or an
    `alignment.PoseViews`, for a tracker with both `best_shot` and `pose`: beside the one best shot the tracker keeps the
    best face of every POSE BIN of a track (alignment.track_views_update_device, two more launches per step, after the
    best update and with its pending resets; the quality of a view is the best shot's without the frontality factor, so a
    sharp profile wins its own bin).  It then owns, over the B = views.bins bins of every slot, `view_gallery`
    [capacity,B,...] in the aligned format, `view_q` float64 [capacity,B] (-1: the bin holds nothing), `view_frame` int64
    [capacity,B], `view_M` float32 [capacity,B,2,3], `view_landmarks` float64 [capacity,B,C,2] and `view_pose` float64
    [capacity,B,18]; `views()` hands them out.  A reborn slot's first served step starts from empty bins.  With `exits`
    every retire call is followed by alignment.track_exit_views_device (one more launch), which moves the views of the
    tracks that call queued into `exit_view_gallery` [Q,B,...], `exit_view_q`, `exit_view_frame`, `exit_view_M`,
    `exit_view_landmarks` and `exit_view_pose`, row for row beside the exit ring; `exit_views()` hands them out, and a
    consumer enrols the bins of a row whose `exit_view_q` is >= 0.  A tracker made without `views` launches nothing more,
    allocates nothing more and returns the same bits.  mesh: None, True (`alignment.FaceMesh.default` of the landmark
    count and out_size, for the default template) or an `alignment.FaceMesh` whose landmark points are `template`: after
    the aligned warp of `step`, `step_active` and `step_live` there is one more launch
    (alignment.warp_mesh_frames_device, from the landmarks and the M that call returns, with `samples`), and
    `mesh_faces` then holds the SHAPE-NORMALISED faces -- every landmark's texture on its template pixel -- row for row
    with the aligned faces that call returned, in `aligned_format`: a view of a [capacity,...] buffer the tracker owns,
    overwritten by the next step, with no download and no synchronisation.  A landmark the decode rejected is (-1,-1)
    and drags its triangles there; a slot without a face gives a zero face, as in `aligned`.  Without `mesh` the tracker
    makes the launches it makes without it and returns the same bits.  flow: None, True (the defaults) or an
    `alignment.LandmarkFlow` whose pyramid fits the network input: `step_flow` then serves a tick WITHOUT the forward, by
    carrying the landmarks of the last step into the new frame with sparse optical flow; see `step_flow`.  The tracker
    then keeps, by device copies alone, the last step's raw landmarks in frame px (before the filter), with
    weights="score" their weights, and the ring slots that step cut from, and owns the two crop sets, their pyramids and
    `flow_flags` and `flow_err` int32 [capacity,C].  Without `flow` the tracker allocates nothing more and `step` returns
    the same bits.  `step_flow_live` is the flow tick of the slots that hold a face and have a usable history, for a loop
    of `update` + `step_live` on the detector's ticks and `step_flow_live` on the others.  For it a flow tracker also owns
    `flow_frame` int32 [capacity], the ring slot every slot's history was found in, and `flow_ready` int32 [capacity]: 1
    exactly when the slot was served with status 0 by the last tick of its stream -- `step`, `step_flow`, `step_active`,
    `step_live` or `step_flow_live` -- and neither `seed` nor `update` has written its crop matrix since (include/flm.h
    states the rule; every one of those calls keeps it by device work alone: a clear for the streams it steps, then one
    launch, alignment.track_flow_history_device, for the rows it served), plus `flow_cursor`, `flow_counts` int32 [6]
    and `flow_fb` float64 [capacity,C], the squared round trip of the forward-backward check that
    `alignment.LandmarkFlow(max_fb=...)` switches on (off by default; -1.0 where it did not run).  After a rows tick
    `flow_flags`, `flow_err` and `flow_fb` are views of the first `budget` rows.  parts: None, True
    (`alignment.FaceParts.default` of the landmark count: right eye, left eye, mouth) or an `alignment.FaceParts`: after
    the aligned warp every step cuts the parts' patches from the ring in one more launch
    (alignment.warp_parts_frames_device, from the landmarks the step returns, with `samples`, `aligned_format` and
    weights="score"'s weights); `part_faces` [rows,R,...], `part_M` float32 [rows,R,2,3] and `part_ok` int32 [rows,R]
    are then views of the tracker's own buffers, row for row beside `aligned`.  openness: None, True
    (`alignment.Openness.default` of the landmark count: both eyes and the inner mouth) or an `alignment.Openness`:
    after the head pose every step measures the openness of its faces and advances their blink state in one more launch
    (alignment.face_openness_device) at the rows' slots; the tracker then owns `openness` float64 [capacity,G,4] and
    `open_state` float64 [capacity,G,8], and a slot no step serves keeps both and its pending reset.  The state of a slot
    is emptied when a track is born there (`seed`, a birth of `update`).  The time step is the step's own `dt` for a
    tracker that smooths -- the rows' dt, waits included, on the rows ticks -- and the Openness's `dt` otherwise;
    `frame_id` is also taken by a tracker with openness alone.  With `smooth` the openness reads the FILTERED landmarks:
    the One-Euro filter lags a blink, and nothing has been measured about that.  Without the two options the tracker
    launches nothing more and allocates nothing more."""

    def __init__(self, model, frame_hw, capacity, out_size=(112, 112), template=None, crop_template=None, n_points=4,
                 thresh=0.0, weights=None, min_points=2, min_score=0.0, min_side=0.0, max_side=float("inf"),
                 crop_samples=1, samples=1, aligned_format=None, frame_format=None, smooth=None, associate=None,
                 best_shot=None, streams=1, pose=None, mesh=None, flow=None, fallback_faces=0, parts=None, openness=None,
                 exits=None, views=None):
        import torch
        if parts is False:
            parts = None
        if parts is not None:
            parts = _parts_for(parts, int(model.n_classes))
        if openness is False:
            openness = None
        if openness is not None:
            openness = _openness_for(openness, int(model.n_classes))
        if isinstance(fallback_faces, bool) or not isinstance(fallback_faces, (int, np.integer)) or fallback_faces < 0:
            raise ValueError("fallback_faces must be an integer >= 0 (got %r)" % (fallback_faces,))
        self.fallback_faces = int(fallback_faces)
        if flow is True:
            flow = alignment.LandmarkFlow()
        elif flow is False:
            flow = None
        if flow is not None and not isinstance(flow, alignment.LandmarkFlow):
            raise ValueError("flow must be None, True or an alignment.LandmarkFlow (got %r)" % (flow,))
        if mesh is not None and mesh is not False and mesh is not True and not isinstance(mesh, alignment.FaceMesh):
            raise ValueError("mesh must be None, True or an alignment.FaceMesh (got %r)" % (mesh,))
        if views is True:
            views = alignment.PoseViews()
        if views is not None and not isinstance(views, alignment.PoseViews):
            raise ValueError("views must be None, True or an alignment.PoseViews (got %r)" % (views,))
        if views is not None and (best_shot is None or best_shot is False or pose is None or pose is False):
            raise ValueError("views needs both best_shot and pose: a view is the best face of a pose bin")
        if exits is not None and not isinstance(exits, alignment.TrackExits):
            if isinstance(exits, bool) or not isinstance(exits, (int, np.integer)):
                raise ValueError("exits must be None, a ring size or an alignment.TrackExits (got %r)" % (exits,))
            exits = alignment.TrackExits(capacity=int(exits))
        if exits is not None and (best_shot is None or best_shot is False):
            raise ValueError("exits needs best_shot: the exit queue holds the best shot of every finished track")
        if pose is True:
            pose = alignment.HeadPose()
        if pose is not None and not isinstance(pose, alignment.HeadPose):
            raise ValueError("pose must be None, True or an alignment.HeadPose (got %r)" % (pose,))
        if best_shot is True:
            best_shot = alignment.BestShot()
        if best_shot is not None and not isinstance(best_shot, alignment.BestShot):
            raise ValueError("best_shot must be None, True or an alignment.BestShot (got %r)" % (best_shot,))
        if associate is None:
            associate = alignment.TrackAssociation()
        elif not isinstance(associate, alignment.TrackAssociation):
            raise ValueError("associate must be None or an alignment.TrackAssociation (got %r)" % (associate,))
        if weights is not None and weights != "score":
            raise ValueError("weights must be None or \"score\" (got %r)" % (weights,))
        if smooth is True:
            smooth = alignment.LandmarkFilter()
        if smooth is not None and not isinstance(smooth, alignment.LandmarkFilter):
            raise ValueError("smooth must be None, True or an alignment.LandmarkFilter (got %r)" % (smooth,))
        _aligned_format(aligned_format, False)
        _frame_format(frame_format)
        fh, fw = [int(v) for v in frame_hw]
        if fw < 2 or fh < 1 or fh * fw * 3 >= 2 ** 31:
            raise ValueError("frames of %dx%d are outside the warp's reach (width >= 2, H*W*3 < 2^31)" % (fh, fw))
        capacity = int(capacity)
        if not 1 <= capacity <= 65535:
            raise ValueError("capacity must be in [1, 65535] (got %d)" % capacity)
        if isinstance(streams, bool) or int(streams) != streams or not 1 <= int(streams) <= capacity or capacity % int(streams):
            raise ValueError("streams must be an integer in [1, capacity] that divides capacity (got %r, capacity %d)"
                             % (streams, capacity))
        oh, ow = [int(v) for v in out_size]
        if oh < 1 or ow < 1:
            raise ValueError("out_size must be positive")
        if samples not in (1, 2, 4) or crop_samples not in (1, 2, 4):
            raise ValueError("samples and crop_samples must be 1, 2 or 4")
        if int(min_points) < 2:
            raise ValueError("min_points must be 2 or more")
        if any(v != v for v in (float(min_score), float(min_side), float(max_side))):
            raise ValueError("min_score, min_side and max_side must not be NaN")
        c = int(model.n_classes)
        ih, iw = int(model.input_height), int(model.input_width)
        if flow is not None:
            flow.check_crop(ih, iw)
        self.flow, self._flow_ok = flow, False   # _flow_ok: the last call was `step` or `step_flow` (step_flow)
        tm = alignment.canonical_template(c, oh, ow) if template is None else template
        tc = alignment.canonical_template(c, ih, iw) if crop_template is None else crop_template
        tm, tc = [t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t) for t in (tm, tc)]
        if tm.shape != (c, 2) or tc.shape != (c, 2):
            raise ValueError("template and crop_template must be [%d,2]" % c)
        self.model, self.capacity, self.frame_hw, self.out_size = model, capacity, (fh, fw), (oh, ow)
        self.n_points, self.thresh, self.weights = n_points, thresh, weights
        self.limits = dict(min_points=int(min_points), min_score=float(min_score), min_side=float(min_side),
                           max_side=float(max_side))
        self.crop_samples, self.samples = crop_samples, samples
        self.aligned_format, self.frame_format = aligned_format, frame_format
        self.smooth, self.filter_state = smooth, None
        self.associate = associate
        self.streams, self.slots_per_stream = int(streams), capacity // int(streams)
        self.best_shot, self.gallery, self._steps = best_shot, None, 0
        self.head_pose, self.pose = pose, None
        self.exit_opts, self.track_id = exits, None
        self.view_opts, self.view_q = views, None
        if mesh is True:
            if template is not None:
                raise ValueError("mesh=True is the mesh of the default template: pass an alignment.FaceMesh whose "
                                 "landmark points are `template`")
            mesh = alignment.FaceMesh.default(c, oh, ow)
        elif mesh is False:
            mesh = None
        if mesh is not None and mesh.n_landmarks != c:
            raise ValueError("the mesh has %d landmark points, the model %d landmarks" % (mesh.n_landmarks, c))
        self.mesh, self.mesh_faces, self._mesh_buf = mesh, None, None
        self._head_model = None if pose is None else pose.model_for(c)
        self.parts, self.part_faces, self.part_ok, self.part_M = parts, None, None, None
        self.open_opts, self.openness, self.open_state = openness, None, None
        self._ws_active = None   # the forward workspace of step_active (_active_workspace)
        self._waiting = False    # step_live has run below capacity: slot_age may hold a wait (_served)
        self._crop_format = alignment.AlignedFormat("nhwc", "uint8")
        self._templates = (np.ascontiguousarray(tm, np.float64), np.ascontiguousarray(tc, np.float64))
        self.m_crop = None    # the device state, allocated by the first call that needs it (_state)

    def _state(self):
        """The device state: every slot starts dead -- an empty box, the identity, TRACK_DEAD."""
        import torch
        if self.m_crop is not None:
            return
        dev = _lib.require_gpu()
        n = self.capacity
        self.template, self.crop_template = [torch.from_numpy(t).to(dev) for t in self._templates]
        self.boxes = torch.zeros((n, 4), dtype=torch.int32, device=dev)
        self._boxes_spare = torch.zeros_like(self.boxes)
        self.frame_slots = torch.zeros((n,), dtype=torch.int32, device=dev)
        self.status = torch.full((n,), _lib.TRACK_DEAD, dtype=torch.int32, device=dev)
        self.m_crop = torch.eye(2, 3, dtype=torch.float32, device=dev).repeat(n, 1, 1).contiguous()
        self.misses = torch.zeros((n,), dtype=torch.int32, device=dev)
        if self.smooth is not None:     # -1: no landmark has a history
            self.filter_state = torch.full((n, int(self.model.n_classes), 6), -1.0, dtype=torch.float64, device=dev)
            self.slot_age = torch.zeros((n,), dtype=torch.float64, device=dev)   # step_live: seconds waited unserved
        self.live_cursor = torch.zeros((1,), dtype=torch.int32, device=dev)      # step_live: where its order starts
        self.live_counts = torch.zeros((4,), dtype=torch.int32, device=dev)      # step_live: what its last gather counted
        if self.best_shot is not None:  # -1: the slot holds no best
            fmt = self.aligned_format or alignment.AlignedFormat()
            c = int(self.model.n_classes)
            self.gallery = torch.zeros(fmt.shape(n, *self.out_size), dtype=fmt.torch_dtype, device=dev)
            self.best_q = torch.full((n,), -1.0, dtype=torch.float64, device=dev)
            self._best_q_spare = torch.full_like(self.best_q, -1.0)
            self.best_frame = torch.full((n,), -1, dtype=torch.int64, device=dev)
            self.best_M = torch.zeros((n, 2, 3), dtype=torch.float32, device=dev)
            self.best_landmarks = torch.full((n, c, 2), -1.0, dtype=torch.float64, device=dev)
            self.best_rec = torch.zeros((n, alignment.QUALITY_REC), dtype=torch.int64, device=dev)
            self._quality_rec = torch.zeros_like(self.best_rec)
            self._best_reset = torch.zeros((n,), dtype=torch.int32, device=dev)
        if self.exit_opts is not None:  # -1: the slot holds no track; the ring starts empty
            q = self.exit_opts.capacity
            self.track_id = torch.full((n,), -1, dtype=torch.int64, device=dev)
            self.born_frame = torch.full((n,), -1, dtype=torch.int64, device=dev)
            self._born = torch.zeros((n,), dtype=torch.int32, device=dev)
            self.exit_row = torch.full((n,), -1, dtype=torch.int32, device=dev)
            self.exit_head = torch.zeros((4,), dtype=torch.int64, device=dev)
            self.exit_faces = torch.zeros(fmt.shape(q, *self.out_size), dtype=fmt.torch_dtype, device=dev)
            self.exit_meta = torch.zeros((q, alignment.EXIT_META), dtype=torch.int64, device=dev)
            self.exit_q = torch.full((q,), -1.0, dtype=torch.float64, device=dev)
            self.exit_M = torch.zeros((q, 2, 3), dtype=torch.float32, device=dev)
            self.exit_landmarks = torch.full((q, c, 2), -1.0, dtype=torch.float64, device=dev)
            self.exit_rec = torch.zeros((q, alignment.QUALITY_REC), dtype=torch.int64, device=dev)
            self._exit_stale = torch.zeros((n,), dtype=torch.bool, device=dev)   # best_q is an earlier track's (_retire)
            self._exit_q_in = torch.full((n,), -1.0, dtype=torch.float64, device=dev)
            self._no_best = torch.full((), -1.0, dtype=torch.float64, device=dev)
        if self.head_pose is not None:  # the not-ok record of a face without landmarks
            empty = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, -1.0, -1.0] + [0.0] * 6
            self.pose = torch.tensor(empty, dtype=torch.float64, device=dev).repeat(n, 1).contiguous()
            self._pose_factor = torch.zeros((n,), dtype=torch.float64, device=dev) if self.best_shot is not None else None
        if self.mesh is not None:       # the faces of the last step, and the mesh's tensors and map made once, here
            mfmt = self.aligned_format or alignment.AlignedFormat()
            self._mesh_buf = torch.zeros(mfmt.shape(n, *self.out_size), dtype=mfmt.torch_dtype, device=dev)
            self.mesh.tensors(dev)
            self.mesh.map(dev, *self.out_size)
        if self.parts is not None:      # the patches, matrices and ok flags of the last step: the rows of `aligned`
            pfmt = self.aligned_format or alignment.AlignedFormat()
            r = len(self.parts)
            self._part_buf = torch.zeros((n, r) + tuple(pfmt.shape(1, *self.parts.size)[1:]), dtype=pfmt.torch_dtype,
                                         device=dev)
            self._part_m_buf = torch.eye(2, 3, dtype=torch.float32, device=dev).repeat(n, r, 1, 1).contiguous()
            self._part_ok_buf = torch.zeros((n, r), dtype=torch.int32, device=dev)
            self.parts.tensors(dev)
        if self.open_opts is not None:  # the not-ok record and the empty state of a slot no step has measured
            g = len(self.open_opts)
            self.openness = torch.tensor([-1.0, -1.0, 0.0, -1.0], dtype=torch.float64, device=dev).repeat(n, g, 1).contiguous()
            self.open_state = torch.tensor(alignment.OPEN_STATE_EMPTY, dtype=torch.float64,
                                           device=dev).repeat(n, g, 1).contiguous()
            self._open_reset = torch.zeros((n,), dtype=torch.int32, device=dev)
        if self.flow is not None:       # (-1,-1): the landmark has no history
            c = int(self.model.n_classes)
            ih, iw = int(self.model.input_height), int(self.model.input_width)
            self._flow_lm = torch.full((n, c, 2), -1.0, dtype=torch.float64, device=dev)   # the last step's RAW landmarks
            self._flow_w = torch.zeros((n, c), dtype=torch.float64, device=dev) if self.weights is not None else None
            self._flow_slots = torch.zeros((n,), dtype=torch.int32, device=dev)            # the ring slots of that step
            self._flow_crops = torch.zeros((2 * n, ih, iw, 3), dtype=torch.uint8, device=dev)   # previous | current
            self._flow_pyr = torch.zeros((2 * n, self.flow.pyramid_bytes(ih, iw)), dtype=torch.uint8, device=dev)
            self._flow_crop_lm = torch.full((n, c, 2), -1.0, dtype=torch.float64, device=dev)
            self._flow_crop_w = torch.zeros((n, c), dtype=torch.float64, device=dev)
            self.flow_err = torch.full((n, c), -1, dtype=torch.int32, device=dev)
            self.flow_flags = torch.zeros((n, c), dtype=torch.int32, device=dev)
            self.flow_fb = torch.full((n, c), -1.0, dtype=torch.float64, device=dev)
            self._flow_out = (self.flow_err, self.flow_flags, self.flow_fb)   # the buffers; the three names are views of them
            # the per-slot history rule (include/flm.h, "the flow tick on rows"): flow_ready[g] == 1 exactly when slot g was
            # served with status 0 by the last tick of its stream and nothing has written its crop matrix since
            self.flow_frame = torch.zeros((n,), dtype=torch.int32, device=dev)    # the ring slot the history was found in
            self.flow_ready = torch.zeros((n,), dtype=torch.int32, device=dev)
            self.flow_cursor = torch.zeros((1,), dtype=torch.int32, device=dev)   # step_flow_live: where its order starts
            self.flow_counts = torch.zeros((6,), dtype=torch.int32, device=dev)   # step_flow_live: what its gather counted
            self._flow_iota = torch.arange(n, dtype=torch.int32, device=dev)      # slot[r] = r: the all-slots ticks
            self._flow_m_before = torch.zeros((n, 2, 3), dtype=torch.float32, device=dev)   # update: m_crop before it
            self._flow_raw_rows = (torch.full((n, c, 2), -1.0, dtype=torch.float64, device=dev)
                                   if self.smooth is not None else None)          # the raw landmarks of a rows tick
            self._flow_rows = None                                                # (raw landmarks, weights, status) of it
        if self.view_opts is not None:  # -1: the bin holds nothing
            b = self.view_opts.bins
            face = tuple(self.gallery.shape[1:])

            def ring(rows):
                return dict(gallery=torch.zeros(fmt.shape(rows * b, *self.out_size), dtype=fmt.torch_dtype,
                                                device=dev).view((rows, b) + face),
                            q=torch.full((rows, b), -1.0, dtype=torch.float64, device=dev),
                            frame=torch.full((rows, b), -1, dtype=torch.int64, device=dev),
                            M=torch.zeros((rows, b, 2, 3), dtype=torch.float32, device=dev),
                            landmarks=torch.full((rows, b, c, 2), -1.0, dtype=torch.float64, device=dev),
                            pose=self.pose[:1].repeat(rows * b, 1).view(rows, b, alignment.POSE_REC).contiguous())
            for name, t in ring(n).items():
                setattr(self, "view_" + name, t)
            self._view_take = torch.full((n,), -1, dtype=torch.int32, device=dev)
            if self.exit_opts is not None:
                for name, t in ring(self.exit_opts.capacity).items():
                    setattr(self, "exit_view_" + name, t)

    def seed(self, slots, boxes, stream=None):
        """Start (or restart) the tracks `slots` from the detector boxes `boxes` (x0,y0,x1,y1), one per slot: the host
        box maths of `face_boxes`, one upload, flm_track_seed, and the results placed in those slots on the device.
        `slots` are global slots, or, with `stream` given, slots of that stream counted from its first one."""
        import torch
        slots = [int(v) for v in slots]
        boxes = [list(b) for b in boxes]
        if stream is not None:
            if isinstance(stream, bool) or int(stream) != stream or not 0 <= int(stream) < self.streams:
                raise ValueError("stream must be in [0, %d) (got %r)" % (self.streams, stream))
            if any(not 0 <= v < self.slots_per_stream for v in slots):
                raise ValueError("the slots of a stream must be in [0, %d)" % self.slots_per_stream)
            slots = [int(stream) * self.slots_per_stream + v for v in slots]
        if len(slots) != len(boxes) or any(len(b) != 4 for b in boxes):
            raise ValueError("seed takes one (x0,y0,x1,y1) box per slot")
        if any(not 0 <= v < self.capacity for v in slots) or len(set(slots)) != len(slots):
            raise ValueError("slots must be distinct and in [0, %d)" % self.capacity)
        n = len(slots)
        if not n:
            return
        self._flow_ok = False
        self._state()
        sq = np.asarray(face_boxes(boxes), np.int32).reshape(n, 4)
        both = torch.from_numpy(np.concatenate([sq.reshape(-1), np.asarray(slots, np.int32)])).to(self.boxes.device)
        bdev, idx = both[:4 * n].view(n, 4), both[4 * n:].to(torch.int64)
        m, st = alignment.track_seed_device(bdev, (self.model.input_height, self.model.input_width), self.frame_hw)
        self.m_crop.index_copy_(0, idx, m)
        self.boxes.index_copy_(0, idx, bdev)
        self.status.index_copy_(0, idx, st)
        self.misses.index_fill_(0, idx, 0)
        if self.filter_state is not None:
            self.filter_state.index_fill_(0, idx, -1.0)
        if self.best_shot is not None:
            self._best_reset.index_fill_(0, idx, 1)
        if self.open_opts is not None:
            self._open_reset.index_fill_(0, idx, 1)
        if self.exit_opts is not None:
            self._born.index_fill_(0, idx, 1)
        if self.flow is not None:
            self.flow_ready.index_fill_(0, idx, 0)

    @staticmethod
    def _host_boxes(boxes, what):
        """Detector boxes from the host as an integer [D,4] array whose values fit int32; ValueError(what) otherwise."""
        arr = np.asarray(boxes)
        if arr.ndim != 2 or arr.shape[1] != 4 or arr.dtype.kind not in "iu":
            raise ValueError(what)
        if arr.size and (arr.min() < -2 ** 31 or arr.max() >= 2 ** 31):
            raise ValueError("a box coordinate does not fit int32")
        return arr

    def _was_empty(self):
        """For a tracker with best_shot or openness, the slots that hold no track now: the association's own test, on the
        device."""
        if self.best_shot is None and self.open_opts is None:
            return None
        fh, fw = self.frame_hw
        b = self.boxes
        return ((b[:, 2].clamp(0, fw) - b[:, 0].clamp(0, fw) <= 0)
                | (b[:, 3].clamp(0, fh) - b[:, 1].clamp(0, fh) <= 0))

    def _mark_births(self, was_empty, slot_det):
        """A birth forgets the slot's best with the next step; a restart is the same face and keeps it, and a skipped
        stream has slot_det == -1 and resets nothing.  The openness state is forgotten by the same rule, through a flag
        of its own that the openness call clears."""
        if self.best_shot is not None:
            births = was_empty & (slot_det >= 0)
            self._best_reset.masked_fill_(births, 1)
            if self.exit_opts is not None:
                self._born.masked_fill_(births, 1)
        if self.open_opts is not None:
            self._open_reset.masked_fill_(was_empty & (slot_det >= 0), 1)

    def update(self, detections, n=None):
        """The boxes of a detector against the tracks, on the device (alignment.track_associate_device with the
        tracker's `associate`): a detection that overlaps a live track confirms it (and restarts it where the two have
        drifted apart, if `refresh_iou` says so); of two tracks on one face the higher slot ends with TRACK_DUPLICATE; a
        track no detection has confirmed in `max_misses` updates ends with TRACK_UNCONFIRMED; every other detection
        starts a track in the lowest slot that holds none.  `detections`: a CUDA int32 [D,4] tensor (x0,y0,x1,y1) --
        nothing is transferred; `n`, a CUDA int32 tensor of one element, then says how many of its rows are valid -- or
        a host list or array of integer boxes: one upload.  Returns CUDA tensors (det_slot int32 [D], slot_det int32
        [capacity], counts int32 [8]) as `track_associate_device` describes them.  No download, no synchronisation.
        May be called between any two steps: it edits the matrices and boxes the NEXT step cuts its crops with, not the
        ones the last aligned warp used.
        A tracker of several streams takes a CUDA int32 [streams,D,4] tensor -- `n` is then None or CUDA int32
        [streams], a negative count skipping the stream (its detector did not run: its tracks are neither confirmed nor
        charged a miss) -- or a host sequence of one entry per stream, a list of integer boxes (empty: the detector ran
        and found nothing) or None (skipped): one upload of boxes and counts.  Returns (det_slot int32 [streams,D] in
        global slots, slot_det int32 [capacity], counts int32 [streams,8]) as `track_associate_streams_device`
        describes them."""
        import torch
        if self.streams > 1:
            return self._update_streams(detections, n)
        if self.capacity > alignment.ASSOC_MAX:
            raise ValueError("update takes a tracker of at most %d slots (capacity %d)" % (alignment.ASSOC_MAX, self.capacity))
        if isinstance(detections, torch.Tensor):
            det = detections
        else:
            det = self._host_boxes(detections, "update takes a CUDA int32 [D,4] tensor or a list of integer (x0,y0,x1,y1) "
                                               "boxes").astype(np.int32)
        if int(det.shape[0]) > alignment.ASSOC_MAX:
            raise ValueError("update takes at most %d detections (got %d)" % (alignment.ASSOC_MAX, int(det.shape[0])))
        if int(det.shape[0]) < 1:
            raise ValueError("update takes at least one row of detections (n says how many are valid)")
        if n is not None and not isinstance(n, torch.Tensor):
            raise ValueError("n must be None or a CUDA int32 tensor of one element")
        self._flow_ok = False
        self._state()
        if not isinstance(det, torch.Tensor):
            det = torch.from_numpy(np.ascontiguousarray(det)).to(self.boxes.device)
        was_empty = self._was_empty()
        self._flow_before_update()
        out = alignment.track_associate_device(det, self.m_crop, self.boxes, self.status, self.misses,
                                               (self.model.input_height, self.model.input_width), self.frame_hw,
                                               n_det=n, state=self.filter_state, assoc=self.associate)
        self._mark_births(was_empty, out[1])
        self._flow_after_update()
        return out

    def _update_streams(self, detections, n):
        import torch
        s, k = self.streams, self.slots_per_stream
        if k > alignment.ASSOC_MAX:
            raise ValueError("update takes at most %d slots per stream (this tracker has %d)" % (alignment.ASSOC_MAX, k))
        if isinstance(detections, torch.Tensor):
            det = detections
            if det.dim() != 3 or int(det.shape[0]) != s or int(det.shape[2]) != 4 or det.dtype != torch.int32:
                raise ValueError("update takes a CUDA int32 [%d,D,4] tensor or one list of integer boxes per stream" % s)
            if n is not None and not isinstance(n, torch.Tensor):
                raise ValueError("n must be None or a CUDA int32 [%d] tensor" % s)
            d = int(det.shape[1])
        else:
            if n is not None:
                raise ValueError("n goes with detections on the device; a host entry of None skips its stream")
            rows = list(detections)
            if len(rows) != s:
                raise ValueError("update takes one entry per stream (%d), got %d" % (s, len(rows)))
            arrs = [None if r is None else
                    self._host_boxes(r if np.size(r) else np.zeros((0, 4), np.int64),
                                     "every stream's entry is None or a list of integer (x0,y0,x1,y1) boxes") for r in rows]
            d = max([1] + [len(a) for a in arrs if a is not None])
        if d > alignment.ASSOC_MAX:
            raise ValueError("update takes at most %d detections per stream (got %d)" % (alignment.ASSOC_MAX, d))
        if d < 1:
            raise ValueError("update takes at least one row of detections per stream (n says how many are valid)")
        self._flow_ok = False
        self._state()
        if not isinstance(detections, torch.Tensor):
            flat = np.zeros(s * d * 4 + s, np.int32)
            pad, cnt = flat[:s * d * 4].reshape(s, d, 4), flat[s * d * 4:]
            for i, a in enumerate(arrs):
                cnt[i] = -1 if a is None else len(a)
                if a is not None and len(a):
                    pad[i, :len(a)] = a
            both = torch.from_numpy(flat).to(self.boxes.device)
            det, n = both[:s * d * 4].view(s, d, 4), both[s * d * 4:]
        was_empty = self._was_empty()
        self._flow_before_update()
        out = alignment.track_associate_streams_device(det, self.m_crop, self.boxes, self.status, self.misses, k,
                                                       (self.model.input_height, self.model.input_width), self.frame_hw,
                                                       n_det=n, state=self.filter_state, assoc=self.associate)
        self._mark_births(was_empty, out[1])
        self._flow_after_update()
        return out

    def _flow_before_update(self):
        """For a flow tracker: a device copy of the crop matrices before the association, for `_flow_after_update`."""
        if self.flow is not None:
            self._flow_m_before.copy_(self.m_crop)

    def _flow_after_update(self):
        """The history rule under `update`: a slot whose crop matrix the association wrote -- a birth or a restart -- has no
        usable history.  One comparison of bits on the device, no download."""
        import torch
        if self.flow is not None:
            wrote = (self.m_crop.view(torch.int32) != self._flow_m_before.view(torch.int32)).flatten(1).any(dim=1)
            self.flow_ready.masked_fill_(wrote, 0)

    def _flow_clear(self, on=None):
        """The history rule, first half of a tick of a flow tracker: flow_ready = 0 for every slot of the streams the tick
        steps.  on: None (all streams) or a CUDA bool [streams] mask."""
        if self.flow is None:
            return
        if on is None:
            self.flow_ready.zero_()
        else:
            self.flow_ready.view(self.streams, self.slots_per_stream).masked_fill_(on.view(-1, 1), 0)

    def _flow_put(self, slot, status, frame_index, lm=None, wd=None):
        """The history rule, second half: the rows served with status 0 become the history of their slots
        (alignment.track_flow_history_device, one launch).  lm None: the all-slots ticks, which have copied their
        landmarks themselves."""
        if self.flow is None:
            return
        rows = {} if lm is None else dict(lm_rows=lm, hist_lm=self._flow_lm)
        if lm is not None and wd is not None and self._flow_w is not None:
            rows.update(w_rows=wd.contiguous(), hist_w=self._flow_w)
        alignment.track_flow_history_device(slot, status, frame_index, self.flow_frame, self.flow_ready, **rows)

    def _stream_frame_index(self, frame_index, nf, named):
        """A per-stream `frame_index`, parsed: None for a contiguous CUDA int32 [streams] tensor, which is used where it
        lies, or the host list of `streams` ring slots, checked against the ring.  named: the streams whose host entries
        count -- the other entries are ignored and come back as 0 -- or None where the host cannot tell: every entry
        counts then, None standing for ring slot 0.  A tracker of one stream also takes a bare integer."""
        import torch
        s = self.streams
        if isinstance(frame_index, torch.Tensor):
            if (frame_index.dtype != torch.int32 or not frame_index.is_cuda or not frame_index.is_contiguous()
                    or tuple(frame_index.shape) != (s,)):
                raise ValueError("frame_index must be a sequence of %d ring slots or a contiguous CUDA int32 [%d] tensor"
                                 % (s, s))
            return None
        if s == 1 and not isinstance(frame_index, (list, tuple, np.ndarray)):
            frame_index = [frame_index]
        try:
            idx = list(frame_index)
        except TypeError:
            idx = None
        if idx is None or len(idx) != s:
            raise ValueError("frame_index must be a sequence of %d ring slots or a contiguous CUDA int32 [%d] tensor"
                             % (s, s))
        if named is None:
            idx, named = [0 if v is None else v for v in idx], range(s)
        keep = set(named)
        if any(idx[i] is None or isinstance(idx[i], bool) or int(idx[i]) != idx[i] or not 0 <= int(idx[i]) < nf
               for i in named):
            raise ValueError("frame_index must name ring slots in [0, %d)" % nf)
        return [int(v) if i in keep else 0 for i, v in enumerate(idx)]

    def _stream_frames(self, frame_index, nf):
        """frame_index of a tracker of several streams -> `frame_slots`, the ring slot of every global slot: a host
        sequence is checked against the ring and uploaded, a CUDA int32 [streams] tensor is used where it lies; the
        expansion over the slots of a stream is a device copy."""
        import torch
        s, k = self.streams, self.slots_per_stream
        idx = self._stream_frame_index(frame_index, nf, range(s))
        self._state()
        if idx is not None:
            frame_index = torch.tensor(idx, dtype=torch.int32).to(self.boxes.device)
        self.frame_slots.view(s, k).copy_(frame_index.view(s, 1).expand(s, k))

    def _step_prologue(self, ring, dt, frame_id, host_dt=False):
        """What `step` and `step_active` check before anything else: frame_id (None: the steps made so far), "dt goes
        with smooth" -- and, for host_dt, dt as the one host number `step` takes -- and the ring's geometry against
        frame_hw.  Returns (frame_id, dt, the slots of the ring)."""
        if self.best_shot is None and self.open_opts is None and frame_id is not None:
            raise ValueError("frame_id goes with best_shot")
        frame_id = self._steps if frame_id is None else alignment._frame_id(frame_id)
        if self.smooth is None and dt is not None:
            raise ValueError("dt goes with smooth")
        if host_dt:
            dt = None if self.smooth is None else self.smooth.time_step(dt)
        nf, rh, rw, _ = (self.frame_format or alignment.FrameFormat.bgr()).ring(ring)
        if (rh, rw) != self.frame_hw:
            raise ValueError("the ring holds %dx%d frames, the tracker was made for %dx%d" % ((rh, rw) + self.frame_hw))
        return frame_id, dt, nf

    def _forward_landmarks(self, ring, src, workspace):
        """The landmark source of `step`, `step_active` and `step_live`: the uint8 crop warp -> model.forward_device.
        Returns (lm on the output grid, wd: the scores or None, the grid's size)."""
        model = self.model
        crops = alignment.warp_frames_device(ring, src["m"], model.input_height, model.input_width, samples=self.crop_samples,
                                             fmt=self._crop_format, frame_index_dev=src["frame_index"],
                                             boxes_dev=src["boxes"], src=self.frame_format)
        out = "landmarks" if self.weights is None else "landmark_stats"
        fb = dict(fallback_faces=self.fallback_faces) if self.fallback_faces else {}   # (0: the call as it always was)
        res = model.forward_device(crops, out, n_points=self.n_points, thresh=self.thresh,
                                   workspace=workspace(int(crops.shape[0]), out), **fb)
        lm, wd = (res, None) if self.weights is None else (res[..., :2], res[..., 2])
        return lm, wd, (model.output_height, model.output_width)

    def _flow_landmarks(self, ring, src, workspace, slot, prev_frame_index):
        """The landmark source of `step_flow` (slot = _flow_iota, prev_frame_index = _flow_slots: every slot) and of
        `step_flow_live` (the snapshot's slot and prev_frame_index: its rows), bound by the caller: the uint8 crop warp
        of every row's PREVIOUS ring slot and of its new one, both with src's matrices, into 2*rows crops -> their
        pyramids in one launch -> alignment.landmark_flow_rows_device from the raw landmarks of the history, read at the
        rows' slots (with `LandmarkFlow(max_fb=...)`, its forward-backward check; without it flow_fb is -1.0).  Returns
        (lm in crop px, wd: the carried weights or None, the crop's size: the grid of these landmarks is the crop
        itself)."""
        n = int(slot.shape[0])
        ih, iw = self.model.input_height, self.model.input_width
        crops, pyr = self._flow_crops[:2 * n], self._flow_pyr[:2 * n]
        for half, slots in ((crops[:n], prev_frame_index), (crops[n:], src["frame_index"])):
            alignment.warp_frames_device(ring, src["m"], ih, iw, samples=self.crop_samples, fmt=self._crop_format,
                                         frame_index_dev=slots, boxes_dev=src["boxes"], src=self.frame_format, out=half)
        alignment.flow_pyramid_device(crops, self.flow.levels, out=pyr)
        self.flow_err, self.flow_flags, self.flow_fb = [t[:n] for t in self._flow_out]
        lm, wd = alignment.landmark_flow_rows_device(
            pyr[:n], pyr[n:], slot, self._flow_lm, src["m"], (ih, iw), self.flow, weights=self._flow_w,
            out=(self._flow_crop_lm[:n], self._flow_crop_w[:n], self.flow_err, self.flow_fb, self.flow_flags))[:2]
        return lm, (None if self.weights is None else wd), (ih, iw)

    def _sequence(self, ring, src, step, best_update, workspace, frame_id, quality_out=None, landmarks=None,
                  history=False, open_dt=None):
        """The step sequence, stated once for `step`, `step_flow` and `step_active`: the landmark source (`landmarks`;
        None: the uint8 crop warp -> model.forward_device) -> (lm, wd) -> the step call -> with history, the raw landmarks
        and weights kept for `step_flow` -> with pose, the head-pose call (at the rows' slots where src has a "slot") ->
        the aligned warp -> with best_shot, the quality call and the best update (with pose, times its factor).
        src: where the matrices ("m"), boxes and ring slots ("frame_index") of the faces are read -- the state itself or
        the snapshot; step, best_update: the caller's wrapper of the two, with what only that wrapper takes bound;
        workspace(batch, mode): the forward workspace, or None for the model's cached ones.  Returns (aligned, m_align,
        lm_frame, status)."""
        model = self.model
        ih, iw = model.input_height, model.input_width
        where = dict(frame_index_dev=src["frame_index"], boxes_dev=src["boxes"], src=self.frame_format)
        lm, wd, grid_hw = (landmarks or self._forward_landmarks)(ring, src, workspace)
        filt = {} if self.smooth is None else dict(filter=self.smooth, state=self.filter_state)
        stepped = step(lm, src["m"], src["boxes"], grid_hw=grid_hw, in_hw=(ih, iw),
                       frame_hw=self.frame_hw, tmpl_crop=self.crop_template, tmpl_align=self.template, weights=wd,
                       **self.limits, **filt)
        lm_frame, m_align, status = stepped[0], stepped[1], stepped[-1]
        if self.flow is not None:   # what `_flow_put` of a rows tick moves to the slots
            self._flow_rows = (lm_frame, wd, status)
        if history:   # (a tracker that smooths had the step write its raw points into _flow_lm)
            if self.smooth is None:
                self._flow_lm.copy_(lm_frame)
            if wd is not None:
                self._flow_w.copy_(wd)
        factor = {}
        if self.head_pose is not None:
            if self.best_shot is not None:
                factor = dict(factor=self._pose_factor[:int(lm_frame.shape[0])])
            alignment.head_pose_device(lm_frame, self._head_model, weights=wd, opts=self.head_pose, slot=src.get("slot"),
                                       out=self.pose, factor_out=factor.get("factor"))
        if self.open_opts is not None:   # one more launch: records and blink state at the rows' slots.  open_dt: the
            # step's own time step (a host number, or the rows' on the device), None for the Openness's dt
            alignment.face_openness_device(lm_frame, self.open_opts, weights=wd, slot=src.get("slot"), out=self.openness,
                                           state=self.open_state, reset=self._open_reset, dt=open_dt, status_rows=status,
                                           frame_id=frame_id)
        aligned = alignment.warp_frames_device(ring, m_align, self.out_size[0], self.out_size[1], samples=self.samples,
                                               fmt=self.aligned_format, **where)
        if self.parts is not None:   # one more launch, into the tracker's own buffers: the rows of `aligned`
            n = int(m_align.shape[0])
            self.part_M, self.part_ok = self._part_m_buf[:n], self._part_ok_buf[:n]
            self.part_faces = alignment.warp_parts_frames_device(
                ring, lm_frame, self.parts, weights=wd, samples=self.samples, fmt=self.aligned_format,
                out=self._part_buf[:n], affines_out=self.part_M, ok_out=self.part_ok, **where)
        if self.mesh is not None:   # one more launch, into the tracker's own buffer: the rows of `aligned`
            n = int(m_align.shape[0])
            self.mesh_faces = alignment.warp_mesh_frames_device(
                ring, lm_frame, m_align, self.mesh, self.out_size[0], self.out_size[1], samples=self.samples,
                fmt=self.aligned_format, out=self._mesh_buf[:n], **where)
        self._steps += 1
        if self.best_shot is not None:
            rec = alignment.face_quality_device(aligned, self.aligned_format, self.best_shot.quality, out=quality_out)
            best_update(aligned, rec, lm_frame, status, gallery=self.gallery, best_frame=self.best_frame, frame_id=frame_id,
                        weights=wd, m=m_align, opts=self.best_shot, best_m=self.best_M, best_lm=self.best_landmarks,
                        best_rec=self.best_rec, **factor)
            if self.view_opts is not None:   # the best update's own pending resets: the caller zeroes them after this
                n = int(aligned.shape[0])
                alignment.track_views_update_device(
                    aligned, rec, lm_frame, self.pose, self.view_q, self.view_frame, self.view_gallery, self._view_take[:n],
                    frame_id, status=status, reset=src.get("reset", self._best_reset), weights=wd, m=m_align,
                    opts=self.view_opts, slot=src.get("slot"), view_m=self.view_M, view_lm=self.view_landmarks,
                    view_pose=self.view_pose)
        return aligned, m_align, lm_frame, status

    def step(self, ring, frame_index, dt=None, frame_id=None):
        """One frame for every slot: `ring` is the frame ring (`frame_format` says how it holds its pixels),
        `frame_index` the ring slot of the new frame -- for a tracker of several streams one ring slot per stream, a
        host sequence (checked against the ring, one upload) or a contiguous CUDA int32 [streams] tensor (used as it is,
        nothing transferred; an index outside the ring gives zero crops): slot t reads the frame of stream
        t // slots_per_stream.  Sequence: the uint8 crop warp with the slots' matrices ->
        model.forward_device -> alignment.track_step_device (landmarks to frame px, the aligned fit, the next crop's
        matrix and box, the status) -> the aligned warp.  Returns CUDA tensors (aligned [capacity,oh,ow,3] float32 or in
        `aligned_format`, M float32 [capacity,2,3] frame px -> aligned px, landmarks float64 [capacity,C,2] in frame px,
        status int32 [capacity]); `status` is the tracker's own tensor, overwritten by the next step or seed.  A slot
        without a face returns zero crops and zero aligned faces, the identity and TRACK_DEAD; a track lost in this
        frame still returns this frame's aligned face, with the reason in its status, and is dead from the next step
        on.  `dt`, for a tracker that smooths: the seconds since the previous step, a host number (None: 1/fps of the
        filter).  `frame_id`, for a tracker with `best_shot`: the host integer `best_frame` records for a face taken
        in this step (None: the number of steps this tracker has made before this one)."""
        return self._step_all(ring, frame_index, dt, frame_id, None)

    def step_flow(self, ring, frame_index, dt=None, frame_id=None):
        """`step` without the forward, for a tracker made with `flow`: the landmarks of the last step are carried into the
        new frame by sparse optical flow and take the forward's place; everything after them -- the track step with its
        filter, both fits, the status and the next crop, then pose, the aligned warp, mesh, best shot and views -- is
        the code of `step`.  Arguments and results as `step`.  Sequence: the uint8 crop warp of the PREVIOUS ring slots
        (`frame_slots` of the last step) and of the new ones, both with the slots' current matrices ->
        alignment.flow_pyramid_device over all of them -> alignment.landmark_flow_rows_device with slot[r] = r from the
        last step's RAW landmarks (before the filter) and, with weights="score", its weights ->
        alignment.track_step_device with the crop as its grid -> the rest of `step`.  `flow_flags` and `flow_err` int32
        [capacity,C], views of the tracker's own buffers over all their rows, say what the flow did with every landmark
        (0, or the alignment.FLOW_* bits that rejected it; a landmark the forward rejected at the key frame stays
        rejected until the next `step`).  No upload beyond `step`'s, no download, no synchronisation.  With
        `LandmarkFlow(max_fb=...)` a landmark that does not come back to within `max_fb` crop px of where it started is
        rejected with alignment.FLOW_FB, and `flow_fb` float64 [capacity,C] (a view as well) holds the squared round
        trips; with max_fb=None the call returns the bits of alignment.landmark_flow_device and `flow_fb` is -1.0.

        May follow only `step` or `step_flow`: `seed`, `update`, `step_active`, `step_live` and `retire(flush=True)` leave
        tracks without a history the device could use, and the next call must be `step`.  THE CALLER KEEPS THE PREVIOUS
        FRAME IN THE RING until this call has run: it is read again here.  The usual loop is `update` + `step` on the
        ticks the detector runs, `step_flow` on the others."""
        if self.flow is None:
            raise ValueError("step_flow needs a tracker made with flow")
        if not self._flow_ok:
            raise ValueError("step_flow may follow only step or step_flow: after seed, update, step_active, step_live or "
                             "retire(flush=True) the next call must be step")
        return self._step_all(ring, frame_index, dt, frame_id, lambda ring, src, workspace: self._flow_landmarks(
            ring, src, workspace, self._flow_iota, self._flow_slots))   # (the state exists once _step_all has begun)

    def _step_all(self, ring, frame_index, dt, frame_id, landmarks):
        """`step` (landmarks None: the forward) and `step_flow` (the flow source), stated once."""
        import functools
        frame_id, dt, nf = self._step_prologue(ring, dt, frame_id, host_dt=True)
        if self.streams == 1:
            frame_index = int(frame_index)
            if not 0 <= frame_index < nf:
                raise ValueError("frame_index must name a ring slot in [0, %d)" % nf)
        elif landmarks is not None:   # check before the copy below: a rejected call leaves the history as it was
            self._stream_frame_index(frame_index, nf, range(self.streams))
        history = self.flow is not None
        if landmarks is not None:
            self._flow_slots.copy_(self.frame_slots)
        if self.streams > 1:
            self._stream_frames(frame_index, nf)
        self._state()
        self._retire(frame_id)
        if self.streams == 1:
            self.frame_slots.fill_(frame_index)
        raw = dict(lm_raw=self._flow_lm) if history and self.smooth is not None else {}
        self._flow_clear()

        def best_update(faces, rec, lm, status, **kw):
            alignment.track_best_update_device(faces, rec, lm, self.best_q, self._best_q_spare, status=status,
                                               reset=self._best_reset, **kw)

        res = self._sequence(
            ring, dict(m=self.m_crop, boxes=self.boxes, frame_index=self.frame_slots),
            functools.partial(alignment.track_step_device, m_next=self.m_crop, boxes_next=self._boxes_spare,
                              status=self.status, dt=dt, **raw),
            best_update, lambda n, out: None, frame_id, quality_out=self._quality_rec if self.best_shot is not None else None,
            landmarks=landmarks, history=history, open_dt=dt)
        self._flow_ok = True
        if history:
            self._flow_put(self._flow_iota, self.status, self.frame_slots)
        self.boxes, self._boxes_spare = self._boxes_spare, self.boxes
        if self.best_shot is not None:
            self.best_q, self._best_q_spare = self._best_q_spare, self.best_q
            self._best_reset.zero_()
        self._retire_served()
        self._served()
        return res

    def annotate(self, ring, landmarks, frame_index=None, annotation=None):
        """Draw what the tracker knows into the frames themselves (alignment.annotate_frames_device, flm_frames_annotate):
        the marks of `utils.plots.draw_marks` at every landmark, an outline and a mosaic of every face, as `annotation`
        (an alignment.FrameAnnotation; None: its defaults, marks alone) says.  `ring`: the ring the step read, in the
        tracker's `frame_format` and of its `frame_hw`; `landmarks`: the landmarks the step returned, CUDA float64
        [rows,C,2] in frame px -- the rejected points and the slots without a face are (-1,-1) and draw nothing;
        `frame_index`: None -- `frame_slots`, the ring slots `step` cut from, one per slot -- or a contiguous CUDA int32
        [rows] tensor.  After `step_active` or `step_live` the landmarks are ROWS, and `frame_slots` is not theirs: pass
        the rows' ring slots as such a tensor.  Nothing is downloaded, nothing synchronises, and the call runs inside
        torch.cuda.set_sync_debug_mode("error").  Returns the regions, CUDA int32 [rows,4] (x0,y0,x1,y1), unclipped.

        The call WRITES the ring: the slot is changed for every later reader -- a later step that cuts from it sees the
        marks, a recorder sees the mosaic.  So call it after the step of that frame, and before the decoder reuses the
        slot.  `prediction.frames_to_bgr_device` of an annotated NV12 slot gives the displayable picture."""
        import torch
        if annotation is not None and not isinstance(annotation, alignment.FrameAnnotation):
            raise ValueError("annotation must be None or an alignment.FrameAnnotation (got %r)" % (annotation,))
        fmt = self.frame_format or alignment.FrameFormat.bgr()
        _, rh, rw, _ = fmt.ring(ring)
        if (rh, rw) != self.frame_hw:
            raise ValueError("the ring holds %dx%d frames, the tracker was made for %dx%d" % ((rh, rw) + self.frame_hw))
        if not isinstance(landmarks, torch.Tensor) or landmarks.dim() != 3:
            raise ValueError("landmarks must be a CUDA float64 [rows,C,2] tensor")
        if frame_index is None:
            self._state()
            frame_index = self.frame_slots
            if int(landmarks.shape[0]) != int(frame_index.shape[0]):
                raise ValueError("frame_index=None goes with the landmarks of `step`, one face per slot (%d): pass the "
                                 "rows' ring slots as a CUDA int32 tensor" % int(frame_index.shape[0]))
        return alignment.annotate_frames_device(ring, landmarks, frame_index_dev=frame_index, opts=annotation, src=fmt)

    def _served(self, slot=None):
        """`step` (slot None: every slot) or `step_active` (the rows' slots, -1 for an inert row) has served slots that
        `step_live` may have left waiting: their wait ends here, so the next `step_live` does not add it to their dt.
        Launches nothing for a tracker whose `step_live` never ran below capacity."""
        import torch
        if self.smooth is None or not self._waiting:
            return
        if slot is None:
            self.slot_age.zero_()
            self._waiting = False
            return
        n = self.capacity
        age = torch.cat([self.slot_age, self.slot_age.new_zeros(1)])       # (an inert row clears the spare entry)
        age.index_fill_(0, torch.where(slot < 0, n, slot).to(torch.int64), 0.0)
        self.slot_age.copy_(age[:n])

    def _active_workspace(self, n, out):
        """The forward workspace `step_active` passes for a batch of n faces, or None (the model's cached path).  The
        model caches four workspaces keyed by batch, and a tracker of S streams can see S different batches: so the
        tracker owns ONE, sized for the largest batch it can see in one launch, min(capacity, model.max_batch) -- the
        forward lays its tensors out for the batch it is given and only asks that the workspace be large enough
        (workspace_bytes does not decrease with the batch).  A batch beyond model.max_batch takes the cached path, which
        slices."""
        if n > self.model.max_batch:
            return None
        if self._ws_active is None:
            fb = dict(fallback_faces=self.fallback_faces) if self.fallback_faces else {}
            self._ws_active = self.model.new_workspace(min(self.capacity, self.model.max_batch), out, self.n_points, **fb)
        return self._ws_active

    def _stream_dt(self, dt, named):
        """The `dt` of `step_active` and `step_live`, parsed -> (a host list of `streams` numbers to upload, the CUDA
        float64 [streams] tensor to use where it lies, the one host number for every stream): exactly one is not None
        for a tracker that smooths, all three are None for one that does not.  named: the streams whose host entries
        count; the other entries are ignored and come back as 0."""
        import math
        import torch
        s = self.streams
        dt_host, dt_dev, dt_scalar = None, None, None
        if self.smooth is not None:
            if isinstance(dt, torch.Tensor):
                if (dt.dtype != torch.float64 or not dt.is_cuda or not dt.is_contiguous() or tuple(dt.shape) != (s,)):
                    raise ValueError("dt must be None, a number, a sequence of %d numbers or a contiguous CUDA float64 "
                                     "[%d] tensor" % (s, s))
                dt_dev = dt
            elif dt is None or isinstance(dt, (int, float, np.integer, np.floating)):
                dt_scalar = self.smooth.time_step(dt)
            else:
                try:
                    dt_host = list(dt)
                except TypeError:
                    dt_host = None
                if dt_host is None or len(dt_host) != s:
                    raise ValueError("dt must be None, a number, a sequence of %d numbers or a contiguous CUDA float64 "
                                     "[%d] tensor" % (s, s))
                for i in named:
                    v = dt_host[i]
                    if v is None or isinstance(v, bool) or not (float(v) > 0.0 and math.isfinite(float(v))):
                        raise ValueError("dt of stream %d must be finite and > 0, got %r" % (i, v))
                keep = set(named)
                dt_host = [float(v) if i in keep else 0.0 for i, v in enumerate(dt_host)]
        return dt_host, dt_dev, dt_scalar

    def _upload(self, dt_host, *ints):
        """One upload of everything that arrived on the host -- dt_host float64, every list of `ints` int32; None: nothing
        to send -- float64 first, so every view is aligned.  Returns the device views in the order given, None for None."""
        import torch
        parts = [None if x is None else np.asarray(x, t) for x, t in [(dt_host, np.float64)] + [(x, np.int32) for x in ints]]
        if all(x is None for x in parts):
            return parts
        up = torch.from_numpy(np.concatenate([x.view(np.uint8) for x in parts if x is not None])).to(self.boxes.device)
        views, off = [], 0
        for x in parts:
            views.append(None if x is None else up[off:off + x.nbytes].view(torch.float64 if x.dtype == np.float64 else torch.int32))
            off += 0 if x is None else x.nbytes
        return views

    def step_active(self, ring, frame_index, active, dt=None, frame_id=None):
        """One frame for the slots of the streams `active` alone, each stream on its own clock; every other stream keeps
        every bit of its state (matrices, boxes, status, filter state, best shot, pending best-shot reset).  Works for any
        `streams` >= 1; `step` and `step_active` may be mixed freely, and both count as a step.

        frame_index: the ring slot of every stream's new frame, a host sequence of `streams` entries (those of streams
        not in `active` are ignored and may be None) or a contiguous CUDA int32 [streams] tensor; a tracker of one
        stream also takes a bare integer.  active: a host sequence of distinct stream ids in [0, streams) -- an empty
        one returns empty tensors, launches nothing and is not counted as a step -- or a contiguous CUDA int32 [A]
        tensor, 1 <= A <= streams, used where it lies (distinct ids; an id outside the range gives slots_per_stream inert
        rows: zero faces, the identity, TRACK_DEAD, slot -1).  With `active` on the device the host cannot tell which
        entries of a host `frame_index` or `dt` are ignored: every entry is then checked, None standing for ring slot 0
        and not allowed in `dt`.  dt, for a tracker that smooths: None (1/fps of the filter), a host number, a host
        sequence of `streams` numbers (entries of inactive streams are ignored, those of active ones must be > 0 and
        finite) or a CUDA float64 [streams] tensor -- the seconds since THAT stream's previous frame (on the device, a
        value that is not > 0 and finite takes the history of the stream's landmarks away and nothing else).  frame_id:
        as `step` takes it.

        Whatever arrives on the host goes up in ONE upload, device arguments cause no transfer, nothing synchronises.
        Sequence: alignment.track_gather_streams_device (the snapshot: the active slots' matrices, boxes, ring slots,
        time steps, best quality and pending resets in compact rows) -> the uint8 crop warp on the snapshot ->
        model.forward_device at batch A*slots_per_stream -> alignment.track_step_rows_device (writes the tracker's
        state at each row's slot) -> the aligned warp (with the snapshot's boxes) -> with best_shot,
        alignment.face_quality_device and alignment.track_best_update_rows_device.  The forward of a batch up to
        model.max_batch runs in one workspace the tracker owns, sized for its largest batch (`_active_workspace`); a
        larger batch takes the model's cached path, which slices.  `frame_slots` keeps what the last `step` wrote.

        Returns CUDA tensors over the N = A*slots_per_stream rows, row a*slots_per_stream + j being slot
        active[a]*slots_per_stream + j: (aligned [N,...], M float32 [N,2,3], landmarks float64 [N,C,2], status int32 [N],
        slots int32 [N])."""
        import functools
        import torch
        s, k = self.streams, self.slots_per_stream
        frame_id, _, nf = self._step_prologue(ring, dt, frame_id)
        # ---- active
        act_host = None
        if isinstance(active, torch.Tensor):
            if (active.dtype != torch.int32 or not active.is_cuda or not active.is_contiguous() or active.dim() != 1
                    or not 1 <= int(active.shape[0]) <= s):
                raise ValueError("active must be a sequence of distinct stream ids in [0, %d) or a contiguous CUDA int32 "
                                 "[A] tensor with 1 <= A <= %d" % (s, s))
            a = int(active.shape[0])
        else:
            try:
                act_host = list(active)
            except TypeError:
                act_host = None
            if (act_host is None or any(isinstance(v, bool) or int(v) != v or not 0 <= int(v) < s for v in act_host)
                    or len(set(int(v) for v in act_host)) != len(act_host)):
                raise ValueError("active must be a sequence of distinct stream ids in [0, %d) or a contiguous CUDA int32 "
                                 "[A] tensor with 1 <= A <= %d" % (s, s))
            act_host = [int(v) for v in act_host]
            a = len(act_host)
        named = range(s) if act_host is None else act_host    # the streams whose host entries count
        # ---- frame_index
        fi_host = self._stream_frame_index(frame_index, nf, act_host)
        dt_host, dt_dev, dt_scalar = self._stream_dt(dt, named)
        self._flow_ok = False
        self._state()
        dev = self.boxes.device
        model = self.model
        n = a * k
        if n == 0:
            c = int(model.n_classes)
            fmt = self.aligned_format or alignment.AlignedFormat()
            return (torch.empty(fmt.shape(0, *self.out_size), dtype=fmt.torch_dtype, device=dev),
                    torch.empty((0, 2, 3), dtype=torch.float32, device=dev),
                    torch.empty((0, c, 2), dtype=torch.float64, device=dev),
                    torch.empty((0,), dtype=torch.int32, device=dev), torch.empty((0,), dtype=torch.int32, device=dev))
        self._retire(frame_id)
        up = self._upload(dt_host, fi_host, act_host)
        dt_dev, frame_index, active = [b if a is None else a for a, b in zip(up, (dt_dev, frame_index, active))]
        best = self.best_shot is not None
        snap = alignment.track_gather_streams_device(
            active, self.m_crop, self.boxes, k, frame_index=frame_index, dt=dt_dev, best_q=self.best_q if best else None,
            reset=self._best_reset if best else None)
        raw = {}
        if self.flow is not None:   # (an id outside [0, streams) matches no stream)
            self._flow_clear((torch.arange(s, dtype=torch.int32, device=dev).view(s, 1) == active.view(1, a)).any(dim=1))
            if self.smooth is not None:
                raw = dict(lm_raw=self._flow_raw_rows[:n])

        def best_update(faces, rec, lm, status_rows, **kw):
            alignment.track_best_update_rows_device(faces, rec, lm, snap["slot"], snap["best_q"], self.best_q,
                                                    status_rows=status_rows, reset_c=snap["reset"], **kw)

        res = self._sequence(
            ring, snap,
            functools.partial(alignment.track_step_rows_device, slot=snap["slot"], m_next=self.m_crop, boxes_next=self.boxes,
                              status=self.status, dt=dt_scalar if dt_dev is None else snap["dt"], **raw),
            best_update, self._active_workspace, frame_id, open_dt=dt_scalar if dt_dev is None else snap["dt"])
        self._flow_put_rows(snap, raw)
        self._retire_served()
        self._served(snap["slot"])
        return res + (snap["slot"],)

    def step_live(self, ring, frame_index, budget, active=None, dt=None, frame_id=None):
        """One frame for the slots that HOLD A FACE, at most `budget` of them: the empty slots of the stepped streams,
        which `step` and `step_active` carry through the forward as zero crops, are no rows here.  A camera sized for 16
        faces usually sees one or two, and the forward is nearly all of a step.  Which slots are live is known only on the
        device; alignment.track_gather_live_device compacts them there into a batch of the fixed size `budget`, a host
        integer in [1, capacity], so nothing is downloaded and nothing synchronises.  Live slots beyond the budget sit the
        tick out with everything intact -- crop, filter history, best shot, pending best-shot reset -- and are served
        first on the next tick (`live_cursor`); the `dt` of a slot that waited includes its wait (`slot_age`).
        `live_counts` int32 [4], the tracker's own, holds (live slots, rows served, live slots left out, the next cursor)
        of the last call: a caller may look at it now and then to size its budget.  Works for any `streams` >= 1;
        `step`, `step_active` and `step_live` may be mixed freely, and all three count as a step.

        frame_index, dt, frame_id: as `step_active` takes them.  active: None (every stream), a host sequence of distinct
        stream ids as `step_active` takes it (an empty one steps no stream: every row is inert), or a contiguous CUDA
        int32 [streams] MASK, non-zero for the streams that delivered a frame, used where it lies; with a mask on the
        device every entry of a host `frame_index` or `dt` is checked.  The slots of a stream that is not active are
        neither read nor written.  Whatever arrives on the host goes up in ONE upload.

        Sequence: alignment.track_gather_live_device, then what `step_active` runs on its snapshot -- the uint8 crop warp
        -> model.forward_device at batch `budget`, in the workspace of `_active_workspace` ->
        alignment.track_step_rows_device -> the aligned warp -> with best_shot, alignment.face_quality_device and
        alignment.track_best_update_rows_device.  `frame_slots` keeps what the last `step` wrote.

        Returns CUDA tensors over the `budget` rows (aligned, M float32 [budget,2,3], landmarks float64 [budget,C,2],
        status int32 [budget], slots int32 [budget]); rows past the served ones are zero faces, the identity, TRACK_DEAD
        and slot -1.  A dead slot is no row, so its `status` keeps the reason it was lost where `step` would overwrite it
        with TRACK_DEAD; `lost()` still names it."""
        return self._step_live(ring, frame_index, budget, active, dt, frame_id, False)

    def step_flow_live(self, ring, frame_index, budget, active=None, dt=None, frame_id=None):
        """`step_live` without the forward, for a tracker made with `flow`: one frame for the slots that hold a face AND
        have a usable history, at most `budget` of them, their landmarks carried into the new frame by sparse optical flow
        as in `step_flow`.  Arguments, checks and results as `step_live`.  The usual loop is `update` + `step_live` on
        the ticks the detector runs -- the forward, for the live faces alone -- and `step_flow_live` on the others.

        Which slots have a history the device knows (`flow_ready`; the rule is stated in include/flm.h): a slot has one
        exactly when the last tick of its stream -- `step`, `step_flow`, `step_active`, `step_live` or this call -- served
        it with status 0 and no `seed` or `update` has written its crop matrix since.  So the call may follow ANY call.  A
        live slot without a history -- born since the last tick, left out by that tick's budget -- is simply no row: every
        bit of its state is kept, `flow_counts[4]` says how many there were, and the next `step_live` serves it.  A live
        slot with a history that THIS budget leaves out loses it (its landmarks would be older than the previous frame)
        and waits for a forward tick too.  The forward is never run here.  THE CALLER KEEPS EVERY STREAM'S PREVIOUS
        FRAME IN THE RING until this call has run.

        Sequence: alignment.track_gather_flow_device (a cursor of its own, `flow_cursor`) -> the uint8 crop warp of the
        snapshot's previous ring slots and of the new ones, both with the snapshot's matrices, into 2*budget crops ->
        alignment.flow_pyramid_device over them in one launch -> alignment.landmark_flow_rows_device (with
        `LandmarkFlow(max_fb=...)`, its forward-backward check) -> alignment.track_step_rows_device with the crop as its
        grid -> what `step_live` runs after its landmarks -> alignment.track_flow_history_device.  `flow_counts` int32
        [6], the tracker's own: (live slots, live slots with a history, rows served, slots with a history left out, live
        slots without a history, the next cursor); `flow_flags`, `flow_err` int32 and `flow_fb` float64 [budget,C] say
        what the flow did with every landmark of every row.  Counts as a step; afterwards `step_flow`'s own host rule asks
        for a `step`, as after `step_live`.  No download, no synchronisation."""
        if self.flow is None:
            raise ValueError("step_flow_live needs a tracker made with flow")
        return self._step_live(ring, frame_index, budget, active, dt, frame_id, True)

    def _flow_put_rows(self, snap, raw):
        """`_flow_put` after a rows tick: the raw landmarks are the step's lm_raw for a tracker that smooths, else the
        landmarks it returned."""
        if self.flow is not None:
            lm_frame, wd, status = self._flow_rows
            self._flow_put(snap["slot"], status, snap["frame_index"], raw.get("lm_raw", lm_frame), wd)
            self._flow_rows = None

    def _step_live(self, ring, frame_index, budget, active, dt, frame_id, flow):
        """`step_live` (flow False: the forward) and `step_flow_live` (the flow source), stated once."""
        import functools
        import torch
        s, k = self.streams, self.slots_per_stream
        frame_id, _, nf = self._step_prologue(ring, dt, frame_id)
        if isinstance(budget, bool) or int(budget) != budget or not 1 <= int(budget) <= self.capacity:
            raise ValueError("budget must be an integer in [1, %d] (got %r)" % (self.capacity, budget))
        budget = int(budget)
        what = ("active must be None, a sequence of distinct stream ids in [0, %d) or a contiguous CUDA int32 [%d] mask"
                % (s, s))
        on_host, named = None, range(s)
        if isinstance(active, torch.Tensor):
            if active.dtype != torch.int32 or not active.is_cuda or not active.is_contiguous() or tuple(active.shape) != (s,):
                raise ValueError(what)
            named = None                                          # the host cannot tell: every host entry counts
        elif active is not None:
            try:
                named = list(active)
            except TypeError:
                raise ValueError(what) from None
            if (any(isinstance(v, bool) or int(v) != v or not 0 <= int(v) < s for v in named)
                    or len(set(int(v) for v in named)) != len(named)):
                raise ValueError(what)
            named = [int(v) for v in named]
            on_host = [1 if i in set(named) else 0 for i in range(s)]
        fi_host = self._stream_frame_index(frame_index, nf, named)
        dt_host, dt_dev, dt_scalar = self._stream_dt(dt, range(s) if named is None else named)
        self._flow_ok = False
        self._state()
        self._retire(frame_id)
        up = self._upload(dt_host, fi_host, on_host)
        dt_dev, frame_index, active = [b if a is None else a for a, b in zip(up, (dt_dev, frame_index, active))]
        best, smooth = self.best_shot is not None, self.smooth is not None
        self._waiting = self._waiting or budget < self.capacity or flow   # (a flow tick leaves the history-less waiting)
        common = dict(stream_on=active, frame_index=frame_index,
                      dt=(dt_scalar if dt_dev is None else dt_dev) if smooth else None, best_q=self.best_q if best else None,
                      reset=self._best_reset if best else None, age=self.slot_age if smooth else None)
        if flow:            # (the gather clears flow_ready for the streams that are on)
            snap = alignment.track_gather_flow_device(
                self.m_crop, self.boxes, self.flow_frame, self.flow_ready, k, self.frame_hw, budget, cursor=self.flow_cursor,
                out=dict(counts=self.flow_counts), **common)
        else:
            snap = alignment.track_gather_live_device(
                self.m_crop, self.boxes, k, self.frame_hw, budget, cursor=self.live_cursor,
                out=dict(counts=self.live_counts), **common)
            if self.flow is not None:
                self._flow_clear(None if active is None else active != 0)
        raw = dict(lm_raw=self._flow_raw_rows[:budget]) if self.flow is not None and smooth else {}

        def best_update(faces, rec, lm, status_rows, **kw):
            alignment.track_best_update_rows_device(faces, rec, lm, snap["slot"], snap["best_q"], self.best_q,
                                                    status_rows=status_rows, reset_c=snap["reset"], **kw)

        res = self._sequence(
            ring, snap,
            functools.partial(alignment.track_step_rows_device, slot=snap["slot"], m_next=self.m_crop, boxes_next=self.boxes,
                              status=self.status, dt=snap.get("dt"), **raw),
            best_update, self._active_workspace, frame_id, landmarks=(lambda ring, src, workspace: self._flow_landmarks(
                ring, src, workspace, snap["slot"], snap["prev_frame_index"])) if flow else None, open_dt=snap.get("dt"))
        self._flow_put_rows(snap, raw)
        self._retire_served()
        return res + (snap["slot"],)

    def _retire(self, frame_id, flush=False):
        """The retire call of a tracker with `exits`, over all slots: before the gather and before anything can overwrite
        a gallery row.  `_exit_stale` marks the slots whose track no step has served since a retire named it: their best_q
        is still the previous track's, which was queued at that birth, so the call reads -1 for them -- a retire that
        sees a birth sets the mark, the step that serves the slot's pending best-shot reset clears it (_retire_served).
        With `views` the exit-views call follows at once and reads this call's exit_row.  The stale mark covers the views
        too: a slot whose bins are still an earlier track's is one whose best_q the retire call reads as -1, so it is
        discarded, gets a negative exit_row, and nothing stale is copied -- the bins are emptied by the same pending reset,
        in the same step, as the best shot.  Launches nothing for a tracker without `exits`."""
        import torch
        if self.exit_opts is None:
            return
        torch.where(self._exit_stale, self._no_best, self.best_q, out=self._exit_q_in)
        torch.logical_or(self._exit_stale, self._born, out=self._exit_stale)
        alignment.track_retire_device(
            self.boxes, self.status, self.frame_hw, self._exit_q_in, self.gallery, self.best_frame, self._born,
            self.track_id, self.born_frame, self.exit_head, self.exit_faces, self.exit_meta, self.exit_q, self.exit_row,
            frame_id, flush=flush, opts=self.exit_opts, best_m=self.best_M, best_lm=self.best_landmarks,
            best_rec=self.best_rec, x_m=self.exit_M, x_lm=self.exit_landmarks, x_rec=self.exit_rec)
        if self.view_opts is not None:
            alignment.track_exit_views_device(
                self.exit_row, self.view_q, self.view_frame, self.view_gallery, self.exit_view_q, self.exit_view_frame,
                self.exit_view_gallery, view_m=self.view_M, view_lm=self.view_landmarks, view_pose=self.view_pose,
                x_view_m=self.exit_view_M, x_view_lm=self.exit_view_landmarks, x_view_pose=self.exit_view_pose)

    def _retire_served(self):
        """After the best update of a step: a slot whose pending best-shot reset the step has used holds its own track's
        best (or none) from here on."""
        if self.exit_opts is not None:
            self._exit_stale.logical_and_(self._best_reset)

    def retire(self, flush=False, frame_id=None):
        """The retire call on demand, for a tracker with `exits`: queues the tracks that have ended since the last tick
        and names the ones that have begun, without stepping.  flush=True ends every held track as well -- the end of a
        video; a later step finds the slots without a track, and only an `update` or a `seed` starts one again.
        frame_id: what the exits record as the frame of their end (None: the number of steps made so far).  Returns
        `exit_head`.  No download, no synchronisation."""
        if self.exit_opts is None:
            raise ValueError("retire() needs a tracker made with exits")
        frame_id = self._steps if frame_id is None else alignment._frame_id(frame_id)
        if flush:
            self._flow_ok = False
        self._state()
        if flush:
            self._flow_clear()
        self._retire(frame_id, flush=bool(flush))
        return self.exit_head

    def exits(self):
        """The exit ring of a tracker with `exits`: CUDA tensors (faces [Q,...] in the aligned format, meta int64 [Q,8],
        q float64 [Q], M float32 [Q,2,3], landmarks float64 [Q,C,2], head int64 [4]), the tracker's own, rows overwritten
        as later tracks end.  No download, no synchronisation: download `head` when convenient and let
        `alignment.exit_rows(head[0], cursor, Q)` name the rows that are new."""
        if self.exit_opts is None:
            raise ValueError("exits() needs a tracker made with exits")
        self._state()
        return self.exit_faces, self.exit_meta, self.exit_q, self.exit_M, self.exit_landmarks, self.exit_head

    def views(self):
        """The pose-binned best shots of every slot, for a tracker with `views`: CUDA tensors (view_gallery
        [capacity,B,...] in the aligned format, view_q float64 [capacity,B] -- -1: the bin holds nothing --, view_frame
        int64 [capacity,B], view_M float32 [capacity,B,2,3], view_landmarks float64 [capacity,B,C,2], view_pose float64
        [capacity,B,18]), the tracker's own, overwritten by later steps.  No download, no synchronisation."""
        if self.view_opts is None:
            raise ValueError("views() needs a tracker made with views")
        self._state()
        return self.view_gallery, self.view_q, self.view_frame, self.view_M, self.view_landmarks, self.view_pose

    def exit_views(self):
        """The views of the finished tracks, for a tracker with `views` and `exits`: CUDA tensors over the Q ring rows of
        `exits()`, row for row (exit_view_gallery [Q,B,...], exit_view_q float64 [Q,B], exit_view_frame int64 [Q,B],
        exit_view_M float32 [Q,B,2,3], exit_view_landmarks float64 [Q,B,C,2], exit_view_pose float64 [Q,B,18]).  A bin
        whose exit_view_q is negative held no face: its other entries are whatever the ring row held before.  No
        download, no synchronisation."""
        if self.view_opts is None:
            raise ValueError("exit_views() needs a tracker made with views")
        if self.exit_opts is None:
            raise ValueError("exit_views() needs a tracker made with exits")
        self._state()
        return (self.exit_view_gallery, self.exit_view_q, self.exit_view_frame, self.exit_view_M, self.exit_view_landmarks,
                self.exit_view_pose)

    def best(self):
        """The best shot of every slot, for a tracker with `best_shot`: CUDA tensors (gallery [capacity,...] in the
        aligned format, best_q float64 [capacity] -- -1: the slot holds none --, best_frame int64 [capacity], best_M
        float32 [capacity,2,3], best_landmarks float64 [capacity,C,2]), the tracker's own, overwritten by later steps.
        No download, no synchronisation."""
        if self.best_shot is None:
            raise ValueError("best() needs a tracker made with best_shot")
        self._state()
        return self.gallery, self.best_q, self.best_frame, self.best_M, self.best_landmarks

    def lost(self):
        """The slots whose status is not 0, as a host list: the one call of the tracker that synchronises.  The caller
        re-seeds them from its detector (or leaves them empty)."""
        self._state()
        return [int(v) for v in (self.status != 0).nonzero().flatten().tolist()]
