"""`get_image_array` of the predict path (reference data/generator.py:29-69) on the device, and the labelled-data
pieces of the evaluation: `read_keypoints` / `get_pairs_from_paths` (:82-160) and the Gaussian target maps
`gaussian_k` / `generate_hm` (:274-296, on the device through `flm_gaussian_heatmaps`).

Same signature, argument meaning and errors.  cv2 is not a dependency: files are decoded
with PIL into BGR (what cv2.imread returns), and an image whose size differs from
(width, height) is resampled on the GPU by `flm_crop_resize`: OpenCV's 8-bit INTER_LINEAR
restated in integer fixed point (11-bit weights, the exact 2x downscale as INTER_AREA), bit-equal
to `oracle/warp_ref.resize_u8_ref`; parity with the cv2 binary itself is unpinned (cv2 is not
installable here).  For crops already at model size -- the hot path -- the resize is the identity,
as in cv2.
"""
from __future__ import annotations

import os
import re

import numpy as np
import six

from .. import _lib


ACCEPTABLE_IMAGE_FORMATS = [".jpg", ".jpeg", ".png", ".bmp"]
ACCEPTABLE_KEYPOINTS_FORMATS = [".pts"]


class DataLoaderError(Exception):
    pass


_NORMS = {"sub_mean": _lib.NORM_SUB_MEAN, "sub_and_divide": _lib.NORM_SUB_AND_DIVIDE, "divide": _lib.NORM_DIVIDE}


def imread_bgr(path, read_image_type=1):
    """cv2.imread(path, 1) stand-in: uint8 HxWx3 in BGR order (or HxW for type 0)."""
    from PIL import Image
    im = Image.open(path)
    if read_image_type == 0:
        return np.asarray(im.convert("L"))
    return np.ascontiguousarray(np.asarray(im.convert("RGB"))[:, :, ::-1])


def resize_u8_device(img_dev, height, width):
    """[H,W,3] uint8 CUDA tensor -> [height,width,3] via flm_crop_resize on the full frame."""
    import torch
    lib = _lib.load()
    h, w = int(img_dev.shape[0]), int(img_dev.shape[1])
    if (h, w) == (height, width):
        return img_dev
    boxes = torch.tensor([[0, 0, w, h]], dtype=torch.int32, device=img_dev.device)
    out = torch.empty((1, height, width, 3), dtype=torch.uint8, device=img_dev.device)
    _lib.check(lib.flm_crop_resize(_lib.stream_ptr(), _lib.ptr(img_dev), h, w, _lib.ptr(boxes), 1,
                                   _lib.ptr(out), height, width), "flm_crop_resize")
    return out[0]


def get_image_array(image, width, height, imgNorm="sub_mean", ordering="channels_first", read_image_type=1):
    """Load image array from input (reference data/generator.py:29-69)."""
    import torch
    if isinstance(image, np.ndarray):
        img = image
    elif isinstance(image, six.string_types):
        if not os.path.isfile(image):
            raise DataLoaderError("get_image_array: path {0} doesn't exist".format(image))
        img = imread_bgr(image, read_image_type)
    else:
        raise DataLoaderError("get_image_array: Can't process input type {0}".format(str(type(image))))
    if imgNorm not in _NORMS:
        return img  # the reference falls through every branch and returns the raw image
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
        raise DataLoaderError("get_image_array: the device path takes uint8 HxWx3 images")
    lib = _lib.load()
    dev = _lib.require_gpu()
    d = resize_u8_device(torch.from_numpy(np.ascontiguousarray(img)).to(dev), height, width)
    out = torch.empty((height, width, 3), dtype=torch.float32, device=dev)
    _lib.check(lib.flm_preprocess(_lib.stream_ptr(), _lib.ptr(d.contiguous()), 1, height, width, _NORMS[imgNorm],
                                  _lib.ptr(out)), "flm_preprocess")
    res = out.cpu().numpy()
    if ordering == "channels_first":
        res = np.rollaxis(res, 2, 0)
    return res


def get_pairs_from_paths(images_path, keypts_path, ignore_non_matching=False):
    """data/generator.py:82-119: [(image path, .pts path)] for every image of `images_path` with an acceptable
    extension, matched by file stem against the `.pts` files of `keypts_path` (os.listdir order).  Two keypoint files
    with one stem, or an image without keypoints (unless ignore_non_matching), raise DataLoaderError."""
    image_files = [(*os.path.splitext(e), os.path.join(images_path, e)) for e in os.listdir(images_path)
                   if os.path.isfile(os.path.join(images_path, e))
                   and os.path.splitext(e)[1] in ACCEPTABLE_IMAGE_FORMATS]
    keypoints_files = {}
    for e in os.listdir(keypts_path):
        full = os.path.join(keypts_path, e)
        if os.path.isfile(full) and os.path.splitext(e)[1] in ACCEPTABLE_KEYPOINTS_FORMATS:
            stem, ext = os.path.splitext(e)
            if stem in keypoints_files:
                raise DataLoaderError("Segmentation file with filename {0} already exists and is ambiguous to"
                                      " resolve with path {1}. Please remove or rename the latter.".format(stem, full))
            keypoints_files[stem] = (ext, full)
    pairs = []
    for stem, _, image_full_path in image_files:
        if stem in keypoints_files:
            pairs.append((image_full_path, keypoints_files[stem][1]))
        elif not ignore_non_matching:
            raise DataLoaderError("No corresponding segmentation found for image {0}.".format(image_full_path))
    return pairs


def read_keypoints(keypts_path):
    """data/generator.py:138-160 (the plain-array form, is_imgaug_kps=False): a `.pts` file as
    scripts/prepare_dataset.py:34-52 writes it -> (float64 [n, 2] array, n_points, version string).
    `{` / `}` lines are skipped; the last line may lack its newline; missing points are stored as `-1 -1`."""
    keypoints, n_points, version = [], None, None
    with open(keypts_path, "r") as fp:
        for line in fp.readlines():
            text = line.strip()
            if re.match(r"{|}", text):
                continue
            if re.match("version", text):
                version = re.findall(r"\d+", text)[0]
            elif re.match("n_points", text):
                n_points = int(re.findall(r"\d+", text)[0])
            else:
                keypoints.append([float(v) for v in text.split()])
    return np.array(keypoints), n_points, version


def gaussian_heatmaps_device(keypoints, height, width, sigma=3):
    """keypoints: CUDA float64 [N,L,2] (x,y) in grid pixels -> CUDA float32 [N,height,width,L]: generate_hm of every
    face (flm_gaussian_heatmaps).  The denominator is Python's `2 * sigma**2`, as gaussian_k evaluates it."""
    import torch
    lib = _lib.load()
    if keypoints.dim() != 3 or keypoints.shape[2] != 2 or not keypoints.is_cuda:
        raise ValueError("gaussian_heatmaps_device needs a CUDA [N,L,2] tensor")
    kp = keypoints.to(torch.float64).contiguous()
    n, l = int(kp.shape[0]), int(kp.shape[1])
    out = torch.empty((n, int(height), int(width), l), dtype=torch.float32, device=kp.device)
    if out.numel() == 0:
        return out
    _lib.check(lib.flm_gaussian_heatmaps(_lib.stream_ptr(), _lib.ptr(kp), n, l, int(height), int(width),
                                         float(2 * sigma ** 2), _lib.ptr(out)), "flm_gaussian_heatmaps")
    return out


def _keypoints_on_device(keypoints):
    import torch
    if isinstance(keypoints, torch.Tensor):
        return keypoints if keypoints.is_cuda else keypoints.to(_lib.require_gpu()), False
    return torch.from_numpy(np.asarray(keypoints, dtype=np.float64)).to(_lib.require_gpu()), True


def gaussian_k(x0, y0, sigma, width, height):
    """data/generator.py:274-279: the [height, width] Gaussian centred at (x0, y0), x along the width, as the float32
    values generate_hm stores (the reference's float64 kernel rounded to float32)."""
    import torch
    kp = torch.tensor([[[float(x0), float(y0)]]], dtype=torch.float64, device=_lib.require_gpu())
    if float(x0) == -1.0 and float(y0) == -1.0:
        # the kernel's missing-point rule belongs to generate_hm (:292); gaussian_k itself draws the Gaussian
        # (the same integers shifted by one: c - (-1) == (c + 1) - 0 exactly)
        hm = gaussian_heatmaps_device(kp + 1.0, height + 1, width + 1, sigma)[0, 1:, 1:, 0]
        return hm.contiguous().cpu().numpy()
    return gaussian_heatmaps_device(kp, height, width, sigma)[0, :, :, 0].cpu().numpy()


def generate_hm(height, width, keypoints, s=3):
    """data/generator.py:282-296: keypoints [L,2] (x,y) -> float32 [height, width, L], one Gaussian per landmark, zeros
    for a keypoint equal to (-1,-1) (:292).  Also takes a batch [N,L,2] -> [N,height,width,L].  numpy in -> numpy out,
    CUDA tensor in -> CUDA tensor out.

    The reference passes (height, width) into gaussian_k's (width, height) slots (:293), so it only runs on square
    maps; here x runs along the width, as intended -- square maps equal the reference."""
    kp, was_np = _keypoints_on_device(keypoints)
    single = kp.dim() == 2
    hm = gaussian_heatmaps_device(kp[None] if single else kp, height, width, s)
    hm = hm[0] if single else hm
    return hm.cpu().numpy() if was_np else hm
