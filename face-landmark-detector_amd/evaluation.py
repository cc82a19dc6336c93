"""Landmark evaluation on labelled faces: the reference's n_points experiment (utils/metrics.py:1-37, :118-154) run
end to end.  The reference's `keypoints_detector/evaluation.py` is an empty placeholder; this fills it.

`evaluate(model, images_path, keypts_path)` reads image / `.pts` pairs (data/generator.py:82-160), or takes arrays,
and per batch of faces: resizes the BGR images to the model input on the device, runs the forward to probabilities,
maps the labelled points to output-grid pixels, draws the Gaussian target maps (generate_hm, sigma 3), decodes both
sets of maps at every n of the sweep in one pass each (flm_decode_sweep), and accumulates the squared residuals of the
three RMSEs in float64 on the device.  The result names the n with the smallest RMSE against the labels.
"""
from __future__ import annotations

import dataclasses

import numpy as np

from . import _lib
from .data import generator
from .utils import metrics


@dataclasses.dataclass
class EvaluationResult:
    """modes: the n_points of each row (0 = all pixels); rmse: float64 [S, 3], columns as metrics.RMSE_LABELS;
    best_n_points: the mode with the smallest RMSE of the predicted points against the labels (column 1);
    n_images: faces evaluated; n_counted: int64 [S], coordinates counted per mode (those the true heatmap decodes)."""
    modes: tuple
    rmse: np.ndarray
    best_n_points: int
    n_images: int
    n_counted: np.ndarray

    def __str__(self):
        rows = ["n_points  " + "  ".join("RMSE%d" % (i + 1) for i in range(3))]
        for n, r in zip(self.modes, self.rmse):
            rows.append("%8d  %s" % (n, "  ".join("%.4f" % v for v in r)))
        rows.append("best n_points (RMSE2): %d over %d faces" % (self.best_n_points, self.n_images))
        return "\n".join(rows)


def _load_dir(images_path, keypts_path, ignore_non_matching):
    pairs = sorted(generator.get_pairs_from_paths(images_path, keypts_path, ignore_non_matching))
    images, keypoints = [], []
    for img_path, kp_path in pairs:
        images.append(generator.imread_bgr(img_path))
        kp, n_points, _ = generator.read_keypoints(kp_path)
        if n_points is not None and kp.shape[0] != n_points:
            raise generator.DataLoaderError("%s: n_points %d but %d points" % (kp_path, n_points, kp.shape[0]))
        keypoints.append(kp)
    return images, keypoints


def _grid_keypoints(kp, h_img, w_img, model):
    """image pixels -> output-grid pixels (x * W'/w_img, y * H'/h_img: the inverse of predict(to_input_space=True));
    a missing point, (-1,-1), stays (-1,-1)."""
    kp = np.asarray(kp, dtype=np.float64)
    missing = np.all(kp == -1.0, axis=1, keepdims=True)
    scaled = kp * np.array([model.output_width / w_img, model.output_height / h_img])
    return np.where(missing, -1.0, scaled)


def evaluate(model, images_path=None, keypts_path=None, *, images=None, keypoints=None, batch_size=64,
             n_points_list=metrics.SWEEP_N_POINTS, sigma=3, thresh=0.0, ignore_non_matching=False):
    """RMSE of `model`'s landmarks for every n of `n_points_list` (see the module docstring).

    Either a directory pair (`images_path` with .jpg/.jpeg/.png/.bmp files, `keypts_path` with .pts files of the same
    stems) or arrays: `images` a sequence of BGR uint8 [h,w,3] images of any size, `keypoints` float64 [N, L, 2] (x,y)
    in image pixels, (-1,-1) for a missing point.  L must equal model.n_classes."""
    import torch
    if images_path is not None or keypts_path is not None:
        if images is not None or keypoints is not None:
            raise ValueError("pass a directory pair or arrays, not both")
        if images_path is None or keypts_path is None:
            raise ValueError("images_path and keypts_path go together")
        images, keypoints = _load_dir(images_path, keypts_path, ignore_non_matching)
    if images is None or keypoints is None:
        raise ValueError("nothing to evaluate: give images_path/keypts_path or images/keypoints")
    if len(images) != len(keypoints):
        raise ValueError("%d images but %d keypoint sets" % (len(images), len(keypoints)))
    if len(images) == 0:
        raise ValueError("no labelled images")
    for k in keypoints:
        if np.shape(k) != (model.n_classes, 2):
            raise ValueError("No of Keypoint not equivalent to model configurations: %s points for n_classes=%d"
                             % (np.shape(k), model.n_classes))   # data/generator.py:517
    modes = tuple(int(n) for n in n_points_list)
    if batch_size < 1:
        raise ValueError("batch_size must be >= 1")
    dev = _lib.require_gpu()
    ih, iw = model.input_height, model.input_width
    oh, ow, l = model.output_height, model.output_width, model.n_classes
    sums = torch.zeros((len(modes), 3), dtype=torch.float64, device=dev)
    counts = torch.zeros((len(modes),), dtype=torch.int64, device=dev)
    for lo in range(0, len(images), batch_size):
        batch = images[lo:lo + batch_size]
        x = torch.empty((len(batch), ih, iw, 3), dtype=torch.uint8, device=dev)
        kp = np.empty((len(batch), l, 2), np.float64)
        for j, img in enumerate(batch):
            img = np.asarray(img)
            if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
                raise ValueError("images must be BGR uint8 [h,w,3]")
            x[j] = generator.resize_u8_device(torch.from_numpy(np.ascontiguousarray(img)).to(dev), ih, iw)
            kp[j] = _grid_keypoints(keypoints[lo + j], img.shape[0], img.shape[1], model)
        probs = model.forward_device(x, "probs").view(len(batch), oh, ow, l)
        kp_dev = torch.from_numpy(kp).to(dev)
        true_maps = generator.gaussian_heatmaps_device(kp_dev, oh, ow, sigma)
        pred_xy = metrics.transfer_target_sweep(probs, modes, thresh)
        true_xy = metrics.transfer_target_sweep(true_maps, modes, thresh)
        s, c = metrics._masked_sq_sums(pred_xy, true_xy, kp_dev.reshape(len(batch), 2 * l))
        sums += s
        counts += c
    rmse = metrics._rmse_table(sums, counts)
    best = modes[int(np.nanargmin(rmse[:, 1]))] if np.isfinite(rmse[:, 1]).any() else modes[0]
    return EvaluationResult(modes=modes, rmse=rmse, best_n_points=best, n_images=len(images),
                            n_counted=counts.cpu().numpy())
