"""Heatmap -> (x, y) decode on the device: mirror of reference utils/metrics.py:46-109.

Same names and argument meaning.  The reference's `transfer_xy_coord` passes
`(n_points, thresh)` into `get_average_xy`'s `(height, width)` slots (:98), so as shipped
EVERY call decodes with n_points=4, thresh=0, whatever the caller passed.  Drop-in rule here:
  * a call that relies on the defaults -- `transfer_target(y)`, `transfer_xy_coord(hm)` -- returns
    what the reference returns (top-4, thresh 0);
  * a call that passes `n_points` / `thresh` explicitly gets what it asked for (the reference would
    silently ignore the arguments) and a one-time warning says so;
  * `as_shipped=True` forces the reference's behaviour, `as_shipped=False` the documented one.
Device limits: 1 <= n_points <= 128 in top-n mode (the reference's own sweep reaches 81, utils/metrics.py:130-133),
<= 96 landmarks per map.
"""
from __future__ import annotations

import warnings

import numpy as np

from .. import _lib

_UNSET = object()
_warned = False


def _resolve(n_points, thresh, as_shipped, dflt_n, dflt_t):
    """(n_points, thresh) a decode call runs with; see the module docstring."""
    global _warned
    explicit = n_points is not _UNSET or thresh is not _UNSET
    if as_shipped is None:
        as_shipped = not explicit
        if explicit and not _warned:
            _warned = True
            warnings.warn("flm_amd.utils.metrics: n_points / thresh are honoured here; the reference as shipped ignores "
                          "them and always decodes top-4 with thresh 0 (utils/metrics.py:98) -- pass as_shipped=True "
                          "for that behaviour", stacklevel=3)
    if as_shipped:
        return 4, 0
    return (dflt_n if n_points is _UNSET else n_points), (dflt_t if thresh is _UNSET else thresh)


def _check_workspace(workspace, nbytes, device):
    """A caller-owned `workspace=` of the decode wrappers: a contiguous uint8 tensor on the maps' device of at least
    `nbytes` bytes (the call's *_workspace_bytes) that starts at a 256-byte aligned address; what it held before does not
    matter (include/flm.h, the buffer contract).  ValueError otherwise."""
    import torch
    if (not isinstance(workspace, torch.Tensor) or workspace.dtype != torch.uint8 or workspace.dim() != 1
            or not workspace.is_contiguous()):
        raise ValueError("workspace must be a contiguous one-dimensional uint8 tensor")
    if workspace.numel() < nbytes:
        raise ValueError("workspace holds %d bytes, the call needs %d" % (workspace.numel(), nbytes))
    if workspace.data_ptr() % 256:
        raise ValueError("workspace must start at a 256-byte aligned address")
    if workspace.device != device:
        raise ValueError("workspace must lie on the maps' device %s (got %s)" % (device, workspace.device))
    return workspace


def _decode_workspace(workspace, nbytes, device):
    import torch
    if workspace is None:
        return torch.empty(max(nbytes, 256), dtype=torch.uint8, device=device)
    return _check_workspace(workspace, nbytes, device)


def decode_device(hm, n_points=4, thresh=0.0, out=None, workspace=None):
    """hm: CUDA float32 [N,H,W,L] contiguous -> CUDA float64 [N,L,2] (x,y).  `workspace`: a caller-owned scratch buffer
    (_check_workspace; flm_decode_workspace_bytes); None: allocated here, as ever."""
    import torch
    lib = _lib.load()
    if hm.dim() != 4 or hm.dtype != torch.float32 or not hm.is_cuda or not hm.is_contiguous():
        raise ValueError("decode_device needs a contiguous CUDA float32 [N,H,W,L] tensor")
    n, h, w, l = [int(v) for v in hm.shape]
    if n == 0:
        return torch.empty((0, l, 2), dtype=torch.float64, device=hm.device)
    mode, npts = (_lib.DECODE_ALL, 0) if n_points < 1 else (_lib.DECODE_TOPN, int(n_points))
    ws = _decode_workspace(workspace, lib.flm_decode_workspace_bytes(n, h, w, l, mode, npts), hm.device)
    if out is None:
        out = torch.empty((n, l, 2), dtype=torch.float64, device=hm.device)
    _lib.check(lib.flm_decode(_lib.stream_ptr(), _lib.ptr(hm), n, h, w, l, mode, npts, float(thresh),
                              _lib.ptr(out), _lib.ptr(ws), ws.numel()), "flm_decode")
    return out


def decode_stats_device(hm, n_points=4, thresh=0.0, out=None, workspace=None):
    """hm: CUDA float32 [N,H,W,L] contiguous -> CUDA float64 [N,L,6] landmark records (flm_decode_stats): per landmark
    x, y, score, var_x, var_y, cov_xy.  x, y are decode_device's bits; score is the mean selected value the reject test of
    utils/metrics.py:78-79 compares (the reference computes it and keeps only the verdict); the moments are the
    value-weighted spread of the selected pixels about (x, y) in px^2.  A rejected landmark reads (-1, -1, score, -1, -1, 0).
    `workspace`: as decode_device (flm_decode_stats_workspace_bytes)."""
    import torch
    lib = _lib.load()
    if hm.dim() != 4 or hm.dtype != torch.float32 or not hm.is_cuda or not hm.is_contiguous():
        raise ValueError("decode_stats_device needs a contiguous CUDA float32 [N,H,W,L] tensor")
    n, h, w, l = [int(v) for v in hm.shape]
    shape = (n, l, _lib.LANDMARK_REC)
    if out is None:
        out = torch.empty(shape, dtype=torch.float64, device=hm.device)
    elif tuple(out.shape) != shape or out.dtype != torch.float64 or not out.is_cuda or not out.is_contiguous():
        raise ValueError("out must be a contiguous CUDA float64 %s tensor" % (shape,))
    if n == 0:
        return out
    mode, npts = (_lib.DECODE_ALL, 0) if n_points < 1 else (_lib.DECODE_TOPN, int(n_points))
    ws = _decode_workspace(workspace, lib.flm_decode_stats_workspace_bytes(n, h, w, l, mode, npts), hm.device)
    _lib.check(lib.flm_decode_stats(_lib.stream_ptr(), _lib.ptr(hm), n, h, w, l, mode, npts, float(thresh),
                                    _lib.ptr(out), _lib.ptr(ws), ws.numel()), "flm_decode_stats")
    return out


def _to_device(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(_lib.require_gpu())


def get_average_xy(hmi, height=96, width=96, n_points=4, thresh=0):
    """utils/metrics.py:46-80.  `height`/`width` must equal the map's dims (the reference builds
    its index grids from them, :61-63); returns [x, y]."""
    hmi = np.asarray(hmi)
    if hmi.ndim != 2:
        raise ValueError("hmi must be 2-D")
    if n_points < 1 and tuple(hmi.shape) != (height, width):
        raise ValueError("height/width must equal hmi.shape in all-pixel mode (utils/metrics.py:61-63)")
    xy = decode_device(_to_device(hmi[None, :, :, None]), n_points, thresh).cpu().numpy()[0, 0]
    return [xy[0], xy[1]]


def transfer_xy_coord(hm, n_points=_UNSET, thresh=_UNSET, as_shipped=None):
    """utils/metrics.py:83-99 (documented defaults n_points=64, thresh=0.2): [H,W,L] -> list of 2L floats."""
    hm = np.asarray(hm)
    assert len(hm.shape) == 3
    n_points, thresh = _resolve(n_points, thresh, as_shipped, 64, 0.2)
    return list(transfer_target(hm[None], thresh, n_points, as_shipped=False)[0])


def transfer_target(y_pred, thresh=_UNSET, n_points=_UNSET, as_shipped=None):
    """utils/metrics.py:102-109 (documented defaults thresh=0, n_points=64): [N,H,W,L] -> float64 [N, 2L]."""
    n_points, thresh = _resolve(n_points, thresh, as_shipped, 64, 0)
    import torch
    if isinstance(y_pred, torch.Tensor):
        hm = y_pred if y_pred.is_cuda else y_pred.to(_lib.require_gpu())
        hm = hm.contiguous().float()
    else:
        hm = _to_device(np.asarray(y_pred))
    out = decode_device(hm, n_points, thresh)
    return out.reshape(out.shape[0], 2 * out.shape[1]).cpu().numpy()


def transfer_target_stats(y_pred, thresh=0, n_points=4):
    """transfer_target's maps -> the landmark records of decode_stats_device: [N,H,W,L] -> float64 [N,L,6].  numpy in ->
    numpy out, torch tensor in -> CUDA tensor out.  `thresh` and `n_points` are honoured as given (defaults: the decode
    the reference runs as shipped, top-4 with thresh 0)."""
    import torch
    was_np = not isinstance(y_pred, torch.Tensor)
    out = decode_stats_device(_maps_on_device(y_pred), n_points, thresh)
    return out.cpu().numpy() if was_np else out


def get_RMSE(y_pred_xy, y_train_xy, pick_not_NA):
    """utils/metrics.py:112-115 (host numpy, unchanged semantics)."""
    res = y_pred_xy[pick_not_NA] - y_train_xy[pick_not_NA]
    return np.sqrt(np.mean(res ** 2))


# ---- the n_points experiment (utils/metrics.py:1-37, :118-154) -------------------------------------------------------
SWEEP_N_POINTS = tuple(k * k for k in range(1, 10)) + (0,)   # `[nw * nw for nw in range(1, 10) + [0]]`, :129-131
RMSE_LABELS = ("(x,y) from est heatmap  VS (x,y) from true heatmap",
               "(x,y) from est heatmap  VS true (x,y)",
               "(x,y) from true heatmap VS true (x,y)")


def decode_sweep_device(hm, n_points_list, thresh=0.0, workspace=None):
    """hm: CUDA float32 [N,H,W,L] contiguous -> CUDA float64 [S,N,L,2]: slice s is decode_device(hm, n_points_list[s],
    thresh) (top-n bit for bit, all-pixel within 1e-9 px), every 16 modes from one read of the maps (flm_decode_sweep).
    `workspace`: as decode_device; it must hold flm_decode_sweep_workspace_bytes of every group of 16 modes."""
    import torch
    lib = _lib.load()
    if hm.dim() != 4 or hm.dtype != torch.float32 or not hm.is_cuda or not hm.is_contiguous():
        raise ValueError("decode_sweep_device needs a contiguous CUDA float32 [N,H,W,L] tensor")
    modes = [max(int(n), 0) for n in n_points_list]   # n_points < 1: all pixels, as decode_device
    if not modes:
        raise ValueError("n_points_list is empty")
    n, h, w, l = [int(v) for v in hm.shape]
    out = torch.empty((len(modes), n, l, 2), dtype=torch.float64, device=hm.device)
    if n == 0:
        return out
    for lo in range(0, len(modes), _lib.SWEEP_MAX_MODES):
        part = modes[lo:lo + _lib.SWEEP_MAX_MODES]
        arr = _lib.int_array(part)
        ws = _decode_workspace(workspace, lib.flm_decode_sweep_workspace_bytes(n, h, w, l, arr, len(part)), hm.device)
        _lib.check(lib.flm_decode_sweep(_lib.stream_ptr(), _lib.ptr(hm), n, h, w, l, arr, len(part), float(thresh),
                                        _lib.ptr(out[lo:lo + len(part)]), _lib.ptr(ws), ws.numel()), "flm_decode_sweep")
    return out


def _maps_on_device(y):
    import torch
    if isinstance(y, torch.Tensor):
        hm = y if y.is_cuda else y.to(_lib.require_gpu())
        return hm.contiguous().float()
    return _to_device(np.asarray(y))


def transfer_target_sweep(y_pred, n_points_list, thresh=0):
    """transfer_target(y_pred, thresh, n) for every n of `n_points_list` in one pass over the maps:
    [N,H,W,L] -> float64 [S, N, 2L].  numpy in -> numpy out, torch tensor in -> CUDA tensor out."""
    import torch
    was_np = not isinstance(y_pred, torch.Tensor)
    out = decode_sweep_device(_maps_on_device(y_pred), n_points_list, thresh)
    out = out.reshape(out.shape[0], out.shape[1], 2 * out.shape[2])
    return out.cpu().numpy() if was_np else out


def _masked_sq_sums(pred_xy, true_xy, actual_xy):
    """Per mode, over the coordinates the true heatmap decoded (`pick_not_NA = (y_train_xy != -1)`, :134): float64
    sums of the squared residuals of the three RMSEs and the count.  pred_xy / true_xy [S,N,2L], actual_xy [N,2L], all
    CUDA float64 -> ([S,3], [S]) on the device."""
    import torch
    pick = true_xy != -1
    act = actual_xy.unsqueeze(0)
    zero = torch.zeros((), dtype=torch.float64, device=pred_xy.device)
    sums = torch.stack([torch.where(pick, (pred_xy - true_xy) ** 2, zero).sum(dim=(1, 2)),
                        torch.where(pick, (pred_xy - act) ** 2, zero).sum(dim=(1, 2)),
                        torch.where(pick, (true_xy - act) ** 2, zero).sum(dim=(1, 2))], dim=1)
    return sums, pick.sum(dim=(1, 2))


def _rmse_table(sums, counts):
    """[S,3] float64 sums and [S] counts -> the [S,3] RMSE table (numpy; NaN where nothing was counted, as np.mean of
    an empty selection)."""
    s = sums.cpu().numpy()
    c = counts.cpu().numpy().astype(np.float64)[:, None]
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.sqrt(s / c)


def plot_keypoints_metric(res, n_points_list=SWEEP_N_POINTS, im_dim=(96, 96)):
    """What get_keypoints_metric draws (:147-153): the three RMSEs against sqrt(n_points), the all-pixel mode at
    im_dim[0]."""
    import matplotlib.pyplot as plt
    xs = [im_dim[0] if int(n) < 1 else float(np.sqrt(int(n))) for n in n_points_list]
    if list(n_points_list) == list(SWEEP_N_POINTS):
        xs = list(range(1, 10)) + [im_dim[0]]
    for i, lab in enumerate(RMSE_LABELS):
        plt.plot(xs, res[:, i], label=lab)
    plt.legend()
    plt.ylabel("RMSE")
    plt.xlabel("n_points")
    plt.show()


def get_keypoints_metric(ytrain_dist, ypred_dist, ytrain_actual, nimage=500, im_dim=(96, 96), plotting=True,
                         n_points_list=None):
    """utils/metrics.py:118-154: for n = 1, 4, ..., 81 and then 0 (all pixels) -- or `n_points_list` -- the three RMSEs
    of the module docstring (:17-20): est. heatmap vs true heatmap, est. heatmap vs true (x,y), true heatmap vs true
    (x,y), over the coordinates the true heatmap decodes (:134).  Returns the [S, 3] float64 table (the reference
    returns nothing; as shipped it cannot run on Python 3).  The maps are decoded with thresh 0 and the
    n asked for (the reference's docstring, not its argument slip at :98); each set of maps is read once
    (transfer_target_sweep) and the residual sums stay on the device in float64.
    ytrain_dist / ypred_dist: [N,H,W,L] maps; ytrain_actual: [N, 2L] true (x,y) in grid pixels."""
    import torch
    modes = list(SWEEP_N_POINTS if n_points_list is None else n_points_list)
    y_pred_xy = transfer_target_sweep(_maps_on_device(ypred_dist[:nimage]), modes, 0)
    y_train_xy = transfer_target_sweep(_maps_on_device(ytrain_dist[:nimage]), modes, 0)
    act = ytrain_actual[:nimage]
    act = (act.to(y_pred_xy.device) if isinstance(act, torch.Tensor)
           else torch.from_numpy(np.ascontiguousarray(act)).to(y_pred_xy.device)).to(torch.float64)
    if tuple(act.shape) != tuple(y_pred_xy.shape[1:]):
        raise ValueError("ytrain_actual must be [N, 2L] = %s, got %s" % (tuple(y_pred_xy.shape[1:]), tuple(act.shape)))
    sums, counts = _masked_sq_sums(y_pred_xy, y_train_xy, act)
    res = _rmse_table(sums, counts)
    for n in modes:   # (:143-144)
        print("n_points to evaluate (x,y) coordinates = {}".format(n))
        print(" RMSE")
    if plotting:
        plot_keypoints_metric(res, modes, im_dim)
    return res
