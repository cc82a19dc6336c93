"""The best-shot calls against what a caller pays without them (the protocol of tools/bench_track.py: one process, the
variants ALTERNATING round by round, HIP events around whole windows, median and range over the windows).

  calls    at 16 and at 512 float16 [K,3,112,112] faces in the matcher's format:
             Q   flm_face_quality (two launches): reads the K faces once -> bytes = K * 75,264
             B   flm_track_best_update with EVERY slot taken (best_q_in = -1; the worst case): reads and writes the K
                 faces -> bytes = 2 * K * 75,264; B0: the same call with no slot taken (best_q_in = +inf)
             T   the torch expression a user would otherwise write, on the device: de-normalise, luma, a conv2d
                 Laplacian, its variance, a comparison and a torch.where copy into the gallery
           The fraction of the HBM rate is bytes / time over --hbm-gbs (8 TB/s, the figure DESIGN.md uses throughout).  Windows
           hold thousands of back-to-back calls: at 16 faces the time per call is launch-bound.
  step     FaceTracker.step at capacity 16 on a 1080p BGR ring, fcn_8 with 256x256 input, bf16, the matcher's format,
           put back to the seeded state before every step as tools/bench_track.py does: P plain, S with best_shot=True,
           P2 plain again (the spread), and W the aligned warp alone on the same matrices.

Prints one JSON line, and writes it to --out.

    python tools/bench_best_shot.py --out profiles/best_shot.json
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import flm_amd  # noqa: F401
from flm_amd import _lib, alignment, prediction
from flm_amd.networks import LANDMARKS_MODELS
from flm_amd.weights import synth_fcn8_weights

import bench_track as bt

OUT, C_PTS = 112, 68
FACE_BYTES = 3 * OUT * OUT * 2


def torch_expression(faces, best_var, gallery, lap_kernel, wy):
    """What a user writes without the library: float32 luma, a conv2d Laplacian, its variance, keep where better."""
    x = (faces.float() + 1.0) * 127.5                                   # [K,3,h,w] RGB
    y = (x * wy).sum(1, keepdim=True)
    lap = torch.nn.functional.conv2d(y, lap_kernel)
    var = lap.var(dim=(1, 2, 3), unbiased=False)
    take = var > best_var
    gallery.copy_(torch.where(take[:, None, None, None], faces, gallery))
    best_var.copy_(torch.where(take, var, best_var))


def calls(k, rounds, window_ms, hbm_gbs):
    g = torch.Generator(device="cuda")
    g.manual_seed(k)
    fmt = alignment.AlignedFormat.matcher()
    raw = torch.randint(0, 256, (k, 3, OUT, OUT), device="cuda", generator=g).float()
    faces = (raw * (1.0 / 127.5) - 1.0).to(torch.float16)
    rec = torch.empty((k, 8), dtype=torch.int64, device="cuda")
    lm = torch.rand((k, C_PTS, 2), dtype=torch.float64, device="cuda") * 100
    w = torch.rand((k, C_PTS), dtype=torch.float64, device="cuda")
    m = torch.zeros((k, 2, 3), dtype=torch.float32, device="cuda")
    none = torch.full((k,), -1.0, dtype=torch.float64, device="cuda")
    full = torch.full((k,), float("inf"), dtype=torch.float64, device="cuda")
    q_out = torch.empty_like(none)
    gallery, bframe = torch.zeros_like(faces), torch.zeros((k,), dtype=torch.int64, device="cuda")
    bm, blm, brec = torch.zeros_like(m), torch.zeros_like(lm), torch.zeros_like(rec)
    alignment.face_quality_device(faces, fmt, out=rec)

    def q():
        alignment.face_quality_device(faces, fmt, out=rec)

    def upd(q_in):
        def fn():
            alignment.track_best_update_device(faces, rec, lm, q_in, q_out, gallery, bframe, 1, weights=w, m=m, best_m=bm,
                                               best_lm=blm, best_rec=brec)
        return fn

    lap_kernel = torch.tensor([[0, 1, 0], [1, -4, 1], [0, 1, 0]], dtype=torch.float32, device="cuda").view(1, 1, 3, 3)
    wy = torch.tensor([0.299, 0.587, 0.114], dtype=torch.float32, device="cuda").view(1, 3, 1, 1)
    t_gallery, t_best = torch.zeros_like(faces), torch.zeros((k,), dtype=torch.float32, device="cuda")

    def t():
        t_best.fill_(-1.0)
        torch_expression(faces, t_best, t_gallery, lap_kernel, wy)

    res = bt.alternate([("Q", q), ("B", upd(none)), ("B0", upd(full)), ("T", t), ("Q2", q)], rounds, window_ms)
    upd(none)()
    torch.cuda.synchronize()
    res["all_taken"] = bool((q_out >= 0).all()) and bool(torch.equal(gallery, faces))
    res["faces"] = k
    for name, nbytes in (("Q", k * FACE_BYTES), ("B", 2 * k * FACE_BYTES)):
        gbs = nbytes / (res[name]["median_ms"] * 1e-3) / 1e9
        res[name]["contract_bytes"] = nbytes
        res[name]["gb_per_s"] = gbs
        res[name]["fraction_of_hbm"] = gbs / hbm_gbs
    return res


def step(rounds, window_ms, k=16):
    model = LANDMARKS_MODELS["fcn_8"](C_PTS, input_height=256, input_width=256, dtype="bf16")
    model.load_weights(synth_fcn8_weights(C_PTS, seed=2))
    ring, ff = bt.rings()["bgr"]
    faces = bt.boxes_for(k, 11 + k)
    fmt = alignment.AlignedFormat.matcher()
    state = {"t": 0}

    def stepper(**kw):
        tr = prediction.FaceTracker(model, (bt.FH, bt.FW), k, out_size=(OUT, OUT), aligned_format=fmt, frame_format=ff, **kw)
        tr.seed(range(k), faces)
        m0, b0 = tr.m_crop.clone(), tr.boxes.clone()

        def fn():
            tr.m_crop.copy_(m0)
            tr.boxes.copy_(b0)
            state["t"] += 1
            return tr.step(ring, state["t"] % 8)
        return tr, fn

    tp, p = stepper()
    ts, s = stepper(best_shot=True)
    m_align = p()[1].clone()
    idx = torch.zeros((k,), dtype=torch.int32, device="cuda")
    boxes = tp.boxes.clone()
    out = torch.empty(fmt.shape(k, OUT, OUT), dtype=torch.float16, device="cuda")

    def warp():
        alignment.warp_frames_device(ring, m_align, OUT, OUT, frame_index_dev=idx, boxes_dev=boxes, fmt=fmt, out=out)

    res = bt.alternate([("P", p), ("S", s), ("W", warp), ("P2", p)], rounds, window_ms)
    res["faces"] = k
    res["S_vs_P_ms"] = res["S"]["median_ms"] - res["P"]["median_ms"]
    res["spread_P_vs_P2_ms"] = res["P2"]["median_ms"] - res["P"]["median_ms"]
    res["slots_with_a_best"] = int((ts.best()[1] >= 0).sum())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=200.0)
    ap.add_argument("--hbm-gbs", type=float, default=8000.0, help="the HBM rate the fractions refer to, GB/s (8 TB/s, as DESIGN.md)")
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    _lib.require_gpu()
    res = {"calls": {str(k): calls(k, a.rounds, a.window_ms, a.hbm_gbs) for k in (16, 512)}, "hbm_gbs": a.hbm_gbs,
           "face_bytes": FACE_BYTES}
    if not a.skip_step:
        res["step"] = step(a.rounds, a.window_ms)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
