"""The frame-space tail against today's crop-space tail on the multi-face stream (BASELINE configs[4], the workload of
`bench.py --config 5`: an 8-slot 1080p ring, 64 frames, 1..16 boxes of 96..400 px per frame, same seed), one process,
the variants ALTERNATING round by round, HIP events around whole steps:

  A   crop_frames_device -> landmarks -> alignment.align_device(crops -> 112x112)      (run twice per round: A and A2,
      whose difference is the run-to-run spread every other difference is read against)
  B1, B2, B4   prediction.align_frames(..., out_size=(112, 112), samples=1 | 2 | 4)

then the two warps alone, back to back as bench.py's hbm_kernels block times the existing one, with the bytes of the
shape model (existing: 196,608 B read + 150,528 B written per face; frames: side^2 * 3 B read + 150,528 B written) over
the mean launch time -- once with the matrices the pipeline produced (synthetic weights: degenerate fits) and once with
matrices that map each face box onto the aligned square with a small rotation (what a trained model would give).
Prints one JSON line.

    python tools/bench_align_frames.py                 # fp32 and bf16
    python tools/bench_align_frames.py --warps-only    # the warps alone
    rocprofv3 --kernel-trace --stats ... -- python tools/bench_align_frames.py --trace --dtypes bf16
                                                       # the same steps, a fixed count of each, no events: per-kernel
                                                       # times inside the step (a run of its own: tracing slows the host)
"""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import flm_amd  # noqa: F401
from flm_amd import alignment, prediction
from flm_amd.networks import LANDMARKS_MODELS
from flm_amd.weights import synth_fcn8_weights

OUT = 112
PEAK_HBM_GBS = 8000.0


def workload(n_frames=64, seed=5):
    rng = np.random.default_rng(seed)
    frames = torch.from_numpy(rng.integers(0, 256, (8, 1080, 1920, 3), dtype=np.uint8)).cuda()
    faces = []
    for _ in range(n_frames):
        fb = []
        for _ in range(int(rng.integers(1, 17))):
            side = int(rng.integers(96, 401))
            x0, y0 = int(rng.integers(0, 1920 - side)), int(rng.integers(0, 1080 - side))
            fb.append((x0, y0, x0 + side, y0 + side))
        faces.append(fb)
    return frames, faces, [f % 8 for f in range(n_frames)]


def event_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def stats(v):
    v = sorted(v)
    return {"median_ms": v[len(v) // 2], "min_ms": v[0], "max_ms": v[-1]}


def pipelines(dtype, frames, faces, slots, rounds, window_ms, trace_steps=0):
    model = LANDMARKS_MODELS["fcn_8"](68, input_height=256, input_width=256, dtype=dtype)
    model.load_weights(synth_fcn8_weights(68, seed=2))
    tmpl = torch.from_numpy(alignment.canonical_template(68, OUT, OUT)).cuda()
    scale = (256 / model.output_width, 256 / model.output_height)

    def crop_space():
        crops, _ = prediction.crop_frames_device(frames, faces, 256, 256, frame_index=slots)
        lm = model.forward_device(crops, "landmarks", n_points=4)
        return alignment.align_device(crops, lm, tmpl, OUT, OUT, scale)

    def frame_space(s):
        return lambda: prediction.align_frames(frames, faces, model, out_size=(OUT, OUT), n_points=4, frame_index=slots,
                                               samples=s)

    variants = [("A", crop_space), ("B1", frame_space(1)), ("A2", crop_space), ("B2", frame_space(2)), ("B4", frame_space(4))]
    for _, fn in variants:           # every shape of the timed windows, twice
        fn()
        fn()
    torch.cuda.synchronize()
    if trace_steps:
        for name, fn in variants:
            if name != "A2":
                for _ in range(trace_steps):
                    fn()
        torch.cuda.synchronize()
        return {"steps_of_each": trace_steps, "faces_per_step": sum(len(f) for f in faces)}, None, None
    reps = max(2, int(math.ceil(window_ms / event_ms(crop_space, 2))))
    times = {name: [] for name, _ in variants}
    for _ in range(rounds):
        for name, fn in variants:
            times[name].append(event_ms(fn, reps))
    k = sum(len(f) for f in faces)
    res = {"faces_per_step": k, "steps_per_window": reps, "windows": rounds}
    for name in times:
        res[name] = stats(times[name])
        res[name]["faces_per_s"] = 1e3 * k / res[name]["median_ms"]
    a = res["A"]["median_ms"]
    res["spread_A_vs_A2"] = {"median_diff_ms": res["A2"]["median_ms"] - a,
                             "window_range_ms": max(times["A"] + times["A2"]) - min(times["A"] + times["A2"])}
    for name in ("B1", "B2", "B4"):
        res[name]["vs_A_ms"] = res[name]["median_ms"] - a
        res[name]["vs_A_rel"] = res[name]["median_ms"] / a - 1.0
    m_crop = crop_space()[1].clone()
    m_frame = frame_space(1)()[1].clone()
    del model
    return res, m_crop, m_frame


def box_fit_matrices(boxes, rng):
    """Each face box onto the aligned square, rotated by up to 0.2 rad about its centre: frame px -> aligned px, and the
    same geometry in the pixels of the 256x256 crop."""
    k = boxes.shape[0]
    mf, mc = np.zeros((k, 2, 3), np.float32), np.zeros((k, 2, 3), np.float32)
    for i in range(k):
        th = rng.uniform(-0.2, 0.2)
        side = float(boxes[i, 2] - boxes[i, 0])
        for out, s, cx, cy in ((mf, OUT / side, boxes[i, 0] + side / 2, boxes[i, 1] + side / 2), (mc, OUT / 256.0, 128.0, 128.0)):
            a, b = s * np.cos(th), s * np.sin(th)
            out[i] = [[a, -b, OUT / 2 - (a * cx - b * cy)], [b, a, OUT / 2 - (b * cx + a * cy)]]
    return torch.from_numpy(mf).cuda(), torch.from_numpy(mc).cuda()


def warps_alone(frames, faces, slots, m_crop, m_frame, reps=20):
    crops, _, boxes_dev, idx_dev = prediction.crop_frames_device(frames, faces, 256, 256, frame_index=slots, return_device=True)
    boxes = boxes_dev.cpu().numpy()
    k = boxes.shape[0]
    side = (boxes[:, 2] - boxes[:, 0]).astype(np.int64)
    bytes_crop = k * (256 * 256 * 3 + OUT * OUT * 12)
    bytes_frame = int((side * side * 3).sum()) + k * OUT * OUT * 12
    fit_f, fit_c = box_fit_matrices(boxes, np.random.default_rng(7))
    dst = torch.empty((k, OUT, OUT, 3), dtype=torch.float32, device="cuda")
    out = {"faces": k, "bytes_model": {"warp_crops": bytes_crop, "warp_frames": bytes_frame}}
    sets = [("box_fit_m", fit_c, fit_f)]
    if m_crop is not None:
        sets.append(("pipeline_m", m_crop, m_frame))
    for tag, mc, mf in sets:
        # frame px -> aligned px scale of the matrices, relative to the box-to-aligned-square scale 112 / side
        rel = (torch.linalg.norm(mf[:, :, 0], dim=1).cpu().numpy() * side / OUT)
        out[tag + "_scale_vs_box_fit"] = {"median": float(np.median(rel)), "min": float(rel.min()), "max": float(rel.max())}
        runs = [("warp_crops", bytes_crop, lambda: alignment.warp_device(crops, mc, OUT, OUT, out=dst))]
        for s in (1, 2, 4):
            runs.append(("warp_frames_s%d" % s, bytes_frame,
                         lambda s=s: alignment.warp_frames_device(frames, mf, OUT, OUT, frame_index_dev=idx_dev,
                                                                  boxes_dev=boxes_dev, samples=s, out=dst)))
        rec = {}
        for name, nbytes, fn in runs:
            fn()
            torch.cuda.synchronize()
            ms = min(event_ms(fn, reps) for _ in range(3))
            rec[name] = {"avg_launch_ms": ms, "gb_per_s": nbytes / ms / 1e6, "frac_of_8tb_s": nbytes / ms / 1e6 / PEAK_HBM_GBS}
        out[tag] = rec
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtypes", default="f32,bf16")
    ap.add_argument("--rounds", type=int, default=7, help="alternating rounds (timed windows per variant)")
    ap.add_argument("--window-ms", type=float, default=300.0, help="least length of one timed window")
    ap.add_argument("--warps-only", action="store_true")
    ap.add_argument("--trace", type=int, nargs="?", const=10, default=0, metavar="STEPS",
                    help="run STEPS steps of A, B1, B2 and B4 after the warm-up and nothing else (for a kernel trace)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_align_frames: no GPU visible (there is nothing to measure on a CPU)")
    frames, faces, slots = workload()
    rec = {"bench": "align_frames", "device": torch.cuda.get_device_name(0), "out_size": [OUT, OUT]}
    m_crop = m_frame = None
    if not args.warps_only:
        for dt in args.dtypes.split(","):
            rec["stream_" + dt], mc, mf = pipelines(dt, frames, faces, slots, args.rounds, args.window_ms, args.trace)
            if m_crop is None:
                m_crop, m_frame = mc, mf
    if args.trace:
        print(json.dumps(rec), flush=True)
        return
    rec["warps_alone"] = warps_alone(frames, faces, slots, m_crop, m_frame)
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
