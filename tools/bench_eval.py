#!/usr/bin/env python3
"""Developer tool: the evaluation path on 264x264x68 maps.

At batch 64 and 512, in one process and alternating round by round (so that clock and thermal drift fall on every
variant alike): the ten-mode sweep (n = 1, 4, ..., 81, 0) in one flm_decode_sweep against the ten separate flm_decode
calls and against the single n = 81 call; flm_gaussian_heatmaps as TB/s of bytes written; and evaluate() in faces/s
(fcn_8 at 256x256 input, synthetic weights, batch 64).  Device events, warm-up first, the median of the rounds.

    python tools/bench_eval.py [--rounds 7] [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import flm_amd  # noqa: E402,F401
from flm_amd.data import generator  # noqa: E402
from flm_amd.utils import metrics  # noqa: E402

SWEEP = list(metrics.SWEEP_N_POINTS)


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--batches", default="64,512")
    ap.add_argument("--json")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    res = {}
    for n in [int(b) for b in args.batches.split(",")]:
        g = torch.Generator(device="cuda").manual_seed(n)
        hm = torch.rand((n, 264, 264, 68), device="cuda", generator=g)
        kp = torch.rand((n, 68, 2), device="cuda", dtype=torch.float64, generator=g) * 263.0
        out = torch.empty((n, 264, 264, 68), device="cuda")
        variants = {
            "sweep10": lambda: metrics.decode_sweep_device(hm, SWEEP),
            "separate10": lambda: [metrics.decode_device(hm, m) for m in SWEEP],
            "single81": lambda: metrics.decode_device(hm, 81),
            "gaussian": lambda: generator.gaussian_heatmaps_device(kp, 264, 264),
        }
        for f in variants.values():   # warm-up (compiles nothing: first-launch and allocator costs)
            f()
        torch.cuda.synchronize()
        times = {k: [] for k in variants}
        for _ in range(args.rounds):
            for k, f in variants.items():
                times[k].append(timed(f, args.reps))
        med = {k: statistics.median(v) for k, v in times.items()}
        nbytes = n * 264 * 264 * 68 * 4
        res["batch%d" % n] = {
            "sweep10_ms": med["sweep10"], "separate10_ms": med["separate10"], "single81_ms": med["single81"],
            "sweep_vs_separate": med["separate10"] / med["sweep10"], "sweep_vs_single81": med["sweep10"] / med["single81"],
            "gaussian_ms": med["gaussian"], "gaussian_TBps": nbytes / med["gaussian"] / 1e9,
            "sweep_read_TBps": nbytes / med["sweep10"] / 1e9,
        }
        del hm, out
        torch.cuda.empty_cache()
    # evaluate() end to end: fcn_8, 256x256 crops (264x264 output grid), batch 64, from arrays
    from flm_amd import evaluation
    from flm_amd.networks import LANDMARKS_MODELS
    from flm_amd.weights import synth_fcn8_weights
    model = LANDMARKS_MODELS["fcn_8"](68, input_height=256, input_width=256)
    model.load_weights(synth_fcn8_weights(68, seed=2))
    rng = np.random.default_rng(0)
    nimg = 256
    images = [rng.integers(0, 256, (256, 256, 3), dtype=np.uint8) for _ in range(nimg)]
    kps = rng.uniform(0, 255, (nimg, 68, 2))
    evaluation.evaluate(model, images=images[:64], keypoints=kps[:64], batch_size=64)
    torch.cuda.synchronize()
    walls = []
    for _ in range(3):
        t0 = time.perf_counter()
        evaluation.evaluate(model, images=images, keypoints=kps, batch_size=64)
        torch.cuda.synchronize()
        walls.append(time.perf_counter() - t0)
    res["evaluate_fcn8_256_batch64"] = {"faces": nimg, "s": statistics.median(walls),
                                        "faces_per_s": nimg / statistics.median(walls)}
    for k, v in res.items():
        print(k, json.dumps(v))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
