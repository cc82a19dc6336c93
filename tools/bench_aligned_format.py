"""Aligned faces in the consumer's format: the conversion in the warp's store against the torch chain behind the warp.

The set-up of tools/bench_align_frames.py (same seed): an 8-slot 1080p ring, 505 faces of 96..400 px, aligned size
112x112, once with matrices that fit each face box onto the aligned square (what a trained model gives) and once with
the matrices the pipeline produces on synthetic weights (degenerate fits).  One process, the variants ALTERNATING window
by window, HIP events around each window of back-to-back launches:

  A, A2   alignment.warp_frames_device, float32 NHWC BGR, alone (the pair gives the run-to-run spread)
  A'      A followed by the chain every caller writes today for a face-embedding network:
          permute(0,3,1,2).flip(1).mul(1/127.5).add(-1).to(float16)
  B_*     warp_frames_device(..., fmt=...): matcher float16, matcher bfloat16, uint8 NHWC, float32 NCHW

Per row: median, min and max of the windows, the byte model (source: side^2 * 3 B per face, as bench_align_frames
counts it; destination: 112*112*3 elements of the type's size; for A' also the chain's reads and writes) and GB/s by
that model.  The gate: every B row is faster than A' by more than the A-against-A2 spread.  B against A is reported, not
gated.  Writes the record to --out and prints it as one JSON line; exits 1 when the gate fails.

    python tools/bench_aligned_format.py
    rocprofv3 --kernel-trace --stats ... -- python tools/bench_aligned_format.py --trace
                                     # a fixed count of each variant, no events: kernel times, in a run of its own
"""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

import flm_amd  # noqa: F401
from flm_amd import alignment, prediction
from flm_amd.alignment import AlignedFormat
from flm_amd.networks import LANDMARKS_MODELS
from flm_amd.weights import synth_fcn8_weights

from bench_align_frames import OUT, box_fit_matrices, event_ms, stats, workload

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def pipeline_matrices(frames, faces, slots):
    model = LANDMARKS_MODELS["fcn_8"](68, input_height=256, input_width=256, dtype="bf16")
    model.load_weights(synth_fcn8_weights(68, seed=2))
    m = prediction.align_frames(frames, faces, model, out_size=(OUT, OUT), n_points=4, frame_index=slots)[1].clone()
    torch.cuda.synchronize()
    del model
    return m


def variants(frames, m, idx_dev, boxes_dev, k):
    """[(name, fn, destination bytes of the byte model)]; every variant writes into buffers allocated once."""
    f32_dst = torch.empty((k, OUT, OUT, 3), dtype=torch.float32, device="cuda")
    npix3 = k * OUT * OUT * 3
    scale, bias = 1.0 / 127.5, -1.0

    def warp(fmt=None, out=None):
        return alignment.warp_frames_device(frames, m, OUT, OUT, frame_index_dev=idx_dev, boxes_dev=boxes_dev,
                                            out=out, fmt=fmt)

    def plain():
        return warp(out=f32_dst)

    def chain():
        return warp(out=f32_dst).permute(0, 3, 1, 2).flip(1).mul(scale).add(bias).to(torch.float16)

    # the chain: flip reads and writes float32, mul and add each read and write float32, the cast reads float32 and
    # writes float16 (permute is a view) -- on top of the warp's own float32 write
    chain_bytes = npix3 * (4 + (4 + 4) * 3 + (4 + 2))
    rows = [("A", plain, npix3 * 4), ("A_chain", chain, chain_bytes)]
    for name, fmt in (("B_matcher_f16", AlignedFormat.matcher("float16")),
                      ("B_matcher_bf16", AlignedFormat.matcher("bfloat16")),
                      ("B_u8_nhwc", AlignedFormat("nhwc", "uint8")),
                      ("B_f32_nchw", AlignedFormat("nchw", "float32"))):
        dst = torch.empty(fmt.shape(k, OUT, OUT), dtype=fmt.torch_dtype, device="cuda")
        rows.append((name, lambda fmt=fmt, dst=dst: warp(fmt, dst), fmt.nbytes(k, OUT, OUT)))
    rows.insert(2, ("A2", plain, npix3 * 4))
    # what is timed is what the tests hold: the matcher tensor of the new call equals the chain's on this workload
    got = warp(AlignedFormat.matcher("float16"))
    exp = chain()
    same = bool(torch.equal(got.view(torch.int16), exp.contiguous().view(torch.int16)))
    return rows, same


def measure(rows, src_bytes, windows, window_ms, trace):
    for _, fn, _ in rows:            # every shape of the timed windows, warmed
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    if trace:
        for _, fn, _ in rows:
            for _ in range(trace):
                fn()
        torch.cuda.synchronize()
        return {"launches_of_each": trace}
    reps = {name: max(10, int(math.ceil(window_ms / event_ms(fn, 10)))) for name, fn, _ in rows}
    times = {name: [] for name, _, _ in rows}
    for _ in range(windows):
        for name, fn, _ in rows:
            times[name].append(event_ms(fn, reps[name]))
    res = {"windows": windows, "launches_per_window": reps}
    for name, _, dst_bytes in rows:
        r = stats(times[name])
        r["bytes_model"] = {"source": src_bytes, "destination": dst_bytes}
        r["gb_per_s"] = (src_bytes + dst_bytes) / r["median_ms"] / 1e6
        res[name] = r
    both = times["A"] + times["A2"]
    spread = max(abs(res["A2"]["median_ms"] - res["A"]["median_ms"]), max(both) - min(both))
    res["spread_A_vs_A2_ms"] = {"median_diff": res["A2"]["median_ms"] - res["A"]["median_ms"],
                                "window_range": max(both) - min(both), "used": spread}
    a, ac = res["A"]["median_ms"], res["A_chain"]["median_ms"]
    gate = True
    for name, _, _ in rows:
        if name.startswith("B_"):
            res[name]["vs_A_ms"] = res[name]["median_ms"] - a
            res[name]["vs_A_chain_ms"] = res[name]["median_ms"] - ac
            res[name]["faster_than_A_chain_by_more_than_spread"] = bool(ac - res[name]["median_ms"] > spread)
            res[name]["slower_than_A_by_more_than_spread"] = bool(res[name]["median_ms"] - a > spread)
            gate = gate and res[name]["faster_than_A_chain_by_more_than_spread"]
    res["gate_every_B_faster_than_A_chain"] = gate
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=9, help="alternating timed windows per variant (at least 7)")
    ap.add_argument("--window-ms", type=float, default=60.0, help="least length of one timed window")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "aligned_format_bench.json"))
    ap.add_argument("--trace", type=int, nargs="?", const=50, default=0, metavar="LAUNCHES",
                    help="run LAUNCHES launches of every variant after the warm-up and nothing else (for a kernel trace)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_aligned_format: no GPU visible (there is nothing to measure on a CPU)")
    if args.windows < 7:
        sys.exit("bench_aligned_format: at least 7 windows")
    frames, faces, slots = workload()
    _, _, boxes_dev, idx_dev = prediction.crop_frames_device(frames, faces, 256, 256, frame_index=slots, return_device=True)
    boxes = boxes_dev.cpu().numpy()
    k = boxes.shape[0]
    side = (boxes[:, 2] - boxes[:, 0]).astype(np.int64)
    src_bytes = int((side * side * 3).sum())
    rec = {"bench": "aligned_format", "device": torch.cuda.get_device_name(0), "faces": k, "out_size": [OUT, OUT],
           "timing": "HIP events around windows of back-to-back launches, variants alternating window by window"}
    sets = [("box_fit_m", box_fit_matrices(boxes, np.random.default_rng(7))[0]),
            ("pipeline_m", pipeline_matrices(frames, faces, slots))]
    ok = True
    for tag, m in sets:
        rows, same = variants(frames, m, idx_dev, boxes_dev, k)
        rec[tag] = measure(rows, src_bytes, args.windows, args.window_ms, args.trace)
        rec[tag]["matcher_f16_equals_chain_bitwise"] = same
        ok = ok and (bool(args.trace) or rec[tag]["gate_every_B_faster_than_A_chain"])
    if not args.trace:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
    print(json.dumps(rec), flush=True)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
