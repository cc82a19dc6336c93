"""A tick on which only some cameras delivered: FaceTracker.step of all streams against FaceTracker.step_active of A of
them (the protocol of tools/bench_track_streams.py: one process, the variants ALTERNATING window by window, 5 windows of
at least 200 ms each, median and [min, max] over the windows; HIP events around whole windows).

Workload: the table row of DESIGN 4.5h -- fcn_8 at 256x256 in bf16, a 1080p BGR ring of 8 slots, the matcher's format,
S = 64 streams of K = 16 slots; stream i reads ring slot (t + i) % 8.

  step             FaceTracker.step of all 64 streams: the only way to serve such a tick without step_active
  active_a<A>      FaceTracker.step_active with A = 64, 32, 16, 4 streams (every 64/A-th stream), `active` and
                   `frame_index` on the device: no transfer
  restore          the two device copies that put the tracker back to its seeded state before every step (inside every
                   timed window above); "*_ms" is the difference of the medians
  forward_b<N>     model.forward_device alone on N = 1024 and 256 crops: how much of a step is the forward, and how
                   much of the gain of a smaller batch the fixed launch chain takes back

Also checks that `step` and step_active with A = 64 leave equal bits (the returned tensors and the tracker's state).
Prints one JSON line and writes it to --out.

    python tools/bench_track_active.py --out profiles/track_active.json
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import flm_amd  # noqa: F401
from flm_amd import _lib, alignment, prediction
from flm_amd.networks import LANDMARKS_MODELS
from flm_amd.weights import synth_fcn8_weights

import bench_track as bt

C, OUT, S, K = 68, 112, 64, 16
ACTIVE = [64, 32, 16, 4]


def bits(x):
    return x.view(torch.int64) if x.dtype == torch.float64 else x.view(torch.int32) if x.dtype == torch.float32 else \
        x.view(torch.int16) if x.dtype in (torch.float16, torch.bfloat16) else x


def run(rounds, window_ms, s=S, k=K, active=ACTIVE):
    model = LANDMARKS_MODELS["fcn_8"](C, input_height=256, input_width=256, dtype="bf16")
    model.load_weights(synth_fcn8_weights(C, seed=2))
    ring, ff = bt.rings()["bgr"]
    fmt = alignment.AlignedFormat.matcher()
    tr = prediction.FaceTracker(model, (bt.FH, bt.FW), k * s, streams=s, out_size=(OUT, OUT), aligned_format=fmt, frame_format=ff)
    for i in range(s):
        tr.seed(range(k), bt.boxes_for(k, 11 + k + i), stream=i)
    m0, b0, st0 = tr.m_crop.clone(), tr.boxes.clone(), tr.status.clone()
    idx = [torch.tensor([(t + i) % 8 for i in range(s)], dtype=torch.int32, device="cuda") for t in range(8)]
    act = {a: torch.arange(0, s, s // a, dtype=torch.int32, device="cuda")[:a].contiguous() for a in active}
    clock = {"t": 0}

    def restore():
        tr.m_crop.copy_(m0)
        tr.boxes.copy_(b0)

    def step():
        restore()
        clock["t"] += 1
        return tr.step(ring, idx[clock["t"] % 8])

    def stepper(a):
        def fn():
            restore()
            clock["t"] += 1
            return tr.step_active(ring, idx[clock["t"] % 8], act[a])
        return fn

    # `step` and step_active of every stream leave the same bits
    same = None
    if s in active:
        tr.status.copy_(st0)
        clock["t"] = 0
        x = [v.clone() for v in step()] + [tr.m_crop.clone(), tr.boxes.clone(), tr.status.clone()]
        tr.status.copy_(st0)
        clock["t"] = 0
        y = list(stepper(s)())
        slots = y.pop()
        y += [tr.m_crop, tr.boxes, tr.status]
        same = bool(torch.equal(slots.cpu(), torch.arange(s * k, dtype=torch.int32))
                    and all(p.dtype == q.dtype and torch.equal(bits(p), bits(q)) for p, q in zip(x, y)))

    crops = {n: torch.randint(0, 256, (n, 256, 256, 3), dtype=torch.uint8, device="cuda") for n in (s * k, s * k // 4)}
    variants = [("step", step)] + [("active_a%d" % a, stepper(a)) for a in active] + [("restore", restore)]
    variants += [("forward_b%d" % n, (lambda x=x: model.forward_device(x, "landmarks", n_points=4))) for n, x in crops.items()]
    w = bt.alternate(variants, rounds, window_ms)
    res = {"streams": s, "slots_per_stream": k, "windows": w, "same_bits_step_and_active_all": same}
    base = w["restore"]["median_ms"]
    res["step_ms"] = w["step"]["median_ms"] - base
    for a in active:
        res["active_a%d_ms" % a] = w["active_a%d" % a]["median_ms"] - base
        res["active_a%d_over_step" % a] = res["active_a%d_ms" % a] / res["step_ms"]
    ns = sorted(crops)
    res["forward_small_over_large"] = w["forward_b%d" % ns[0]]["median_ms"] / w["forward_b%d" % ns[1]]["median_ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=200.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    _lib.require_gpu()
    rec = {"bench": "track_active", "device": torch.cuda.get_device_name(0), "frame": [bt.FH, bt.FW], "landmarks": C}
    rec.update(run(a.rounds, a.window_ms))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
