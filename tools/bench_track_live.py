"""Stepping only the slots that hold a face: FaceTracker.step of every slot against FaceTracker.step_live (the protocol
of tools/bench_track_active.py: one process, the variants ALTERNATING window by window, 5 windows of at least 200 ms each,
median and [min, max] over the windows; HIP events around whole windows).

Workload: that of DESIGN 4.5h/i -- fcn_8 at 256x256 in bf16, a 1080p BGR ring of 8 slots, the matcher's format, S = 64
streams of K = 16 slots; stream i reads ring slot (t + i) % 8.

  step               FaceTracker.step of a tracker whose 1024 slots all hold a face
  step_sparse        FaceTracker.step of a tracker with two faces per camera (128 live slots): what such a tracker pays
                     without step_live -- the empty slots are zero crops, the forward runs on them all the same
  live_128_b256      FaceTracker.step_live of that tracker at budget 256, `frame_index` on the device
  live_1024_b1024    FaceTracker.step_live of the full tracker at budget 1024
  gather             alignment.track_gather_live_device alone on the full tracker: the one launch step_live adds
  restore_*          the two device copies that put a tracker back to its seeded state before every step (inside every
                     timed window above); "*_ms" is the difference of the medians

Also checks that `step` and step_live of a full tracker leave equal bits (the returned tensors and the tracker's state),
and reports `live_counts` of both trackers.  Prints one JSON line and writes it to --out.

    python tools/bench_track_live.py --out profiles/track_live.json
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
SPARSE_BUDGET = 256


def bits(x):
    return x.view(torch.int64) if x.dtype == torch.float64 else x.view(torch.int32) if x.dtype == torch.float32 else \
        x.view(torch.int16) if x.dtype in (torch.float16, torch.bfloat16) else x


def run(rounds, window_ms, s=S, k=K):
    model = LANDMARKS_MODELS["fcn_8"](C, input_height=256, input_width=256, dtype="bf16")
    model.load_weights(synth_fcn8_weights(C, seed=2))
    ring, ff = bt.rings()["bgr"]
    fmt = alignment.AlignedFormat.matcher()
    make = lambda: prediction.FaceTracker(model, (bt.FH, bt.FW), k * s, streams=s, out_size=(OUT, OUT), aligned_format=fmt,
                                          frame_format=ff)
    full, sparse = make(), make()
    for i in range(s):
        boxes = bt.boxes_for(k, 11 + k + i)
        full.seed(range(k), boxes, stream=i)
        sparse.seed([i % k, (i + 5) % k], boxes[:2], stream=i)            # two faces per camera, in slots that differ
    seeded = {tr: (tr.m_crop.clone(), tr.boxes.clone(), tr.status.clone()) for tr in (full, sparse)}
    idx = [torch.tensor([(t + i) % 8 for i in range(s)], dtype=torch.int32, device="cuda") for t in range(8)]
    clock = {"t": 0}

    def restorer(tr):
        def fn():
            tr.m_crop.copy_(seeded[tr][0])
            tr.boxes.copy_(seeded[tr][1])
        return fn

    def stepper(tr, budget=None):
        restore = restorer(tr)

        def fn():
            restore()
            clock["t"] += 1
            fi = idx[clock["t"] % 8]
            return tr.step(ring, fi) if budget is None else tr.step_live(ring, fi, budget)
        return fn

    def gather():
        return alignment.track_gather_live_device(full.m_crop, full.boxes, k, full.frame_hw, s * k, frame_index=idx[0],
                                                  cursor=full.live_cursor, out=dict(counts=full.live_counts))

    # `step` and step_live of a tracker whose slots are all live leave the same bits: row r is slot r
    full.status.copy_(seeded[full][2])
    clock["t"] = 0
    x = [v.clone() for v in stepper(full)()] + [full.m_crop.clone(), full.boxes.clone(), full.status.clone()]
    full.status.copy_(seeded[full][2])
    clock["t"] = 0
    y = list(stepper(full, s * k)())
    slots = y.pop()
    y += [full.m_crop, full.boxes, full.status]
    same = bool(torch.equal(slots.cpu(), torch.arange(s * k, dtype=torch.int32))
                and all(p.dtype == q.dtype and torch.equal(bits(p), bits(q)) for p, q in zip(x, y)))
    counts = {}
    for name, tr, budget in (("full", full, s * k), ("sparse", sparse, SPARSE_BUDGET)):
        stepper(tr, budget)()
        counts[name] = tr.live_counts.tolist()

    variants = [("step", stepper(full)), ("step_sparse", stepper(sparse)),
                ("live_128_b%d" % SPARSE_BUDGET, stepper(sparse, SPARSE_BUDGET)), ("live_1024_b1024", stepper(full, s * k)),
                ("gather", gather), ("restore_full", restorer(full)), ("restore_sparse", restorer(sparse))]
    w = bt.alternate(variants, rounds, window_ms)
    res = {"streams": s, "slots_per_stream": k, "windows": w, "same_bits_step_and_live_all": same, "live_counts": counts}
    for name, base in (("step", "restore_full"), ("live_1024_b1024", "restore_full"), ("step_sparse", "restore_sparse"),
                       ("live_128_b%d" % SPARSE_BUDGET, "restore_sparse")):
        res[name + "_ms"] = w[name]["median_ms"] - w[base]["median_ms"]
    res["gather_ms"] = w["gather"]["median_ms"]
    res["live_all_minus_step_ms"] = res["live_1024_b1024_ms"] - res["step_ms"]
    res["live_128_over_step_sparse"] = res["live_128_b%d_ms" % SPARSE_BUDGET] / res["step_sparse_ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=200.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    _lib.require_gpu()
    rec = {"bench": "track_live", "device": torch.cuda.get_device_name(0), "frame": [bt.FH, bt.FW], "landmarks": C}
    rec.update(run(a.rounds, a.window_ms))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
