"""What the head pose costs (the protocol of tools/bench_track.py: one process, the variants ALTERNATING window by window,
HIP events around whole windows, median and [min, max] over the windows).

  launch   alignment.head_pose_device alone at 64 and at 1024 rows of 68 landmarks with the default six-point model,
           weighted, and the same rows scattered to slots.  Windows hold thousands of back-to-back calls.
  step     FaceTracker.step at S = 64 streams of K = 16 slots (the workload of tools/bench_track_live.py: fcn_8 at
           256x256 in bf16, a 1080p BGR ring, the matcher's format), put back to the seeded state before every step:
           P a tracker with pose=None -- the step of a tracker as it was before the pose existed --, H one with
           pose=True, P2 the plain one again (the spread), R the restore alone.

Prints one JSON line, and writes it to --out.

    python tools/bench_head_pose.py --out profiles/head_pose.json
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


def launch(n, rounds, window_ms):
    g = torch.Generator(device="cuda")
    g.manual_seed(n)
    rec = torch.rand((n, C, _lib.LANDMARK_REC), dtype=torch.float64, device="cuda", generator=g) * 400.0
    rec[..., 2] = rec[..., 2] / 400.0
    lm, w = rec[..., :2], rec[..., 2]
    model = alignment.HeadModel.default(C)
    out = torch.empty((n, alignment.POSE_REC), dtype=torch.float64, device="cuda")
    fac = torch.empty((n,), dtype=torch.float64, device="cuda")
    slot = torch.randperm(n, device="cuda", generator=g).to(torch.int32)

    def dense():
        alignment.head_pose_device(lm, model, weights=w, out=out, factor_out=fac)

    def rows():
        alignment.head_pose_device(lm, model, weights=w, slot=slot, out=out, factor_out=fac)

    res = bt.alternate([("dense", dense), ("rows", rows), ("dense2", dense)], rounds, window_ms)
    torch.cuda.synchronize()
    res["rows_n"] = n
    res["ok_records"] = int((out[:, 14] == 1.0).sum())
    return res


def step(rounds, window_ms, s=S, k=K):
    model = LANDMARKS_MODELS["fcn_8"](C, input_height=256, input_width=256, dtype="bf16")
    model.load_weights(synth_fcn8_weights(C, seed=2))
    ring, ff = bt.rings()["bgr"]
    fmt = alignment.AlignedFormat.matcher()
    idx = [torch.tensor([(t + i) % 8 for i in range(s)], dtype=torch.int32, device="cuda") for t in range(8)]
    clock = {"t": 0}

    def stepper(**kw):
        tr = prediction.FaceTracker(model, (bt.FH, bt.FW), k * s, streams=s, out_size=(OUT, OUT), aligned_format=fmt,
                                    frame_format=ff, **kw)
        for i in range(s):
            tr.seed(range(k), bt.boxes_for(k, 11 + k + i), stream=i)
        m0, b0 = tr.m_crop.clone(), tr.boxes.clone()

        def restore():
            tr.m_crop.copy_(m0)
            tr.boxes.copy_(b0)

        def fn():
            restore()
            clock["t"] += 1
            return tr.step(ring, idx[clock["t"] % 8])
        return tr, fn, restore

    tp, p, restore = stepper()
    th, h, _ = stepper(pose=True)
    w = bt.alternate([("P", p), ("H", h), ("R", restore), ("P2", p)], rounds, window_ms)
    res = {"streams": s, "slots_per_stream": k, "windows": w}
    res["step_plain_ms"] = w["P"]["median_ms"] - w["R"]["median_ms"]
    res["step_pose_ms"] = w["H"]["median_ms"] - w["R"]["median_ms"]
    res["pose_minus_plain_ms"] = w["H"]["median_ms"] - w["P"]["median_ms"]
    res["spread_P_vs_P2_ms"] = w["P2"]["median_ms"] - w["P"]["median_ms"]
    res["pose_share_of_step"] = res["pose_minus_plain_ms"] / res["step_plain_ms"]
    res["ok_records"] = int((th.pose[:, 14] == 1.0).sum())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=200.0)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    _lib.require_gpu()
    rec = {"bench": "head_pose", "device": torch.cuda.get_device_name(0), "landmarks": C,
           "launch": {str(n): launch(n, a.rounds, a.window_ms) for n in (64, 1024)}}
    if not a.skip_step:
        rec["step"] = step(a.rounds, a.window_ms)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
