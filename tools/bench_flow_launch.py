"""The landmark-flow launches alone, without a tracker (the protocol of tools/bench_track_flow.py: one process, the
variants ALTERNATING window by window, 5 windows of at least 200 ms each, median and [min, max] over the windows; HIP
events around whole windows).  Run it once per tree with --root to compare two trees.

Workload: N crops of 256x256 BGR, each a textured frame (a coarse random image upsampled, plus +-12 grey levels of
detail) seen twice under fresh noise of +-2 grey levels, so the levels converge as on a video; the identity matrix
(frame px = crop px); 68 landmarks per crop at random all over it; the flow with its defaults (4 levels, radius 7, 10
iterations).

    flow_64, flow_1024                alignment.landmark_flow_device (flm_landmark_flow) on 64 / 1024 crops
    rows_iota_1024                    alignment.landmark_flow_rows_device on the same 1024 crops with slot[r] = r and no
                                      check: the launch FaceTracker.step_flow makes where the rows form serves it
    flow_rows_256, flow_rows_256_fb   alignment.landmark_flow_rows_device on 256 rows with slot[r] = r, without and with
                                      max_fb = 1

    python tools/bench_flow_launch.py --root /path/to/a/built/tree --out profiles/x.json
"""
import argparse
import json
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--window-ms", type=float, default=200.0)
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                help="the tree whose package is measured (default: this one)")
ap.add_argument("--out", default=None)
args = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.abspath(args.root))

import torch  # noqa: E402

import flm_amd  # noqa: F401,E402
from flm_amd import _lib, alignment  # noqa: E402

import bench_track as bt  # noqa: E402

C, IN = 68, 256


def inputs(n, seed=3):
    """(pyramids [2n, bytes]: previous | current, matrices, landmarks in frame px) of n textured crops."""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    coarse = torch.randint(32, 224, (n, 3, IN // 8, IN // 8), device="cuda", generator=g).float()
    base = torch.nn.functional.interpolate(coarse, size=(IN, IN), mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
    base = base + torch.randint(-12, 13, (n, IN, IN, 3), device="cuda", generator=g).float()
    crops = torch.cat([(base + torch.randint(-2, 3, (n, IN, IN, 3), device="cuda", generator=g).float())
                       .clamp_(0, 255).to(torch.uint8) for _ in range(2)]).contiguous()
    pyr = alignment.flow_pyramid_device(crops, alignment.LandmarkFlow().levels)
    m = torch.tensor([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]], dtype=torch.float32, device="cuda").repeat(n, 1, 1).contiguous()
    lm = torch.rand((n, C, 2), dtype=torch.float64, device="cuda", generator=g) * (IN - 1)
    return pyr, m, lm


def main():
    _lib.require_gpu()
    flow, flow_fb = alignment.LandmarkFlow(), alignment.LandmarkFlow(max_fb=1.0)
    rec = {"bench": "flow_launch", "device": torch.cuda.get_device_name(0), "root": os.path.abspath(args.root),
           "landmarks": C, "crop": [IN, IN], "flow": repr(flow)}
    outs, shares = {}, {}

    def all_slots(name, n):
        pyr, m, lm = inputs(n)

        def fn():
            outs[name] = alignment.landmark_flow_device(pyr[:n], pyr[n:], lm, m, (IN, IN), flow, out=outs.get(name))
        return fn

    def rows(name, n, f):
        pyr, m, lm = inputs(n)
        iota = torch.arange(n, dtype=torch.int32, device="cuda")

        def fn():
            outs[name] = alignment.landmark_flow_rows_device(pyr[:n], pyr[n:], iota, lm, m, (IN, IN), f, out=outs.get(name))
        return fn

    variants = [("flow_64", all_slots("flow_64", 64)), ("flow_1024", all_slots("flow_1024", 1024)),
                ("rows_iota_1024", rows("rows_iota_1024", 1024, flow)),
                ("flow_rows_256", rows("flow_rows_256", 256, flow)),
                ("flow_rows_256_fb", rows("flow_rows_256_fb", 256, flow_fb))]
    w = bt.alternate(variants, args.rounds, args.window_ms)
    rec["windows"] = w
    for name, _ in variants:
        rec[name + "_ms"] = w[name]["median_ms"]
        flags = outs[name][-1]
        shares[name] = float((flags == 0).double().mean())
    rec["accepted_share"] = shares
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")
    print(json.dumps(rec), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
