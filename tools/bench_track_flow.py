"""A tick without the forward: FaceTracker.step against FaceTracker.step_flow (the protocol of tools/bench_track_live.py:
one process, the variants ALTERNATING window by window, 5 windows of at least 200 ms each, median and [min, max] over the
windows; HIP events around whole windows).

Workload: that of DESIGN 4.5h/i -- fcn_8 at 256x256 in bf16, a 1080p BGR ring of 8 slots, the matcher's format, S = 64
streams of K = 16 slots, every slot holding a face; stream i reads ring slot (t + i) % 8.  The flow has its defaults
(4 levels, radius 7, 10 iterations).

  step, step2        FaceTracker.step of a tracker made with flow (twice: the spread of the method)
  step_plain         FaceTracker.step of a tracker made without flow: what the two history copies cost
  flow_noise         step_flow on the ring of random bytes: two frames share nothing, no level converges, every landmark
                     runs max_iter iterations on every level -- the most a flow tick can cost.  THE GATE reads this row.
  flow_still         step_flow on a ring whose slots hold one textured frame under fresh noise of +-2 grey levels: the
                     levels converge, as on a video
  restore, restore_flow   the device copies that put a tracker back to its state before every call (inside every timed
                     window above: matrices and boxes; for a flow tick also the raw landmarks it starts from, so that
                     every tick carries the landmarks of a forward and not the rejections of the tick before);
                     "*_ms" is the difference of the medians
  launches           the launches a flow tick adds, one by one, at 64 and 1024 rows: one uint8 crop warp (a tick makes
                     two), the pyramid of 2N crops with its GB/s by the byte model (2N crops read once, 2N pyramids
                     written once), the flow of N x 68 landmarks on the still ring
  --parent DIR       `step` of the tree DIR (the parent commit, built) at the same workload, in a child process that runs
                     this file's --step-only on that tree
  still              the still scene of tools/bench_track.py (one frame repeated under fresh noise, 8 faces, the crop
                     held): the standard deviation over time of the landmarks on forward ticks against flow ticks (one
                     forward, then flow ticks alone), the share of landmarks the flow accepts, and, with the crop NOT
                     held, how many of the 8 tracks are alive after 1, 5 and 20 consecutive flow ticks (random weights:
                     the forward's landmarks are no face, so the fit that places the next crop is arbitrary)

The gate: flow_noise_ms < 0.5 * step_ms, in this process; the tool exits 1 where it fails.  Prints one JSON line and
writes it to --out.

    python tools/bench_track_flow.py --parent /path/to/the/parent/tree --out profiles/track_flow.json
"""
import argparse
import json
import os
import subprocess
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--window-ms", type=float, default=200.0)
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                help="the tree whose package is measured (default: this one)")
ap.add_argument("--step-only", action="store_true", help="measure `step` alone: runs on a tree without the flow")
ap.add_argument("--parent", default=None, help="a built tree of the parent commit: its `step` is measured in a child process")
ap.add_argument("--still", type=int, default=60, help="ticks of the still scene")
ap.add_argument("--out", default=None)
args = ap.parse_args()
sys.path.insert(0, os.path.join(os.path.abspath(args.root), "tools"))
sys.path.insert(0, os.path.abspath(args.root))

import torch  # noqa: E402

import flm_amd  # noqa: F401,E402
from flm_amd import _lib, alignment, prediction  # noqa: E402
from flm_amd.networks import LANDMARKS_MODELS  # noqa: E402
from flm_amd.weights import synth_fcn8_weights  # noqa: E402

import bench_track as bt  # noqa: E402

C, OUT, S, K, IN = 68, 112, 64, 16, 256


def still_ring(seed=17):
    """8 slots of one textured frame (the scene of bench_track.still) under fresh noise of +-2 grey levels."""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    coarse = torch.randint(32, 224, (1, 3, bt.FH // 8, bt.FW // 8), device="cuda", generator=g).float()
    base = torch.nn.functional.interpolate(coarse, size=(bt.FH, bt.FW), mode="bilinear", align_corners=False)[0].permute(1, 2, 0)
    base = base + torch.randint(-12, 13, (bt.FH, bt.FW, 3), device="cuda", generator=g).float()
    ring = torch.empty((8, bt.FH, bt.FW, 3), dtype=torch.uint8, device="cuda")
    for r in range(8):
        ring[r] = (base + torch.randint(-2, 3, (bt.FH, bt.FW, 3), device="cuda", generator=g).float()).clamp_(0, 255).to(torch.uint8)
    return ring


def tracker(model, s, k, **kw):
    tr = prediction.FaceTracker(model, (bt.FH, bt.FW), k * s, streams=s, out_size=(OUT, OUT),
                                aligned_format=alignment.AlignedFormat.matcher(), **kw)
    for i in range(s):
        tr.seed(range(k), bt.boxes_for(k, 11 + k + i), stream=i)
    return tr


class Held:
    """A tracker put back to its seeded crops before every call; for a flow tick also to the history of a forward."""

    def __init__(self, tr, ring, idx):
        self.tr, self.ring, self.idx, self.t = tr, ring, idx, 0
        self.m0, self.b0 = tr.m_crop.clone(), tr.boxes.clone()
        self.lm0 = None

    def restore(self):
        self.tr.m_crop.copy_(self.m0)
        self.tr.boxes.copy_(self.b0)

    def restore_flow(self):
        self.restore()
        self.tr._flow_lm.copy_(self.lm0)

    def step(self):
        self.restore()
        self.t += 1
        return self.tr.step(self.ring, self.idx[self.t % 8])

    def arm(self):
        """One forward, whose raw landmarks every flow tick starts from."""
        self.step()
        self.lm0 = self.tr._flow_lm.clone()

    def flow(self):
        self.restore_flow()
        self.t += 1
        return self.tr.step_flow(self.ring, self.idx[self.t % 8])


def launches(ring, n, rounds, window_ms):
    """The launches a flow tick adds, at n rows."""
    flow = alignment.LandmarkFlow()
    boxes = torch.tensor(prediction.face_boxes(bt.boxes_for(n, 7)), dtype=torch.int32, device="cuda")
    m, _ = alignment.track_seed_device(boxes, (IN, IN), (bt.FH, bt.FW))
    u8 = alignment.AlignedFormat("nhwc", "uint8")
    crops = torch.empty((2 * n, IN, IN, 3), dtype=torch.uint8, device="cuda")
    pyr = torch.empty((2 * n, flow.pyramid_bytes(IN, IN)), dtype=torch.uint8, device="cuda")
    slots = [torch.full((n,), v, dtype=torch.int32, device="cuda") for v in (0, 1)]
    g = torch.Generator(device="cuda")
    g.manual_seed(3)
    lm_crop = torch.rand((n, C, 2), dtype=torch.float64, device="cuda", generator=g) * (IN - 1)
    lm = alignment.landmarks_from_crop_device(lm_crop, m, (IN, IN), (IN, IN))     # frame px of points all over the crop
    outs = alignment.landmark_flow_device(pyr[:n], pyr[n:], lm, m, (IN, IN), flow)

    def warp(half=0):
        alignment.warp_frames_device(ring, m, IN, IN, fmt=u8, frame_index_dev=slots[half], boxes_dev=boxes, out=crops[half * n:(half + 1) * n])

    def pyramid():
        alignment.flow_pyramid_device(crops, flow.levels, out=pyr)

    def run_flow():
        alignment.landmark_flow_device(pyr[:n], pyr[n:], lm, m, (IN, IN), flow, out=outs)

    warp(0)
    warp(1)
    pyramid()
    w = bt.alternate([("crop_warp", warp), ("pyramid", pyramid), ("flow", run_flow)], rounds, window_ms)
    nbytes = 2 * n * (IN * IN * 3 + flow.pyramid_bytes(IN, IN))
    flags = outs[3]
    return {"rows": n, "windows": w, "pyramid_bytes_moved": nbytes,
            "pyramid_GBps": nbytes / (w["pyramid"]["median_ms"] * 1e-3) / 1e9,
            "flow_accepted_share": float((flags == 0).double().mean())}


def still(model, n, k=8, skip=5):
    """The still scene: forward ticks against flow ticks on a held crop, and the closed loop of flow ticks."""
    g = torch.Generator(device="cuda")
    g.manual_seed(17)
    ring = still_ring()
    faces = bt.boxes_for(k, 11 + k)
    res = {"ticks": n, "faces": k, "noise_grey_levels": 2}
    series = {}
    for name in ("forward", "flow"):
        tr = prediction.FaceTracker(model, (bt.FH, bt.FW), k, out_size=(OUT, OUT), flow=True)
        tr.seed(range(k), faces)
        m0, b0 = tr.m_crop.clone(), tr.boxes.clone()
        lms, acc = [], []
        for r in range(n):
            tr.m_crop.copy_(m0)
            tr.boxes.copy_(b0)
            if name == "forward" or r == 0:
                lm = tr.step(ring, r % 8)[2]
            else:
                lm = tr.step_flow(ring, r % 8)[2]
                acc.append(float((tr.flow_flags == 0).double().mean()))
            lms.append(lm.clone())
        series[name] = torch.stack(lms[skip:])
        if acc:
            res["flow_accepted_share_mean"] = sum(acc) / len(acc)
            res["flow_accepted_share_last"] = acc[-1]
    ok = (series["forward"] >= 0).all(0).all(-1) & (series["flow"] >= 0).all(0).all(-1)    # points both kept throughout
    res["points"] = int(ok.sum())
    for name, lm in series.items():
        sd = lm.std(0)[ok]
        res[name + "_landmark_std_px_mean"] = float(sd.mean()) if int(ok.sum()) else None
        res[name + "_landmark_std_px_max"] = float(sd.max()) if int(ok.sum()) else None
    tr = prediction.FaceTracker(model, (bt.FH, bt.FW), k, out_size=(OUT, OUT), flow=True)
    tr.seed(range(k), faces)
    m0, b0, s0 = tr.m_crop.clone(), tr.boxes.clone(), tr.status.clone()
    tr.step(ring, 0)
    tr.m_crop.copy_(m0)      # the crop of the first flow tick is the seeded one; from there on the loop is closed
    tr.boxes.copy_(b0)
    tr.status.copy_(s0)
    alive = []
    for r in range(1, 21):
        alive.append(int((tr.step_flow(ring, r % 8)[3] == 0).sum()))
    res["alive_after_flow_ticks"] = {str(r): alive[r - 1] for r in (1, 5, 20)}
    return res


def main():
    _lib.require_gpu()
    model = LANDMARKS_MODELS["fcn_8"](C, input_height=IN, input_width=IN, dtype="bf16")
    model.load_weights(synth_fcn8_weights(C, seed=2))
    ring, _ = bt.rings()["bgr"]
    idx = [torch.tensor([(t + i) % 8 for i in range(S)], dtype=torch.int32, device="cuda") for t in range(8)]
    rec = {"bench": "track_flow", "device": torch.cuda.get_device_name(0), "frame": [bt.FH, bt.FW], "landmarks": C,
           "streams": S, "slots_per_stream": K, "model": "fcn_8 68 classes 256x256 bf16"}
    if args.step_only:
        h = Held(tracker(model, S, K), ring, idx)
        w = bt.alternate([("step", h.step), ("step2", h.step), ("restore", h.restore)], args.rounds, args.window_ms)
        rec.update(windows=w, step_ms=w["step"]["median_ms"] - w["restore"]["median_ms"],
                   spread_step_vs_step2_ms=w["step2"]["median_ms"] - w["step"]["median_ms"])
        print(json.dumps(rec), flush=True)
        return 0
    noise, plain = Held(tracker(model, S, K, flow=True), ring, idx), Held(tracker(model, S, K), ring, idx)
    calm = Held(tracker(model, S, K, flow=True), still_ring(), idx)
    noise.arm()
    calm.arm()
    variants = [("step", noise.step), ("step_plain", plain.step), ("flow_noise", noise.flow), ("flow_still", calm.flow),
                ("step2", noise.step), ("restore", noise.restore), ("restore_flow", noise.restore_flow)]
    w = bt.alternate(variants, args.rounds, args.window_ms)
    rec["windows"] = w
    for name, base in (("step", "restore"), ("step2", "restore"), ("step_plain", "restore"), ("flow_noise", "restore_flow"),
                       ("flow_still", "restore_flow")):
        rec[name + "_ms"] = w[name]["median_ms"] - w[base]["median_ms"]
    rec["spread_step_vs_step2_ms"] = rec["step2_ms"] - rec["step_ms"]
    rec["history_copies_ms"] = rec["step_ms"] - rec["step_plain_ms"]
    rec["flow_noise_over_step"] = rec["flow_noise_ms"] / rec["step_ms"]
    rec["flow_still_over_step"] = rec["flow_still_ms"] / rec["step_ms"]
    rec["flow_accepted_share"] = {"noise": float((noise.tr.flow_flags == 0).double().mean()),
                                  "still": float((calm.tr.flow_flags == 0).double().mean())}
    rec["gate_flow_under_half_a_step"] = bool(rec["flow_noise_ms"] < 0.5 * rec["step_ms"])
    rec["launches"] = {str(n): launches(calm.ring, n, args.rounds, args.window_ms) for n in (64, 1024)}
    rec["still"] = still(model, args.still)
    if args.parent:
        cmd = [sys.executable, os.path.abspath(__file__), "--root", os.path.abspath(args.parent), "--step-only",
               "--rounds", str(args.rounds), "--window-ms", str(args.window_ms)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            sys.exit("bench_track_flow: the parent's run failed:\n" + r.stderr[-2000:])
        parent = json.loads(r.stdout.strip().splitlines()[-1])
        rec["parent"] = {k: parent[k] for k in ("step_ms", "spread_step_vs_step2_ms", "windows")}
        rec["step_vs_parent_ms"] = rec["step_ms"] - parent["step_ms"]
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")
    print(json.dumps(rec), flush=True)
    return 0 if rec["gate_flow_under_half_a_step"] else 1


if __name__ == "__main__":
    sys.exit(main())
