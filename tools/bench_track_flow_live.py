"""A flow tick for the slots that hold a face: FaceTracker.step_flow_live against step_flow and step_live (the protocol of
tools/bench_track_flow.py: one process, the variants ALTERNATING window by window, 5 windows of at least 200 ms each,
median and [min, max] over the windows; HIP events around whole windows; the parent commit's variants in a child process
that runs this file's --parent-only on that tree).

Workload: that of DESIGN 4.5h/i -- fcn_8 at 256x256 in bf16, a 1080p BGR ring of 8 slots, the matcher's format, S = 64
streams of K = 16 slots; stream i reads ring slot (t + i) % 8.  The flow has its defaults (4 levels, radius 7, 10
iterations).  SPARSE: two faces per camera, 128 live slots.  FULL: every slot holds a face.  STILL: a ring whose slots hold
one textured frame under fresh noise of +-2 grey levels (the levels converge, as on a video).  NOISE: the ring of random
bytes (no level converges: the most a flow tick can cost).

Every timed call is preceded, inside its window, by the device copies that put the tracker back -- matrices and boxes,
and for a flow tick the history a forward left (raw landmarks, flow_frame, flow_ready) -- and "*_ms" is the difference of
the medians of the call's windows and of those copies alone.

  this tree and, with --parent, the parent's tree (the rows the parent can run):
    flow_all_sparse_still / _noise    step_flow over all 1024 slots of the SPARSE tracker
    flow_all_full_still               step_flow of the FULL tracker
    live_128_b256                     step_live of the SPARSE flow tracker at budget 256
    step_full, step_full2             step of the FULL flow tracker, twice: the spread of the method
  this tree alone:
    flow_live_128_b256_still / _noise step_flow_live of the SPARSE tracker at budget 256
    flow_live_1024_b1024_still        step_flow_live of the FULL tracker at budget 1024
    gather_flow, history_put          the two launches a live flow tick adds, alone, over 1024 slots / 1024 rows
    flow_rows_256, flow_rows_256_fb   flm_landmark_flow_rows on 256 rows of the still ring without and with max_fb = 1

THE TIMING CONDITION: flow_live_128_b256_still_ms + spread < flow_all_sparse_still_ms of the PARENT's tree (this tree's
where no parent is given), and the same on NOISE; spread = |step_full2_ms - step_full_ms| of this process.  The tool exits 1
where it fails.  Prints one JSON line and writes it to --out.

    python tools/bench_track_flow_live.py --parent /path/to/the/parent/tree --out profiles/track_flow_live.json
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
ap.add_argument("--parent-only", action="store_true", help="measure only what a tree without step_flow_live can run")
ap.add_argument("--parent", default=None, help="a built tree of the parent commit, measured in a child process")
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

C, OUT, S, K, IN, BUDGET = 68, 112, 64, 16, 256, 256
HISTORY = ("_flow_lm", "flow_frame", "flow_ready")            # (the parent's tree has the first alone)


def still_ring(seed=17):
    """8 slots of one textured frame under fresh noise of +-2 grey levels (the ring of tools/bench_track_flow.py)."""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    coarse = torch.randint(32, 224, (1, 3, bt.FH // 8, bt.FW // 8), device="cuda", generator=g).float()
    base = torch.nn.functional.interpolate(coarse, size=(bt.FH, bt.FW), mode="bilinear", align_corners=False)[0].permute(1, 2, 0)
    base = base + torch.randint(-12, 13, (bt.FH, bt.FW, 3), device="cuda", generator=g).float()
    ring = torch.empty((8, bt.FH, bt.FW, 3), dtype=torch.uint8, device="cuda")
    for r in range(8):
        ring[r] = (base + torch.randint(-2, 3, (bt.FH, bt.FW, 3), device="cuda", generator=g).float()).clamp_(0, 255).to(torch.uint8)
    return ring


def tracker(model, sparse):
    tr = prediction.FaceTracker(model, (bt.FH, bt.FW), K * S, streams=S, out_size=(OUT, OUT),
                                aligned_format=alignment.AlignedFormat.matcher(), flow=True)
    for i in range(S):
        boxes = bt.boxes_for(K, 11 + K + i)
        if sparse:
            tr.seed([i % K, (i + 5) % K], boxes[:2], stream=i)        # two faces per camera, in slots that differ
        else:
            tr.seed(range(K), boxes, stream=i)
    return tr


class Held:
    """A tracker put back before every call: to its seeded crops, and for a flow tick to the history of one forward."""

    def __init__(self, tr, ring, idx):
        self.tr, self.ring, self.idx, self.t = tr, ring, idx, 0
        self.m0, self.b0 = tr.m_crop.clone(), tr.boxes.clone()
        self.restore()
        self.t += 1
        tr.step(ring, idx[1])                                         # the forward every flow tick starts from
        self.slots0 = tr.frame_slots.clone()
        self.hist = {k: getattr(tr, k).clone() for k in HISTORY if hasattr(tr, k)}
        if "flow_ready" in self.hist:  # every seeded slot has a history, as it has a crop: random weights lose tracks at will,
            b = self.b0                # and the restored crops make them live again
            self.hist["flow_ready"].copy_(((b[:, 2] > b[:, 0]) & (b[:, 3] > b[:, 1])).to(torch.int32))

    def restore(self):
        self.tr.m_crop.copy_(self.m0)
        self.tr.boxes.copy_(self.b0)

    def restore_flow(self):
        self.restore()
        self.tr.frame_slots.copy_(self.slots0)
        for k, v in self.hist.items():
            getattr(self.tr, k).copy_(v)
        self.tr._flow_ok = True        # the host rule of step_flow, set by hand: the history above IS that of a `step`

    def frame(self):
        self.t += 1
        return self.idx[self.t % 8]

    def step(self):
        self.restore()
        return self.tr.step(self.ring, self.frame())

    def live(self):
        self.restore()
        return self.tr.step_live(self.ring, self.frame(), BUDGET)

    def flow_all(self):
        self.restore_flow()
        return self.tr.step_flow(self.ring, self.frame())

    def flow_live(self, budget):
        def fn():
            self.restore_flow()
            return self.tr.step_flow_live(self.ring, self.frame(), budget)
        return fn


def launches(full, ring, rounds, window_ms):
    """The two launches a live flow tick adds, over 1024 slots, and the rows kernel with and without the check."""
    tr = full.tr
    n = S * K
    full.restore_flow()
    iota = torch.arange(n, dtype=torch.int32, device="cuda")
    zeros = torch.zeros((n,), dtype=torch.int32, device="cuda")
    ready0 = torch.ones((n,), dtype=torch.int32, device="cuda")
    ready, frame = ready0.clone(), zeros.clone()
    cursor = torch.zeros((1,), dtype=torch.int32, device="cuda")
    out = {}

    def gather():
        ready.copy_(ready0)
        out.update(alignment.track_gather_flow_device(tr.m_crop, tr.boxes, frame, ready, K, tr.frame_hw, n,
                                                      frame_index=full.idx[0], cursor=cursor, out=out or None))

    def put():
        alignment.track_flow_history_device(iota, zeros, zeros, frame, ready, lm_rows=full.hist["_flow_lm"], hist_lm=tr._flow_lm)

    rows = BUDGET
    u8 = alignment.AlignedFormat("nhwc", "uint8")
    crops = torch.empty((2 * rows, IN, IN, 3), dtype=torch.uint8, device="cuda")
    m, boxes = tr.m_crop[:rows].contiguous(), tr.boxes[:rows].contiguous()
    for half in (0, 1):
        alignment.warp_frames_device(ring, m, IN, IN, fmt=u8, frame_index_dev=torch.full((rows,), half, dtype=torch.int32, device="cuda"),
                                     boxes_dev=boxes, out=crops[half * rows:(half + 1) * rows])
    pyr = alignment.flow_pyramid_device(crops, tr.flow.levels)
    flows = {name: alignment.LandmarkFlow(max_fb=fb) for name, fb in (("flow_rows_256", None), ("flow_rows_256_fb", 1.0))}
    outs = {}

    def rows_flow(name):
        def fn():
            outs[name] = alignment.landmark_flow_rows_device(pyr[:rows], pyr[rows:], iota[:rows], full.hist["_flow_lm"], m, (IN, IN),
                                                             flows[name], out=outs.get(name))
        return fn

    w = bt.alternate([("gather_flow", gather), ("history_put", put), ("ready_copy", lambda: ready.copy_(ready0))] +
                     [(name, rows_flow(name)) for name in flows], rounds, window_ms)
    res = {"windows": w, "gather_flow_ms": w["gather_flow"]["median_ms"] - w["ready_copy"]["median_ms"],
           "history_put_ms": w["history_put"]["median_ms"], "flow_rows_256_ms": w["flow_rows_256"]["median_ms"],
           "flow_rows_256_fb_ms": w["flow_rows_256_fb"]["median_ms"]}
    res["fb_over_no_fb"] = res["flow_rows_256_fb_ms"] / res["flow_rows_256_ms"]
    f0, f1 = outs["flow_rows_256"][4], outs["flow_rows_256_fb"][4]
    res["accepted_share"] = {"without": float((f0 == 0).double().mean()), "with_max_fb_1": float((f1 == 0).double().mean())}
    return res


def main():
    _lib.require_gpu()
    model = LANDMARKS_MODELS["fcn_8"](C, input_height=IN, input_width=IN, dtype="bf16")
    model.load_weights(synth_fcn8_weights(C, seed=2))
    noise_ring, _ = bt.rings()["bgr"]
    calm_ring = still_ring()
    idx = [torch.tensor([(t + i) % 8 for i in range(S)], dtype=torch.int32, device="cuda") for t in range(8)]
    rec = {"bench": "track_flow_live", "device": torch.cuda.get_device_name(0), "frame": [bt.FH, bt.FW], "landmarks": C,
           "streams": S, "slots_per_stream": K, "faces_sparse": 2 * S, "budget_sparse": BUDGET,
           "model": "fcn_8 68 classes 256x256 bf16", "tree": "parent" if args.parent_only else "this"}
    sparse_still, sparse_noise = Held(tracker(model, True), calm_ring, idx), Held(tracker(model, True), noise_ring, idx)
    full = Held(tracker(model, False), calm_ring, idx)
    variants = [("flow_all_sparse_still", sparse_still.flow_all, "restore_flow_sparse"),
                ("flow_all_sparse_noise", sparse_noise.flow_all, "restore_flow_sparse"),
                ("flow_all_full_still", full.flow_all, "restore_flow_full"),
                ("live_128_b256", sparse_still.live, "restore_sparse"),
                ("step_full", full.step, "restore_full"), ("step_full2", full.step, "restore_full")]
    if not args.parent_only:
        variants += [("flow_live_128_b256_still", sparse_still.flow_live(BUDGET), "restore_flow_sparse"),
                     ("flow_live_128_b256_noise", sparse_noise.flow_live(BUDGET), "restore_flow_sparse"),
                     ("flow_live_1024_b1024_still", full.flow_live(S * K), "restore_flow_full")]
    copies = [("restore_sparse", sparse_still.restore), ("restore_full", full.restore),
              ("restore_flow_sparse", sparse_still.restore_flow), ("restore_flow_full", full.restore_flow)]
    w = bt.alternate([(n, f) for n, f, _ in variants] + copies, args.rounds, args.window_ms)
    rec["windows"] = w
    for name, _, base in variants:
        rec[name + "_ms"] = w[name]["median_ms"] - w[base]["median_ms"]
    rec["spread_ms"] = abs(rec["step_full2_ms"] - rec["step_full_ms"])
    if not args.parent_only:
        sparse_still.flow_live(BUDGET)()
        rec["flow_counts_sparse"] = sparse_still.tr.flow_counts.tolist()
        rec["flow_accepted_share"] = {"still": float((sparse_still.tr.flow_flags[:2 * S] == 0).double().mean())}
        sparse_noise.flow_live(BUDGET)()
        rec["flow_accepted_share"]["noise"] = float((sparse_noise.tr.flow_flags[:2 * S] == 0).double().mean())
        full.flow_live(S * K)()
        rec["flow_counts_full"] = full.tr.flow_counts.tolist()
        rec["launches"] = launches(full, calm_ring, args.rounds, args.window_ms)
        rec["flow_live_all_minus_flow_all_ms"] = rec["flow_live_1024_b1024_still_ms"] - rec["flow_all_full_still_ms"]
        rec["gather_plus_put_ms"] = rec["launches"]["gather_flow_ms"] + rec["launches"]["history_put_ms"]
        rec["flow_live_all_explained"] = bool(rec["flow_live_all_minus_flow_all_ms"] <= rec["gather_plus_put_ms"] + rec["spread_ms"])
    ref = rec
    if args.parent:
        cmd = [sys.executable, os.path.abspath(__file__), "--root", os.path.abspath(args.parent), "--parent-only",
               "--rounds", str(args.rounds), "--window-ms", str(args.window_ms)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            sys.exit("bench_track_flow_live: the parent's run failed:\n" + r.stderr[-2000:])
        ref = json.loads(r.stdout.strip().splitlines()[-1])
        rec["parent"] = {k: v for k, v in ref.items() if k.endswith("_ms") or k == "windows"}
        for name in ("step_full", "live_128_b256", "flow_all_sparse_still", "flow_all_full_still"):
            rec[name + "_vs_parent_ms"] = rec[name + "_ms"] - ref[name + "_ms"]
        rec["spread_parent_ms"] = ref["spread_ms"]
    ok = True
    if not args.parent_only:
        for scene in ("still", "noise"):
            mine, theirs = rec["flow_live_128_b256_%s_ms" % scene], ref["flow_all_sparse_%s_ms" % scene]
            rec["flow_live_over_flow_all_" + scene] = mine / theirs
            rec["gate_cheaper_than_step_flow_" + scene] = bool(mine + rec["spread_ms"] < theirs)
            ok = ok and rec["gate_cheaper_than_step_flow_" + scene]
        rec["flow_live_over_step_live_still"] = rec["flow_live_128_b256_still_ms"] / rec["live_128_b256_ms"]
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")
    print(json.dumps(rec), flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
