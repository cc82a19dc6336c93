"""What the face parts and the openness cost (the protocol of tools/bench_track.py: one process, the variants ALTERNATING
window by window, HIP events around whole windows, median and [min, max] over the windows).

  parts     alignment.warp_parts_frames_device -- ONE launch for the three default parts, patches of 32x48 in the
            matcher's format -- at 64 and 1024 faces on a 1080p ring, BGR and NV12, against the COMPOSITION of the calls a
            user had before: per part the slice of its landmarks and weights, alignment.similarity_device and
            alignment.warp_frames_device into the part's own output (3 fits + 3 warps + the slices).  With --parent TREE
            the composition is ALSO measured in a child process on a built tree of the parent commit, on the same box.
  openness  alignment.face_openness_device at 64 and 1024 rows, records alone and with the blink state, beside
            alignment.head_pose_device at the same rows (its baseline).
  step      FaceTracker.step at 64 streams x 16 slots (the workload of tools/bench_head_pose.py) and step_flow_live at
            budget 256 over two faces per camera (the workload of tools/bench_track_flow_live.py), each put back to its
            seeded state before every call: P a tracker without the two options, X one with parts=True and
            openness=True, P2 the plain one again (the spread), R the restore alone.  With --parent TREE the plain
            trackers are also measured on the parent's tree.

Prints one JSON line, and writes it to --out.  The event windows of the small launches are bound by the Python wrappers;
`--trace N` makes a few launches at N faces and nothing else, for the kernels' own durations under a kernel trace.

    python tools/bench_parts.py --parent /path/to/built/parent --out profiles/face_parts.json
    rocprofv3 --kernel-trace --stats ... -- python tools/bench_parts.py --trace 1024
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
ap.add_argument("--parent-only", action="store_true", help="measure only what a tree without the face parts can run")
ap.add_argument("--parent", default=None, help="a built tree of the parent commit, measured in a child process")
ap.add_argument("--skip-step", action="store_true")
ap.add_argument("--trace", type=int, default=0, metavar="N", help="only a few launches at N faces, for a kernel trace")
ap.add_argument("--out", default=None)
args = ap.parse_args()
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.abspath(args.root))

import torch  # noqa: E402

import flm_amd  # noqa: F401,E402
from flm_amd import _lib, alignment, prediction  # noqa: E402
from flm_amd.networks import LANDMARKS_MODELS  # noqa: E402
from flm_amd.weights import synth_fcn8_weights  # noqa: E402

import bench_track as bt  # noqa: E402

C, OUT, S, K, IN, BUDGET = 68, 112, 64, 16, 256, 256
PATCH = (32, 48)
RANGES = ((36, 42), (42, 48), (48, 68))


def default_templates():
    """FaceParts.default's templates, restated from canonical_template so that the parent's tree can make them too."""
    base = alignment.canonical_template(68, 2, 2)
    ph, pw = PATCH
    out = []
    for lo, hi in RANGES:
        p = base[lo:hi]
        mn, mx = p.min(axis=0), p.max(axis=0)
        s = 0.8 * (pw - 1) / (mx[0] - mn[0])
        out.append(torch.from_numpy((p - (mn + mx) / 2) * s + [(pw - 1) / 2, (ph - 1) / 2]).cuda())
    return out


def faces(k, seed):
    """k faces of 68 landmarks of 100..300 px, anywhere in the frame, their scores, ring slots and boxes."""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    tm = torch.from_numpy(alignment.canonical_template(68, 2, 2)).cuda()
    side = torch.rand((k, 1, 1), dtype=torch.float64, device="cuda", generator=g) * 200.0 + 100.0
    org = torch.rand((k, 1, 2), dtype=torch.float64, device="cuda", generator=g)
    org = org * torch.tensor([bt.FW - 301.0, bt.FH - 301.0], dtype=torch.float64, device="cuda")
    lm = (tm[None] * side + org).contiguous()
    w = torch.rand((k, 68), dtype=torch.float64, device="cuda", generator=g) * 0.9 + 0.1
    idx = torch.randint(0, 8, (k,), dtype=torch.int32, device="cuda", generator=g)
    boxes = torch.tensor([0, 0, bt.FW, bt.FH], dtype=torch.int32, device="cuda").repeat(k, 1).contiguous()
    return lm, w, idx, boxes


def parts(k, source, rounds, window_ms):
    ring, ff = bt.rings()[source]
    fmt = alignment.AlignedFormat.matcher()
    lm, w, idx, boxes = faces(k, k)
    tmpl = default_templates()
    outs = [torch.empty(fmt.shape(k, *PATCH), dtype=fmt.torch_dtype, device="cuda") for _ in RANGES]

    def composed():
        for (lo, hi), t, o in zip(RANGES, tmpl, outs):
            m = alignment.similarity_device(lm[:, lo:hi], t, weights=w[:, lo:hi])
            alignment.warp_frames_device(ring, m, PATCH[0], PATCH[1], frame_index_dev=idx, boxes_dev=boxes, fmt=fmt, src=ff,
                                         out=o)

    variants = [("composed", composed)]
    if not args.parent_only:
        fp = alignment.FaceParts.default(68, PATCH)
        one = torch.empty((k, 3) + tuple(fmt.shape(1, *PATCH)[1:]), dtype=fmt.torch_dtype, device="cuda")

        def fused():
            alignment.warp_parts_frames_device(ring, lm, fp, weights=w, frame_index_dev=idx, boxes_dev=boxes, fmt=fmt, src=ff,
                                               out=one)

        variants += [("one_launch", fused), ("composed2", composed)]
    res = bt.alternate(variants, rounds, window_ms)
    torch.cuda.synchronize()
    if not args.parent_only:
        for r in range(3):   # the two forms compute the same patches
            assert torch.equal(one[:, r].view(torch.int16), outs[r].view(torch.int16)), (k, source, r)
        res["ratio_one_launch_to_composed"] = res["one_launch"]["median_ms"] / res["composed"]["median_ms"]
    return res


def openness(n, rounds, window_ms):
    g = torch.Generator(device="cuda")
    g.manual_seed(n)
    rec = torch.rand((n, C, _lib.LANDMARK_REC), dtype=torch.float64, device="cuda", generator=g) * 400.0
    rec[..., 2] = rec[..., 2] / 400.0
    lm, w = rec[..., :2], rec[..., 2]
    model = alignment.HeadModel.default(C)
    pose = torch.empty((n, alignment.POSE_REC), dtype=torch.float64, device="cuda")
    variants = [("head_pose", lambda: alignment.head_pose_device(lm, model, weights=w, out=pose))]
    if not args.parent_only:
        opts = alignment.Openness.default(C)
        out = torch.empty((n, 3, alignment.OPEN_REC), dtype=torch.float64, device="cuda")
        state = torch.tensor(alignment.OPEN_STATE_EMPTY, dtype=torch.float64, device="cuda").repeat(n, 3, 1).contiguous()
        reset = torch.zeros((n,), dtype=torch.int32, device="cuda")
        slot = torch.randperm(n, device="cuda", generator=g).to(torch.int32)
        variants += [("records", lambda: alignment.face_openness_device(lm, opts, weights=w, out=out)),
                     ("records_state", lambda: alignment.face_openness_device(lm, opts, weights=w, out=out, state=state,
                                                                              reset=reset, dt=0.04)),
                     ("records_state_rows", lambda: alignment.face_openness_device(lm, opts, weights=w, slot=slot, out=out,
                                                                                   state=state, reset=reset, dt=0.04)),
                     ("head_pose2", variants[0][1])]
    res = bt.alternate(variants, rounds, window_ms)
    torch.cuda.synchronize()
    if not args.parent_only:
        res["ok_records"] = int((out[..., 2] == 1.0).sum())
    return res


def step(rounds, window_ms):
    model = LANDMARKS_MODELS["fcn_8"](C, input_height=IN, input_width=IN, dtype="bf16")
    model.load_weights(synth_fcn8_weights(C, seed=2))
    ring, ff = bt.rings()["bgr"]
    fmt = alignment.AlignedFormat.matcher()
    idx = [torch.tensor([(t + i) % 8 for i in range(S)], dtype=torch.int32, device="cuda") for t in range(8)]
    clock = {"t": 0}

    def frame():
        clock["t"] += 1
        return idx[clock["t"] % 8]

    def full(**kw):     # every slot holds a face: FaceTracker.step
        tr = prediction.FaceTracker(model, (bt.FH, bt.FW), K * S, streams=S, out_size=(OUT, OUT), aligned_format=fmt,
                                    frame_format=ff, **kw)
        for i in range(S):
            tr.seed(range(K), bt.boxes_for(K, 11 + K + i), stream=i)
        m0, b0 = tr.m_crop.clone(), tr.boxes.clone()

        def restore():
            tr.m_crop.copy_(m0)
            tr.boxes.copy_(b0)

        def fn():
            restore()
            return tr.step(ring, frame())
        return fn, restore

    def sparse(**kw):   # two faces per camera: step_flow_live at budget 256, from the history of one forward
        tr = prediction.FaceTracker(model, (bt.FH, bt.FW), K * S, streams=S, out_size=(OUT, OUT), aligned_format=fmt,
                                    frame_format=ff, flow=True, **kw)
        for i in range(S):
            tr.seed([i % K, (i + 5) % K], bt.boxes_for(K, 11 + K + i)[:2], stream=i)
        m0, b0 = tr.m_crop.clone(), tr.boxes.clone()
        tr.step(ring, idx[1])
        hist = {k: getattr(tr, k).clone() for k in ("_flow_lm", "flow_frame", "flow_ready")}
        hist["flow_ready"].copy_(((b0[:, 2] > b0[:, 0]) & (b0[:, 3] > b0[:, 1])).to(torch.int32))

        def restore():
            tr.m_crop.copy_(m0)
            tr.boxes.copy_(b0)
            for k, v in hist.items():
                getattr(tr, k).copy_(v)

        def fn():
            restore()
            return tr.step_flow_live(ring, frame(), BUDGET)
        return fn, restore

    out = {"streams": S, "slots_per_stream": K, "budget": BUDGET}
    for name, make in (("step", full), ("step_flow_live", sparse)):
        p, restore = make()
        variants = [("P", p)]
        if not args.parent_only:
            variants.append(("X", make(parts=True, openness=True)[0]))
        variants += [("R", restore), ("P2", p)]
        w = bt.alternate(variants, rounds, window_ms)
        r = {"windows": w, "plain_ms": w["P"]["median_ms"] - w["R"]["median_ms"],
             "spread_P_vs_P2_ms": w["P2"]["median_ms"] - w["P"]["median_ms"]}
        if not args.parent_only:
            r["with_parts_and_openness_ms"] = w["X"]["median_ms"] - w["R"]["median_ms"]
            r["added_ms"] = w["X"]["median_ms"] - w["P"]["median_ms"]
        out[name] = r
    return out


def trace(n, calls=50):
    """--trace N: `calls` launches of the parts warp (BGR, NV12) and of the openness call (records + state) at N faces and
    nothing else, for `rocprofv3 --kernel-trace --stats`: the event windows above are bound by the Python wrappers at
    these sizes, the kernels' own durations come from the trace."""
    fmt = alignment.AlignedFormat.matcher()
    lm, w, idx, boxes = faces(n, n)
    fp = alignment.FaceParts.default(68, PATCH)
    one = torch.empty((n, 3) + tuple(fmt.shape(1, *PATCH)[1:]), dtype=fmt.torch_dtype, device="cuda")
    opts = alignment.Openness.default(C)
    out = torch.empty((n, 3, alignment.OPEN_REC), dtype=torch.float64, device="cuda")
    state = torch.tensor(alignment.OPEN_STATE_EMPTY, dtype=torch.float64, device="cuda").repeat(n, 3, 1).contiguous()
    reset = torch.zeros((n,), dtype=torch.int32, device="cuda")
    for ring, ff in bt.rings().values():
        for _ in range(calls):
            alignment.warp_parts_frames_device(ring, lm, fp, weights=w, frame_index_dev=idx, boxes_dev=boxes, fmt=fmt, src=ff,
                                               out=one)
    for _ in range(calls):
        alignment.face_openness_device(lm, opts, weights=w, out=out, state=state, reset=reset, dt=0.04)
        alignment.part_affines_device(lm, fp, weights=w)
    torch.cuda.synchronize()
    print(json.dumps({"bench": "face_parts_trace", "faces": n, "calls": calls}), flush=True)


def main():
    _lib.require_gpu()
    if args.trace:
        return trace(args.trace)
    rec = {"bench": "face_parts", "device": torch.cuda.get_device_name(0), "landmarks": C, "patch": list(PATCH),
           "parent_only": bool(args.parent_only),
           "parts": {"%s_%d" % (src, k): parts(k, src, args.rounds, args.window_ms) for src in ("bgr", "nv12") for k in (64, 1024)},
           "openness": {str(n): openness(n, args.rounds, args.window_ms) for n in (64, 1024)}}
    if not args.skip_step:
        rec["tracker"] = step(args.rounds, args.window_ms)
    if args.parent:     # the same measurements on the parent's tree, in a process of its own
        cmd = [sys.executable, os.path.abspath(__file__), "--parent-only", "--root", args.parent, "--rounds", str(args.rounds),
               "--window-ms", str(args.window_ms)] + (["--skip-step"] if args.skip_step else [])
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("the parent's measurement failed:\n" + r.stderr[-3000:])
        rec["parent"] = json.loads(r.stdout.strip().splitlines()[-1])
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
