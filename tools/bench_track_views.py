"""What the pose-binned best shots cost (the protocol of tools/bench_track.py: one process, the variants ALTERNATING window
by window, HIP events around whole windows, median and [min, max] over the windows).

  launch   flm_track_views_update through ctypes (back to back the wrapper is host-bound) at N = 64 and N = 1024 rows, B = 3
           bins, faces of 112x112x3 float16 (75264 bytes), every optional record given: U0 with no face taken (every bin
           already holds a better one: the steady state of a tracker), U1 with every face taken (a reset in every row: N
           faces copied per call), W0 the wrapper of U0.  flm_track_exit_views at K = 1024 slots and a ring of 256: X0 with
           no slot exiting, X64 with 64.
  step     FaceTracker.step at S = 64 streams of K = 16 slots (the workload of tools/bench_track_exits.py: fcn_8 at 256x256
           in bf16, a 1080p BGR ring, the matcher's format) with best_shot, pose and exits=256, put back to the seeded state
           before every step: P a tracker without views -- it makes the launches of a tracker as it was before views
           existed, and no other --, V one with views=True, P2 the plain one again (the spread), R the restore alone.

Prints one JSON line, and writes it to --out.

    python tools/bench_track_views.py --out profiles/track_views.json
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

C, OUT, S, K, Q, B = 68, 112, 64, 16, 256, 3
FB = OUT * OUT * 3 * 2


def update_launch(n, rounds, window_ms):
    dev = "cuda"
    g = torch.Generator(device=dev)
    g.manual_seed(n)
    rec = torch.zeros((n, 8), dtype=torch.int64, device=dev)
    rec[:, 0], rec[:, 3], rec[:, 5] = 12544, 12100, 12100 * 256 * 50      # sharpness 50 of sharp_ref 100, all exposed
    pose = torch.zeros((n, alignment.POSE_REC), dtype=torch.float64, device=dev)
    pose[:, 14] = 1.0
    pose[:, 6] = torch.rand((n,), dtype=torch.float64, device=dev, generator=g) * 1.6 - 0.8   # all three bins
    t = dict(faces=torch.randint(0, 256, (n, FB), dtype=torch.uint8, device=dev, generator=g), rec=rec,
             lm=torch.rand((n, C, 2), dtype=torch.float64, device=dev, generator=g) * 100.0,
             w=torch.rand((n, C), dtype=torch.float64, device=dev, generator=g), status=torch.zeros((n,), dtype=torch.int32, device=dev),
             reset0=torch.zeros((n,), dtype=torch.int32, device=dev), reset1=torch.ones((n,), dtype=torch.int32, device=dev),
             m=torch.zeros((n, 2, 3), dtype=torch.float32, device=dev), pose=pose,
             view_q=torch.full((n, B), 2.0, dtype=torch.float64, device=dev), view_frame=torch.zeros((n, B), dtype=torch.int64, device=dev),
             view_gallery=torch.zeros((n, B, FB), dtype=torch.uint8, device=dev), view_m=torch.zeros((n, B, 2, 3), dtype=torch.float32, device=dev),
             view_lm=torch.zeros((n, B, C, 2), dtype=torch.float64, device=dev),
             view_pose=torch.zeros((n, B, alignment.POSE_REC), dtype=torch.float64, device=dev),
             take=torch.zeros((n,), dtype=torch.int32, device=dev))
    opts = alignment.PoseViews()
    co = opts.struct()
    p = lambda name: _lib.ptr(t[name])
    call = _lib.load().flm_track_views_update

    def args(reset):
        return (_lib.stream_ptr(), p("faces"), FB, n, p("rec"), p("status"), p(reset), p("lm"), 2, p("w"), 1, C, p("m"), 7,
                _lib.C.byref(co), None, 0, p("pose"), p("view_q"), p("view_frame"), p("view_gallery"), p("view_m"), p("view_lm"),
                p("view_pose"), p("take"))

    a0, a1 = args("reset0"), args("reset1")

    def none_taken():
        call(*a0)

    def all_taken():                              # the reset empties the bins, so the face is taken again in every call
        call(*a1)

    def wrapper():
        alignment.track_views_update_device(t["faces"], t["rec"], t["lm"], t["pose"], t["view_q"], t["view_frame"], t["view_gallery"],
                                            t["take"], 7, status=t["status"], reset=t["reset0"], weights=t["w"], m=t["m"], opts=opts,
                                            view_m=t["view_m"], view_lm=t["view_lm"], view_pose=t["view_pose"])

    w0 = bt.alternate([("U0", none_taken), ("W0", wrapper), ("U0b", none_taken)], rounds, window_ms)
    torch.cuda.synchronize()
    assert int((t["take"] >= 0).sum()) == 0
    w1 = bt.alternate([("U1", all_taken), ("U1b", all_taken)], rounds, window_ms)
    torch.cuda.synchronize()
    assert int((t["take"] >= 0).sum()) == n
    t["view_q"].fill_(2.0)
    return {"rows": n, "bins": B, "face_bytes": FB, "windows": {**w0, **w1}, "none_taken_ms": w0["U0"]["median_ms"],
            "none_taken_wrapper_ms": w0["W0"]["median_ms"], "all_taken_ms": w1["U1"]["median_ms"],
            "all_taken_gbytes_per_s": 2 * n * FB / (w1["U1"]["median_ms"] * 1e-3) / 1e9,
            "spread_U0_ms": w0["U0b"]["median_ms"] - w0["U0"]["median_ms"]}


def exit_launch(k, exiting, rounds, window_ms):
    dev = "cuda"
    g = torch.Generator(device=dev)
    g.manual_seed(k)
    t = dict(view_q=torch.rand((k, B), dtype=torch.float64, device=dev, generator=g), view_frame=torch.zeros((k, B), dtype=torch.int64, device=dev),
             view_gallery=torch.randint(0, 256, (k, B, FB), dtype=torch.uint8, device=dev, generator=g),
             view_m=torch.zeros((k, B, 2, 3), dtype=torch.float32, device=dev), view_lm=torch.zeros((k, B, C, 2), dtype=torch.float64, device=dev),
             view_pose=torch.zeros((k, B, alignment.POSE_REC), dtype=torch.float64, device=dev),
             x_view_q=torch.zeros((Q, B), dtype=torch.float64, device=dev), x_view_frame=torch.zeros((Q, B), dtype=torch.int64, device=dev),
             x_view_gallery=torch.zeros((Q, B, FB), dtype=torch.uint8, device=dev), x_view_m=torch.zeros((Q, B, 2, 3), dtype=torch.float32, device=dev),
             x_view_lm=torch.zeros((Q, B, C, 2), dtype=torch.float64, device=dev),
             x_view_pose=torch.zeros((Q, B, alignment.POSE_REC), dtype=torch.float64, device=dev),
             none=torch.full((k,), -1, dtype=torch.int32, device=dev), some=torch.full((k,), -1, dtype=torch.int32, device=dev))
    t["some"][::k // exiting][:exiting] = torch.arange(exiting, dtype=torch.int32, device=dev)
    p = lambda name: _lib.ptr(t[name])
    call = _lib.load().flm_track_exit_views

    def args(rows):
        return (_lib.stream_ptr(), p(rows), k, Q, B, FB, C, p("view_q"), p("view_frame"), p("view_gallery"), p("view_m"), p("view_lm"),
                p("view_pose"), p("x_view_q"), p("x_view_frame"), p("x_view_gallery"), p("x_view_m"), p("x_view_lm"), p("x_view_pose"))

    a0, a1 = args("none"), args("some")
    w = bt.alternate([("X0", lambda: call(*a0)), ("X64", lambda: call(*a1)), ("X0b", lambda: call(*a0))], rounds, window_ms)
    torch.cuda.synchronize()
    assert torch.equal(t["x_view_gallery"][:exiting], t["view_gallery"][::k // exiting][:exiting])
    return {"slots": k, "ring": Q, "bins": B, "face_bytes": FB, "exiting": exiting, "windows": w,
            "none_exiting_ms": w["X0"]["median_ms"], "exiting_ms": w["X64"]["median_ms"],
            "spread_X0_ms": w["X0b"]["median_ms"] - w["X0"]["median_ms"]}


def step(rounds, window_ms, s=S, k=K):
    model = LANDMARKS_MODELS["fcn_8"](C, input_height=256, input_width=256, dtype="bf16")
    model.load_weights(synth_fcn8_weights(C, seed=2))
    ring, ff = bt.rings()["bgr"]
    fmt = alignment.AlignedFormat.matcher()
    idx = [torch.tensor([(t + i) % 8 for i in range(s)], dtype=torch.int32, device="cuda") for t in range(8)]
    clock = {"t": 0}

    def stepper(**kw):
        tr = prediction.FaceTracker(model, (bt.FH, bt.FW), k * s, streams=s, out_size=(OUT, OUT), aligned_format=fmt,
                                    frame_format=ff, best_shot=True, pose=True, exits=Q, **kw)
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
    tv, v, _ = stepper(views=True)
    w = bt.alternate([("P", p), ("V", v), ("R", restore), ("P2", p)], rounds, window_ms)
    torch.cuda.synchronize()
    res = {"streams": s, "slots_per_stream": k, "ring": Q, "bins": tv.view_opts.bins, "windows": w}
    res["step_plain_ms"] = w["P"]["median_ms"] - w["R"]["median_ms"]
    res["step_views_ms"] = w["V"]["median_ms"] - w["R"]["median_ms"]
    res["views_minus_plain_ms"] = w["V"]["median_ms"] - w["P"]["median_ms"]
    res["spread_P_vs_P2_ms"] = w["P2"]["median_ms"] - w["P"]["median_ms"]
    res["views_share_of_step"] = res["views_minus_plain_ms"] / res["step_plain_ms"]
    res["bins_filled"] = int((tv.view_q >= 0).sum())
    res["taken_in_last_step"] = int((tv._view_take >= 0).sum())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=200.0)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    _lib.require_gpu()
    rec = {"bench": "track_views", "device": torch.cuda.get_device_name(0),
           "update": [update_launch(n, a.rounds, a.window_ms) for n in (64, 1024)],
           "exit_views": exit_launch(1024, 64, a.rounds, a.window_ms)}
    if not a.skip_step:
        rec["step"] = step(a.rounds, a.window_ms)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
