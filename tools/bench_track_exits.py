"""What the exit queue costs (the protocol of tools/bench_track.py: one process, the variants ALTERNATING window by window,
HIP events around whole windows, median and [min, max] over the windows).

  launch   alignment.track_retire_device alone at K = 1024 slots, a ring of 256 rows, faces of 112x112x3 bf16 (75264
           bytes), every optional record given: E0 with no track ending (the steady state of a tracker), E0raw the same
           through ctypes without the wrapper's checks (back to back the wrapper is host-bound), E64 with 64 tracks
           ending in every call -- their ids are put back before each call, and R64 is that restore alone.
  step     FaceTracker.step at S = 64 streams of K = 16 slots (the workload of tools/bench_head_pose.py: fcn_8 at 256x256 in
           bf16, a 1080p BGR ring, the matcher's format, best_shot=True), put back to the seeded state before every step:
           P a tracker without exits -- it makes the launches of a tracker as it was before exits existed, and no other --,
           X one with exits=256, P2 the plain one again (the spread), R the restore alone.

Prints one JSON line, and writes it to --out.

    python tools/bench_track_exits.py --out profiles/track_exits.json
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

C, OUT, S, K, Q = 68, 112, 64, 16, 256
FH, FW = 1080, 1920


def launch(k, ending, rounds, window_ms):
    dev = "cuda"
    g = torch.Generator(device=dev)
    g.manual_seed(k)
    fb = OUT * OUT * 3 * 2
    t = dict(
        boxes=torch.tensor([[100, 100, 300, 300]], dtype=torch.int32, device=dev).repeat(k, 1).contiguous(),
        status=torch.zeros((k,), dtype=torch.int32, device=dev), best_q=torch.rand((k,), dtype=torch.float64, device=dev, generator=g),
        gallery=torch.randint(0, 256, (k, fb), dtype=torch.uint8, device=dev, generator=g),
        best_frame=torch.zeros((k,), dtype=torch.int64, device=dev), best_m=torch.zeros((k, 2, 3), dtype=torch.float32, device=dev),
        best_lm=torch.zeros((k, C, 2), dtype=torch.float64, device=dev),
        best_rec=torch.zeros((k, alignment.QUALITY_REC), dtype=torch.int64, device=dev),
        born=torch.zeros((k,), dtype=torch.int32, device=dev), track_id=torch.arange(k, dtype=torch.int64, device=dev),
        born_frame=torch.zeros((k,), dtype=torch.int64, device=dev), head=torch.zeros((4,), dtype=torch.int64, device=dev),
        x_faces=torch.zeros((Q, fb), dtype=torch.uint8, device=dev), x_meta=torch.zeros((Q, alignment.EXIT_META), dtype=torch.int64, device=dev),
        x_q=torch.zeros((Q,), dtype=torch.float64, device=dev), x_m=torch.zeros((Q, 2, 3), dtype=torch.float32, device=dev),
        x_lm=torch.zeros((Q, C, 2), dtype=torch.float64, device=dev),
        x_rec=torch.zeros((Q, alignment.QUALITY_REC), dtype=torch.int64, device=dev),
        exit_row=torch.zeros((k,), dtype=torch.int32, device=dev))
    ids0 = t["track_id"].clone()
    opts = alignment.TrackExits(Q)

    def retire():
        alignment.track_retire_device(t["boxes"], t["status"], (FH, FW), t["best_q"], t["gallery"], t["best_frame"], t["born"],
                                      t["track_id"], t["born_frame"], t["head"], t["x_faces"], t["x_meta"], t["x_q"], t["exit_row"],
                                      7, opts=opts, best_m=t["best_m"], best_lm=t["best_lm"], best_rec=t["best_rec"], x_m=t["x_m"],
                                      x_lm=t["x_lm"], x_rec=t["x_rec"])

    co = opts.struct()
    p = lambda n: _lib.ptr(t[n])
    args = (_lib.stream_ptr(), p("boxes"), p("status"), k, FH, FW, p("best_q"), p("gallery"), fb, p("best_frame"), p("best_m"),
            p("best_lm"), C, p("best_rec"), 7, 0, _lib.C.byref(co), p("born"), p("track_id"), p("born_frame"), p("head"), Q,
            p("x_faces"), p("x_meta"), p("x_q"), p("x_m"), p("x_lm"), p("x_rec"), p("exit_row"))
    call = _lib.load().flm_track_retire

    def raw():                                    # the two launches without the wrapper's checks
        call(*args)

    def restore():
        t["track_id"].copy_(ids0)

    def ending_call():
        restore()
        retire()

    w0 = bt.alternate([("E0", retire), ("E0raw", raw), ("E0b", retire)], rounds, window_ms)
    torch.cuda.synchronize()
    assert int(t["head"][0]) == 0 and int((t["exit_row"] != -1).sum()) == 0
    t["boxes"][::k // ending][:ending] = 0        # `ending` slots spread over the chunk lose their face
    w1 = bt.alternate([("E64", ending_call), ("R64", restore), ("E64b", ending_call)], rounds, window_ms)
    torch.cuda.synchronize()
    assert int((t["exit_row"] >= 0).sum()) == ending
    return {"slots": k, "ring": Q, "face_bytes": fb, "ending": ending, "windows": {**w0, **w1},
            "retire_none_ending_ms": w0["E0"]["median_ms"], "retire_none_ending_raw_ms": w0["E0raw"]["median_ms"],
            "retire_ending_ms": w1["E64"]["median_ms"] - w1["R64"]["median_ms"],
            "spread_E0_ms": w0["E0b"]["median_ms"] - w0["E0"]["median_ms"]}


def step(rounds, window_ms, s=S, k=K):
    model = LANDMARKS_MODELS["fcn_8"](C, input_height=256, input_width=256, dtype="bf16")
    model.load_weights(synth_fcn8_weights(C, seed=2))
    ring, ff = bt.rings()["bgr"]
    fmt = alignment.AlignedFormat.matcher()
    idx = [torch.tensor([(t + i) % 8 for i in range(s)], dtype=torch.int32, device="cuda") for t in range(8)]
    clock = {"t": 0}

    def stepper(**kw):
        tr = prediction.FaceTracker(model, (bt.FH, bt.FW), k * s, streams=s, out_size=(OUT, OUT), aligned_format=fmt,
                                    frame_format=ff, best_shot=True, **kw)
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
    tx, x, _ = stepper(exits=Q)
    w = bt.alternate([("P", p), ("X", x), ("R", restore), ("P2", p)], rounds, window_ms)
    torch.cuda.synchronize()
    res = {"streams": s, "slots_per_stream": k, "ring": Q, "windows": w}
    res["step_plain_ms"] = w["P"]["median_ms"] - w["R"]["median_ms"]
    res["step_exits_ms"] = w["X"]["median_ms"] - w["R"]["median_ms"]
    res["exits_minus_plain_ms"] = w["X"]["median_ms"] - w["P"]["median_ms"]
    res["spread_P_vs_P2_ms"] = w["P2"]["median_ms"] - w["P"]["median_ms"]
    res["exits_share_of_step"] = res["exits_minus_plain_ms"] / res["step_plain_ms"]
    res["head"] = tx.exit_head.tolist()
    res["tracks_named"] = int((tx.track_id >= 0).sum())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=200.0)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    _lib.require_gpu()
    rec = {"bench": "track_exits", "device": torch.cuda.get_device_name(0), "launch": launch(1024, 64, a.rounds, a.window_ms)}
    if not a.skip_step:
        rec["step"] = step(a.rounds, a.window_ms)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
