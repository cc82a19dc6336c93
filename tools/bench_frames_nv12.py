"""The NV12 ring as the stream's source against the BGR ring (the method of tools/bench_align_frames.py: BASELINE
configs[4], the workload of `bench.py --config 5` -- an 8-slot 1080p ring, 64 frames, 1..16 boxes of 96..400 px per
frame, same seed -- one process, the variants ALTERNATING round by round, HIP events around whole steps):

  A   prediction.align_frames on the BGR ring                      (run twice per round: A and A2, whose difference is
                                                                    the run-to-run spread every other difference is read
                                                                    against)
  B   prediction.align_frames(frame_format=nv12) on the NV12 ring   the direct path
  C   prediction.frames_to_bgr_device of the 8 slots the step touches, then A's calls on the result: what an NV12 caller
      has without B

The NV12 ring is a decoder's: pitch 2048, U,V rows from row 1088, BT.709; the BGR ring of A is flm_frames_to_bgr of
it, so all three variants compute on the same pixels and must return the same tensors (checked before anything is
timed).  Then the three frame-reading kernels alone, with the bytes of the shape model (read: side^2 * 3 B per face from
BGR, side^2 * 1.5 B from NV12; written: the crops or the aligned faces) over the mean launch time.  Prints one JSON line.

    python tools/bench_frames_nv12.py                   # bf16 stream; --dtypes f32,bf16 for both
    python tools/bench_frames_nv12.py --kernels-only
"""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import flm_amd  # noqa: F401
from flm_amd import _lib, alignment, prediction
from flm_amd.networks import LANDMARKS_MODELS
from flm_amd.weights import synth_fcn8_weights

OUT = 112
FH, FW, PITCH, UV_ROW = 1080, 1920, 2048, 1088
PEAK_HBM_GBS = 8000.0


def workload(n_frames=64, seed=5):
    """bench_align_frames' workload, its BGR frames taken to NV12 (float transform, chroma as the 2x2 mean) on the device."""
    rng = np.random.default_rng(seed)
    bgr = torch.from_numpy(rng.integers(0, 256, (8, FH, FW, 3), dtype=np.uint8)).cuda()
    faces = []
    for _ in range(n_frames):
        fb = []
        for _ in range(int(rng.integers(1, 17))):
            side = int(rng.integers(96, 401))
            x0, y0 = int(rng.integers(0, FW - side)), int(rng.integers(0, FH - side))
            fb.append((x0, y0, x0 + side, y0 + side))
        faces.append(fb)
    kr, kb = 0.2126, 0.0722
    b, g, r = [bgr[..., c].float() for c in range(3)]
    yf = kr * r + (1 - kr - kb) * g + kb * b
    cb = ((b - yf) / (2 * (1 - kb))).view(8, FH // 2, 2, FW // 2, 2).mean((2, 4))
    cr = ((r - yf) / (2 * (1 - kr))).view(8, FH // 2, 2, FW // 2, 2).mean((2, 4))
    ring = torch.randint(0, 256, (8, UV_ROW + FH // 2, PITCH), dtype=torch.uint8, device="cuda")
    ring[:, :FH, :FW] = (16 + 219 * yf / 255).round().clamp(0, 255).to(torch.uint8)
    uv = torch.stack([(128 + 224 * cb / 255).round().clamp(0, 255), (128 + 224 * cr / 255).round().clamp(0, 255)], -1)
    ring[:, UV_ROW:, :FW] = uv.to(torch.uint8).view(8, FH // 2, FW)
    del bgr
    return ring, faces, [f % 8 for f in range(n_frames)]


def event_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def stats(v):
    v = sorted(v)
    return {"median_ms": v[len(v) // 2], "min_ms": v[0], "max_ms": v[-1]}


def pipelines(dtype, ring, bgr, nv, faces, slots, rounds, window_ms, samples):
    model = LANDMARKS_MODELS["fcn_8"](68, input_height=256, input_width=256, dtype=dtype)
    model.load_weights(synth_fcn8_weights(68, seed=2))
    scratch = torch.empty_like(bgr)
    kw = dict(out_size=(OUT, OUT), n_points=4, frame_index=slots, samples=samples)

    def a():
        return prediction.align_frames(bgr, faces, model, **kw)

    def b():
        return prediction.align_frames(ring, faces, model, frame_format=nv, **kw)

    def c():
        prediction.frames_to_bgr_device(ring, nv, out=scratch)
        return prediction.align_frames(scratch, faces, model, **kw)

    variants = [("A", a), ("B", b), ("A2", a), ("C", c)]
    ref = [t.clone() for t in a()]
    same = {name: all(torch.equal(x, y) for x, y in zip(fn(), ref)) for name, fn in variants}   # (also the warm-up)
    if not all(same.values()):
        sys.exit("bench_frames_nv12: the variants do not return A's tensors (%s): nothing is timed" % same)
    for _, fn in variants:
        fn()
    torch.cuda.synchronize()
    reps = max(2, int(math.ceil(window_ms / event_ms(a, 2))))
    times = {name: [] for name, _ in variants}
    for _ in range(rounds):
        for name, fn in variants:
            times[name].append(event_ms(fn, reps))
    k = sum(len(f) for f in faces)
    res = {"faces_per_step": k, "steps_per_window": reps, "windows": rounds, "samples": samples, "same_tensors_as_A": same}
    for name in times:
        res[name] = stats(times[name])
        res[name]["faces_per_s"] = 1e3 * k / res[name]["median_ms"]
    res["spread_A_vs_A2"] = {"median_diff_ms": res["A2"]["median_ms"] - res["A"]["median_ms"],
                             "window_range_ms": max(times["A"] + times["A2"]) - min(times["A"] + times["A2"])}
    res["B_vs_C_ms"] = res["B"]["median_ms"] - res["C"]["median_ms"]
    res["B_vs_A_ms"] = res["B"]["median_ms"] - res["A"]["median_ms"]
    res["C_vs_A_ms"] = res["C"]["median_ms"] - res["A"]["median_ms"]
    del model
    return res


def box_fit_matrices(boxes, rng):
    """Each face box onto the aligned square, rotated by up to 0.2 rad about its centre (what a trained model would give)."""
    k = boxes.shape[0]
    mf = np.zeros((k, 2, 3), np.float32)
    for i in range(k):
        th = rng.uniform(-0.2, 0.2)
        side = float(boxes[i, 2] - boxes[i, 0])
        s, cx, cy = OUT / side, boxes[i, 0] + side / 2, boxes[i, 1] + side / 2
        a, b = s * np.cos(th), s * np.sin(th)
        mf[i] = [[a, -b, OUT / 2 - (a * cx - b * cy)], [b, a, OUT / 2 - (b * cx + a * cy)]]
    return torch.from_numpy(mf).cuda()


def kernels_alone(ring, bgr, nv, faces, slots, reps=20):
    crops, _, boxes_dev, idx_dev = prediction.crop_frames_device(bgr, faces, 256, 256, frame_index=slots, return_device=True)
    boxes = boxes_dev.cpu().numpy()
    k = boxes.shape[0]
    side = (boxes[:, 2] - boxes[:, 0]).astype(np.int64)
    area = int((side * side).sum())
    m = box_fit_matrices(boxes, np.random.default_rng(7))
    dst = torch.empty((k, OUT, OUT, 3), dtype=torch.float32, device="cuda")
    fmt = alignment.AlignedFormat.matcher("float16")
    dst16 = torch.empty(fmt.shape(k, OUT, OUT), dtype=torch.float16, device="cuda")
    scratch = torch.empty_like(bgr)
    crop_out, warp_out, warp16_out = k * 256 * 256 * 3, k * OUT * OUT * 12, k * OUT * OUT * 6
    # the crops as the warps: boxes and slots on the device already, the C calls alone
    lib, C = _lib.load(), _lib.C
    crop_dst = torch.empty((k, 256, 256, 3), dtype=torch.uint8, device="cuda")
    cs = nv.struct(ring)
    nv_stride = ring[0].numel()

    def crop_bgr():
        _lib.check(lib.flm_crop_resize_frames(_lib.stream_ptr(), _lib.ptr(bgr), FH * FW * 3, 8, FH, FW, _lib.ptr(boxes_dev),
                                              _lib.ptr(idx_dev), k, _lib.ptr(crop_dst), 256, 256), "flm_crop_resize_frames")

    def crop_nv12():
        _lib.check(lib.flm_crop_resize_frames_src(_lib.stream_ptr(), _lib.ptr(ring), nv_stride, 8, FH, FW, _lib.ptr(boxes_dev),
                                                  _lib.ptr(idx_dev), k, _lib.ptr(crop_dst), 256, 256, C.byref(cs)),
                   "flm_crop_resize_frames_src")

    crop_nv12()
    if not torch.equal(crop_dst, crops):
        sys.exit("bench_frames_nv12: the NV12 crops are not the BGR crops: nothing is timed")
    runs = [("frames_to_bgr_8_slots", 8 * FH * FW * 3 // 2 + 8 * FH * FW * 3,
             lambda: prediction.frames_to_bgr_device(ring, nv, out=scratch)),
            ("crop_bgr", area * 3 + crop_out, crop_bgr), ("crop_nv12", area * 3 // 2 + crop_out, crop_nv12)]
    for s in (1, 2, 4):
        runs.append(("warp_bgr_s%d" % s, area * 3 + warp_out,
                     lambda s=s: alignment.warp_frames_device(bgr, m, OUT, OUT, frame_index_dev=idx_dev, boxes_dev=boxes_dev,
                                                              samples=s, out=dst)))
        runs.append(("warp_nv12_s%d" % s, area * 3 // 2 + warp_out,
                     lambda s=s: alignment.warp_frames_device(ring, m, OUT, OUT, frame_index_dev=idx_dev, boxes_dev=boxes_dev,
                                                              samples=s, out=dst, src=nv)))
    runs.append(("warp_bgr_matcher_f16_s2", area * 3 + warp16_out,
                 lambda: alignment.warp_frames_device(bgr, m, OUT, OUT, frame_index_dev=idx_dev, boxes_dev=boxes_dev, samples=2,
                                                      out=dst16, fmt=fmt)))
    runs.append(("warp_nv12_matcher_f16_s2", area * 3 // 2 + warp16_out,
                 lambda: alignment.warp_frames_device(ring, m, OUT, OUT, frame_index_dev=idx_dev, boxes_dev=boxes_dev, samples=2,
                                                      out=dst16, fmt=fmt, src=nv)))
    rec = {"faces": k, "note": "the model's bytes count every face's box once, not the lines a gather really touches"}
    for name, nbytes, fn in runs:
        fn()
        fn()
        torch.cuda.synchronize()
        ms = min(event_ms(fn, reps) for _ in range(3))
        rec[name] = {"avg_launch_ms": ms, "bytes_model": nbytes, "gb_per_s": nbytes / ms / 1e6,
                     "frac_of_8tb_s": nbytes / ms / 1e6 / PEAK_HBM_GBS}
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtypes", default="bf16")
    ap.add_argument("--rounds", type=int, default=7, help="alternating rounds (timed windows per variant)")
    ap.add_argument("--window-ms", type=float, default=300.0, help="least length of one timed window")
    ap.add_argument("--samples", type=int, default=2, help="samples per axis of the alignment warp in the steps")
    ap.add_argument("--kernels-only", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_frames_nv12: no GPU visible (there is nothing to measure on a CPU)")
    ring, faces, slots = workload()
    nv = alignment.FrameFormat.nv12(FH, FW, matrix="bt709", uv_row=UV_ROW)
    bgr = prediction.frames_to_bgr_device(ring, nv)
    rec = {"bench": "frames_nv12", "device": torch.cuda.get_device_name(0), "out_size": [OUT, OUT],
           "ring": {"slots": 8, "frame": [FH, FW], "pitch": PITCH, "uv_row": UV_ROW, "matrix": "bt709",
                    "nv12_bytes": ring.numel(), "bgr_bytes": bgr.numel()}}
    if not args.kernels_only:
        for dt in args.dtypes.split(","):
            rec["stream_" + dt] = pipelines(dt, ring, bgr, nv, faces, slots, args.rounds, args.window_ms, args.samples)
    rec["kernels_alone"] = kernels_alone(ring, bgr, nv, faces, slots)
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
