"""The tracker's per-frame step against the path that starts from detector boxes, and the fused flm_track_step against
the separate launches it replaces (one process, the variants ALTERNATING round by round, HIP events around whole
windows, median and range over the windows; the method of tools/bench_frames_nv12.py).

  stream   an 8-slot 1080p ring (BGR, and a decoder's NV12: pitch 2048, U,V rows from row 1088, BT.709), K = 1, 8, 64
           faces of 96..400 px in one frame, fcn_8 with 256x256 input, bf16 and f32:
             T   FaceTracker.step -- no upload; before every step the tracker's matrices and boxes are put back to the
                 seeded state by two device copies (a few KiB, inside the timed window), so that every step cuts the
                 same K crops whatever the random-weight network says about them
             A   prediction.align_frames on the same K detector boxes: box maths on the host, one upload, crop / resize,
                 forward, flm_landmarks_to_frame, the fit, the aligned warp.  align_frames is what it was before the
                 tracker existed, so A is that path as it stands
           T and A run the same forward and the same aligned warp; they differ in the front (a rotated uint8 warp
           against crop / resize behind an upload) and in the launches between the forward and the aligned warp.
  fused    flm_track_step alone against flm_landmarks_from_crop + two flm_similarity_from_landmarks_weighted calls on
           the same faces (68 landmarks): three of the launches it replaces -- the status tests and the box have no
           launch of their own to compare with.  Thousands of back-to-back launches per window: the time per call is
           launch-bound, which is the point of fusing.
  --smooth adds to every stream row
             S   FaceTracker(smooth=True).step, put back to the seeded state like T (the filter state keeps its
                 history: every step filters); the same launches as T, the track step with its One-Euro filter
           and to every fused row flm_track_step_filtered on the same faces.
  --still N  (instead of the timings) a still scene: one 1080p BGR frame repeated N times with fresh noise of +-2 grey
           levels on every repeat, 8 faces, bf16; a tracker with smooth=True and one without follow it from the same
           seed, twice: in closed loop (every crop placed by the landmarks before it), and with the crop held (matrices
           and boxes put back to the seeded state before every step, as in the stream rows: the decode's answer to the
           pixel noise on a fixed crop is then the filter's only input).  Reports, over the repeats after the first 10
           and over the tracks both trackers kept throughout, the standard deviation over time of the landmarks (frame
           px) and of the entries of m_align (its translation in aligned px), filtered against unfiltered, and how
           many tracks were alive after 1, 2, 5, ... repeats (with random weights the closed loop loses them).

Prints one JSON line, and writes it to --out.

    python tools/bench_track.py --out profiles/track_step.json
    python tools/bench_track.py --smooth --out profiles/track_step_smooth.json
    python tools/bench_track.py --still 200 --out profiles/track_still.json
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


def rings(seed=5):
    """An NV12 ring of random bytes and the BGR ring the kernels compute from it: both paths see the same pixels."""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    ring = torch.randint(0, 256, (8, UV_ROW + FH // 2, PITCH), dtype=torch.uint8, device="cuda", generator=g)
    nv = alignment.FrameFormat.nv12(FH, FW, matrix="bt709", uv_row=UV_ROW)
    return {"bgr": (prediction.frames_to_bgr_device(ring, nv), None), "nv12": (ring, nv)}


def boxes_for(k, seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(k):
        side = int(rng.integers(96, 401))
        x0, y0 = int(rng.integers(0, FW - side)), int(rng.integers(0, FH - side))
        out.append((x0, y0, x0 + side, y0 + side))
    return out


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
    return {"median_ms": v[len(v) // 2], "min_ms": v[0], "max_ms": v[-1], "windows": len(v)}


def alternate(variants, rounds, window_ms):
    """Every variant warmed, then `rounds` rounds of one timed window per variant, in turn."""
    for _, fn in variants:
        fn()
        fn()
    torch.cuda.synchronize()
    reps = {name: max(2, int(math.ceil(window_ms / max(event_ms(fn, 2), 1e-4)))) for name, fn in variants}
    times = {name: [] for name, _ in variants}
    for _ in range(rounds):
        for name, fn in variants:
            times[name].append(event_ms(fn, reps[name]))
    res = {name: dict(stats(t), calls_per_window=reps[name]) for name, t in times.items()}
    return res


def stream(model, ring, ff, k, rounds, window_ms, samples, smooth=False):
    faces = boxes_for(k, 11 + k)
    tr = prediction.FaceTracker(model, (FH, FW), k, out_size=(OUT, OUT), samples=samples, frame_format=ff)
    tr.seed(range(k), faces)
    m0, b0 = tr.m_crop.clone(), tr.boxes.clone()
    state = {"t": 0}

    def stepper(tracker):
        def fn():
            tracker.m_crop.copy_(m0)
            tracker.boxes.copy_(b0)
            state["t"] += 1
            return tracker.step(ring, state["t"] % 8)
        return fn

    t = stepper(tr)

    def a():
        state["t"] += 1
        return prediction.align_frames(ring, [faces], model, out_size=(OUT, OUT), n_points=4, frame_index=[state["t"] % 8],
                                       samples=samples, frame_format=ff)

    variants = [("T", t), ("A", a), ("T2", t)]
    if smooth:
        ts = prediction.FaceTracker(model, (FH, FW), k, out_size=(OUT, OUT), samples=samples, frame_format=ff, smooth=True)
        ts.seed(range(k), faces)
        variants.insert(1, ("S", stepper(ts)))
    res = alternate(variants, rounds, window_ms)
    res["tracked_after_one_step"] = int((t()[3] == 0).sum())
    res["faces"] = k
    res["T_vs_A_ms"] = res["T"]["median_ms"] - res["A"]["median_ms"]
    res["spread_T_vs_T2_ms"] = res["T2"]["median_ms"] - res["T"]["median_ms"]
    if smooth:
        res["S_vs_T_ms"] = res["S"]["median_ms"] - res["T"]["median_ms"]
    return res


def fused(k, c, rounds, window_ms, smooth=False):
    rng = np.random.default_rng(3)
    tc = torch.from_numpy(alignment.canonical_template(c, 256, 256)).cuda()
    ta = torch.from_numpy(alignment.canonical_template(c, OUT, OUT)).cuda()
    boxes = torch.from_numpy(np.asarray(prediction.face_boxes(boxes_for(k, 11 + k)), np.int32)).cuda()
    m, _ = alignment.track_seed_device(boxes, (256, 256), (FH, FW))
    lm = torch.from_numpy(alignment.canonical_template(c, 264, 264)[None] + rng.normal(0, 2.0, (k, c, 2))).cuda()
    w = torch.from_numpy(rng.uniform(0.1, 1.0, (k, c))).cuda()
    o = dict(lm_frame=torch.empty((k, c, 2), dtype=torch.float64, device="cuda"),
             m_align=torch.empty((k, 2, 3), dtype=torch.float32, device="cuda"),
             m_next=torch.empty((k, 2, 3), dtype=torch.float32, device="cuda"),
             boxes_next=torch.empty((k, 4), dtype=torch.int32, device="cuda"),
             status=torch.empty((k,), dtype=torch.int32, device="cuda"))
    lib, C = _lib.load(), _lib.C
    opts = _lib.TrackOpts.make()
    s = 256 / 264
    sep_lm, sep_a, sep_n = torch.empty_like(o["lm_frame"]), torch.empty_like(o["m_align"]), torch.empty_like(o["m_next"])

    def one():
        _lib.check(lib.flm_track_step(_lib.stream_ptr(), _lib.ptr(lm), 2, _lib.ptr(w), 1, _lib.ptr(m), _lib.ptr(boxes), k, c, s, s,
                                      256, 256, FH, FW, _lib.ptr(tc), _lib.ptr(ta), C.byref(opts), _lib.ptr(o["lm_frame"]),
                                      _lib.ptr(o["m_align"]), _lib.ptr(o["m_next"]), _lib.ptr(o["boxes_next"]),
                                      _lib.ptr(o["status"])), "flm_track_step")

    filt = _lib.TrackFilter.make()
    fstate = torch.full((k, c, 6), -1.0, dtype=torch.float64, device="cuda")

    def filtered():
        _lib.check(lib.flm_track_step_filtered(_lib.stream_ptr(), _lib.ptr(lm), 2, _lib.ptr(w), 1, _lib.ptr(m), _lib.ptr(boxes), k,
                                               c, s, s, 256, 256, FH, FW, _lib.ptr(tc), _lib.ptr(ta), C.byref(opts),
                                               _lib.ptr(o["lm_frame"]), _lib.ptr(o["m_align"]), _lib.ptr(o["m_next"]),
                                               _lib.ptr(o["boxes_next"]), _lib.ptr(o["status"]), C.byref(filt), 1.0 / 30.0,
                                               _lib.ptr(fstate), None), "flm_track_step_filtered")

    def three():
        sp = _lib.stream_ptr()
        _lib.check(lib.flm_landmarks_from_crop(sp, _lib.ptr(lm), 2, _lib.ptr(m), k, c, s, s, _lib.ptr(sep_lm)), "from_crop")
        for t, dst in ((ta, sep_a), (tc, sep_n)):
            _lib.check(lib.flm_similarity_from_landmarks_weighted(sp, _lib.ptr(sep_lm), 2, _lib.ptr(w), 1, _lib.ptr(t), k, c, 1.0,
                                                                  1.0, _lib.ptr(dst)), "fit")

    one()
    three()
    torch.cuda.synchronize()
    ok = o["status"] == 0
    if not (torch.equal(o["lm_frame"], sep_lm) and torch.equal(o["m_align"], sep_a) and torch.equal(o["m_next"][ok], sep_n[ok])):
        sys.exit("bench_track: the fused step does not return the separate calls' tensors: nothing is timed")
    variants = [("fused", one), ("three_launches", three), ("fused2", one)]
    if smooth:
        variants.insert(1, ("filtered", filtered))
    res = alternate(variants, rounds, window_ms)
    if smooth:
        res["filtered_vs_fused_ms"] = res["filtered"]["median_ms"] - res["fused"]["median_ms"]
    res.update(faces=k, landmarks=c, tracked=int(ok.sum()),
               fused_vs_three_ms=res["fused"]["median_ms"] - res["three_launches"]["median_ms"],
               spread_fused_vs_fused2_ms=res["fused2"]["median_ms"] - res["fused"]["median_ms"])
    return res


def still(model, n, k, samples, hold, skip=10, seed=17):
    """The still scene of the module's docstring -> the jitter of both trackers; hold: the crop is held."""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    # a textured frame: blocks of 8 px of random colour under fine grain, so that the bilinear crops have structure
    coarse = torch.randint(32, 224, (1, 3, FH // 8, FW // 8), device="cuda", generator=g).float()
    base = torch.nn.functional.interpolate(coarse, size=(FH, FW), mode="bilinear", align_corners=False)[0].permute(1, 2, 0)
    base = base + torch.randint(-12, 13, (FH, FW, 3), device="cuda", generator=g).float()
    ring = torch.zeros((8, FH, FW, 3), dtype=torch.uint8, device="cuda")
    faces = boxes_for(k, 11 + k)
    trackers = {}
    for name, smooth in (("filtered", True), ("unfiltered", None)):
        tr = prediction.FaceTracker(model, (FH, FW), k, out_size=(OUT, OUT), samples=samples, smooth=smooth)
        tr.seed(range(k), faces)
        trackers[name] = (tr, [], [], [])
    m0, b0 = tr.m_crop.clone(), tr.boxes.clone()
    for r in range(n):
        noise = torch.randint(-2, 3, (FH, FW, 3), device="cuda", generator=g).float()
        ring[r % 8] = (base + noise).clamp_(0, 255).to(torch.uint8)
        for tr, lms, ms, sts in trackers.values():
            if hold:
                tr.m_crop.copy_(m0)
                tr.boxes.copy_(b0)
            _, m_align, lm, st = tr.step(ring, r % 8)
            lms.append(lm.clone())
            ms.append(m_align.clone())
            sts.append(st.clone())
    kept = torch.ones((k,), dtype=torch.bool, device="cuda")
    for _, _, _, sts in trackers.values():
        kept &= (torch.stack(sts) == 0).all(0)
    res = {"repeats": n, "skipped": skip, "faces": k, "tracks_kept_by_both": int(kept.sum()), "noise_grey_levels": 2}
    marks = [r for r in (1, 2, 3, 5, 10, 20, 50, 100, 200, 500, 1000) if r <= n]
    for name, (_, lms, ms, sts) in trackers.items():
        alive = (torch.stack(sts) == 0).cumprod(0).sum(1).tolist()
        res["alive_after_" + name] = {str(r): int(alive[r - 1]) for r in marks}
    for name, (_, lms, ms, _) in trackers.items():
        lm = torch.stack(lms[skip:])[:, kept]                  # [T, kept, C, 2]
        ma = torch.stack(ms[skip:])[:, kept].double()          # [T, kept, 2, 3]
        row = {}
        if int(kept.sum()):
            ok = (lm >= 0).all(0).all(-1)                      # points never rejected
            sd = lm.std(0)[ok]                                 # [points, 2]
            row["landmark_std_px_mean"] = float(sd.mean())
            row["landmark_std_px_median"] = float(sd.median())
            row["landmark_std_px_max"] = float(sd.max())
            row["points"] = int(ok.sum())
            msd = ma.std(0)
            row["m_align_translation_std_px_mean"] = float(msd[:, :, 2].mean())
            row["m_align_linear_std_mean"] = float(msd[:, :, :2].mean())
        res[name] = row
    if res["filtered"] and res["unfiltered"]:
        for key in ("landmark_std_px_mean", "m_align_translation_std_px_mean", "m_align_linear_std_mean"):
            res["ratio_" + key] = res["filtered"][key] / max(res["unfiltered"][key], 1e-300)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtypes", default="bf16,f32")
    ap.add_argument("--faces", default="1,8,64")
    ap.add_argument("--sources", default="bgr,nv12")
    ap.add_argument("--rounds", type=int, default=5, help="alternating rounds (timed windows per variant)")
    ap.add_argument("--window-ms", type=float, default=250.0, help="least length of one timed window")
    ap.add_argument("--samples", type=int, default=2, help="samples per axis of the aligned warp")
    ap.add_argument("--smooth", action="store_true", help="add the rows of the smoothing tracker and the filtered step")
    ap.add_argument("--still", type=int, default=0, metavar="N",
                    help="instead of the timings: the jitter over N noisy repeats of one frame, filtered against unfiltered")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_track: no GPU visible (there is nothing to measure on a CPU)")
    if args.still:
        model = LANDMARKS_MODELS["fcn_8"](68, input_height=256, input_width=256, dtype="bf16")
        model.load_weights(synth_fcn8_weights(68, seed=2))
        rec = {"bench": "track_still", "device": torch.cuda.get_device_name(0), "out_size": [OUT, OUT], "frame": [FH, FW],
               "model": "fcn_8 68 classes 256x256 bf16", "aligned_samples": args.samples,
               "closed_loop": still(model, args.still, 8, args.samples, False),
               "held_crop": still(model, args.still, 8, args.samples, True)}
        emit(rec, args.out)
        return
    ks = [int(v) for v in args.faces.split(",")]
    rec = {"bench": "track_step", "device": torch.cuda.get_device_name(0), "out_size": [OUT, OUT], "frame": [FH, FW],
           "model": "fcn_8 68 classes 256x256", "aligned_samples": args.samples, "stream": {}, "fused": {}}
    src = rings()
    for dt in args.dtypes.split(","):
        model = LANDMARKS_MODELS["fcn_8"](68, input_height=256, input_width=256, dtype=dt)
        model.load_weights(synth_fcn8_weights(68, seed=2))
        for name in args.sources.split(","):
            ring, ff = src[name]
            for k in ks:
                rec["stream"]["%s_%s_k%d" % (dt, name, k)] = stream(model, ring, ff, k, args.rounds, args.window_ms, args.samples,
                                                                        args.smooth)
                print("# %s %s k=%d done" % (dt, name, k), file=sys.stderr, flush=True)
        del model
    for k in ks:
        rec["fused"]["k%d" % k] = fused(k, 68, args.rounds, args.window_ms, args.smooth)
    emit(rec, args.out)


def emit(rec, out):
    print(json.dumps(rec), flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
