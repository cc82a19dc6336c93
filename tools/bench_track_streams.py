"""Several streams in one tracker against one tracker per stream (the protocol of tools/bench_track_assoc.py: one
process, the variants ALTERNATING window by window, 5 windows of at least 200 ms each, median and range over the windows;
HIP events around whole windows).

  assoc   for S = 1, 8, 64 streams at (K, D) = (16,16) and (64,64) slots and detections PER STREAM, on the clustered
          scenes of tools/bench_track_assoc.py (one seed per stream), 68 landmarks of filter state, max_misses = 2,
          refresh_iou = 0.6:
            batched     ONE flm_track_associate_streams call
            per_stream  S flm_track_associate calls on the streams' slices of the same tensors, one after the other:
                        what a caller does without the batched call
          The calls edit the tracker's state, so it is put back before every repetition by five device copies inside
          the timed window; "restore" is those copies alone, and "*_ms" the difference of the medians.  "*_steady" is
          the same repeated on the state it left, nothing put back.
  step    FaceTracker(streams=S, capacity=16*S).step against S trackers of capacity 16 stepped one after the other
          (fcn_8 at 256x256, bf16, a 1080p BGR ring of 8 slots, the matcher's format; stream i reads ring slot
          (t + i) % 8); the trackers are put back to their seeded state before every step, as in tools/bench_track.py,
          and those copies are measured alone too.

Prints one JSON line, and writes it to --out after each part.

    python tools/bench_track_streams.py --out profiles/track_streams.json
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import flm_amd  # noqa: F401
from flm_amd import _lib, alignment, prediction
from flm_amd.networks import LANDMARKS_MODELS
from flm_amd.weights import synth_fcn8_weights

import bench_track as bt

FH, FW, IN, C = 270, 480, 64, 68
SIZES = [(16, 16), (64, 64)]
STREAMS = [1, 8, 64]
OPTS = dict(max_misses=2, refresh_iou=0.6)
OUT = 112


def clustered(k, d, seed, lo=8, hi=120):
    """The scene of tools/bench_track_assoc.py: track boxes [K,4] and detector boxes [D,4] of one stream."""
    rng = np.random.default_rng(seed)

    def box():
        w, h = rng.integers(lo, hi + 1, 2)
        x0, y0 = rng.integers(-w // 3, FW - 2 * w // 3), rng.integers(-h // 3, FH - 2 * h // 3)
        return np.array([x0, y0, x0 + w, y0 + h])

    def near(b, amp):
        return b + np.maximum(1, (b[2] - b[0]) // 10) * rng.integers(-amp, amp + 1, 4) // 4

    tracks = np.stack([box() for _ in range(k)])
    dets = np.stack([box() for _ in range(d)])
    n = max(1, min(k, d) // 3)
    for t, j in zip(rng.permutation(k)[:n], rng.permutation(d)[:n]):
        dets[j] = near(tracks[t], 3)
        dets[j][[1, 3]] -= int(abs((dets[j][3] - dets[j][1]) * 0.1))
    for t in rng.permutation(k)[:k // 8]:
        tracks[t] = near(tracks[(t + 1) % k], 1)
    for t in rng.permutation(k)[:(k + 4) // 5]:
        tracks[t] = 0
    return tracks.astype(np.int32), dets.astype(np.int32)


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def assoc_case(s, k, d):
    """-> (batched, per_stream, restore, counts of the batched call, whether both ways leave the same bits)."""
    tr, de = zip(*[clustered(k, d, 1000 * k + d + 31 * i) for i in range(s)])
    tracks, dets = np.concatenate(tr), np.stack(de)
    n = s * k
    rng = np.random.default_rng(n)
    live = tracks[:, 2] > tracks[:, 0]
    init = [dev(rng.normal(0, 1, (n, 2, 3)).astype(np.float32)), dev(tracks), dev(np.where(live, 0, 1).astype(np.int32)),
            dev(rng.integers(0, 2, n).astype(np.int32)), dev(rng.normal(50, 20, (n, C, 6)))]
    work = [t.clone() for t in init]
    m, b, st, mi, fs = work
    det = dev(dets)
    ds = torch.empty((s, d), dtype=torch.int32, device="cuda")
    sd = torch.empty((n,), dtype=torch.int32, device="cuda")
    cnt = torch.empty((s, 8), dtype=torch.int32, device="cuda")
    lib, o = _lib.load(), _lib.TrackAssocOpts.make(**OPTS)
    p = _lib.ptr
    a = (p(det), None, s, d, k, C, IN, IN, FH, FW, _lib.C.byref(o), p(m), p(b), p(st), p(mi), p(fs), p(ds), p(sd), p(cnt))
    per = [(p(det[i]), None, d, k, C, IN, IN, FH, FW, _lib.C.byref(o), p(m[i * k:]), p(b[i * k:]), p(st[i * k:]), p(mi[i * k:]),
            p(fs[i * k:]), p(ds[i]), p(sd[i * k:]), p(cnt[i])) for i in range(s)]

    def batched():
        _lib.check(lib.flm_track_associate_streams(_lib.stream_ptr(), *a), "flm_track_associate_streams")

    def per_stream():
        sp = _lib.stream_ptr()
        for x in per:
            _lib.check(lib.flm_track_associate(sp, *x), "flm_track_associate")

    def restore():
        for w, i in zip(work, init):
            w.copy_(i)

    restore()
    batched()
    got = [t.clone() for t in work + [sd, cnt]]
    counts = cnt.sum(0).tolist()
    restore()
    per_stream()
    same = all(torch.equal(x.view(torch.int64) if x.dtype == torch.float64 else x.view(torch.int32),
                           y.view(torch.int64) if y.dtype == torch.float64 else y.view(torch.int32))
               for x, y in zip(got, work + [sd, cnt]))
    batched.keep = (o, det, init, work, ds, sd, cnt)
    return batched, per_stream, restore, counts, same


def run_assoc(rounds, window_ms):
    res = {"windows": {}, "counts": {}, "same_bits_both_ways": {}}
    for k, d in SIZES:
        variants = []
        for s in STREAMS:
            batched, per_stream, restore, counts, same = assoc_case(s, k, d)
            key = "s%d_k%d_d%d" % (s, k, d)
            res["counts"][key], res["same_bits_both_ways"][key] = counts, same

            def both(call, restore=restore):
                def fn():
                    restore()
                    call()
                return fn
            variants += [(key + "_restore_and_batched", both(batched)), (key + "_restore_and_per_stream", both(per_stream)),
                         (key + "_restore", restore), (key + "_batched_steady", batched), (key + "_per_stream_steady", per_stream)]
        w = bt.alternate(variants, rounds, window_ms)
        res["windows"].update(w)
        for s in STREAMS:
            key = "s%d_k%d_d%d" % (s, k, d)
            for how in ("batched", "per_stream"):
                res["%s_%s_ms" % (key, how)] = w["%s_restore_and_%s" % (key, how)]["median_ms"] - w[key + "_restore"]["median_ms"]
    return res


def run_step(rounds, window_ms, streams, k=16):
    model = LANDMARKS_MODELS["fcn_8"](C, input_height=256, input_width=256, dtype="bf16")
    model.load_weights(synth_fcn8_weights(C, seed=2))
    ring, ff = bt.rings()["bgr"]
    fmt = alignment.AlignedFormat.matcher()
    kw = dict(out_size=(OUT, OUT), aligned_format=fmt, frame_format=ff)
    res = {"slots_per_stream": k, "windows": {}}
    clock = {"t": 0}
    for s in streams:
        faces = [bt.boxes_for(k, 11 + k + i) for i in range(s)]
        one = prediction.FaceTracker(model, (bt.FH, bt.FW), k * s, streams=s, **kw)
        many = [prediction.FaceTracker(model, (bt.FH, bt.FW), k, **kw) for _ in range(s)]
        for i in range(s):
            if s > 1:
                one.seed(range(k), faces[i], stream=i)
            else:
                one.seed(range(k), faces[i])
            many[i].seed(range(k), faces[i])
        saved = [(tr, tr.m_crop.clone(), tr.boxes.clone()) for tr in [one] + many]
        idx = [torch.tensor([(t + i) % 8 for i in range(s)], dtype=torch.int32, device="cuda") for t in range(8)]

        def restore_one(saved=saved):
            tr, m0, b0 = saved[0]
            tr.m_crop.copy_(m0)
            tr.boxes.copy_(b0)

        def restore_many(saved=saved):
            for tr, m0, b0 in saved[1:]:
                tr.m_crop.copy_(m0)
                tr.boxes.copy_(b0)

        def step_one(one=one, idx=idx, s=s, restore_one=restore_one):
            restore_one()
            clock["t"] += 1
            return one.step(ring, idx[clock["t"] % 8] if s > 1 else clock["t"] % 8)

        def step_many(many=many, restore_many=restore_many):
            restore_many()
            clock["t"] += 1
            for i, tr in enumerate(many):
                out = tr.step(ring, (clock["t"] + i) % 8)
            return out

        # both ways compute the same faces: stream by stream, bit for bit
        clock["t"] = 0
        a = [x.clone() for x in step_one()]
        clock["t"] = 0
        restore_many()
        clock["t"] += 1
        same = True
        for i, tr in enumerate(many):
            o = tr.step(ring, (clock["t"] + i) % 8)
            same = same and all(torch.equal(x[i * k:(i + 1) * k], y) for x, y in zip(a, o))
        key = "s%d" % s
        w = bt.alternate([(key + "_one_tracker", step_one), (key + "_trackers_in_turn", step_many),
                          (key + "_one_tracker_restore", restore_one), (key + "_trackers_in_turn_restore", restore_many)],
                         rounds, window_ms)
        res["windows"].update(w)
        res[key + "_same_bits_both_ways"] = bool(same)
        res[key + "_one_tracker_ms"] = w[key + "_one_tracker"]["median_ms"] - w[key + "_one_tracker_restore"]["median_ms"]
        res[key + "_trackers_in_turn_ms"] = (w[key + "_trackers_in_turn"]["median_ms"]
                                             - w[key + "_trackers_in_turn_restore"]["median_ms"])
        del one, many, saved
        torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=200.0)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--step-streams", default="1,8,64")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    _lib.require_gpu()
    rec = {"bench": "track_streams", "device": torch.cuda.get_device_name(0), "frame": [FH, FW], "landmarks": C}

    def save():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(json.dumps(rec, indent=1) + "\n")

    rec["assoc"] = run_assoc(a.rounds, a.window_ms)
    save()
    if not a.skip_step:
        rec["step"] = run_step(a.rounds, a.window_ms, [int(v) for v in a.step_streams.split(",")])
        save()
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
