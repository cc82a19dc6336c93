"""flm_track_associate against what a caller pays without it (the protocol of tools/bench_track.py: variants ALTERNATING
round by round, 5 windows of at least 200 ms each, median and range over the windows).

  --assoc   (this build) flm_track_associate through ctypes at (K, D) = (16,16), (64,64), (1024,1024) on clustered boxes of
            8..120 px in a 270x480 frame (a third of the slots and detections have a partner, a fifth of the slots is
            free, some tracks sit in pairs), 68 landmarks of filter state, max_misses = 2, refresh_iou = 0.6.  The call
            edits the tracker's state, so the state is put back before every call by five device copies inside the timed
            window; "restore" is those copies alone, and "associate_ms" the difference of the two medians.  "steady" is
            the call repeated on the state it left (every track matched or settled).  "degenerate" is K = D = 1024 with
            every box the same and the duplicate rule off: 1024 matches in 1024 rounds, the most the matching can take;
            it leaves the state as it found it, so nothing is put back.  HIP events around whole windows.
  --reseed  (any build; with --root on the tree of the commit before the association existed) one re-seed cycle of a
            FaceTracker at the same sizes and boxes, as INTEGRATION A had it: lost() (the synchronisation and a download),
            the boxes' download, a greedy IoU match in numpy on the host, seed() of the unmatched detections into the lost
            slots (one upload, flm_track_seed, the index copies).  Wall clock around whole windows, every cycle ended
            by a synchronisation; the tracker is put back before every cycle by the same device copies, which are
            measured alone too.

Prints one JSON line, and writes it to --out.

    python tools/bench_track_assoc.py --assoc --out profiles/track_associate.json
    python tools/bench_track_assoc.py --reseed --root /path/to/the/parent/tree
"""
import argparse
import json
import math
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--assoc", action="store_true")
ap.add_argument("--reseed", action="store_true")
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                help="the tree whose package is measured (default: this one)")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--window-ms", type=float, default=200.0)
ap.add_argument("--out", default=None)
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import flm_amd  # noqa: E402,F401
from flm_amd import _lib, alignment, prediction  # noqa: E402

FH, FW, IN, C = 270, 480, 64, 68
SIZES = [(16, 16), (64, 64), (1024, 1024)]


class Stub:
    n_classes, input_height, input_width, output_height, output_width = C, IN, IN, 72, 72


def clustered(k, d, seed, lo=8, hi=120):
    """The scene of tests/test_gpu_track_assoc.py: track boxes [K,4] and detector boxes [D,4]."""
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


def stats(v):
    v = sorted(v)
    return {"median_ms": v[len(v) // 2], "min_ms": v[0], "max_ms": v[-1], "windows": len(v)}


def event_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def wall_ms(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def alternate(variants, timer):
    for _, fn in variants:
        fn()
        fn()
    torch.cuda.synchronize()
    reps = {name: max(2, int(math.ceil(args.window_ms / max(timer(fn, 2), 1e-4)))) for name, fn in variants}
    times = {name: [] for name, _ in variants}
    for _ in range(args.rounds):
        for name, fn in variants:
            times[name].append(timer(fn, reps[name]))
    return {name: dict(stats(t), calls_per_window=reps[name]) for name, t in times.items()}


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def assoc_case(tracks, dets, opts):
    """-> (call, restore, counts tensor) for flm_track_associate on the tracker state `tracks` stands for."""
    k, d = len(tracks), len(dets)
    rng = np.random.default_rng(k)
    live = (tracks[:, 2] > tracks[:, 0])
    m0 = dev(rng.normal(0, 1, (k, 2, 3)).astype(np.float32))
    b0, s0 = dev(tracks), dev(np.where(live, 0, 1).astype(np.int32))
    mi0 = dev(rng.integers(0, 2, k).astype(np.int32))
    st0 = dev(rng.normal(50, 20, (k, C, 6)))
    m, b, s, mi, st = [t.clone() for t in (m0, b0, s0, mi0, st0)]
    det = dev(dets)
    ds = torch.empty((d,), dtype=torch.int32, device="cuda")
    sd = torch.empty((k,), dtype=torch.int32, device="cuda")
    cnt = torch.empty((8,), dtype=torch.int32, device="cuda")
    lib, o = _lib.load(), _lib.TrackAssocOpts.make(**opts)
    a = (_lib.ptr(det), None, d, k, C, IN, IN, FH, FW, _lib.C.byref(o), _lib.ptr(m), _lib.ptr(b), _lib.ptr(s), _lib.ptr(mi),
         _lib.ptr(st), _lib.ptr(ds), _lib.ptr(sd), _lib.ptr(cnt))

    def call():
        _lib.check(lib.flm_track_associate(_lib.stream_ptr(), *a), "flm_track_associate")

    def restore():
        m.copy_(m0)
        b.copy_(b0)
        s.copy_(s0)
        mi.copy_(mi0)
        st.copy_(st0)

    call.keep = (o, det, m0, b0, s0, mi0, st0, m, b, s, mi, st, ds, sd)
    return call, restore, cnt


def run_assoc():
    res = {}
    variants = []
    counts = {}
    for k, d in SIZES:
        tracks, dets = clustered(k, d, 1000 * k + d)
        call, restore, cnt = assoc_case(tracks, dets, dict(max_misses=2, refresh_iou=0.6))
        restore()
        call()
        counts["k%d_d%d" % (k, d)] = cnt.tolist()

        def both(call=call, restore=restore):
            restore()
            call()
        variants += [("k%d_d%d_restore_and_associate" % (k, d), both), ("k%d_d%d_restore" % (k, d), restore),
                     ("k%d_d%d_steady" % (k, d), call)]
    same = np.tile(np.array([100, 60, 160, 120], np.int32), (1024, 1))
    call, _, cnt = assoc_case(same, same, dict(square=False, dup_iou=2.0))
    call()
    counts["degenerate_k1024_d1024"] = cnt.tolist()
    variants.append(("degenerate_k1024_d1024", call))
    res["windows"] = alternate(variants, event_ms)
    res["counts"] = counts
    for k, d in SIZES:
        w = res["windows"]
        res["k%d_d%d_associate_ms" % (k, d)] = (w["k%d_d%d_restore_and_associate" % (k, d)]["median_ms"]
                                               - w["k%d_d%d_restore" % (k, d)]["median_ms"])
    return res


def host_match(tracks, dets, match_iou=0.3):
    """Greedy IoU assignment in numpy -> the indices of the detections no live track took."""
    live = np.flatnonzero((tracks[:, 2] > tracks[:, 0]) & (tracks[:, 3] > tracks[:, 1]))
    t = tracks[live].astype(np.int64)
    q = dets.astype(np.int64)
    w = np.minimum(t[:, None, 2], q[None, :, 2]) - np.maximum(t[:, None, 0], q[None, :, 0])
    h = np.minimum(t[:, None, 3], q[None, :, 3]) - np.maximum(t[:, None, 1], q[None, :, 1])
    inter = np.where((w > 0) & (h > 0), w * h, 0)
    area_t = (t[:, 2] - t[:, 0]) * (t[:, 3] - t[:, 1])
    area_q = (q[:, 2] - q[:, 0]) * (q[:, 3] - q[:, 1])
    iou = inter / np.maximum(area_t[:, None] + area_q[None, :] - inter, 1)
    ti, qi = np.nonzero(iou >= match_iou)
    order = np.argsort(-iou[ti, qi], kind="stable")
    t_used, q_used = np.zeros(len(t), bool), np.zeros(len(q), bool)
    for p in order:
        a, b = ti[p], qi[p]
        if not t_used[a] and not q_used[b]:
            t_used[a] = q_used[b] = True
    return np.flatnonzero(~q_used)


def run_reseed():
    res = {}
    variants = []
    info = {}
    for k, d in SIZES:
        tracks, dets = clustered(k, d, 1000 * k + d)
        sq = np.asarray(prediction.face_boxes(dets.tolist()), np.int32)
        tr = prediction.FaceTracker(Stub(), (FH, FW), k)
        tr._state()
        live = tracks[:, 2] > tracks[:, 0]
        m0 = dev(np.random.default_rng(k).normal(0, 1, (k, 2, 3)).astype(np.float32))
        b0, s0 = dev(tracks), dev(np.where(live, 0, 1).astype(np.int32))

        def restore(tr=tr, m0=m0, b0=b0, s0=s0):
            tr.m_crop.copy_(m0)
            tr.boxes.copy_(b0)
            tr.status.copy_(s0)

        def cycle(tr=tr, sq=sq, restore=restore, info=info, key="k%d_d%d" % (k, d)):
            restore()
            lost = tr.lost()                                   # the synchronisation and a download
            boxes = tr.boxes.cpu().numpy()                     # what the host match needs
            new = host_match(boxes, sq)
            n = min(len(lost), len(new))
            tr.seed(lost[:n], sq[new[:n]].tolist())
            info[key] = {"lost": len(lost), "unmatched_detections": int(len(new)), "seeded": int(n)}
        variants += [("k%d_d%d_restore_and_cycle" % (k, d), cycle), ("k%d_d%d_restore" % (k, d), restore)]
    res["windows"] = alternate(variants, wall_ms)
    res["cycles"] = info
    for k, d in SIZES:
        w = res["windows"]
        res["k%d_d%d_cycle_ms" % (k, d)] = (w["k%d_d%d_restore_and_cycle" % (k, d)]["median_ms"]
                                           - w["k%d_d%d_restore" % (k, d)]["median_ms"])
    return res


def main():
    if not torch.cuda.is_available():
        sys.exit("bench_track_assoc: no GPU visible (there is nothing to measure on a CPU)")
    if args.assoc == args.reseed:
        sys.exit("bench_track_assoc: give --assoc or --reseed")
    rec = {"bench": "track_associate" if args.assoc else "track_reseed_cycle", "device": torch.cuda.get_device_name(0),
           "frame": [FH, FW], "landmarks": C, "has_associate": hasattr(prediction.FaceTracker, "update")}
    rec.update(run_assoc() if args.assoc else run_reseed())
    print(json.dumps(rec), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
