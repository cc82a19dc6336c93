"""fallback_faces: what the per-face fallback costs when nothing raises, what it gains when something does,
and how many faces raise on peaked maps.

Protocol: every configuration runs in a process of its OWN (this file with --child), one timed window per process; the
parent starts the processes of a group in turn, round after round (A B C A B C), so every configuration has `--rounds`
windows taken at alternating times, and reports per configuration the median and [min, max] of its windows and, beside
every difference, the spread |window 1 - window 2| of the group's B = 0 configuration.  B = 0 runs the launches of the
tree without the feature, so it is the reference.  A window: `--warmup` forwards, then `--steps` forwards between two
device events; after it one more forward under flm_profile_* gives the per-launch times, and fallback_counts gives R.

Workload: model.forward_device(crops uint8 [N,256,256,3], "landmarks", n_points) of the 68-class fcn_8 -- the forward of
bench.py's step (the similarity fit and the warp behind it do not depend on the option).

Groups (--groups, default all):
  idle_bf16   bf16 512 faces, n = 4, synthetic weights: B = 0 | 8 | 32 (nothing raises: three near-empty launches added)
  idle_f32    fp32 64 faces, the same
  peaked      bf16 512 faces, n = 4, peaked_cases weights bilinear32 and scaled16: B = 0 | 8 | 32 | 128
  peaked_all  bilinear32 again at B = 0 | 512 (B = n: the per-face path whatever R is)
  blank       bf16 512 faces, n = 4, synthetic weights, k = 1 | 8 | 32 blank crops among random ones.  A blank crop's lists
              are the longest of the batch but still inside the default capacity, so the k faces are made to raise by a
              candidate_cap_div that puts the capacity between the two fills (found per run): B = 0 | 8 | 32 | 128
  share       R per batch of 512 bf16 faces for every case of the peaked table at n = 4 and n = 25 (one process, no timing)

    python tools/bench_face_fallback.py --out profiles/face_fallback.json
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=2)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--groups", default="idle_bf16,idle_f32,peaked,peaked_all,blank,share")
ap.add_argument("--child", default=None, help="JSON of one configuration: run it and print one JSON line")
ap.add_argument("--out", default=None)
args = ap.parse_args()

H = W = 256


def configs(group):
    if group == "idle_bf16":
        return [dict(dtype="bf16", n=512, n_points=4, weights="synth", B=b) for b in (0, 8, 32)]
    if group == "idle_f32":
        return [dict(dtype="f32", n=64, n_points=4, weights="synth", B=b) for b in (0, 8, 32)]
    if group == "peaked":
        return [dict(dtype="bf16", n=512, n_points=4, weights=w, B=b) for w in ("bilinear32", "scaled16") for b in (0, 8, 32, 128)]
    if group == "peaked_all":   # B = n: every face that raised is redone per face, however many
        return [dict(dtype="bf16", n=512, n_points=4, weights="bilinear32", B=b) for b in (0, 512)]
    if group == "blank":
        return [dict(dtype="bf16", n=512, n_points=4, weights="synth", forced=k, B=b) for k in (1, 8, 32) for b in (0, 8, 32, 128)]
    raise SystemExit("unknown group %r" % group)


def name_of(c):
    return "%s_%d_%s%s_n%d_B%d" % (c["dtype"], c["n"], c["weights"], "_forced%d" % c["forced"] if c.get("forced") else "",
                                   c["n_points"], c["B"])


def _model(dtype, weights):
    import peaked_cases as P
    from flm_amd.networks import LANDMARKS_MODELS
    from flm_amd.weights import synth_fcn8_weights
    base = synth_fcn8_weights(68, seed=2)
    model = LANDMARKS_MODELS["fcn_8"](68, input_height=H, input_width=W, dtype=dtype)
    model.load_weights(base if weights == "synth" else P.case_weights(base, weights))
    return model


def _fills(model, xd, n_points, opts):
    """cand_cnt[0..n) and the capacity of one forward (host copy)."""
    import ctypes as C

    import torch
    from flm_amd import _lib
    n = int(xd.shape[0])
    ws = model.new_workspace(n, "landmarks", n_points, opts)
    model.forward_device(xd, "landmarks", n_points=n_points, workspace=ws, opts=opts)
    fo = model._opts(opts)

    def off(key):
        return _lib.load().flm_fcn8_workspace_offset_opts(key, n, H, W, 68, model._dt, _lib.OUT_LANDMARKS, _lib.DECODE_TOPN,
                                                          n_points, C.byref(fo))
    cnt = ws[off(b"cand_cnt"):off(b"cand_cnt") + 4 * n].view(torch.int32).cpu().numpy()
    return cnt, int(off(b"cand_cap"))


def child(c):
    import numpy as np
    import torch

    import flm_amd  # noqa: F401
    from flm_amd import _lib
    _lib.require_gpu()
    L = _lib.load()
    model = _model(c["dtype"], c["weights"])
    n, n_points, B = c["n"], c["n_points"], c["B"]
    rng = np.random.default_rng(11)
    crops = rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    opts = None
    rec = dict(c, name=name_of(c))
    if c.get("forced"):
        k = c["forced"]
        faces = np.linspace(0, n - 1, k).astype(int)      # spread over the batch
        blank = np.zeros(n, bool)
        blank[faces] = True
        crops[blank] = 128
        xd = torch.from_numpy(crops).cuda()
        cnt, cap = _fills(model, xd, n_points, None)
        lo, hi = int(cnt[~blank].max()), int(cnt[blank].min())
        rec.update(fill_random_max=lo, fill_blank_min=hi, cap=cap)
        if not lo < hi:
            raise SystemExit("the random faces' lists (%d) are not shorter than the blank ones' (%d)" % (lo, hi))
        div = next((d for d in range(2, 200) if lo < (68 * 64 * n_points * 4 // d + 63) // 64 * 64 < hi), None)
        if div is None:
            raise SystemExit("no candidate_cap_div separates the fills %d and %d" % (lo, hi))
        opts = dict(candidate_cap_div=div)
        rec["candidate_cap_div"] = div
    else:
        xd = torch.from_numpy(crops).cuda()
    kw = dict(n_points=n_points, opts=opts)
    if B:
        kw["fallback_faces"] = B
    ref = model.forward_device(xd, "landmarks", n_points=n_points, opts=dict(opts or {}, landmark_candidates=0)).clone()
    for _ in range(args.warmup):
        got = model.forward_device(xd, "landmarks", **kw)
    rec["bit_equal_to_materialised"] = bool(torch.equal(got.view(torch.int64), ref.view(torch.int64)))
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(args.steps):
        model.forward_device(xd, "landmarks", **kw)
    b.record()
    torch.cuda.synchronize()
    rec["step_ms"] = a.elapsed_time(b) / args.steps
    if B:
        rec["fallback_counts"] = model.fallback_counts().cpu().tolist()
    # per-launch times of one more forward
    import ctypes as C
    L.flm_profile_enable(256)
    L.flm_profile_reset()
    model.forward_device(xd, "landmarks", **kw)
    torch.cuda.synchronize()
    launches, i = {}, 0
    nm, ms = C.create_string_buffer(64), C.c_float()
    while L.flm_profile_read(i, nm, 64, C.byref(ms)) == 0:
        launches[nm.value.decode()] = launches.get(nm.value.decode(), 0.0) + float(ms.value)
        i += 1
    L.flm_profile_disable()
    keep = ("up3_sub", "tau", "up3", "decode", "fallback_plan", "up3_rows", "decode_rows", "up3_fallback", "decode_fallback")
    rec["launch_ms"] = {k: round(v, 4) for k, v in launches.items() if k in keep}
    rec["forward_launch_sum_ms"] = round(sum(launches.values()), 4)
    print(json.dumps(rec), flush=True)


def share():
    """R per batch of 512 bf16 faces (every fourth crop blank) for every case of the peaked table."""
    import numpy as np
    import torch

    import flm_amd  # noqa: F401
    import peaked_cases as P
    n = 512
    crops = np.random.default_rng(12).integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    crops[::4] = 128
    xd = torch.from_numpy(crops).cuda()
    out = {}
    for case in P.CASE_NAMES:
        model = _model("bf16", case)
        for n_points in (4, 25):
            model.forward_device(xd, "landmarks", n_points=n_points, fallback_faces=n)
            counts = model.fallback_counts().cpu().tolist()
            _, redo = model.fallback_rows()
            redo = redo.cpu().numpy()
            out["%s_n%d" % (case, n_points)] = dict(R=counts[0], share=counts[0] / n, R_blank=int(redo[::4].sum()),
                                                    R_random=int(redo.sum() - redo[::4].sum()))
        del model
        torch.cuda.empty_cache()
    print(json.dumps(dict(name="share", n=n, blank_faces=n // 4, cases=out)), flush=True)


def run_child(cfg):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", json.dumps(cfg), "--steps", str(args.steps),
           "--warmup", str(args.warmup)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)   # (a hung child ends the whole run)
    if r.returncode != 0:
        raise SystemExit("bench_face_fallback: %s failed:\n%s" % (cfg, r.stderr[-3000:]))
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    if args.child:
        cfg = json.loads(args.child)
        return share() if cfg == "share" else child(cfg)
    rec = {"bench": "face_fallback", "shape": [H, W], "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds,
           "groups": {}}
    for group in args.groups.split(","):
        if group == "share":
            rec["share"] = run_child("share")
            continue
        cfgs = configs(group)
        runs = {name_of(c): [] for c in cfgs}
        for _ in range(args.rounds):
            for c in cfgs:
                runs[name_of(c)].append(run_child(c))
        g = {}
        for c in cfgs:
            rs = runs[name_of(c)]
            ms = [r["step_ms"] for r in rs]
            g[name_of(c)] = dict(windows_ms=ms, median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms),
                                 fallback_counts=rs[-1].get("fallback_counts"), launch_ms=rs[-1]["launch_ms"],
                                 bit_equal_to_materialised=all(r["bit_equal_to_materialised"] for r in rs),
                                 **{k: rs[-1][k] for k in ("candidate_cap_div", "fill_random_max", "fill_blank_min", "cap") if k in rs[-1]})
        # differences against the B = 0 configuration of the same workload, its own spread beside them
        for c in cfgs:
            if c["B"]:
                base = g[name_of(dict(c, B=0))]
                spread = abs(base["windows_ms"][0] - base["windows_ms"][1]) if len(base["windows_ms"]) > 1 else None
                d = g[name_of(c)]
                d["minus_B0_ms"] = d["median_ms"] - base["median_ms"]
                d["spread_B0_ms"] = spread
                d["within_spread"] = None if spread is None else bool(abs(d["minus_B0_ms"]) <= spread)
        rec["groups"][group] = g
        print("%s done" % group, file=sys.stderr, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")
    print(json.dumps(rec), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
