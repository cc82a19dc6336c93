"""Shape-normalised faces: what the piecewise-affine warp over the landmark mesh costs beside the similarity warp.

The set-up of tools/bench_track.py (same seeds): an 8-slot 1080p ring, BGR and NV12 (pitch 2048), faces of 96..400 px,
aligned size 112x112, uint8 NCHW out, the default 68 + 8 mesh (142 triangles).  The matrices fit each face box onto the
aligned square; the landmarks are M^-1 of the template under a smooth deformation of 2 % of the face, so every
triangle has an affine of its own.  One process, the variants ALTERNATING window by window, HIP events around each
window of back-to-back launches.

  warp    per K in 64, 1024 and per ring format: flm_warp_affine_frames_src (sim, sim2: the pair gives the run-to-run
          spread) against flm_warp_mesh_frames (mesh) and flm_warp_mesh_frames with aff_out (mesh_aff).  Per row the
          byte model -- source: side^2 * 3 B per face (BGR; 1.5 B per pixel for NV12), destination 112*112*3 B per
          face, for the mesh also one map byte per pixel per face and its landmarks and matrix -- and GB/s by it; the
          ratio mesh / sim.
  step    FaceTracker.step at 64 streams x 16 slots with and without mesh=True, and plain2, a second window of the plain
          step: |plain2 - plain| is the spread that the difference has to be read against.

Writes the record to --out and prints it as one JSON line.

    python tools/bench_mesh.py
    rocprofv3 --kernel-trace --stats ... -- python tools/bench_mesh.py --trace 50 --skip-step
                                     # a fixed count of each warp variant, no events: kernel times, in a run of its own
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

import flm_amd  # noqa: F401
from flm_amd import _lib, alignment, prediction
from flm_amd.networks import LANDMARKS_MODELS
from flm_amd.weights import synth_fcn8_weights

import bench_track as bt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT, C = bt.OUT, 68


def faces(k, mesh, seed):
    """(m float32 [K,2,3], lm float64 [K,C,2], boxes int32 [K,4], ring slots int32 [K], the sides) on the device."""
    rng = np.random.default_rng(seed)
    boxes = np.array(bt.boxes_for(k, seed), np.int32)
    side = (boxes[:, 2] - boxes[:, 0]).astype(np.float64)
    m = np.zeros((k, 2, 3), np.float32)
    lm = np.zeros((k, C, 2), np.float64)
    tmpl = mesh.points[:C]
    for i in range(k):
        th, s = rng.uniform(-0.2, 0.2), OUT / side[i]
        cx, cy = boxes[i, 0] + side[i] / 2, boxes[i, 1] + side[i] / 2
        a, b = s * np.cos(th), s * np.sin(th)
        m[i] = [[a, -b, OUT / 2 - (a * cx - b * cy)], [b, a, OUT / 2 - (b * cx + a * cy)]]
        mi = m[i].astype(np.float64)
        inv = np.linalg.inv(mi[:, :2])
        # a smooth deformation of 2 % of the face, one period over the aligned square: no triangle folds over
        ph = rng.uniform(0, 2 * np.pi, 2)
        bend = 0.02 * OUT * np.sin(2 * np.pi * tmpl[:, ::-1] / OUT + ph)
        lm[i] = (tmpl + bend - mi[:, 2]) @ inv.T
    slots = rng.integers(0, 8, k).astype(np.int32)
    dev = lambda x: torch.from_numpy(x).cuda()
    return dev(m), dev(lm), dev(boxes), dev(slots), side


def run_warp(rounds, window_ms, trace):
    mesh = alignment.FaceMesh.default(C, OUT, OUT)
    fmt = alignment.AlignedFormat("nchw", "uint8")
    res = {"triangles": mesh.n_triangles, "windows": {}}
    for source, (ring, ff) in bt.rings().items():
        for k in (64, 1024):
            m, lm, boxes, slots, side = faces(k, mesh, 100 + k)
            dst = [torch.empty(fmt.shape(k, OUT, OUT), dtype=torch.uint8, device="cuda") for _ in range(2)]
            aff = torch.empty((k, mesh.n_triangles, 2, 3), dtype=torch.float32, device="cuda")
            where = dict(frame_index_dev=slots, boxes_dev=boxes, fmt=fmt, src=ff)

            def sim(m=m, dst=dst, where=where):
                return alignment.warp_frames_device(ring, m, OUT, OUT, out=dst[0], **where)

            def msh(m=m, lm=lm, dst=dst, where=where, aff=None):
                return alignment.warp_mesh_frames_device(ring, lm, m, mesh, OUT, OUT, out=dst[1], affines_out=aff, **where)

            key = "%s_k%d" % (source, k)
            rows = [(key + "_sim", sim), (key + "_mesh", msh), (key + "_sim2", sim),
                    (key + "_mesh_aff", lambda msh=msh, aff=aff: msh(aff=aff))]
            if trace:
                for _, fn in rows:
                    for _ in range(3 + trace):
                        fn()
                torch.cuda.synchronize()
                continue
            w = bt.alternate(rows, rounds, window_ms)
            res["windows"].update(w)
            px = 3.0 if source == "bgr" else 1.5
            src_bytes = float((side * side * px).sum())
            dst_bytes = k * OUT * OUT * 3
            mesh_extra = k * (OUT * OUT + C * 16 + 24) + mesh.n_points * 16 + mesh.n_triangles * 12
            sim_ms, sim2_ms, mesh_ms = (w[key + t]["median_ms"] for t in ("_sim", "_sim2", "_mesh"))
            res[key] = {
                "sim_ms": sim_ms, "sim2_ms": sim2_ms, "mesh_ms": mesh_ms, "mesh_aff_ms": w[key + "_mesh_aff"]["median_ms"],
                "spread_sim_vs_sim2_ms": abs(sim2_ms - sim_ms), "mesh_over_sim": mesh_ms / sim_ms,
                "bytes_model": {"source": src_bytes, "destination": dst_bytes, "mesh_extra": mesh_extra},
                "sim_gb_per_s": (src_bytes + dst_bytes) / sim_ms / 1e6,
                "mesh_gb_per_s": (src_bytes + dst_bytes + mesh_extra) / mesh_ms / 1e6,
                "traffic_ratio_by_model": (src_bytes + dst_bytes + mesh_extra) / (src_bytes + dst_bytes)}
    return res


def run_step(rounds, window_ms, streams=64, k=16):
    model = LANDMARKS_MODELS["fcn_8"](C, input_height=256, input_width=256, dtype="bf16")
    model.load_weights(synth_fcn8_weights(C, seed=2))
    ring, ff = bt.rings()["bgr"]
    kw = dict(out_size=(OUT, OUT), aligned_format=alignment.AlignedFormat.matcher(), frame_format=ff, streams=streams)
    trackers = {"plain": prediction.FaceTracker(model, (bt.FH, bt.FW), k * streams, **kw),
                "mesh": prediction.FaceTracker(model, (bt.FH, bt.FW), k * streams, mesh=True, **kw)}
    for tr in trackers.values():
        for i in range(streams):
            tr.seed(range(k), bt.boxes_for(k, 11 + k + i), stream=i)
    saved = {name: (tr.m_crop.clone(), tr.boxes.clone()) for name, tr in trackers.items()}
    idx = [torch.tensor([(t + i) % 8 for i in range(streams)], dtype=torch.int32, device="cuda") for t in range(8)]
    clock = {"t": 0}

    def step(name):
        tr = trackers[name]
        tr.m_crop.copy_(saved[name][0])      # synthetic weights lose tracks at will: every step starts from the seeds
        tr.boxes.copy_(saved[name][1])
        clock["t"] += 1
        return tr.step(ring, idx[clock["t"] % 8])

    clock["t"] = 0
    a = [x.clone() for x in step("plain")]
    clock["t"] = 0
    b = step("mesh")
    same = all(torch.equal(x, y) for x, y in zip(a, b))
    w = bt.alternate([("plain", lambda: step("plain")), ("mesh", lambda: step("mesh")), ("plain2", lambda: step("plain"))],
                     rounds, window_ms)
    p, q, mm = w["plain"]["median_ms"], w["plain2"]["median_ms"], w["mesh"]["median_ms"]
    return {"streams": streams, "slots_per_stream": k, "windows": w, "plain_ms": p, "plain2_ms": q, "mesh_ms": mm,
            "spread_plain_vs_plain2_ms": abs(q - p), "mesh_minus_plain_ms": mm - p, "other_outputs_same_bits": bool(same)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=100.0)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--trace", type=int, default=0, metavar="LAUNCHES",
                    help="run LAUNCHES launches of every warp variant after a warm-up and nothing else (for a kernel trace)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_bench.json"))
    a = ap.parse_args()
    _lib.require_gpu()
    rec = {"bench": "mesh", "device": torch.cuda.get_device_name(0), "frame": [bt.FH, bt.FW], "out_size": [OUT, OUT],
           "timing": "HIP events around windows of back-to-back launches, variants alternating window by window"}
    rec["warp"] = run_warp(a.rounds, a.window_ms, a.trace)
    if not a.skip_step and not a.trace:
        rec["step"] = run_step(a.rounds, a.window_ms)
    if not a.trace:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
