"""What writing the result back into the frames costs (the protocol of tools/bench_track.py: one process, the variants
ALTERNATING window by window, HIP events around whole windows of at least --window-ms, median and [min, max] over the
windows).

  call     flm_frames_annotate through ctypes at 64 and at 1024 faces of 68 landmarks whose box is about 200 px, on a 64-slot
           1080p ring, BGR and NV12 (BT.709, pitch 2048, U,V rows from row 1088): OFF the regions alone, M the marks, B an
           outline of 3 px, R8 / R16 a mosaic of 8 / 16 px cells, ALL = M + B + R8, W the Python wrapper of ALL.  Face f
           lies in slot f % 64: one face per frame at 64, sixteen overlapping faces per frame at 1024.  For the mosaics the
           bytes of the cells (each read once and written once) are counted on the host from the regions, and the achieved
           bytes/s is set against the 8 TB/s this project quotes for the chip.
  host     what a caller pays today for the marks alone: download of the frames that hold a face, utils.plots.draw_marks on
           the host, upload.  Wall clock, three repetitions (it is hundreds of milliseconds).
  worst    the input the k <= 4096 cap exists for: 4096 faces with the same full-frame region on one frame, R8.  Every
           workgroup of face f scans f regions and then finds its cells taken.  Three single calls.

Prints one JSON line, and writes it to --out.

    python tools/bench_annotate.py --out profiles/frames_annotate.json
"""
import argparse
import ctypes as C
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import flm_amd  # noqa: F401
from flm_amd import _lib, alignment
from flm_amd.utils import plots

import bench_track as bt

FH, FW, NF, NC = 1080, 1920, 64, 68
PITCH, UV_ROW = 2048, 1088
HBM = 8e12


def make_faces(k, seed, same=None):
    """lm float64 [k,68,2] with a landmark box of about 200 px, and the ring slot of every face."""
    rng = np.random.default_rng(seed)
    lm = np.empty((k, NC, 2))
    for f in range(k):
        side = rng.uniform(180.0, 220.0)
        x0, y0 = rng.uniform(20.0, FW - 20.0 - side), rng.uniform(90.0, FH - 40.0 - side)
        lm[f] = [x0, y0] + rng.uniform(0.0, side, (NC, 2))
        lm[f, 0], lm[f, 1] = (x0, y0), (x0 + side, y0 + side)
    if same is not None:
        lm[:] = same
    return lm, (np.arange(k) % NF).astype(np.int32)


def cell_bytes(regions, fi, s, per_pixel):
    """Bytes of the union of the cells, per frame, that the mosaic replaces."""
    total = 0
    for f in np.unique(fi):
        grid = np.zeros(((FH + s - 1) // s, (FW + s - 1) // s), bool)
        for x0, y0, x1, y1 in regions[fi == f]:
            x0, y0, x1, y1 = max(x0, 0), max(y0, 0), min(x1, FW), min(y1, FH)
            if x1 > x0 and y1 > y0:
                grid[y0 // s:(y1 - 1) // s + 1, x0 // s:(x1 - 1) // s + 1] = True
        ys, xs = np.nonzero(grid)
        total += int(((np.minimum((xs + 1) * s, FW) - xs * s) * (np.minimum((ys + 1) * s, FH) - ys * s)).sum())
    return total * per_pixel


def caller(ring, ff, lm_d, fi_d, reg, **opts):
    nf, fh, fw, stride = ff.ring(ring)
    co, cs = _lib.AnnotateOpts.make(**opts), ff.struct(ring)
    call, args = _lib.load().flm_frames_annotate, (_lib.ptr(ring), stride, nf, fh, fw, C.byref(cs), _lib.ptr(fi_d),
                                                   _lib.ptr(lm_d), 2, int(lm_d.shape[0]), NC, C.byref(co), _lib.ptr(reg))

    def fn():
        _lib.check(call(_lib.stream_ptr(), *args), "flm_frames_annotate")
    fn.keep = (co, cs)
    return fn


def alternate(variants, rounds, window_ms):
    """bench_track.alternate with windows that are at least window_ms long: the calls per window come from a warm run of
    100 calls (back to back a call is launch-bound, and its first calls are the slow ones) with a half in hand, and the
    shortest window that was timed is reported."""
    for _, fn in variants:
        fn()
        fn()
    torch.cuda.synchronize()
    reps = {name: max(2, int(math.ceil(1.5 * window_ms / max(bt.event_ms(fn, 100), 1e-4)))) for name, fn in variants}
    times = {name: [] for name, _ in variants}
    for _ in range(rounds):
        for name, fn in variants:
            times[name].append(bt.event_ms(fn, reps[name]))
    return {name: dict(bt.stats(t), calls_per_window=reps[name], shortest_window_ms=min(t) * reps[name])
            for name, t in times.items()}


def host_baseline(ring, lm, fi, reps=3):
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for f in np.unique(fi):
            img = ring[int(f)].cpu().numpy()
            for face in lm[fi == f]:
                plots.draw_marks(img, face)
            ring[int(f)].copy_(torch.from_numpy(img))
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return dict(bt.stats(times), frames=int(len(np.unique(fi))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=200.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    _lib.require_gpu()
    g = torch.Generator(device="cuda")
    g.manual_seed(3)
    formats = {"bgr": (alignment.FrameFormat.bgr(), (NF, FH, FW, 3), 3.0),
               "nv12": (alignment.FrameFormat.nv12(FH, FW, matrix="bt709", uv_row=UV_ROW), (NF, UV_ROW + FH // 2, PITCH), 1.5)}
    rec = {"what": "flm_frames_annotate, 64-slot 1080p ring, 68 landmarks, faces of about 200 px", "rounds": args.rounds,
           "window_ms": args.window_ms, "device": torch.cuda.get_device_name(0), "hbm_bytes_per_s_quoted": HBM, "call": {}}
    for name, (ff, shape, bpp) in formats.items():
        ring = torch.randint(0, 256, shape, dtype=torch.uint8, device="cuda", generator=g)
        for k in (64, 1024):
            lm, fi = make_faces(k, seed=k)
            lm_d, fi_d = torch.from_numpy(lm).cuda(), torch.from_numpy(fi).cuda()
            reg = torch.zeros((k, 4), dtype=torch.int32, device="cuda")
            note = alignment.FrameAnnotation(marks=True, box=3, redact=8)
            variants = [("OFF", caller(ring, ff, lm_d, fi_d, reg, marks=0)), ("M", caller(ring, ff, lm_d, fi_d, reg)),
                        ("B", caller(ring, ff, lm_d, fi_d, reg, marks=0, box=3)),
                        ("R8", caller(ring, ff, lm_d, fi_d, reg, marks=0, redact=8)),
                        ("R16", caller(ring, ff, lm_d, fi_d, reg, marks=0, redact=16)),
                        ("ALL", caller(ring, ff, lm_d, fi_d, reg, marks=1, box=3, redact=8)),
                        ("W", lambda: alignment.annotate_frames_device(ring, lm_d, fi_d, note, ff, regions_out=reg))]
            res = alternate(variants, args.rounds, args.window_ms)
            regions = reg.cpu().numpy()
            for v, s in (("R8", 8), ("R16", 16)):
                moved = 2 * cell_bytes(regions, fi, s, bpp)
                bps = moved / (res[v]["median_ms"] * 1e-3)
                res[v].update(bytes_read_and_written=int(moved), bytes_per_s=bps, share_of_quoted_hbm=bps / HBM)
            rec["call"]["%s_k%d" % (name, k)] = res
        if name == "bgr":
            rec["host"] = {}
            for k in (64, 1024):
                lm, fi = make_faces(k, seed=k)
                rec["host"]["bgr_k%d" % k] = host_baseline(ring, lm, fi)
            # the degenerate input: 4096 faces, one frame, the same full-frame region
            lm, _ = make_faces(4096, seed=1, same=np.tile([[0.0, 0.0], [FW - 1.0, FH - 1.0]], (NC // 2, 1)))
            lm_d, fi_d = torch.from_numpy(lm).cuda(), torch.zeros(4096, dtype=torch.int32, device="cuda")
            reg = torch.zeros((4096, 4), dtype=torch.int32, device="cuda")
            fn = caller(ring, ff, lm_d, fi_d, reg, marks=0, redact=8)
            fn()
            torch.cuda.synchronize()
            rec["worst"] = dict(bt.stats([bt.event_ms(fn, 1) for _ in range(3)]), faces=4096,
                                region=reg[0].cpu().tolist(), what="4096 identical full-frame regions on one frame, R8, BGR")
        del ring
        torch.cuda.empty_cache()
    bt.emit(rec, args.out)


if __name__ == "__main__":
    main()
