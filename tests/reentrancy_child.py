"""The child processes of tests/test_gpu_reentrancy.py: `main(part)` runs one part on the GPU and prints one line,
"RESULT " + JSON, that the parent asserts on.  Every part compares concurrent calls -- one thread and one
torch.cuda.Stream per caller, started on a barrier -- with the same calls made serially, alone, on the default stream of
the same process, bit for bit (arena.same_bits).  A thread that has not finished when its join times out ends the child
with the status 3; nothing is retried.

The C-ABI parts ("cold", "mixed") call libflm_hip.so through ctypes, which releases the GIL for the length of the call:
the host sides of the launchers really overlap.  Every caller owns its inputs, outputs and workspaces, carved from an
arena of its own (tests/arena.py) so that the guards around them are checked too; the callers share the packed blobs,
read-only."""
import ctypes as C
import json
import os
import sys
import threading
import traceback

import numpy as np
import torch

from arena import Arena, same_bits

import flm_amd  # noqa: F401
from flm_amd import _lib, alignment, graphs, prediction
from flm_amd.networks import LANDMARKS_MODELS
from flm_amd.networks.fcn import decode_mode_of
from flm_amd.weights import synth_fcn8_weights

WORKERS = 4          # a process opens four hardware queues by default: four callers and no more
JOIN_S = 90.0
HEAD = ("fc6", "fc7", "score5", "fuse4", "seg_feats")
BURST = 256          # standalone decodes per worker and round in part "mixed"
SCRUB = 0xCD         # what outputs and workspaces hold before every call: a call that did nothing cannot pass
_OUT = {"probs": _lib.OUT_PROBS, "classmap": _lib.OUT_CLASSMAP, "landmarks": _lib.OUT_LANDMARKS,
        "landmark_stats": _lib.OUT_LANDMARKS_STATS}
# every knob include/flm.h marks bit-neutral ("f32_two_level" is the one that is not) with its legal values
NEUTRAL_KNOBS = [("bf16_big_tiles", (0, 1, 2, 3)), ("bf16_lds_dma", (0, 1)), ("bf16_mfma16", (0, 1)),
                 ("bf16_halo_mfma16", (0, 1)), ("f32_lean_tile", (0, 1)), ("bf16_group_n", (0, 1, 2, 4, 8, 16, 32)),
                 ("bf16_conv3_halo", (0, 1, 2)), ("bf16_score1x1", (0, 1)), ("bf16_fused_tail", (0, 1)),
                 ("decode_lds_dma", (0, 1)), ("posmajor_order", (0, 1)), ("warp_rows", (0, 1, 4)),
                 ("up3_cand8", (0, 1, 2, 3, 4, 5, 6, 7)), ("up3_cand8_rows", (0, 1, 2, 4, 8)), ("up3_wreg", (0, 1)),
                 ("f32_fc6_rows", (0, 64, 128))]

lib = None
_PARAMS = None


def _sptr(stream):
    return C.c_void_p(stream.cuda_stream)


def _model(dtype, h, w, blobs):
    """A vanilla fcn_8, 68 classes, of this input size on the one blob of its type (the blob does not depend on the size)."""
    global _PARAMS
    model = LANDMARKS_MODELS["fcn_8"](68, input_height=h, input_width=w, dtype=dtype)
    if dtype not in blobs:
        if _PARAMS is None:
            _PARAMS = synth_fcn8_weights(68, seed=2)
        model.load_weights(_PARAMS)
        blobs[dtype] = model._packed
    model._packed = blobs[dtype]
    return model


def _nbytes(shape, dtype):
    return int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()


def _diff(name, ref, got):
    """None when the two dicts of tensors agree bit for bit, else what differs."""
    bad = []
    for k in ref:
        if not same_bits(ref[k], got[k]):
            a, b = ref[k].flatten(), got[k].flatten()
            ne = (a != b) & ~(torch.isnan(a) & torch.isnan(b)) if a.is_floating_point() else a != b
            bad.append("%s: %d of %d elements differ" % (k, int(ne.sum()), a.numel()))
    return "%s: %s" % (name, "; ".join(bad)) if bad else None


class Job:
    """One call on buffers of its own inside one arena.  regions: the arena's; inputs: {region: numpy array};
    launch(job, stream pointer) -> status; results(job) -> {name: copy of a tensor the call wrote}; scrub: the regions
    the call writes."""

    def __init__(self, name, fill, regions, inputs, launch, results, scrub):
        self.name = name
        self.arena = Arena(fill, regions, "cuda")
        self.v = {r: self.arena.put(r, d) for r, d in inputs.items()}
        self._launch, self._results, self._scrub = launch, results, scrub
        self.ref = None
        self.scrub()

    def run(self, stream):
        """The call on `stream`; None, or the failing status with this thread's own message."""
        rc = self._launch(self, _sptr(stream))
        if rc != 0:
            return "%s failed (%d): %s" % (self.name, rc, lib.flm_last_error().decode())
        return None

    def results(self):
        return self._results(self)

    def scrub(self):
        for r in self._scrub:
            self.arena.region(r).fill_(SCRUB)

    def check(self, where):
        """After the call has finished on the current stream: [] or what is wrong against the serial reference."""
        bad = []
        d = _diff("%s %s" % (where, self.name), self.ref, self.results())
        if d:
            bad.append(d)
        try:
            self.arena.check_guards()
        except AssertionError as e:
            bad.append("%s %s: %s" % (where, self.name, e))
        return bad


def forward_job(tag, model, n, out, npts=0, thresh=0.0, opts=None, seed=0, fill=0x4B):
    h, w, c = model.input_height, model.input_width, model.n_classes
    x = np.random.default_rng(4000 + seed + 7 * n + h + w).integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    oh, ow = model.output_height, model.output_width
    shape, dt = {"probs": ((n, oh * ow, c), torch.float32), "classmap": ((n, oh, ow), torch.int32),
                 "landmarks": ((n, c, 2), torch.float64), "landmark_stats": ((n, c, _lib.LANDMARK_REC), torch.float64)}[out]
    om = _OUT[out]
    dmode, np_ = decode_mode_of(npts) if out in ("landmarks", "landmark_stats") else (0, 0)
    fo = model._opts(opts)
    regions = [("x", x.nbytes, 16, True), ("ws", model.workspace_bytes(n, out, npts, opts), 256), ("out", _nbytes(shape, dt), 16)]

    def launch(job, sp):
        ws = job.arena.region("ws")
        return lib.flm_fcn_forward_opts(sp, model._arch, _lib.ptr(model._packed), _lib.ptr(job.v["x"]), _lib.IN_U8_BGR, n, h, w,
                                        c, model._dt, om, dmode, np_, float(thresh), _lib.ptr(job.arena.view("out", dt, shape)),
                                        _lib.ptr(ws), ws.numel(), C.byref(fo))

    def results(job):
        res = {"out": job.arena.view("out", dt, shape).clone()}
        for nm in HEAD:
            res[nm] = model.intermediate(nm, n, out, npts, opts, workspace=job.arena.region("ws")).clone()
        return res
    return Job("%s %s %dx%dx%d %s n_points=%d thresh=%g %s" % (tag, model.dtype, n, h, w, out, npts, thresh, opts or ""),
               fill, regions, {"x": x}, launch, results, ("ws", "out"))


def decode_job(tag, kind, shape, npts, thresh, seed, repeat=1, modes=None, fill=0x4B):
    """kind: "decode", "stats" or "sweep" on float32 maps [n,h,w,l]; `repeat` > 1: a burst of that many calls back to back,
    each into an output slot of its own (they share the maps and, one after the other on one stream, the workspace)."""
    n, h, w, l = shape
    hm = np.random.default_rng(500 + seed).random(shape, dtype=np.float32)
    mode = int(npts > 0)
    if kind == "sweep":
        arr = _lib.int_array(modes)
        wsb, oshape = lib.flm_decode_sweep_workspace_bytes(n, h, w, l, arr, len(modes)), (len(modes), n, l, 2)
    elif kind == "stats":
        wsb, oshape = lib.flm_decode_stats_workspace_bytes(n, h, w, l, mode, npts), (n, l, _lib.LANDMARK_REC)
    else:
        wsb, oshape = lib.flm_decode_workspace_bytes(n, h, w, l, mode, npts), (n, l, 2)
    assert wsb > 0, (tag, kind)
    slot = _nbytes(oshape, torch.float64)
    oshape = (repeat,) + oshape
    regions = [("hm", hm.nbytes, 16, True), ("ws", max(wsb, 256), 256), ("out", repeat * slot, 16)]

    def launch(job, sp):
        ws, out = job.arena.region("ws"), job.arena.region("out").data_ptr()
        hmp, wsp, wsn, th = _lib.ptr(job.v["hm"]), _lib.ptr(ws), ws.numel(), float(thresh)
        for i in range(repeat):
            op = C.c_void_p(out + i * slot)
            if kind == "sweep":
                rc = lib.flm_decode_sweep(sp, hmp, n, h, w, l, arr, len(modes), th, op, wsp, wsn)
            else:
                rc = (lib.flm_decode_stats if kind == "stats" else lib.flm_decode)(sp, hmp, n, h, w, l, mode, npts, th, op, wsp, wsn)
            if rc != 0:
                return rc
        return 0
    return Job("%s %s x%d %s n_points=%s thresh=%g" % (tag, kind, repeat, "x".join(map(str, shape)), modes or npts, thresh), fill, regions,
               {"hm": hm}, launch, lambda job: {"out": job.arena.view("out", torch.float64, oshape).clone()}, ("ws", "out"))


def _similarities(k, src_hw, dst_hw, seed):
    """[k,2,3] float32 source -> destination similarities that map the whole source onto the destination, slightly rotated."""
    rng = np.random.default_rng(seed)
    m = np.zeros((k, 2, 3), np.float32)
    for i in range(k):
        s = min(dst_hw[0] / src_hw[0], dst_hw[1] / src_hw[1]) * (0.9 + 0.3 * rng.random())
        th = (rng.random() - 0.5) * 0.3
        a, b = s * np.cos(th), s * np.sin(th)
        cx, cy = (src_hw[1] - 1) / 2, (src_hw[0] - 1) / 2
        m[i] = [[a, -b, (dst_hw[1] - 1) / 2 - (a * cx - b * cy)], [b, a, (dst_hw[0] - 1) / 2 - (b * cx + a * cy)]]
    return m


def warp_fmt_job(tag, seed, fill=0x4B):
    """flm_warp_affine_fmt, uint8 source, 64-pixel rows (the form knob "warp_rows" chooses), NCHW bfloat16 RGB out."""
    fmt = alignment.AlignedFormat(layout="nchw", dtype="bfloat16", channels="rgb", scale=1 / 127.5, bias=-1.0)
    cf = fmt.struct()
    n, hs, ws_, hd, wd = 3, 40, 52, 32, 64
    img = np.random.default_rng(600 + seed).integers(0, 256, (n, hs, ws_, 3), dtype=np.uint8)
    m = _similarities(n, (hs, ws_), (hd, wd), 610 + seed)
    regions = [("src", img.nbytes, 16, True), ("m", m.nbytes, 16, True), ("dst", fmt.nbytes(n, hd, wd), fmt.itemsize)]

    def launch(job, sp):
        return lib.flm_warp_affine_fmt(sp, _lib.ptr(job.v["src"]), 1, n, hs, ws_, _lib.ptr(job.v["m"]),
                                       _lib.ptr(job.arena.region("dst")), hd, wd, C.byref(cf))
    return Job(tag + " warp_affine_fmt", fill, regions, {"src": img, "m": m}, launch,
               lambda job: {"dst": job.arena.region("dst").clone()}, ("dst",))


def crop_frames_job(tag, seed, fill=0x4B):
    nf, fh, fw, oh, ow = 2, 45, 61, 32, 32
    frames = np.random.default_rng(700 + seed).integers(0, 256, (nf, fh, fw, 3), dtype=np.uint8)
    boxes = np.array([[-7, 5, 20, 32], [40, -9, 70, 21], [30, 30, 70, 70], [-5, -5, fw + 5, fh + 5], [fw - 9, fh - 9, fw, fh],
                      [fw + 3, 2, fw + 20, 19], [10, fh - 4, 40, fh + 26]], np.int32)
    k = boxes.shape[0]
    idx = (np.arange(k, dtype=np.int32) + seed) % nf
    regions = [("frames", frames.nbytes, 16, True), ("boxes", boxes.nbytes, 16, True), ("idx", idx.nbytes, 16, True),
               ("out", k * oh * ow * 3, 16)]

    def launch(job, sp):
        return lib.flm_crop_resize_frames(sp, _lib.ptr(job.v["frames"]), fh * fw * 3, nf, fh, fw, _lib.ptr(job.v["boxes"]),
                                          _lib.ptr(job.v["idx"]), k, _lib.ptr(job.arena.region("out")), oh, ow)
    return Job(tag + " crop_resize_frames", fill, regions, {"frames": frames, "boxes": boxes, "idx": idx}, launch,
               lambda job: {"out": job.arena.region("out").clone()}, ("out",))


def quality_job(tag, seed, fill=0x4B):
    k, h, w = 3, 37, 32
    faces = np.random.default_rng(800 + seed).uniform(0, 255, (k, h, w, 3)).astype(np.float32)
    regions = [("faces", faces.nbytes, 16, True), ("rec", k * _lib.QUALITY_REC * 8, 16)]

    def launch(job, sp):
        return lib.flm_face_quality(sp, _lib.ptr(job.v["faces"]), k, h, w, None, None, _lib.ptr(job.arena.region("rec")))
    return Job(tag + " face_quality", fill, regions, {"faces": faces}, launch,
               lambda job: {"rec": job.arena.region("rec").clone()}, ("rec",))


def track_job(tag, seed, fill=0x4B):
    """One flm_track_step on the caller's own state: 3 faces, 68 landmarks, a 64-pixel input on a 72-pixel grid."""
    k, c, IN, GRID, FH, FW = 3, 68, 64, 72, 270, 480
    rng = np.random.default_rng(900 + seed)
    tc = alignment.canonical_template(c, IN, IN).astype(np.float64)
    ta = alignment.canonical_template(c, 112, 112).astype(np.float64)
    lm = (tc[None] + rng.normal(0, 1.0, (k, c, 2))) * (GRID / IN)
    lm = np.ascontiguousarray(np.where(lm < 0, 0.0, lm))
    lm[1, :5] = -1.0                                             # rejected points
    m = np.zeros((k, 2, 3), np.float32)
    boxes = np.zeros((k, 4), np.int32)
    for f in range(k):
        s, th = rng.uniform(0.4, 1.5), np.deg2rad(rng.uniform(-30, 30))
        cx, cy = rng.uniform(120, 360), rng.uniform(80, 190)
        a, b = s * np.cos(th), s * np.sin(th)
        m[f] = [[a, -b, (IN - 1) / 2 - (a * cx - b * cy)], [b, a, (IN - 1) / 2 - (b * cx + a * cy)]]
        boxes[f] = [int(cx) - 40, int(cy) - 40, int(cx) + 40, int(cy) + 40]
    opts = _lib.TrackOpts.make()
    outs = {"lm_frame": (torch.float64, (k, c, 2)), "m_align": (torch.float32, (k, 2, 3)), "m_next": (torch.float32, (k, 2, 3)),
            "boxes_next": (torch.int32, (k, 4)), "status": (torch.int32, (k,))}
    regions = [("lm", lm.nbytes, 16, True), ("m", m.nbytes, 16, True), ("boxes", boxes.nbytes, 16, True),
               ("tc", tc.nbytes, 16, True), ("ta", ta.nbytes, 16, True)] + [(nm, _nbytes(shp, dt), 16) for nm, (dt, shp) in outs.items()]

    def launch(job, sp):
        r = job.arena.region
        return lib.flm_track_step(sp, _lib.ptr(job.v["lm"]), 2, None, 1, _lib.ptr(job.v["m"]), _lib.ptr(job.v["boxes"]), k, c,
                                  IN / GRID, IN / GRID, IN, IN, FH, FW, _lib.ptr(job.v["tc"]), _lib.ptr(job.v["ta"]), C.byref(opts),
                                  _lib.ptr(r("lm_frame")), _lib.ptr(r("m_align")), _lib.ptr(r("m_next")), _lib.ptr(r("boxes_next")),
                                  _lib.ptr(r("status")))
    return Job(tag + " track_step", fill, regions, {"lm": lm, "m": m, "boxes": boxes, "tc": tc, "ta": ta}, launch,
               lambda job: {nm: job.arena.view(nm, dt, shp).clone() for nm, (dt, shp) in outs.items()}, tuple(outs))


def _serial_reference(jobs):
    """Every job alone on the default stream, with the knobs at their defaults; the buffers are scrubbed again afterwards."""
    bad = []
    s = torch.cuda.current_stream()
    for j in jobs:
        err = j.run(s)
        if err:
            bad.append("serial " + err)
            continue
        torch.cuda.synchronize()
        j.ref = j.results()
        try:
            j.arena.check_guards()
        except AssertionError as e:
            bad.append("serial %s: %s" % (j.name, e))
        j.scrub()
    torch.cuda.synchronize()
    return bad


def _run_threads(targets):
    """Start one daemon thread per target and join each with a time limit; a thread that has not finished ends the child."""
    errors = []

    def guarded(fn, i):
        try:
            torch.cuda.set_device(0)
            fn(i)
        except BaseException:
            errors.append("thread %d: %s" % (i, traceback.format_exc()))
    threads = [threading.Thread(target=guarded, args=(fn, i), daemon=True) for i, fn in enumerate(targets)]
    for t in threads:
        t.start()
    for i, t in enumerate(threads):
        t.join(JOIN_S)
        if t.is_alive():
            print("RESULT " + json.dumps({"fails": ["thread %d had not finished after %g s" % (i, JOIN_S)] + errors}), flush=True)
            os._exit(3)
    return errors


# ---- part "cold": the first call of the process, of every kind, by four threads at once ---------------------------------
def part_cold():
    blobs = {}
    m128, m64, mb = _model("f32", 128, 128, blobs), _model("f32", 64, 64, blobs), _model("bf16", 96, 160, blobs)
    torch.cuda.synchronize()
    per_thread = [[forward_job("t%d" % i, m128, 32, "landmarks", 4, seed=i),     # two positions per fc6 tile: the permutation
                   forward_job("t%d" % i, m64, 64, "landmarks", 4, seed=i),      # the rows-per-tile model and its cache
                   forward_job("t%d" % i, mb, 3, "landmarks", 4, seed=i),
                   decode_job("t%d" % i, "decode", (3, 50, 37, 68), 4, 0.0, seed=i),   # 68 landmarks: the LDS-DMA form
                   decode_job("t%d" % i, "stats", (3, 50, 37, 68), 4, 0.0, seed=i)] for i in range(WORKERS)]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream() for _ in range(WORKERS)]
    gate = threading.Barrier(WORKERS)
    fails = []

    def caller(i):
        with torch.cuda.stream(streams[i]):
            for j in per_thread[i]:
                gate.wait(JOIN_S)            # every first call of a kind is made by all four at once
                err = j.run(streams[i])
                if err:
                    fails.append("concurrent " + err)
            streams[i].synchronize()
    fails += _run_threads([caller] * WORKERS)
    torch.cuda.synchronize()
    rows = lib.flm_debug_query(b"igemm_posmajor_rows", 0)
    got = [[j.results() for j in jobs] for jobs in per_thread]
    for jobs in per_thread:
        for j in jobs:
            try:
                j.arena.check_guards()
            except AssertionError as e:
                fails.append("concurrent %s: %s" % (j.name, e))
            j.scrub()
    fails += _serial_reference([j for jobs in per_thread for j in jobs])
    compared = 0
    for jobs, gs in zip(per_thread, got):
        for j, g in zip(jobs, gs):
            if j.ref is not None:
                d = _diff("cold " + j.name, j.ref, g)
                compared += len(j.ref)
                if d:
                    fails.append(d)
    # callers with different inputs must not have produced the same landmarks (the comparison above is not vacuous)
    distinct = not same_bits(got[0][0]["out"], got[1][0]["out"])
    return {"fails": fails, "compared": compared, "igemm_posmajor_rows": rows, "distinct": distinct}


# ---- part "mixed": warm, different kernels and shapes in flight together, and a knob flipper -----------------------------
def part_mixed():
    blobs = {}
    f = {hw: _model("f32", hw[0], hw[1], blobs) for hw in ((32, 32), (96, 160), (64, 64))}
    b = {hw: _model("bf16", hw[0], hw[1], blobs) for hw in ((32, 32), (96, 160), (64, 64))}
    small = dict(candidate_cap_div=4096)          # lists that overflow: the gated fallback writes the result
    th = (0.0, 0.9986, 0.9992)                    # the standalone decodes' reject levels, one per worker (top-4 mean ~ 0.9987)
    tf = (0.0, 0.01, 0.02)                        # the forwards'
    work = [
        [forward_job("w0", f[(32, 32)], 1, "probs", seed=0), forward_job("w0", f[(96, 160)], 3, "landmarks", 4, tf[0], seed=0),
         forward_job("w0", f[(64, 64)], 20, "landmarks", 25, tf[0], seed=0), forward_job("w0", f[(64, 64)], 20, "landmark_stats", 4, tf[0], seed=1),
         forward_job("w0", b[(96, 160)], 3, "landmarks", 4, tf[0], small, seed=2),
         decode_job("w0", "sweep", (3, 50, 37, 68), 0, th[0], seed=0, modes=(0, 1, 4, 25)), track_job("w0", 0)],
        [forward_job("w1", b[(32, 32)], 1, "classmap", seed=3), forward_job("w1", b[(96, 160)], 3, "landmarks", 25, tf[1], seed=3),
         forward_job("w1", b[(64, 64)], 20, "landmarks", 4, tf[1], seed=3), forward_job("w1", b[(64, 64)], 20, "landmark_stats", 4, tf[1], seed=4),
         forward_job("w1", f[(64, 64)], 20, "landmarks", 4, tf[1], small, seed=5),
         warp_fmt_job("w1", 1), quality_job("w1", 1)],
        [forward_job("w2", f[(96, 160)], 3, "classmap", seed=6), forward_job("w2", b[(64, 64)], 20, "probs", seed=6),
         forward_job("w2", f[(32, 32)], 1, "landmarks", 4, tf[2], seed=6), forward_job("w2", b[(32, 32)], 1, "landmarks", 25, tf[2], seed=7),
         forward_job("w2", f[(64, 64)], 20, "probs", seed=8),
         decode_job("w2", "sweep", (3, 50, 37, 68), 0, th[2], seed=2, modes=(4, 1, 25)), crop_frames_job("w2", 2)],
    ]
    # Every round opens with a burst the three workers start together: BURST standalone decodes each, back to back, every
    # call into a slot of its own and every worker with its own reject level.  The launchers' host sides are a few
    # microseconds per call; a value that travelled through process state would have to be overwritten inside one of
    # them, which only thousands of overlapping calls make likely (the module docstring of test_gpu_reentrancy.py has the count).
    for i, jobs in enumerate(work):
        jobs.insert(0, decode_job("w%d" % i, "decode", (3, 50, 37, 68), 4, th[i], seed=10 + i, repeat=BURST))
    torch.cuda.synchronize()
    fails = _serial_reference([j for jobs in work for j in jobs])
    rejected = [int((jobs[0].ref["out"][0] == -1).sum()) for jobs in work]
    burst_gate = threading.Barrier(len(work))
    streams = [torch.cuda.Stream() for _ in work]
    gate = threading.Barrier(len(work) + 1)
    done = threading.Event()
    rounds, flips, calls = 8, [0], [0]
    dummy = torch.zeros(64, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def worker(i):
        with torch.cuda.stream(streams[i]):
            gate.wait(JOIN_S)
            for r in range(rounds):
                for k, j in enumerate(work[i]):
                    if k == 0:
                        burst_gate.wait(30.0)
                    err = j.run(streams[i])
                    calls[0] += 1
                    if err:
                        fails.append("round %d %s" % (r, err))
                if i == 0:      # an argument error while the others launch: no launch happens, the message is this thread's
                    rc = lib.flm_fcn_forward_opts(_sptr(streams[i]), 100 + r, _lib.ptr(dummy), _lib.ptr(dummy), 0, 1, 32, 32, 68, 0,
                                                  0, 0, 0, 0.0, _lib.ptr(dummy), _lib.ptr(dummy), 64, None)
                    msg = lib.flm_last_error().decode()
                    if rc != -1 or "unknown architecture %d" % (100 + r) not in msg:
                        fails.append("round %d: the bad call returned %d with '%s'" % (r, rc, msg))
                streams[i].synchronize()
                for j in work[i]:
                    fails.extend(j.check("round %d" % r))
                    j.scrub()
            streams[i].synchronize()

    def flipper(_i):
        found = {}
        for key, _vals in NEUTRAL_KNOBS:
            v = C.c_int()
            _lib.check(lib.flm_get_tuning(key.encode(), C.byref(v)), "get_tuning")
            found[key] = v.value
        gate.wait(JOIN_S)
        turn = 0
        try:
            while not done.is_set():
                for key, vals in NEUTRAL_KNOBS:
                    v = vals[turn % len(vals)]
                    if lib.flm_set_tuning(key.encode(), v) != 0:
                        fails.append("flm_set_tuning(%s, %d) refused: %s" % (key, v, lib.flm_last_error().decode()))
                    flips[0] += 1
                turn += 1
                done.wait(0.0005)      # (lets the workers have the interpreter; the flips go on for as long as they work)
        finally:
            for key, v in found.items():
                lib.flm_set_tuning(key.encode(), v)

    finished = [0]
    lock = threading.Lock()

    def worker_then_signal(i):
        try:
            worker(i)
        except BaseException:
            burst_gate.abort()       # (the others must not wait for a worker that is gone)
            raise
        finally:
            with lock:
                finished[0] += 1
                if finished[0] == len(work):
                    done.set()
    fails += _run_threads([worker_then_signal] * len(work) + [lambda _i: flipper(_i)])
    torch.cuda.synchronize()
    after = {}
    for key, _vals in NEUTRAL_KNOBS + [("f32_two_level", ())]:
        v = C.c_int()
        lib.flm_get_tuning(key.encode(), C.byref(v))
        after[key] = v.value
    defaults = dict(bf16_big_tiles=1, bf16_lds_dma=1, bf16_mfma16=1, bf16_halo_mfma16=1, f32_two_level=1, f32_lean_tile=1,
                    bf16_group_n=0, bf16_conv3_halo=1, bf16_score1x1=1, bf16_fused_tail=1, decode_lds_dma=1, posmajor_order=1,
                    warp_rows=1, up3_cand8=1, up3_cand8_rows=0, up3_wreg=0, f32_fc6_rows=0)
    if after != defaults:
        fails.append("knobs after the flipper: %r" % (after,))
    return {"fails": fails, "calls": calls[0], "rounds": rounds, "flips": flips[0], "jobs": sum(len(w) for w in work), "burst": BURST,
            "rejected_per_worker": rejected}


# ---- part "model": one FcnModel shared by four streams (networks/fcn.py, the cached workspaces) ---------------------------
def part_model():
    blobs = {}
    model = _model("f32", 128, 128, blobs)
    rng = np.random.default_rng(77)
    xs = [torch.from_numpy(rng.integers(0, 256, (32, 128, 128, 3), dtype=np.uint8)).cuda() for _ in range(WORKERS)]
    sizes = (32, 8, 5, 3, 2, 1, 6)               # more keys than the cache holds per stream
    assert len(sizes) > model._ws_cap

    def lm(x, **kw):
        return model.forward_device(x, "landmarks", n_points=4, **kw)
    ref = {(i, n): lm(xs[i][:n].contiguous()).clone() for i in range(WORKERS) for n in sizes}
    ref_fc6 = model.intermediate("fc6", 6, "landmarks", 4).clone()       # (the last serial forward: caller 3, 6 faces)
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream() for _ in range(WORKERS)]
    out = {"same_key": [], "rotate": [], "two_streams": [], "caller_owned": [], "intermediate": [], "fails": []}

    def cmp(where, what, want, got):
        ne = int(((want != got) & ~(torch.isnan(want) & torch.isnan(got))).sum())
        if ne or not same_bits(want, got):
            out[where].append("%s: %d of %d landmark coordinates differ from the serial call" % (what, ne, want.numel()))

    # four threads, one batch size: the cache key is the same for all
    gate = threading.Barrier(WORKERS)
    got = [[] for _ in range(WORKERS)]

    def same_key(i):
        with torch.cuda.stream(streams[i]):
            gate.wait(JOIN_S)
            for _rep in range(3):
                got[i].append(lm(xs[i]))
            streams[i].synchronize()
    out["same_key"] += _run_threads([same_key] * WORKERS)
    torch.cuda.synchronize()
    for i in range(WORKERS):
        for rep, g in enumerate(got[i]):
            cmp("same_key", "caller %d call %d" % (i, rep), ref[(i, 32)], g)

    # batch sizes in rotation, each thread from another start: evictions while other streams run
    gate2 = threading.Barrier(WORKERS)
    got2 = [[] for _ in range(WORKERS)]

    def rotate(i):
        with torch.cuda.stream(streams[i]):
            gate2.wait(JOIN_S)
            for rep in range(2 * len(sizes)):
                n = sizes[(rep + 2 * i) % len(sizes)]
                got2[i].append((n, lm(xs[i][:n].contiguous())))
            streams[i].synchronize()
    out["rotate"] += _run_threads([rotate] * WORKERS)
    torch.cuda.synchronize()
    for i in range(WORKERS):
        for rep, (n, g) in enumerate(got2[i]):
            cmp("rotate", "caller %d call %d (%d faces)" % (i, rep, n), ref[(i, n)], g)
    cached = len(model._ws)

    # no thread at all: stream A, and at once, without a sync, stream B -- same key, different inputs
    with torch.cuda.stream(streams[0]):
        ga = lm(xs[0])
    with torch.cuda.stream(streams[1]):
        gb = lm(xs[1])
    torch.cuda.synchronize()
    cmp("two_streams", "stream A", ref[(0, 32)], ga)
    cmp("two_streams", "stream B", ref[(1, 32)], gb)

    # intermediate() finds the workspace of the last forward on the current stream
    with torch.cuda.stream(streams[2]):
        lm(xs[3][:6].contiguous())
        with torch.cuda.stream(streams[3]):
            lm(xs[0][:6].contiguous())           # another stream's forward at the same key in between
        fc6 = model.intermediate("fc6", 6, "landmarks", 4).clone()
    torch.cuda.synchronize()
    if not same_bits(fc6, ref_fc6):
        out["intermediate"].append("fc6 of the last forward on this stream: %d of %d elements differ"
                                   % (int((fc6 != ref_fc6).sum()), fc6.numel()))

    # caller-owned workspaces and outputs
    own = [(model.new_workspace(32, "landmarks", 4), torch.empty((32, 68, 2), dtype=torch.float64, device="cuda")) for _ in range(WORKERS)]
    for _ws, o in own:
        o.fill_(-7.0)
    torch.cuda.synchronize()
    gate3 = threading.Barrier(WORKERS)

    def caller_owned(i):
        with torch.cuda.stream(streams[i]):
            gate3.wait(JOIN_S)
            for _rep in range(3):
                lm(xs[i], workspace=own[i][0], out_tensor=own[i][1])
            streams[i].synchronize()
    out["caller_owned"] += _run_threads([caller_owned] * WORKERS)
    torch.cuda.synchronize()
    for i in range(WORKERS):
        cmp("caller_owned", "caller %d" % i, ref[(i, 32)], own[i][1])
    out["cached_workspaces"] = cached
    out["ws_cap"] = model._ws_cap
    return out


# ---- part "align": prediction.align_frames from two threads on two streams, the default template cold ----------------------
def part_align():
    blobs = {}
    model = _model("f32", 64, 64, blobs)
    rng = np.random.default_rng(31)
    rings = [torch.from_numpy(rng.integers(0, 256, (2, 270, 480, 3), dtype=np.uint8)).cuda() for _ in range(2)]
    faces = [[[(10, 20, 110, 130), (200, 40, 330, 160)], [(300, 100, 470, 260), (0, 0, 90, 90), (50, 150, 140, 250)]],
             [[(30, 30, 150, 160), (220, 60, 340, 170), (5, 5, 60, 70)], [(280, 90, 460, 250), (60, 140, 150, 240)]]]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream() for _ in range(2)]
    gate = threading.Barrier(2)
    got = [None, None]
    fails = []

    def call(i):
        return prediction.align_frames(rings[i], faces[i], model, out_size=(112, 112), n_points=4, weights="score")

    def caller(i):
        with torch.cuda.stream(streams[i]):
            gate.wait(JOIN_S)
            for _rep in range(3):
                got[i] = call(i)           # the first of these uploads the module's template: both threads at once
            streams[i].synchronize()
    fails += _run_threads([caller] * 2)
    torch.cuda.synchronize()
    names = ("aligned", "m", "landmarks", "boxes", "weights")
    for i in range(2):
        ref = call(i)
        torch.cuda.synchronize()
        d = _diff("align_frames caller %d" % i, dict(zip(names, ref)), dict(zip(names, got[i])))
        if d:
            fails.append(d)
    tm = prediction._TEMPLATES[(68, 112, 112, str(rings[0].device))]
    if not np.array_equal(tm.cpu().numpy(), alignment.canonical_template(68, 112, 112)):
        fails.append("the cached template is not the canonical template")
    return {"fails": fails, "faces": [int(g[0].shape[0]) for g in got]}


# ---- part "graphs": two captured pipelines, each replayed from its own thread on its own stream ----------------------------
def part_graphs():
    blobs = {}
    model = _model("f32", 128, 128, blobs)
    rng = np.random.default_rng(61)
    ns = (1, 5)
    pipes = [graphs.CapturedPipeline(model, n, n_points=4) for n in ns]       # captured one after the other, here
    crops = [[torch.from_numpy(rng.integers(0, 256, (n, 128, 128, 3), dtype=np.uint8)).cuda() for _rep in range(3)] for n in ns]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream() for _ in ns]
    gate = threading.Barrier(len(ns))
    got = [[] for _ in ns]
    fails = []

    def replay(i):
        with torch.cuda.stream(streams[i]):
            gate.wait(JOIN_S)
            for x in crops[i]:
                got[i].append([t.clone() for t in pipes[i](x)])
            streams[i].synchronize()
    fails += _run_threads([replay] * len(ns))
    torch.cuda.synchronize()
    for i, n in enumerate(ns):
        for rep, x in enumerate(crops[i]):
            lm_e = model.forward_device(x, "landmarks", n_points=4)
            al_e, m_e = alignment.align_device(x, lm_e, pipes[i].template, 128, 128, pipes[i].scale)
            torch.cuda.synchronize()
            d = _diff("pipeline of %d faces, replay %d" % (n, rep), {"landmarks": lm_e, "aligned": al_e, "m": m_e},
                      dict(zip(("landmarks", "aligned", "m"), got[i][rep])))
            if d:
                fails.append(d)
    return {"fails": fails, "replays": sum(len(g) for g in got)}


PARTS = {"cold": part_cold, "mixed": part_mixed, "model": part_model, "align": part_align, "graphs": part_graphs}


def main(part):
    global lib
    torch.cuda.set_device(0)
    lib = _lib.load()
    try:
        res = PARTS[part]()
    except BaseException:
        res = {"fails": ["the child raised: " + traceback.format_exc()]}
    print("RESULT " + json.dumps(res), flush=True)
    sys.stdout.flush()
    os._exit(0)      # (daemon threads and captured graphs need no orderly teardown)
