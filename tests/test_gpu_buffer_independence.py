"""The buffer contract of include/flm.h ("what a call may assume about its buffers"), held on the device: in one call the
result depends on nothing the workspace, the output or the gaps of the packed blob held before, nor on the memory beside
any operand, and nothing outside the workspace and the output is written.

Every case runs its call three times, each time with the input, the workspace, the output (and the packed blob, where the
case covers it) carved from one allocation pre-filled with a byte (tests/arena.py): 0x00 -- what the fresh pages of a test
process read as, the reference --, then 0x4B (1.33e7 as float32 and as bfloat16: a finite stray operand survives a ReLU,
which swallows a NaN), then 0xFF (NaN in both types, all ones as an integer).  The three runs must agree BIT FOR BIT
(arena.same_bits; no tolerance anywhere) in the output and in every named intermediate the workspace layout holds --
act<i>, f1 .. f5, fc6, fc7, score5, fuse4, seg_feats with their pad class columns, and the probability region where the
call materialises it --; every byte of the 4 MiB guards on both sides of every operand must still hold the fill, and the
inputs must be unchanged.  The workspace and the blob start at an address that is 256 modulo 512, the input and the output
at 16 modulo 32: what the header promises and no better.  The values themselves are pinned by the other modules at these
same shapes (test_gpu_fp32_layers.py, test_gpu_bf16_layers.py, test_gpu_encoder_layers.py, test_gpu_decode.py, ...).

Audit by reading, before the first run: the integer fields of the workspaces.  A fill that reached a counter, a length or an
index would steer WRITES, not values, so each was traced to the statement that initialises it in the same call.

    field (include/flm.h name)         what it is                                  initialised in the same call by
    cand_cnt [n] + flag [n]            keys appended per face; overflow flag       hipMemsetAsync, csrc/flm_api_fcn.hip forward_impl
                                                                                   ("FLM_HIP(hipMemsetAsync(cnt, 0, ...))"),
                                                                                   issued before the three launches that add to it
    cand_sub                           per (face, tile, wave, sampled phase)       csrc/flm_convt.hip convt_kernel, "if (SAMPLE)":
                                       16 MT maxima as float bits; read as         every workgroup of the sampling launch stores all
                                       VALUES by cand_tau_kernel                   sub * 16 MT entries of its four waves (classes
                                                                                   >= C as 0); grid = n * tiles per face, which is
                                                                                   convt_sample_slots() / (4 sub) -- no slot is left
    cand_tau [n][C]                    float thresholds                            csrc/flm_cand.hip cand_tau_kernel /
                                                                                   cand_tau_small_kernel: every (face, c < C)
    cand_keys [n][cap]                 order_bits(p) << 32 | class << 17 | pixel   only [0, min(cand_cnt[face], cap)) is read
                                                                                   (cand_merge_kernel, "const unsigned cnt = min(");
                                                                                   the class and pixel of a key select a bucket in
                                                                                   LDS (bounded by nc) and enter x, y as values
    decode keys [n][chunks][L][n_max]  (value, pixel) lists per chunk              csrc/flm_decode.hip store_list: every workgroup
                                                                                   (chunk, face) stores ranks 0 .. n_max-1 of every
                                                                                   channel c < L; decode_plan never makes an empty
                                                                                   chunk (chunks = ceil(HW / chunk_px)); the pixel
                                                                                   of a key only enters x, y
    decode / stats sums                float64 partial sums, 3 or 6 per            lane_sums_write / group_sums_flush (flm_decode.hip)
      [n][chunks][L][3 | 6]            (chunk, landmark)                           and their six-sum forms (flm_decode_stats.hip):
                                                                                   every (chunk, c < L)
    probability region as scratch      up3_wreg: bf16 copy of seg_feats with a     csrc/flm_up3_wreg.hip up3_xpack_kernel: one thread
                                       zero ring, no integer                       per 16 bytes of the copy, ring included
    split-K slices                     float32 partial sums, no integer            written by the slices, summed by the reduce launch

No field is used before the call has written it; the only one that steers a write (cand_cnt: the base of a key range, the
gate of the fallback launches) is the one the memset clears.  The csrc/ tree has no other global counter, ticket or index
(the igemm's tap masks, the candidate kernels' wave counters and the merge's histograms live in LDS and are cleared there).

Shapes (the smallest that reach each launch form; vanilla fcn_8, 68 classes): 1 x 32 x 32 (split-K in fc6, fc7, the score
convs and enc3; fc6 all padding but its centre tap), 3 x 96 x 160 (ragged tiles everywhere), 20 x 64 x 64 (above the split-K
brackets, partial last tiles), 32 x 128 x 128 (two positions per fc6 tile, the position permutation), 64 x 64 x 64 with
f32_fc6_rows = 64 (the 64-row fc6 form, read back through flm_debug_query("igemm_posmajor_rows"); forced, as
tests/test_gpu_igemm_rows64.py forces it at this shape: split-K launches keep 128 rows unless the knob says 64).  Outputs: probs, logits, classmap, landmarks with n = 4 and
25 (candidate path), with landmark_candidates = 0, with n_points = 0, landmark_stats, and the overflow fallback
(candidate_cap_div = 4096, the flag is read back).  Knobs: f32_lean_tile = 0, f32_two_level = 0, f32_fc6_rows 64 and 128
(fp32) and the bf16 launch knobs, always left through _lib.tuning.  Generic class layouts C = 1, 17, 65, 96; fcn_32; the VGG,
MobileNet and ResNet50 encoders; one arena serving three calls in a row without a refill; the packed blob packed into
pre-filled buffers (set_weights(packed=)); the standalone decodes with caller-owned workspaces; the image kernels.

Result on an MI355X, unmodified kernels: all 119 cases pass -- no byte of any output or named intermediate depends on the
fill, every guard is intact after every call, no input changed.  Nothing to fix in a kernel or a launcher; no real finding.

Fault injection (a scratch build, not committed; wrong values only -- no counter, length or index touched; run once).  The
write-out of score5 skips the pad class columns C .. Cp-1 (conv_layer hands the implicit GEMM cout = C instead of Cp for
that launch, so neither the tile epilogue nor the split-K reduce stores them), the columns flm_pack.hip promises "come out
as exact zeros".  The suite as it stood passes on fresh pages, where the unwritten columns read as the zeros they should
be.  Here 42 of the 119 cases fail and 77 pass: every case whose layout has pad columns -- all 26 bf16 68-class cases
(Cp = 72), fcn_8 with C = 1, 17, 65 in both types (C = 96 has none and passes), fcn_32 C = 17 in both types, the three bf16
encoder cases, both reuse cases (at their third, bf16, call), the blob cases fcn_8 C = 68 bf16, C = 17 bf16 and fcn_32 C = 17
fp32 -- and none without: every fp32 68-class case (Cp = 68), the decodes and the image kernels pass.  What they report,
fcn_8 C = 17 at 3 x 64 x 96 in either type: with 0x4B only score5 differs (270 of 576 elements, the first at column 17: 0.0
with 0x00, 13323083.0 with 0x4B) -- the stray finite value is multiplied by up5's packed zero rows and vanishes, which is
exactly the over-read-times-zero class the issue names --; with 0xFF the NaN survives the multiplication and fuse4,
seg_feats (9216 of 9216 elements) and the output are NaN throughout.  fcn_32 C = 17: score5 180 of 384 elements, the
output NaN with 0xFF.  The guards stay intact in every failing case: the fault is in values only.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from arena import FILLS, Arena, same_bits

pytestmark = pytest.mark.gpu

HEAD = ("fc6", "fc7", "score5", "fuse4", "seg_feats")


@pytest.fixture(scope="module")
def flm():
    import flm_amd
    from flm_amd import _lib
    _lib.load()
    yield flm_amd
    _PARAMS.clear()
    _BLOBS.clear()


# ---- weights: one synthetic set on the host at a time, one packed blob per (model, classes, type) on the device -----
_PARAMS = {}
_BLOBS = {}
_ENCODERS = {"fcn_8_vgg": "vgg", "fcn_8_mobilenet": "mobilenet", "fcn_8_resnet50": "resnet50"}


def _params(arch, c):
    from flm_amd.weights import synth_fcn32_weights, synth_fcn8_weights
    if (arch, c) not in _PARAMS:
        _PARAMS.clear()
        if arch in _ENCODERS:
            import enc_chain_cases
            assert c == 68
            _PARAMS[(arch, c)] = enc_chain_cases.encoder_params(_ENCODERS[arch])
        else:
            _PARAMS[(arch, c)] = (synth_fcn32_weights if arch == "fcn_32" else synth_fcn8_weights)(c, seed=2)
    return _PARAMS[(arch, c)]


def _model(arch, c, dtype, h, w):
    """A model of this input size on the blob of its (arch, classes, type): the blob does not depend on the input size, so
    it is packed once."""
    from flm_amd.networks import LANDMARKS_MODELS
    model = LANDMARKS_MODELS[arch](c, input_height=h, input_width=w, dtype=dtype)
    key = (arch, c, dtype)
    if key not in _BLOBS:
        if _BLOBS and next(iter(_BLOBS))[:2] != key[:2]:
            _BLOBS.clear()
        model.load_weights(_params(arch, c))
        _BLOBS[key] = model._packed
    model._packed = _BLOBS[key]
    return model


def _crops(n, h, w, seed=0):
    return np.random.default_rng(1000 + seed + 7 * n + h + w).integers(0, 256, (n, h, w, 3), dtype=np.uint8)


# ---- one forward inside an arena ----------------------------------------------------------------------------------------
def _out_spec(model, n, out):
    from flm_amd import _lib
    oh, ow, c = model.output_height, model.output_width, model.n_classes
    return {"probs": ((n, oh * ow, c), torch.float32), "logits": ((n, oh, ow, c), torch.float32),
            "classmap": ((n, oh, ow), torch.int32), "landmarks": ((n, c, 2), torch.float64),
            "landmark_stats": ((n, c, _lib.LANDMARK_REC), torch.float64)}[out]


def _nbytes(shape, dtype):
    return int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()


def _names(model, ws_probs):
    return (["act%d" % i for i in range(len(model.encoder_layer_names()))] + ["f%d" % k for k in range(1, 6)] + list(HEAD)
            + (["probs"] if ws_probs else []))


def _forward_in(arena, model, x, out, n_points, thresh, opts, ws_probs, post=None):
    """The forward on the arena's "x", "ws" and "out"; returns {name: copy} of the output and the named intermediates."""
    n = x.shape[0]
    shape, dt = _out_spec(model, n, out)
    xt = arena.put("x", x)
    ws = arena.region("ws")
    ot = arena.view("out", dt, shape)
    got = model.forward_device(xt, out, n_points=n_points, thresh=thresh, out_tensor=ot, workspace=ws, opts=opts)
    torch.cuda.synchronize()
    assert got.data_ptr() == ot.data_ptr()
    arena.check_guards()
    res = {"out": ot.clone()}
    for name in _names(model, ws_probs):
        try:
            res[name] = model.intermediate(name, n, out, n_points, opts, workspace=ws).clone()
        except KeyError:                     # (fcn_32 has no fuse4 / seg_feats)
            assert model._fcn32 and name in ("fuse4", "seg_feats"), name
    if post is not None:
        post(model, ws)
    return res


def _compare(label, ref, got, fill):
    bad = []
    for name in ref:
        if not same_bits(ref[name], got[name]):
            a, b = ref[name].flatten(), got[name].flatten()
            if a.is_floating_point():
                diff = (a != b) & ~(torch.isnan(a) & torch.isnan(b))
            else:
                diff = a != b
            idx = torch.nonzero(diff).flatten()
            first = int(idx[0]) if idx.numel() else -1
            bad.append("%s: %d of %d elements differ (first at %d: %r with 0x00, %r with 0x%02X)"
                       % (name, idx.numel(), a.numel(), first, a[first].item() if first >= 0 else None,
                          b[first].item() if first >= 0 else None, fill))
    if bad:
        print("%s, fill 0x%02X:\n  %s" % (label, fill, "\n  ".join(bad)))
    return bad


def _independent(label, model, x, out, n_points=0, thresh=0.0, opts=None, ws_probs=False, post=None):
    """The three runs of one forward and their comparison; returns the 0x00 run's tensors."""
    n = x.shape[0]
    shape, dt = _out_spec(model, n, out)
    regions = [("x", x.nbytes, 16, True), ("ws", model.workspace_bytes(n, out, n_points, opts), 256),
               ("out", _nbytes(shape, dt), 16)]
    ref, bad = None, []
    for fill in FILLS:
        got = _forward_in(Arena(fill, regions, "cuda"), model, x, out, n_points, thresh, opts, ws_probs, post)
        if ref is None:
            ref = got
            assert all(bool(torch.isfinite(v.float()).all()) for k, v in ref.items() if k not in ("out", "probs")), label
        else:
            bad += _compare(label, ref, got, fill)
    assert not bad, (label, bad)
    return ref


# the outputs of the 68-class graphs: (id, out, n_points, opts, probability region materialised)
OUTPUTS = [("probs", "probs", 0, None, False), ("logits", "logits", 0, None, False), ("classmap", "classmap", 0, None, False),
           ("lm4", "landmarks", 4, None, False), ("lm25", "landmarks", 25, None, False),
           ("lm4-nocand", "landmarks", 4, dict(landmark_candidates=0), True), ("lm-allpixel", "landmarks", 0, None, True),
           ("stats4", "landmark_stats", 4, None, False), ("lm4-overflow", "landmarks", 4, dict(candidate_cap_div=4096), True)]


def _overflow_flag_is_up(n_points):
    """post hook of the overflow case: the candidate launch raised the flag, so the gated fallback is what wrote the result."""
    def post(model, ws):
        from flm_amd import _lib
        fo = model._opts(dict(candidate_cap_div=4096))
        n = post.n
        off = _lib.load().flm_fcn_workspace_offset_opts(model._arch, b"cand_cnt", n, model.input_height, model.input_width,
                                                        model.n_classes, model._dt, _lib.OUT_LANDMARKS, _lib.DECODE_TOPN,
                                                        n_points, C.byref(fo))
        assert off >= 0
        cnt = ws[off:off + 4 * (n + 1)].view(torch.int32).cpu().numpy()
        assert cnt[n] != 0, "the lists did not overflow: the fallback did not run"
    return post


def _run_output(label, model, x, spec, post=None):
    oid, out, n_points, opts, ws_probs = spec
    if oid == "lm4-overflow":
        post = _overflow_flag_is_up(n_points)
        post.n = x.shape[0]
    return _independent("%s %s" % (label, oid), model, x, out, n_points, 0.0, opts, ws_probs, post)


# ---- fcn_8 vanilla, 68 classes, fp32 ------------------------------------------------------------------------------------
F32_SHAPES = [(1, 32, 32), (3, 96, 160), (20, 64, 64), (32, 128, 128), (64, 64, 64)]


@pytest.mark.parametrize("spec", OUTPUTS, ids=[s[0] for s in OUTPUTS])
@pytest.mark.parametrize("n,h,w", F32_SHAPES, ids=["%dx%dx%d" % s for s in F32_SHAPES])
def test_fcn8_f32(flm, n, h, w, spec):
    from flm_amd import _lib
    lib = _lib.load()
    model = _model("fcn_8", 68, "f32", h, w)
    x = _crops(n, h, w)
    label = "fcn_8 f32 %dx%dx%d" % (n, h, w)
    if (n, h, w) != (64, 64, 64):
        _run_output(label, model, x, spec)
        return
    # the 64-row fc6 form, forced: a split-K launch keeps 128 rows unless the knob says 64 (include/flm.h, "f32_fc6_rows")
    def rows64(model, ws):
        assert lib.flm_debug_query(b"igemm_posmajor_rows", 0) == 64
    with _lib.tuning(f32_fc6_rows=64):
        if spec[0] == "lm4-overflow":
            _run_output(label + " rows64", model, x, spec)
            assert lib.flm_debug_query(b"igemm_posmajor_rows", 0) == 64
        else:
            _run_output(label + " rows64", model, x, spec, post=rows64)


F32_KNOBS = [dict(f32_lean_tile=0), dict(f32_two_level=0), dict(f32_fc6_rows=64), dict(f32_fc6_rows=128)]


@pytest.mark.parametrize("knob", F32_KNOBS, ids=["%s=%d" % kv for k in F32_KNOBS for kv in k.items()])
@pytest.mark.parametrize("n,h,w", [(3, 96, 160), (20, 64, 64)], ids=["3x96x160", "20x64x64"])
def test_fcn8_f32_knobs(flm, n, h, w, knob):
    from flm_amd import _lib
    model = _model("fcn_8", 68, "f32", h, w)
    x = _crops(n, h, w)
    with _lib.tuning(**knob):
        for spec in (OUTPUTS[0], OUTPUTS[3]):     # probs, landmarks n = 4
            _run_output("fcn_8 f32 %dx%dx%d %s" % (n, h, w, knob), model, x, spec)
        if "f32_fc6_rows" in knob:
            assert _lib.load().flm_debug_query(b"igemm_posmajor_rows", 0) == knob["f32_fc6_rows"]


# ---- the same graph in bf16 ---------------------------------------------------------------------------------------------
BF16_KNOBS = [{}, dict(up3_cand8=0), dict(up3_cand8=3), dict(up3_cand8_rows=1), dict(up3_cand8_rows=8), dict(up3_wreg=1),
              dict(bf16_fused_tail=0), dict(bf16_score1x1=0), dict(bf16_conv3_halo=0), dict(bf16_conv3_halo=2),
              dict(bf16_big_tiles=0), dict(bf16_big_tiles=2), dict(bf16_group_n=8)]


def _knob_id(k):
    return ",".join("%s=%d" % kv for kv in k.items()) or "defaults"


@pytest.mark.parametrize("knob", BF16_KNOBS, ids=[_knob_id(k) for k in BF16_KNOBS])
@pytest.mark.parametrize("n,h,w", [(3, 96, 160), (20, 64, 64)], ids=["3x96x160", "20x64x64"])
def test_fcn8_bf16(flm, n, h, w, knob):
    from flm_amd import _lib
    model = _model("fcn_8", 68, "bf16", h, w)
    x = _crops(n, h, w)
    # the defaults take every output; a knob the outputs whose launches it changes (the candidate knobs: the landmarks)
    specs = OUTPUTS if not knob else [s for s in OUTPUTS if s[0] in ("probs", "lm4", "lm25", "stats4", "lm4-overflow")]
    with _lib.tuning(**knob):
        for spec in specs:
            _run_output("fcn_8 bf16 %dx%dx%d %s" % (n, h, w, _knob_id(knob)), model, x, spec)


# ---- generic class layouts, fcn_32, the other encoders --------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("c", [1, 17, 65, 96])
def test_fcn8_generic_classes(flm, c, dtype):
    n, h, w = 3, 64, 96
    model = _model("fcn_8", c, dtype, h, w)
    x = _crops(n, h, w, seed=c)
    label = "fcn_8 %s C=%d %dx%dx%d" % (dtype, c, n, h, w)
    _independent(label + " probs", model, x, "probs")
    _independent(label + " landmarks", model, x, "landmarks", n_points=4, ws_probs=True)   # no candidate path: materialised


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_fcn32_c17(flm, dtype):
    n, h, w = 2, 64, 96
    model = _model("fcn_32", 17, dtype, h, w)
    x = _crops(n, h, w, seed=32)
    _independent("fcn_32 %s C=17 probs" % dtype, model, x, "probs")
    _independent("fcn_32 %s C=17 landmarks" % dtype, model, x, "landmarks", n_points=4, ws_probs=True)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("arch", list(_ENCODERS))
def test_other_encoders(flm, arch, dtype):
    """Strides, the residual add, the depthwise kernel, the max-pool: every act<i> of the 13 / 27 / 54 layers is compared."""
    n, h, w = 2, 64, 64
    model = _model(arch, 68, dtype, h, w)
    _independent("%s %s %dx%dx%d probs" % (arch, dtype, n, h, w), model, _crops(n, h, w, seed=5), "probs")


# ---- one block serving changing batches, never refilled ------------------------------------------------------------------
@pytest.mark.parametrize("fill", FILLS[1:], ids=["0x4B", "0xFF"])
def test_reuse_without_refill(flm, fill):
    """20 x 64 x 64 landmarks, then 3 x 64 x 64 probs, then 3 x 64 x 64 landmarks with up3_wreg = 1 (bf16) in the same bytes:
    every later call runs on what the earlier ones left (and, beyond that, on the fill) and must give the bits it gives in
    a 0x00 arena of its own."""
    from flm_amd import _lib
    h = w = 64
    f32, bf16 = _model("fcn_8", 68, "f32", h, w), _model("fcn_8", 68, "bf16", h, w)
    x20, x3 = _crops(20, h, w), _crops(3, h, w, seed=3)
    calls = [(f32, x20, "landmarks", 4, {}), (f32, x3, "probs", 0, {}), (bf16, x3, "landmarks", 4, dict(up3_wreg=1))]

    def regions(group):
        return [("x", max(x.nbytes for _m, x, *_ in group), 16, True),
                ("ws", max(m.workspace_bytes(x.shape[0], out, npts) for m, x, out, npts, _k in group), 256),
                ("out", max(_nbytes(*_out_spec(m, x.shape[0], out)) for m, x, out, _n, _k in group), 16)]
    shared = Arena(fill, regions(calls), "cuda")
    bad = []
    for i, (model, x, out, npts, knob) in enumerate(calls):
        with _lib.tuning(**knob):
            ref = _forward_in(Arena(0x00, regions([calls[i]]), "cuda"), model, x, out, npts, 0.0, None, False)
            got = _forward_in(shared, model, x, out, npts, 0.0, None, False)
        bad += _compare("call %d (%s %s %d faces)" % (i, model.dtype, out, x.shape[0]), ref, got, fill)
    assert not bad, bad


# ---- the packed blob: packed into pre-filled buffers -----------------------------------------------------------------------
BLOB_CASES = [("fcn_8", 68, "f32", (3, 96, 160)), ("fcn_8", 68, "bf16", (3, 96, 160)), ("fcn_8", 17, "bf16", (3, 64, 96)),
              ("fcn_32", 17, "f32", (2, 64, 96)), ("fcn_8_resnet50", 68, "f32", (2, 64, 64))]


@pytest.mark.parametrize("arch,c,dtype,shape", BLOB_CASES, ids=["%s-C%d-%s" % b[:3] for b in BLOB_CASES])
def test_packed_blob_gaps(flm, arch, c, dtype, shape):
    """set_weights(packed=) into blobs pre-filled with each pattern: the pack writes every byte the forward reads, so the
    outputs agree; the gaps between the blob's 256-byte regions keep whatever the buffer held."""
    from flm_amd.networks import LANDMARKS_MODELS
    n, h, w = shape
    params = _params(arch, c)
    x = _crops(n, h, w, seed=11)
    label = "%s C=%d %s blob" % (arch, c, dtype)
    ref, bad = None, []
    outs = [("probs", 0)] + ([("landmarks", 4)] if c == 68 else [])
    for fill in FILLS:
        model = LANDMARKS_MODELS[arch](c, input_height=h, input_width=w, dtype=dtype)
        need = model.packed_bytes()
        blob = Arena(fill, [("blob", need, 256)], "cuda")
        model.set_weights(params, packed=blob.region("blob"))
        torch.cuda.synchronize()
        assert model._packed.data_ptr() == blob.region("blob").data_ptr() and model._packed.data_ptr() % 512 == 256
        blob.check_guards()
        packed = blob.region("blob").clone()
        got = {}
        for out, npts in outs:
            shp, dt = _out_spec(model, n, out)
            a = Arena(fill, [("x", x.nbytes, 16, True), ("ws", model.workspace_bytes(n, out, npts), 256),
                             ("out", _nbytes(shp, dt), 16)], "cuda")
            for k, v in _forward_in(a, model, x, out, npts, 0.0, None, False).items():
                got["%s/%s" % (out, k)] = v
        blob.check_guards()
        assert torch.equal(blob.region("blob"), packed), "the forward wrote into the packed blob"
        if ref is None:
            ref = got
        else:
            bad += _compare(label, ref, got, fill)
    assert not bad, (label, bad)


# ---- the standalone decodes with caller-owned workspaces -------------------------------------------------------------------
MAPS = [((3, 50, 37, 68), {}, (0, 1, 4, 25, 64, 81)), ((3, 50, 37, 68), dict(decode_lds_dma=0), (0, 1, 4, 25, 64, 81)),
        ((1, 24, 24, 80), {}, (0, 1, 4, 25, 64, 81)), ((1, 8, 9, 3), {}, (0, 1, 4, 25, 64, 81, 128))]


@pytest.mark.parametrize("shape,knob,modes", MAPS, ids=["3x50x37x68", "3x50x37x68-nodma", "1x24x24x80", "1x8x9x3"])
def test_standalone_decodes(flm, shape, knob, modes):
    """flm_decode and flm_decode_stats through the wrappers' workspace= and out=, flm_decode_sweep through ctypes: 3 x 50 x
    37 x 68 (chunks end inside a tile; the LDS-DMA ring and, with decode_lds_dma = 0, the register prefetch), 1 x 24 x 24 x
    80, and 1 x 8 x 9 x 3 with n_points up to 128 (a map smaller than the list)."""
    from flm_amd import _lib
    from flm_amd.utils.metrics import decode_device, decode_stats_device
    lib = _lib.load()
    n, h, w, l = shape
    hm = np.random.default_rng(77 + l).random(shape, dtype=np.float32)
    arr = _lib.int_array(modes)
    calls = [("decode n=%d" % m, lib.flm_decode_workspace_bytes(n, h, w, l, int(m > 0), m), (n, l, 2)) for m in modes]
    calls += [("stats n=%d" % m, lib.flm_decode_stats_workspace_bytes(n, h, w, l, int(m > 0), m), (n, l, _lib.LANDMARK_REC))
              for m in modes]
    calls += [("sweep", lib.flm_decode_sweep_workspace_bytes(n, h, w, l, arr, len(modes)), (len(modes), n, l, 2))]
    bad = []
    with _lib.tuning(**knob):
        for ci, (what, wsb, oshape) in enumerate(calls):
            assert wsb > 0, what
            ref = None
            for fill in FILLS:
                a = Arena(fill, [("hm", hm.nbytes, 16, True), ("ws", max(wsb, 256), 256), ("out", _nbytes(oshape, torch.float64), 16)],
                          "cuda")
                hmt = a.put("hm", hm)
                out = a.view("out", torch.float64, oshape)
                ws = a.region("ws")
                if what == "sweep":
                    _lib.check(lib.flm_decode_sweep(_lib.stream_ptr(), _lib.ptr(hmt), n, h, w, l, arr, len(modes), 0.0,
                                                    _lib.ptr(out), _lib.ptr(ws), ws.numel()), "flm_decode_sweep")
                else:
                    m = modes[ci % len(modes)]
                    (decode_device if what.startswith("decode") else decode_stats_device)(hmt, m, 0.0, out=out, workspace=ws)
                torch.cuda.synchronize()
                a.check_guards()
                got = {"out": out.clone()}
                if ref is None:
                    ref = got
                    assert bool(torch.isfinite(ref["out"]).all()), what
                else:
                    bad += _compare("%s %s %s" % (shape, knob, what), ref, got, fill)
    assert not bad, bad


# ---- the image kernels: inputs and outputs in the arena, no workspace ---------------------------------------------------------
def _image_case(label, regions, inputs, call):
    """regions: arena regions; inputs: {region: numpy array}; call(views) runs the kernel on the arena's views (inputs by
    name, writable regions as uint8) and returns the output tensor, which lies in the arena."""
    ref, bad = None, []
    for fill in FILLS:
        a = Arena(fill, regions, "cuda")
        views = {name: a.put(name, data) for name, data in inputs.items()}
        for name, *_ in regions:
            if name not in views:
                views[name] = a.region(name)
        out = call(views)
        torch.cuda.synchronize()
        lo = out.data_ptr() - a.buf.data_ptr()
        assert 0 <= lo and lo + out.numel() * out.element_size() <= a.nbytes, "the output must lie in the arena"
        a.check_guards()
        got = {"out": out.clone()}
        if ref is None:
            ref = got
        else:
            bad += _compare(label, ref, got, fill)
    assert not bad, (label, bad)
    return ref["out"]


def _similarities(k, src_hw, dst_hw, seed):
    """[k,2,3] float32 source -> destination similarities that map the whole source onto the destination, slightly rotated:
    every border of the source is sampled, the last row and column of the last image included, and some taps fall outside
    (clamped)."""
    rng = np.random.default_rng(seed)
    m = np.zeros((k, 2, 3), np.float32)
    for i in range(k):
        s = min(dst_hw[0] / src_hw[0], dst_hw[1] / src_hw[1]) * (0.9 + 0.3 * rng.random())
        th = (rng.random() - 0.5) * 0.3
        a, b = s * np.cos(th), s * np.sin(th)
        cx, cy = (src_hw[1] - 1) / 2, (src_hw[0] - 1) / 2
        m[i] = [[a, -b, (dst_hw[1] - 1) / 2 - (a * cx - b * cy)], [b, a, (dst_hw[0] - 1) / 2 - (b * cx + a * cy)]]
    return m


WARPS = [("u8-64wide", np.uint8, (3, 40, 52), (32, 64), {}), ("u8-64wide-rows0", np.uint8, (3, 40, 52), (32, 64), dict(warp_rows=0)),
         ("u8-64wide-rows4", np.uint8, (3, 40, 52), (32, 64), dict(warp_rows=4)), ("u8-odd", np.uint8, (3, 33, 47), (29, 31), {}),
         ("u8-2col", np.uint8, (2, 9, 2), (16, 64), {}), ("f32", np.float32, (3, 40, 52), (32, 64), {}),
         ("f32-2col", np.float32, (2, 9, 2), (15, 17), {})]


@pytest.mark.parametrize("wid,dtype,src,dst,knob", WARPS, ids=[w[0] for w in WARPS])
def test_warp_device(flm, wid, dtype, src, dst, knob):
    from flm_amd import _lib, alignment
    n, hs, ws_ = src
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (n, hs, ws_, 3)).astype(dtype)
    m = _similarities(n, (hs, ws_), dst, 9)
    regions = [("src", img.nbytes, 16, True), ("m", m.nbytes, 16, True), ("dst", n * dst[0] * dst[1] * 3 * 4, 16)]
    with _lib.tuning(**knob):
        out = _image_case("warp_device " + wid, regions, {"src": img, "m": m},
                          lambda v: alignment.warp_device(v["src"], v["m"], dst[0], dst[1],
                                                          out=v["dst"].view(torch.float32).view(n, dst[0], dst[1], 3)))
    assert bool(torch.isfinite(out).all()) and float(out.max()) > 0


FMTS = [("nchw-bf16-rgb", dict(layout="nchw", dtype="bfloat16", channels="rgb", scale=1 / 127.5, bias=-1.0), torch.bfloat16),
        ("nhwc-u8", dict(layout="nhwc", dtype="uint8"), torch.uint8)]


@pytest.mark.parametrize("fid,kw,tdt", FMTS, ids=[f[0] for f in FMTS])
def test_warp_device_fmt(flm, fid, kw, tdt):
    """The formatted warp: its destination needs the alignment of its element and no more (include/flm.h), so it is placed
    at exactly that."""
    from flm_amd import alignment
    fmt = alignment.AlignedFormat(**kw)
    n, hs, ws_, hd, wd = 3, 40, 52, 32, 64
    img = np.random.default_rng(6).integers(0, 256, (n, hs, ws_, 3), dtype=np.uint8)
    m = _similarities(n, (hs, ws_), (hd, wd), 10)
    es = fmt.itemsize
    regions = [("src", img.nbytes, 16, True), ("m", m.nbytes, 16, True), ("dst", fmt.nbytes(n, hd, wd), es)]
    _image_case("warp_device fmt " + fid, regions, {"src": img, "m": m},
                lambda v: alignment.warp_device(v["src"], v["m"], hd, wd, fmt=fmt,
                                                out=v["dst"].view(tdt).view(fmt.shape(n, hd, wd))))


@pytest.mark.parametrize("pixel", ["bgr", "nv12"])
def test_warp_frames_device(flm, pixel):
    """Faces warped straight from a ring of frames; the last face reads the last frame, whose last row and column it
    samples.  NV12: a ring with an odd pitch."""
    from flm_amd import alignment
    nf, fh, fw, k, hd, wd = 2, 36, 50, 3, 32, 64
    rng = np.random.default_rng(8)
    if pixel == "bgr":
        frames, src = rng.integers(0, 256, (nf, fh, fw, 3), dtype=np.uint8), None
    else:
        frames, src = rng.integers(0, 256, (nf, fh + fh // 2, fw + 3), dtype=np.uint8), alignment.FrameFormat.nv12(fh, fw)
    m = _similarities(k, (fh, fw), (hd, wd), 12)
    idx = np.array([0, 1, nf - 1], np.int32)
    for samples in (1, 2):
        regions = [("frames", frames.nbytes, 16, True), ("m", m.nbytes, 16, True), ("idx", idx.nbytes, 16, True),
                   ("dst", k * hd * wd * 3 * 4, 16)]
        out = _image_case("warp_frames_device %s samples=%d" % (pixel, samples), regions, {"frames": frames, "m": m, "idx": idx},
                          lambda v: alignment.warp_frames_device(v["frames"], v["m"], hd, wd, frame_index_dev=v["idx"],
                                                                 samples=samples, src=src,
                                                                 out=v["dst"].view(torch.float32).view(k, hd, wd, 3)))
        assert bool(torch.isfinite(out).all()) and float(out[-1].max()) > 0


def test_crop_faces_device(flm):
    """Boxes that poke out of every side of the frame, one that covers its last row and column exactly, one that misses it."""
    from flm_amd import prediction
    fh, fw, oh, ow = 45, 61, 32, 32
    frame = np.random.default_rng(13).integers(0, 256, (fh, fw, 3), dtype=np.uint8)
    boxes = np.array([[-7, 5, 20, 32], [40, -9, 70, 21], [30, 30, 70, 70], [-5, -5, fw + 5, fh + 5], [fw - 9, fh - 9, fw, fh],
                      [fw + 3, 2, fw + 20, 19], [10, fh - 4, 40, fh + 26]], np.int32)
    k = boxes.shape[0]
    regions = [("frame", frame.nbytes, 16, True), ("boxes", boxes.nbytes, 16, True), ("out", k * oh * ow * 3, 16)]
    out = _image_case("crop_faces_device", regions, {"frame": frame, "boxes": boxes},
                      lambda v: prediction.crop_faces_device(v["frame"], None, oh, ow, boxes_dev=v["boxes"],
                                                             out=v["out"].view(k, oh, ow, 3)))
    assert int(out[5].max()) == 0 and int(out[4].max()) > 0


def test_frames_to_bgr_device(flm):
    from flm_amd import alignment, prediction
    nf, fh, fw = 2, 36, 50
    frames = np.random.default_rng(14).integers(0, 256, (nf, fh + fh // 2, fw + 3), dtype=np.uint8)
    ff = alignment.FrameFormat.nv12(fh, fw, matrix="bt709")
    regions = [("frames", frames.nbytes, 16, True), ("out", nf * fh * fw * 3, 16)]
    _image_case("frames_to_bgr_device", regions, {"frames": frames},
                lambda v: prediction.frames_to_bgr_device(v["frames"], ff, out=v["out"].view(nf, fh, fw, 3)))
