"""Cases shared by the oracle-chain tests, the encoder-layer gate and tests/golden/make_encoder_chain_golden.py: the three
registry encoders on the project's synthetic weights (the seeds tests/test_gpu_forward.py uses), uint8 BGR inputs from
default_rng(7), and the arithmetics of oracle/fcn_bf16_ref.py's Arith."""
import ctypes
import hashlib

import numpy as np
import torch
import torch.nn.functional as F

ENCODERS = (("vgg", "synth_vgg_weights", 4), ("mobilenet", "synth_mobilenet_weights", 5),
            ("resnet50", "synth_resnet50_weights", 6))
CPU_SHAPES = ((1, 32, 32), (2, 64, 96))
ARITHS = {"f64": dict(rounding=False), "bf16": dict(), "bf16_acc32": dict(accum=torch.float32),
          "f32": dict(fp32=True), "f32_acc32": dict(fp32=True, accum=torch.float32)}
INPUT_SEED = 7
SAMPLES = 256

_PARAMS = {}


def encoder_params(enc, keep=1):
    """The 68-class synthetic fcn_8 weights of `enc`; at most `keep` sets stay cached (ResNet50's are 1.7 GB)."""
    from flm_amd import weights as W
    if enc not in _PARAMS:
        while len(_PARAMS) >= keep:
            _PARAMS.pop(next(iter(_PARAMS)))
        synth, seed = next((s, sd) for e, s, sd in ENCODERS if e == enc)
        _PARAMS[enc] = getattr(W, synth)(68, seed=seed)
    return _PARAMS[enc]


def crops(n, h, w):
    return np.random.default_rng(INPUT_SEED).integers(0, 256, (n, h, w, 3), dtype=np.uint8)


def digest(a) -> str:
    a = np.ascontiguousarray(np.asarray(a, np.float64))
    return hashlib.sha256(a.tobytes()).hexdigest()[:32]


def sample(a) -> np.ndarray:
    a = np.asarray(a, np.float64).ravel()
    return a[np.random.default_rng(11).choice(a.size, min(a.size, SAMPLES), replace=False)]


def platform_probe() -> str:
    """Digest of a handful of torch CPU convolutions of the kinds the encoders use, float64 and float32.  Equal digests
    on two machines: their convolution kernels sum in the same order, and bit-level comparisons of oracle outputs
    between them mean something."""
    rng = np.random.default_rng(123)
    h = hashlib.sha256()
    for dt in (torch.float64, torch.float32):
        for cin, cout, k, s, g, hw in ((3, 32, 3, 2, 1, 32), (3, 64, 7, 2, 1, 32), (64, 64, 3, 1, 1, 15), (256, 64, 1, 1, 1, 7),
                                       (128, 128, 3, 2, 128, 16), (256, 512, 1, 2, 1, 7), (512, 512, 3, 1, 1, 2)):
            x = torch.from_numpy(rng.standard_normal((2, cin, hw, hw + 3))).to(dt)
            w = torch.from_numpy(rng.standard_normal((cout, cin // g, k, k))).to(dt)
            h.update(F.conv2d(x, w, None, stride=s, padding=k // 2, groups=g).to(torch.float64).numpy().tobytes())
    return h.hexdigest()[:32]


def check_chain_against_table(model, enc, run=None):
    """The oracle's chain of `enc` against the layer table the library reports for `model`: one table row per step, same
    name, source, shortcut, stride, kernel, activation, fused pool and widths; with `run` (the chain's NHWC outputs at
    the model's input size) also the same grids.  (Without `run` the grids are still held: the gate asserts that each
    device tensor, whose shape is the table's, has the shape of the oracle's output for the device's input.)"""
    from flm_amd import _lib
    from oracle import fcn_bf16_ref as B
    chain = B.ENCODER_CHAINS[enc]
    names = model.encoder_layer_names()
    assert names == tuple(st.name for st in chain)
    assert _lib.load().flm_fcn_encoder_layers(model._arch) == len(chain)
    p = encoder_params(enc)
    for i, st in enumerate(chain):
        t = model.encoder_layer(i)
        src = "x" if t.src < 0 else names[t.src]
        assert src == st.inputs[0], (st.name, src, st.inputs)
        assert (names[t.res],) == st.inputs[1:] if t.res >= 0 else len(st.inputs) == 1, (st.name, t.res, st.inputs)
        assert (t.stride, t.activation, t.pool) == (st.stride, st.relu, st.pool), (st.name, t.stride, t.activation, t.pool)
        assert (t.kind == _lib.ENC_MAXPOOL3) == (st.op == "maxpool3") and (t.kind == _lib.ENC_MB_DW) == st.depthwise, st.name
        if st.op == "conv":
            k = p[st.name + ("/depthwise_kernel" if st.depthwise else "/kernel")]
            assert k.shape[:3] == (t.kernel, t.kernel, t.cin) and (t.cout == t.cin if st.depthwise else k.shape[3] == t.cout), st.name
            assert st.kw.get("pad", 0) == t.kernel // 2, st.name
        else:
            assert (t.kernel, t.cin) == (3, t.cout), st.name
        if run is not None:
            xin = run[st.inputs[0]][1]
            assert xin.shape[1:] == (t.in_h, t.in_w, t.cin) and run[st.name][1].shape[1:] == (t.out_h, t.out_w, t.cout), st.name
    # f1..f5 of the head are the chain's levels
    for k, lv in enumerate(B.ENCODER_LEVELS[enc]):
        assert lv in names, lv
    last = model.encoder_layer(len(chain) - 1)
    assert (last.out_h, last.out_w) == (model.input_height // 32, model.input_width // 32)
    bad = _lib.EncLayerInfo()
    assert _lib.load().flm_fcn_encoder_layer(model._arch, len(chain), 64, 96, ctypes.byref(bad)) == -1
