"""CPU checks of the encoder chains of oracle/fcn_bf16_ref.py (ENCODER_CHAINS: VGG, MobileNet, ResNet50, one Step per layer).

  * the free-running encoders, now run_chain over those steps, against what the commit BEFORE the restatement computed
    (tests/golden/encoder_chain_golden.npz, recorded there by tests/golden/make_encoder_chain_golden.py): every level
    f1..f5, at 1 x 32 x 32 and 2 x 64 x 96, in all five arithmetics (float64 = fcn_ref's; bf16 rounding points with float64 and
    with float32 sums; the exact-fp32 folded form with float64 and with float32 sums).  Bit for bit (digests of the whole
    exact and stored tensors) wherever torch's CPU convolutions sum in the order they did on the recording machine
    (enc_chain_cases.platform_probe); on any machine the 256 recorded samples of each level to 1e-10 of the level's
    maximum where sums are float64 and nothing is rounded, 1e-4 with float32 sums, 5e-2 where a last-bit difference can
    flip a bf16 rounding that later layers amplify -- a wrong source, stride, shortcut or activation moves a level by
    its own size.  The bit-for-bit branch is the one expected on the build machines (x86-64, the torch build this
    repository pins, where the golden was recorded and re-checked); a machine whose probe differs -- another CPU
    generation or thread count may change torch's blocking -- takes the tolerance branch only and prints that it did;
  * one step at a time: encoder_layer_ref on the chain's own stored outputs gives the free-running bits, every layer,
    every arithmetic;
  * the chains, written from the reference's network files, against the library's layer table (flm_fcn_encoder_layer, which
    the GPU gate uses to locate buffers): names, sources, shortcuts, strides, kernel sizes, activations, widths, grids.
"""
import numpy as np
import pytest

import flm_amd  # noqa: F401
import enc_chain_cases as cases
from flm_amd.networks import LANDMARKS_MODELS
from oracle import fcn_bf16_ref as B
from oracle import fcn_ref

ENCS = [e for e, _, _ in cases.ENCODERS]


@pytest.fixture(scope="module")
def gold(golden_dir):
    import os
    g = np.load(os.path.join(golden_dir, "encoder_chain_golden.npz"))
    dig = dict(line.split("=") for line in g["digests"].tolist())
    return g, dig, str(g["probe"]) == cases.platform_probe()


_RUNS = {}


def _run(enc, shape, arith):
    """{name: (exact, stored)} NHWC of the free-running chain; one (encoder, shape) cached at a time."""
    key = (enc, shape)
    if key not in _RUNS:
        _RUNS.clear()
        _RUNS[key] = {}
    if arith not in _RUNS[key]:
        x = np.stack([fcn_ref.get_image_array_ref(c) for c in cases.crops(*shape)])
        out = B.run_chain(B.ENCODER_CHAINS[enc], B.Arith(**cases.ARITHS[arith]), B._nchw(x), cases.encoder_params(enc))
        _RUNS[key][arith] = {k: (B._nhwc(e), B._nhwc(s)) for k, (e, s) in out.items()}
    return _RUNS[key][arith]


TOL = {"f64": 1e-10, "f32": 1e-10, "f32_acc32": 1e-4, "bf16": 5e-2, "bf16_acc32": 5e-2}


@pytest.mark.parametrize("shape", cases.CPU_SHAPES, ids=lambda s: "%dx%dx%d" % s)
@pytest.mark.parametrize("enc", ENCS)
def test_free_running_encoders_compute_what_they_did_before_the_chains(gold, enc, shape):
    g, dig, same_platform = gold
    p = cases.encoder_params(enc)
    x = np.stack([fcn_ref.get_image_array_ref(c) for c in cases.crops(*shape)])
    for arith, kw in cases.ARITHS.items():
        levels = B._ENCODERS[enc](B.Arith(**kw), B._nchw(x), p)
        assert len(levels) == 5
        for k, (e, s) in enumerate(levels):
            key = "%s/%dx%dx%d/%s/f%d" % ((enc,) + shape + (arith, k + 1))
            e, s = B._nhwc(e), B._nhwc(s)
            d = np.abs(cases.sample(s) - g[key]).max() / np.abs(g[key]).max()
            assert d <= TOL[arith], (key, d)
            if same_platform:
                assert "%s,%s" % (cases.digest(e), cases.digest(s)) == dig[key], key
    print("%s %s: five levels x five arithmetics %s" % (enc, shape, "bit for bit" if same_platform else
                                                         "within tolerance (another platform's summation order)"))
    # the levels are the chain's steps
    run = _run(enc, shape, "bf16")
    lv = B._ENCODERS[enc](B.Arith(), B._nchw(x), p)
    for name, (_, s) in zip(B.ENCODER_LEVELS[enc], lv):
        assert np.array_equal(run[name][1], B._nhwc(s)), name


@pytest.mark.parametrize("shape", cases.CPU_SHAPES, ids=lambda s: "%dx%dx%d" % s)
@pytest.mark.parametrize("enc", ENCS)
def test_one_step_at_a_time_gives_the_free_running_bits(enc, shape):
    p = cases.encoder_params(enc)
    for arith, kw in cases.ARITHS.items():
        run = _run(enc, shape, arith)
        for st in B.ENCODER_CHAINS[enc]:
            xin = tuple(run[i][1] for i in st.inputs)
            e, s = B.encoder_layer_ref(enc, st.name, xin if len(xin) > 1 else xin[0], p, **kw)
            assert np.array_equal(e, run[st.name][0]) and np.array_equal(s, run[st.name][1]), (arith, st.name)
            if arith in ("bf16", "bf16_acc32") and st.op == "conv":
                assert np.array_equal(s, B.round_bf16(e)), (arith, st.name)      # every encoder map is stored as bf16
            else:
                assert np.array_equal(s, e), (arith, st.name)
    # the three arithmetics are three: rounding moves a layer, float32 storage of scale / shift moves it less
    last = B.ENCODER_CHAINS[enc][-1].name
    a, b, c = (_run(enc, shape, k)[last][0] for k in ("f64", "f32", "bf16"))
    m = np.abs(a).max()
    assert 0 < np.abs(b - a).max() < 1e-5 * m < np.abs(c - a).max() < 0.2 * m


@pytest.mark.parametrize("name,enc", [("fcn_8_vgg", "vgg"), ("fcn_8_mobilenet", "mobilenet"), ("fcn_8_resnet50", "resnet50"),
                                      ("fcn_32_vgg", "vgg"), ("fcn_32_mobilenet", "mobilenet"), ("fcn_32_resnet50", "resnet50")])
def test_chains_agree_with_the_library_layer_table(name, enc):
    cases.check_chain_against_table(LANDMARKS_MODELS[name](68, input_height=64, input_width=96), enc, _run(enc, (2, 64, 96), "f32"))


class _Float32Device:
    """Stands in for a model in bf16_gate.check_layers: `intermediate("act<i>")` is the chain run free with float32 sums --
    a legitimate implementation of every layer in another summation order, which the gate must pass."""

    def __init__(self, enc, dtype, shape):
        import torch
        self.dtype = dtype
        arith = "bf16_acc32" if dtype == "bf16" else "f32_acc32"
        self.outs = [torch.from_numpy(_run(enc, shape, arith)[st.name][1]) for st in B.ENCODER_CHAINS[enc]]

    def intermediate(self, name, n, out):
        return self.outs[int(name[3:])]


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("enc", ENCS)
def test_gate_passes_float32_accumulation_and_fails_a_wrong_layer(enc, dtype):
    from bf16_gate import check_layers
    shape = (1, 32, 32)
    p = cases.encoder_params(enc)
    dev = _Float32Device(enc, dtype, shape)
    rep = check_layers(dev, p, cases.crops(*shape), 1, "probs", label="float32 sums, %s %s" % (enc, dtype), dtype=dtype,
                       encoder=enc, head=False)
    chain = B.ENCODER_CHAINS[enc]
    assert list(rep) == [st.name for st in chain]
    for st in chain:
        r = rep[st.name]
        assert r["ok"] and r["nonzero"] >= 0.25, (st.name, r)
        if st.op == "conv":
            assert 0 < r["e32"] < 1e-6 and r["slack"] < B.SLACK_CAP, (st.name, r)   # K <= 4,608: nowhere near the cap
    # one element of one layer off by one bf16 step (bf16) / by 1e-4 of the maximum (fp32): that layer fails; so may the
    # layers that read it (their outputs here were computed from the right input); every other layer still passes
    k = len(chain) // 2
    victim = chain[k] if chain[k].op == "conv" else chain[k + 1]
    t = dev.outs[[st.name for st in chain].index(victim.name)]
    i = int(np.argmax(t.numpy()))
    t.view(-1)[i] += float(B.ulp_bf16(t.view(-1)[i].item())) if dtype == "bf16" else 1e-4 * float(t.max())
    with pytest.raises(AssertionError) as err:
        check_layers(dev, p, cases.crops(*shape), 1, "probs", label="one element off", dtype=dtype, encoder=enc, head=False)
    failed = {st.name for st in chain if "'%s':" % st.name in str(err.value)}
    assert victim.name in failed and failed <= {victim.name} | {st.name for st in chain if victim.name in st.inputs}, failed
