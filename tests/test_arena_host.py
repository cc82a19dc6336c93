"""tests/arena.py on CPU tensors: the carving, the alignment (what was asked for and no better), the guard check."""
import numpy as np
import pytest
import torch

from arena import FILLS, GUARD, Arena, same_bits

SPECS = [("x", 3 * 5 * 7 * 3, 16, True), ("ws", 1000, 256), ("out", 4 * 33, 4), ("blob", 777, 256, True), ("b", 5, 1)]


@pytest.mark.parametrize("fill", FILLS)
def test_carving_and_alignment(fill):
    a = Arena(fill, SPECS, guard=4096)
    base = a.buf.data_ptr()
    assert base % 512 == 0
    prev_end = 0
    for name, nbytes, align, *_ in SPECS:
        r = a.region(name)
        assert r.numel() == nbytes and r.dtype == torch.uint8
        assert r.data_ptr() - base == a.offset(name)
        assert r.data_ptr() % (2 * align) == align, (name, "aligned to %d and no better" % align)
        assert a.offset(name) - prev_end >= 4096, (name, "guard in front")
        prev_end = a.offset(name) + nbytes
    assert a.nbytes - prev_end == 4096
    assert bool((a.buf == fill).all())            # regions too, until something is put there
    gaps = a.gaps()
    assert len(gaps) == len(SPECS) + 1 and gaps[0][0] == 0 and gaps[-1][1] == a.nbytes
    assert sum(hi - lo for lo, hi in gaps) + sum(s[1] for s in SPECS) == a.nbytes
    a.check_guards()


def test_default_guard_is_4_mib():
    a = Arena(0x4B, [("ws", 300, 256)])
    assert GUARD == 4 << 20 and a.offset("ws") >= GUARD and a.nbytes - a.offset("ws") - 300 == GUARD
    assert a.offset("ws") % 512 == 256


def test_views_and_put():
    a = Arena(0xFF, SPECS, guard=1024)
    x = np.arange(3 * 5 * 7 * 3, dtype=np.uint8).reshape(3, 5, 7, 3)
    v = a.put("x", x)
    assert v.shape == (3, 5, 7, 3) and v.data_ptr() == a.region("x").data_ptr()
    assert np.array_equal(v.numpy(), x)
    out = a.view("out", torch.float32, (33,))
    assert torch.isnan(out).all()                  # 0xFF is NaN as float32 ...
    assert torch.isnan(a.view("ws", torch.bfloat16, (500,)).float()).all()   # ... and as bfloat16
    k = Arena(0x4B, [("f", 8, 4)], guard=64)
    assert abs(float(k.view("f", torch.float32, (2,))[0]) - 1.33e7) < 1e5
    assert abs(float(k.view("f", torch.bfloat16, (4,))[0]) - 1.33e7) < 1e5
    with pytest.raises(ValueError):
        a.view("out", torch.float32, (34,))
    a.check_guards()


def test_guard_check_sees_one_byte_on_either_side_and_a_changed_input():
    for where in ("before", "after"):
        a = Arena(0x00, SPECS, guard=512)
        off = a.offset("ws") - 1 if where == "before" else a.offset("ws") + 1000
        a.buf[off] = 1
        with pytest.raises(AssertionError, match="guard bytes changed"):
            a.check_guards()
    a = Arena(0x4B, SPECS, guard=512)
    a.region("ws").fill_(7)                         # writing inside a writable region is what a call does
    a.region("out")[-1] = 9
    a.put("blob", torch.arange(777, dtype=torch.int64).to(torch.uint8))
    a.check_guards()
    a.region("blob")[776] ^= 1
    with pytest.raises(AssertionError, match="read-only region 'blob'"):
        a.check_guards()
    a.region("blob")[776] ^= 1
    a.check_guards()
    a.buf[a.nbytes - 1] = 0                         # the last byte of the last guard
    with pytest.raises(AssertionError, match="guard bytes changed"):
        a.check_guards()


def test_bad_regions_are_refused():
    for bad in ([("a", 0, 16)], [("a", 8, 3)], [("a", 8, 512)], [("a", 8, 16), ("a", 8, 16)]):
        with pytest.raises(ValueError):
            Arena(0, bad, guard=64)
    with pytest.raises(ValueError):
        Arena(256, [("a", 8, 16)])


def test_same_bits():
    nan = torch.tensor([float("nan"), 1.0])
    assert same_bits(nan, nan.clone()) and not torch.equal(nan, nan.clone())
    assert not same_bits(torch.tensor([0.0]), torch.tensor([-0.0]))
    assert not same_bits(torch.zeros(2), torch.zeros(3)) and not same_bits(torch.zeros(2), torch.zeros(2, dtype=torch.float64))


# ---- the caller-owned buffers the arena serves: set_weights(packed=) and the decode wrappers' workspace= ---------------
# (the argument checks run before anything touches a GPU, so CPU tensors reach every refusal but the last, "not CUDA")

def test_set_weights_packed_argument_checks():
    import flm_amd  # noqa: F401
    from flm_amd.networks import LANDMARKS_MODELS
    model = LANDMARKS_MODELS["fcn_8"](17, input_height=64, input_width=96, dtype="bf16")
    need = model.packed_bytes()
    assert need > 0 and need == LANDMARKS_MODELS["fcn_8"](17, input_height=32, input_width=32, dtype="bf16").packed_bytes()
    a = Arena(0x4B, [("blob", need, 256), ("odd", need, 128)], guard=64)
    for bad, msg in ((np.zeros(need, np.uint8), "uint8 tensor"),
                     (torch.zeros(need, dtype=torch.int8), "uint8 tensor"),
                     (torch.zeros((2, need), dtype=torch.uint8), "one-dimensional"),
                     (torch.zeros(2 * need, dtype=torch.uint8)[::2], "contiguous"),
                     (a.region("blob")[:need - 1], "the blob needs %d" % need),
                     (a.region("odd"), "256-byte aligned"),
                     (a.region("blob"), "CUDA")):
        with pytest.raises(ValueError, match=msg):
            model.set_weights({}, packed=bad)     # refused before the parameters are looked at
    assert model._packed is None
    a.check_guards()


def test_decode_workspace_argument_checks():
    import flm_amd  # noqa: F401
    from flm_amd.utils import metrics
    cpu = torch.device("cpu")
    a = Arena(0xFF, [("ws", 1024, 256), ("odd", 1024, 64)], guard=64)
    assert metrics._check_workspace(a.region("ws"), 1024, cpu).data_ptr() == a.region("ws").data_ptr()
    assert metrics._check_workspace(a.region("ws"), 0, cpu) is not None
    for bad, msg in ((None, "uint8 tensor"), (torch.zeros(1024), "uint8 tensor"),
                     (torch.zeros((4, 256), dtype=torch.uint8), "one-dimensional"),
                     (a.region("ws")[:1000], "the call needs 1024"),
                     (a.region("odd"), "256-byte aligned")):
        with pytest.raises(ValueError, match=msg):
            metrics._check_workspace(bad, 1024, cpu)
    with pytest.raises(ValueError, match="maps' device"):
        metrics._check_workspace(a.region("ws"), 1024, torch.device("cuda", 0))
    assert metrics._decode_workspace(None, 10, cpu).numel() == 256     # the default: allocated, as before
