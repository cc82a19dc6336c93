"""FaceTracker.annotate on the GPU: a tracker on one stream and on three streams of two slots, a BGR and an NV12 ring, with
and without `smooth`, on a synthetic ring with synthetic weights.  After the seed (whose boxes are the one upload) the
sequence step, annotate, step, annotate runs inside torch.cuda.set_sync_debug_mode("error").  Every annotate is compared,
over the WHOLE ring and bit for bit, with tests/annotate_ref.py on the ring, the landmarks and `frame_slots` downloaded
before it.  A second tracker that never annotates, on a ring of its own, is bit-equal on every step output up to the
first annotate -- and, since the second step reads slots the first annotate did not touch, after it too."""
import numpy as np
import pytest
import torch

import annotate_ref as aref

pytestmark = pytest.mark.gpu
RH, RW, NF, CAP = 270, 480, 6, 6
PITCH, UV_ROW, ROWS = 512, 272, 408
BOXES = [(40, 30, 140, 130), (200, 20, 290, 110), (300, 120, 400, 220), (60, 150, 150, 240), (330, 10, 400, 80)]   # slot 5: no face


@pytest.fixture(scope="module")
def mods():
    import flm_amd  # noqa: F401
    from flm_amd import _lib, alignment, prediction
    _lib.load()
    return _lib, alignment, prediction


@pytest.fixture(scope="module")
def model():
    from flm_amd.networks import LANDMARKS_MODELS
    from flm_amd.weights import synth_fcn8_weights
    m = LANDMARKS_MODELS["fcn_8"](68, input_height=64, input_width=64, dtype="bf16")
    m.load_weights(synth_fcn8_weights(68, seed=2))
    return m


@pytest.fixture(scope="module")
def rings():
    rng = np.random.default_rng(77)
    return {"bgr": rng.integers(0, 256, (NF, RH, RW, 3), dtype=np.uint8),
            "nv12": rng.integers(0, 256, (NF, ROWS, PITCH), dtype=np.uint8)}


class sync_error:
    """Inside: a transfer or a synchronisation raises (checked on entry)."""

    def __init__(self, probe):
        self.probe = probe

    def __enter__(self):
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            with pytest.raises(RuntimeError):                          # (the mode is live in this build: a download raises)
                self.probe.item()
        except BaseException:
            torch.cuda.set_sync_debug_mode("default")
            raise

    def __exit__(self, *exc):
        torch.cuda.set_sync_debug_mode("default")


def view_bits(x):
    return x.view(torch.int64) if x.dtype == torch.float64 else x.view(torch.int32) if x.dtype == torch.float32 else x


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(view_bits(a), view_bits(b))


@pytest.mark.parametrize("smooth", [None, True])
@pytest.mark.parametrize("streams", [1, 3])
@pytest.mark.parametrize("source", ["bgr", "nv12"])
def test_annotate_after_each_step(mods, model, rings, source, streams, smooth):
    L, A, P = mods
    ff = None if source == "bgr" else A.FrameFormat.nv12(RH, RW, matrix="bt709", uv_row=UV_ROW)
    note = A.FrameAnnotation(marks=True, box=2, redact=8, box_color=(255, 64, 0))
    ring, ring_plain = torch.from_numpy(rings[source]).cuda(), torch.from_numpy(rings[source]).cuda()
    make = lambda: P.FaceTracker(model, (RH, RW), CAP, frame_format=ff, smooth=smooth, streams=streams)
    tr, plain = make(), make()
    for t in (tr, plain):
        t.seed(list(range(len(BOXES))), BOXES)
    # synthetic weights lose tracks at will: between the steps both trackers get the seeded crops back, from device copies
    seeded = [x.clone() for x in (tr.boxes, tr.m_crop, tr.status)]

    def pin(t):
        t.boxes.copy_(seeded[0])
        t.m_crop.copy_(seeded[1])
        t.status.copy_(seeded[2])
    # one stream: a host slot number; three streams: a slot per stream, on the device before the mode is entered
    frames = [2, 4] if streams == 1 else [torch.tensor(v, dtype=torch.int32, device="cuda") for v in ([1, 3, 5], [0, 2, 4])]
    probe = torch.zeros(1, device="cuda")
    steps, regions, before = [], [], []
    with sync_error(probe):
        for fi in frames:
            res = tr.step(ring, fi)
            # (clones are device copies: what the restatement is given is what annotate was given)
            before.append((ring.clone(), res[2].clone(), tr.frame_slots.clone()))
            steps.append([x.clone() for x in res])
            regions.append(tr.annotate(ring, res[2], annotation=note))
            pin(tr)
    for i, fi in enumerate(frames):
        ref = plain.step(ring_plain, fi)
        for a, b in zip(steps[i], ref):
            assert same(a, b), (i, source, streams, smooth)            # annotating changed nothing a later step returned
        pin(plain)                                                     # (after the comparison: status is the tracker's own tensor)
    assert torch.equal(ring_plain, torch.from_numpy(rings[source]).cuda())             # a step writes no frame
    ring_now = [before[1][0], ring]                                    # the ring after annotate 0 is the ring before step 1
    for i in range(2):
        r0, lm, slots = [x.cpu().numpy() for x in before[i]]
        kw = dict(marks=1, box=2, redact=8, box_bgr=(255, 64, 0))
        if source == "bgr":
            want, reg = aref.annotate_bgr(r0, lm, slots, **kw)
        else:
            want, reg = aref.annotate_nv12(r0, RH, RW, UV_ROW, "bt709", lm, slots, **kw)
        assert np.array_equal(regions[i].cpu().numpy(), reg), i
        got = ring_now[i].cpu().numpy()
        diff = np.argwhere(got != want)
        assert not len(diff), (i, len(diff), diff[:5].tolist())
        assert not np.array_equal(want, r0)                            # something was drawn
        if streams == 1:
            assert (slots == frames[i]).all()
            touched = [f for f in range(NF) if not np.array_equal(want[f], r0[f])]
            assert touched == [frames[i]]                              # only the slot the step cut from
    assert (regions[0][5] == 0).all().item()                           # the slot without a face: (-1,-1) everywhere, no region
    # rows need their own frame indices, and the ring must be the tracker's
    with pytest.raises(ValueError, match="frame_index=None goes with the landmarks of `step`"):
        tr.annotate(ring, steps[0][2][:3])
    reg = tr.annotate(ring, steps[0][2][:3], frame_index=tr.frame_slots[:3].contiguous(), annotation=A.FrameAnnotation(marks=False))
    assert tuple(reg.shape) == (3, 4) and torch.equal(reg, regions[0][:3])
    other = torch.zeros((2, 64, 64, 3), dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError):
        tr.annotate(other, steps[0][2])
