"""FaceTracker(mesh=...) on the GPU: a tracker of 2 streams x 2 slots with synthetic weights on a synthetic ring.  After
`step`, `step_active` and `step_live`, `tracker.mesh_faces` equals alignment.warp_mesh_frames_device on the landmarks
and the M that call returned, bit for bit, and everything the call returns -- and the state it leaves -- equals, bit for
bit, that of a tracker made without `mesh`."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
RH, RW, NF, CAP, STREAMS = 128, 160, 4, 4, 2
SPS = CAP // STREAMS
OUT = (24, 20)
BOXES = [(20, 16, 84, 80), (70, 40, 150, 120), (40, 30, 110, 100)]     # slot 3: no face


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


def view_bits(x):
    return x.view(torch.int64) if x.dtype == torch.float64 else x.view({4: torch.int32, 2: torch.int16, 1: torch.uint8}[x.element_size()]) \
        if x.is_floating_point() else x


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(view_bits(a), view_bits(b))


@pytest.mark.parametrize("fmt_name", ["float32", "matcher"])
def test_mesh_faces_of_every_kind_of_step(mods, model, fmt_name):
    _, A, P = mods
    fmt = None if fmt_name == "float32" else A.AlignedFormat.matcher()
    rng = np.random.default_rng(21)
    ring = torch.from_numpy(rng.integers(0, 256, (NF, RH, RW, 3), dtype=np.uint8)).cuda()
    make = lambda **kw: P.FaceTracker(model, (RH, RW), CAP, out_size=OUT, streams=STREAMS, samples=2, aligned_format=fmt, **kw)
    tr, plain = make(mesh=True), make()
    assert plain.mesh is None and plain.mesh_faces is None and isinstance(tr.mesh, A.FaceMesh)
    assert (tr.mesh.n_landmarks, tr.mesh.n_anchors) == (68, 8)
    for t in (tr, plain):
        t.seed(list(range(len(BOXES))), BOXES)
    buf = tr._mesh_buf
    assert tuple(buf.shape) == (fmt or A.AlignedFormat()).shape(CAP, *OUT)
    seeded = [x.clone() for x in (tr.boxes, tr.m_crop, tr.status)]

    def pin(t):          # synthetic weights lose tracks at will: every call starts from the seeded crops
        t.boxes.copy_(seeded[0])
        t.m_crop.copy_(seeded[1])
        t.status.copy_(seeded[2])

    def expect(res, slots, fi):
        """warp_mesh_frames_device on what the call returned: row r reads the frame of its slot's stream, with the box its
        slot had before the call; an inert row (slot -1) has no face."""
        sl = slots.cpu().numpy()
        idx = np.array([fi[s // SPS] if s >= 0 else 0 for s in sl], np.int32)
        b0 = seeded[0].cpu().numpy()
        boxes = np.array([b0[s] if s >= 0 else (0, 0, 0, 0) for s in sl], np.int32)
        return A.warp_mesh_frames_device(ring, res[2], res[1].contiguous(), tr.mesh, OUT[0], OUT[1],
                                         frame_index_dev=torch.from_numpy(idx).cuda(), boxes_dev=torch.from_numpy(boxes).cuda(),
                                         samples=2, fmt=fmt)

    calls = [
        ("step", lambda t: t.step(ring, [1, 3]), torch.arange(CAP, dtype=torch.int32), [1, 3]),
        ("step_active", lambda t: t.step_active(ring, [None, 2], [1]), None, [0, 2]),
        ("step_live", lambda t: t.step_live(ring, [0, 1], 3), None, [0, 1]),
    ]
    for name, call, slots, fi in calls:
        got, ref = call(tr), call(plain)
        assert len(got) == len(ref) and all(same(a, b) for a, b in zip(got, ref)), name       # the other outputs: unchanged
        for attr in ("boxes", "m_crop", "status", "frame_slots"):
            assert same(getattr(tr, attr), getattr(plain, attr)), (name, attr)
        slots = got[4] if slots is None else slots
        n = int(got[0].shape[0])
        faces = tr.mesh_faces
        assert faces.data_ptr() == buf.data_ptr() and tr._mesh_buf is buf                     # the tracker's own buffer
        assert faces.dtype == got[0].dtype and tuple(faces.shape) == tuple(got[0].shape)      # row for row with `aligned`
        want = expect(got, slots, fi)
        assert same(faces, want), name
        sl = slots.cpu().long()
        b0 = seeded[0].cpu()[sl.clamp(min=0)]
        live = (sl >= 0) & (b0[:, 2] > b0[:, 0]) & (b0[:, 3] > b0[:, 1])
        assert live.any() and not same(faces[live.to(faces.device)], got[0][live.to(faces.device)]), name   # not the similarity's faces
        if (~live).any():                                                                      # a row without a face: a zero face
            dead = (~live).to(faces.device)
            assert same(faces[dead], got[0][dead]), name
        assert n == {"step": CAP, "step_active": SPS, "step_live": 3}[name]
        pin(tr)
        pin(plain)


def test_tracker_rejects_a_mesh_it_cannot_use(mods, model):
    _, A, P = mods
    with pytest.raises(ValueError):
        P.FaceTracker(model, (RH, RW), CAP, mesh="default")
    with pytest.raises(ValueError):      # five landmark points for a model of 68
        P.FaceTracker(model, (RH, RW), CAP, out_size=OUT, mesh=A.FaceMesh.default(5, *OUT))
    with pytest.raises(ValueError):      # mesh=True is the default template's mesh
        P.FaceTracker(model, (RH, RW), CAP, out_size=OUT, template=A.canonical_template(68, *OUT) + 1.0, mesh=True)
    assert P.FaceTracker(model, (RH, RW), CAP, out_size=OUT, mesh=False).mesh is None
