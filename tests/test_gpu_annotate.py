"""flm_frames_annotate on the GPU, through ctypes, on rings pre-filled with seeded junk: the WHOLE ring tensor -- the pitch
padding, the rows between the planes and the slots no face names included -- and `regions` are compared bit for bit with
tests/annotate_ref.py.

Rings of 48x64 frames: BGR with 3 slots; NV12 with pitch 80, the U,V rows from row 50 and a junk row after them, BT.601
and BT.709.  K in {1, 5, 130} (130: more than one wave of faces for the mosaic's scan), C in {1, 5, 68}, lm_stride 2 and
FLM_LANDMARK_REC.  The faces (`POOL`) are the cases that can go wrong: two and three faces of one frame whose regions share
cells (the ownership rule), identical regions (the tie), the same pixels named in another slot, a face with every point
rejected, regions partly and wholly outside the frame, landmarks at (0,0), (fw-1,fh-1) and just past the frame, odd
corners on NV12, frame indices -1 and nframes, NaN and inf among the points, a face whose region is the whole frame.
Options: redact 2, 8 and 64 (a cell taller than the frame), box 1, 3 and 16 (thicker than half a region), each layer alone,
all three together, all off.  Then the two Python wrappers on the same cases, and their refusals that need device
tensors."""
import ctypes as C

import numpy as np
import pytest
import torch

import annotate_ref as aref

pytestmark = pytest.mark.gpu
FH, FW, NF = 48, 64, 3
PITCH, UV_ROW, ROWS = 80, 50, 75
NAN, INF = float("nan"), float("inf")
RINGS = ("bgr", "bt601", "bt709")
JUNK = 0x5A5A5A5A


@pytest.fixture(scope="module")
def mods():
    import flm_amd  # noqa: F401
    from flm_amd import _lib, alignment, prediction
    _lib.load()
    return _lib, alignment, prediction


@pytest.fixture(scope="module")
def rings():
    """Seeded junk: every byte of every slot, padding included."""
    rng = np.random.default_rng(41)
    return {"bgr": rng.integers(0, 256, (NF, FH, FW, 3), dtype=np.uint8),
            "bt601": rng.integers(0, 256, (NF, ROWS, PITCH), dtype=np.uint8),
            "bt709": rng.integers(0, 256, (NF, ROWS, PITCH), dtype=np.uint8)}


def face(rng, c, cx, cy, spread):
    return np.array([cx, cy], np.float64) + rng.uniform(-spread, spread, (c, 2))


def faces(k, c, seed=0):
    """(lm float64 [k,c,2], frame index int32 [k]): the first k faces of the pool, then seeded faces anywhere."""
    rng = np.random.default_rng(1000 * k + 10 * c + seed)
    a = face(rng, c, 20, 20, 8)
    a[c // 2] = (-1.0, -1.0) if c > 2 else a[c // 2]                     # a rejected point inside a face
    pool = [(a, 0), (face(rng, c, 26, 24, 8), 0), (a.copy(), 0), (a.copy(), 1), (np.full((c, 2), -1.0), 0),
            (face(rng, c, 23, 17, 6), 0), (face(rng, c, 60, 44, 8), 2), (face(rng, c, 90, 70, 5), 2)]
    p = face(rng, c, 4, 4, 3).clip(0)
    p[0] = (0.0, 0.0)
    pool.append((p, 1))
    p = face(rng, c, 60, 45, 2)
    p[-1] = (FW - 1.0, FH - 1.0)
    pool.append((p, 1))
    pool.append((np.tile([[float(FW), 20.0]], (c, 1)), 2))             # just past the frame: P is empty
    p = np.tile([[62.0, 46.0]], (c, 1))
    p[-1] = (FW + 0.5, FH + 0.2)                                       # (c == 1: this point alone -- its disc would reach in)
    pool.append((p, 0))
    pool.append((np.tile([[33.0, 21.0]], (c, 1)), 2))                  # odd corners: R = (33,21,34,22)
    pool.append((face(rng, c, 30, 30, 5), -1))
    pool.append((face(rng, c, 30, 30, 5), NF))
    p = face(rng, c, 40, 10, 5)
    p[0], p[-1] = (NAN, 5.0), (INF, INF)
    pool.append((p, 2))
    p = face(rng, c, 30, 20, 10)
    p[0], p[-1] = (0.0, 0.0), (FW - 1.0, FH - 1.0)                     # the whole frame of slot 1
    pool.append((p, 1))
    while len(pool) < k:
        pool.append((face(rng, c, rng.uniform(-5, 70), rng.uniform(-5, 53), rng.uniform(1, 10)), int(rng.integers(-1, NF + 1))))
    pool = pool[:k]
    return np.stack([p for p, _ in pool]), np.array([f for _, f in pool], np.int32)


def reference(rings, kind, lm, fi, **opts):
    if kind == "bgr":
        return aref.annotate_bgr(rings[kind], lm, fi, **opts)
    return aref.annotate_nv12(rings[kind], FH, FW, UV_ROW, kind, lm, fi, **opts)


def frame_format(A, kind):
    return A.FrameFormat.bgr() if kind == "bgr" else A.FrameFormat.nv12(FH, FW, matrix=kind, uv_row=UV_ROW)


def run(mods, rings, kind, lm, fi, stride=2, null_src=False, **opts):
    """The C call on a fresh copy of the ring -> (ring bytes, regions) on the host."""
    L, A, _ = mods
    ring = torch.from_numpy(rings[kind]).cuda()
    k, c = lm.shape[:2]
    if stride == 2:
        lm_d = torch.from_numpy(lm).cuda()
    else:                                                              # landmark records: x, y and four columns of NaN
        rec = np.full((k, c, stride), NAN)
        rec[..., :2] = lm
        lm_d = torch.from_numpy(rec).cuda()
    fi_d = None if fi is None else torch.from_numpy(fi).cuda()
    reg = torch.full((k, 4), JUNK, dtype=torch.int32, device="cuda")
    co = L.AnnotateOpts.make(opts.get("marks", 1), opts.get("box", 0), opts.get("redact", 0), opts.get("margin"),
                             opts.get("mark_bgr"), opts.get("box_bgr"))
    cs = frame_format(A, kind).struct(ring)
    stride_bytes = ring[0].numel()
    L.check(L.load().flm_frames_annotate(L.stream_ptr(), L.ptr(ring), stride_bytes, NF, FH, FW,
                                         None if null_src else C.byref(cs), None if fi_d is None else L.ptr(fi_d),
                                         L.ptr(lm_d), stride, k, c, C.byref(co), L.ptr(reg)), "flm_frames_annotate")
    torch.cuda.synchronize()
    return ring.cpu().numpy(), reg.cpu().numpy()


def check(got, want, what):
    assert np.array_equal(got[1], want[1]), ("regions", what)
    diff = np.argwhere(got[0] != want[0])
    assert not len(diff), (what, len(diff), diff[:5].tolist())


ALL = dict(marks=1, box=3, redact=8, mark_bgr=(10, 200, 250), box_bgr=(255, 128, 0))


@pytest.mark.parametrize("c", [1, 5, 68])
@pytest.mark.parametrize("k", [1, 5, 130])
@pytest.mark.parametrize("kind", RINGS)
def test_batches_and_strides(mods, rings, kind, k, c):
    lm, fi = faces(k, c)
    for opts in (ALL, dict()):                                         # all three layers; the defaults: marks alone
        want = reference(rings, kind, lm, fi, **opts)
        assert not np.array_equal(want[0], rings[kind]) or k == 1      # (something is drawn)
        for stride in (2, 6):
            check(run(mods, rings, kind, lm, fi, stride=stride, **opts), want, (kind, k, c, stride, sorted(opts)))


OPTIONS = {"redact2": dict(marks=0, redact=2), "redact8": dict(marks=0, redact=8), "redact64": dict(marks=0, redact=64),
           "box1": dict(marks=0, box=1), "box3": dict(marks=0, box=3, box_bgr=(1, 2, 3)), "box16": dict(marks=0, box=16),
           "marks": dict(mark_bgr=(255, 255, 255)), "all": dict(ALL, redact=2, box=1, margin=(0.0, 0.0, 0.0, 0.0)),
           "wide": dict(ALL, redact=64, box=16, margin=(4.0, 0.0, 4.0, 0.5))}


@pytest.mark.parametrize("name", sorted(OPTIONS))
@pytest.mark.parametrize("kind", RINGS)
def test_each_layer_alone_and_together(mods, rings, kind, name):
    lm, fi = faces(130, 5, seed=1)
    want = reference(rings, kind, lm, fi, **OPTIONS[name])
    assert not np.array_equal(want[0], rings[kind])
    check(run(mods, rings, kind, lm, fi, **OPTIONS[name]), want, (kind, name))


@pytest.mark.parametrize("kind", RINGS)
def test_all_layers_off_leaves_the_ring_untouched(mods, rings, kind):
    lm, fi = faces(130, 5, seed=2)
    got = run(mods, rings, kind, lm, fi, marks=0)
    assert np.array_equal(got[0], rings[kind])
    assert np.array_equal(got[1], aref.regions(lm)) and (got[1][4] == 0).all()       # regions are still written, over the junk
    assert (got[1][13] != 0).any()                                     # ... also for a face whose frame index is -1


@pytest.mark.parametrize("kind", RINGS)
def test_a_null_frame_index_is_slot_zero(mods, rings, kind):
    lm, _ = faces(20, 5, seed=3)
    want = reference(rings, kind, lm, None, **ALL)
    assert np.array_equal(want[0][1:], rings[kind][1:])
    check(run(mods, rings, kind, lm, None, **ALL), want, kind)
    if kind == "bgr":                                                  # a NULL format is the BGR24 ring
        check(run(mods, rings, kind, lm, None, null_src=True, **ALL), want, "null src")


def test_three_faces_sharing_cells_in_every_order(mods, rings):
    """The ownership rule: whichever face comes first, every shared cell is averaged once, from its original bytes."""
    rng = np.random.default_rng(9)
    trio = [face(rng, 5, 24, 20, 9), face(rng, 5, 30, 24, 9), face(rng, 5, 27, 28, 9)]
    first = None
    for order in ((0, 1, 2), (2, 1, 0), (1, 0, 2), (0, 0, 0)):         # (the last: three identical regions)
        lm, fi = np.stack([trio[i] for i in order]), np.zeros(3, np.int32)
        for kind in RINGS:
            for s in (2, 8):
                want = reference(rings, kind, lm, fi, marks=0, redact=s)
                check(run(mods, rings, kind, lm, fi, marks=0, redact=s), want, (order, kind, s))
                if order != (0, 0, 0):
                    first = first or {}
                    assert np.array_equal(first.setdefault((kind, s), want[0]), want[0])     # the order plays no part


# ---- the two Python wrappers ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", RINGS)
def test_the_wrappers_on_the_same_cases(mods, rings, kind):
    L, A, P = mods
    lm, fi = faces(130, 68, seed=4)
    ff = frame_format(A, kind)
    opts = dict(marks=True, box=3, redact=8, mark_color=(10, 200, 250), box_color=(255, 128, 0))
    want = reference(rings, kind, lm, fi, **ALL)
    rec = np.full((130, 68, 6), NAN)
    rec[..., :2] = lm
    for how in ("device", "records", "plain-host-index", "plain-device-index", "out"):
        ring = torch.from_numpy(rings[kind]).cuda()
        lm_d, fi_d = torch.from_numpy(lm).cuda(), torch.from_numpy(fi).cuda()
        if how == "device":
            reg = A.annotate_frames_device(ring, lm_d, fi_d, A.FrameAnnotation(**opts), ff if kind != "bgr" else None)
        elif how == "records":                                         # a view of a record tensor is read in place
            reg = A.annotate_frames_device(ring, torch.from_numpy(rec).cuda()[..., :2], fi_d, A.FrameAnnotation(**opts), ff)
        elif how == "plain-host-index":
            reg = P.annotate_frames(ring, lm_d, fi.tolist(), None if kind == "bgr" else ff, **opts)
        elif how == "plain-device-index":
            reg = P.annotate_frames(ring, lm_d, fi_d, ff, **opts)
        else:
            mine = torch.full((130, 4), JUNK, dtype=torch.int32, device="cuda")
            reg = A.annotate_frames_device(ring, lm_d, fi_d, A.FrameAnnotation(**opts), ff, regions_out=mine)
            assert reg is mine
        assert reg.dtype == torch.int32 and tuple(reg.shape) == (130, 4)
        check((ring.cpu().numpy(), reg.cpu().numpy()), want, (kind, how))
    # no index: slot 0; the defaults: marks alone
    ring = torch.from_numpy(rings[kind]).cuda()
    reg = P.annotate_frames(ring, torch.from_numpy(lm).cuda(), frame_format=ff)
    check((ring.cpu().numpy(), reg.cpu().numpy()), reference(rings, kind, lm, None), (kind, "defaults"))
    # no face: nothing is launched
    reg = A.annotate_frames_device(ring, torch.zeros((0, 68, 2), dtype=torch.float64, device="cuda"), src=ff)
    assert tuple(reg.shape) == (0, 4)


def test_the_wrappers_refuse_what_they_must(mods, rings):
    L, A, P = mods
    k, c = 4, 5
    ring = torch.from_numpy(rings["bgr"]).cuda()
    nv = torch.from_numpy(rings["bt601"]).cuda()
    lm = torch.zeros((k, c, 2), dtype=torch.float64, device="cuda")
    fi = torch.zeros(k, dtype=torch.int32, device="cuda")
    ff = A.FrameFormat.nv12(FH, FW, uv_row=UV_ROW)
    before = ring.clone()
    flat = ring.view(-1)
    # overlap with the ring
    with pytest.raises(ValueError, match="lm and the ring"):
        A.annotate_frames_device(ring, flat[:k * c * 16].view(torch.float64).view(k, c, 2))
    with pytest.raises(ValueError, match="lm and the ring"):           # a record view whose gaps reach into the ring
        A.annotate_frames_device(ring, flat[-k * c * 48:].view(torch.float64).view(k, c, 6)[..., :2])
    with pytest.raises(ValueError, match="regions_out and the ring"):
        A.annotate_frames_device(ring, lm, regions_out=flat[16:16 + k * 16].view(torch.int32).view(k, 4))
    with pytest.raises(ValueError, match="frame_index_dev and the ring"):
        A.annotate_frames_device(ring, lm, frame_index_dev=flat[:k * 4].view(torch.int32))
    both = torch.zeros(k * c * 2 + k * 2, dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError, match="lm and regions_out"):
        A.annotate_frames_device(ring, both[:k * c * 2].view(k, c, 2), regions_out=both[k * c * 2 - 1:k * c * 2 - 1 + k * 2].view(torch.int32).view(k, 4))
    # wrong type
    for bad in (lm.float(), lm.cpu(), lm.tolist()):
        with pytest.raises(ValueError, match="CUDA float64"):
            A.annotate_frames_device(ring, bad)
    with pytest.raises(ValueError, match="frame_index_dev"):
        A.annotate_frames_device(ring, lm, frame_index_dev=fi.long())
    with pytest.raises(ValueError, match="regions_out"):
        A.annotate_frames_device(ring, lm, regions_out=torch.zeros((k, 4), dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError, match="frames must be"):
        A.annotate_frames_device(ring.float(), lm)
    with pytest.raises(ValueError, match="NV12 ring"):
        A.annotate_frames_device(ring, lm, src=ff)
    with pytest.raises(ValueError, match="FrameAnnotation"):
        A.annotate_frames_device(ring, lm, opts=L.AnnotateOpts.make())
    # wrong shape
    for bad in (lm[0], lm[..., :1], torch.zeros((k, c, 3), dtype=torch.float64, device="cuda")):
        with pytest.raises(ValueError, match="CUDA float64"):
            A.annotate_frames_device(ring, bad)
    with pytest.raises(ValueError, match="frame_index_dev"):
        A.annotate_frames_device(ring, lm, frame_index_dev=torch.zeros(k + 1, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match="regions_out"):
        A.annotate_frames_device(ring, lm, regions_out=torch.zeros((k, 3), dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match="frame_index"):
        P.annotate_frames(ring, lm, frame_index=[0, 1])
    with pytest.raises(ValueError, match="4096 with redact"):
        A.annotate_frames_device(ring, torch.zeros((4097, 1, 2), dtype=torch.float64, device="cuda"), opts=A.FrameAnnotation(redact=2))
    with pytest.raises(ValueError, match="pitch"):
        A.annotate_frames_device(nv, lm, src=A.FrameFormat.nv12(FH, 96, uv_row=UV_ROW))
    with pytest.raises(ValueError, match="U,V rows"):
        A.annotate_frames_device(nv, lm, src=A.FrameFormat.nv12(FH, FW, uv_row=60))
    # wrong layout
    with pytest.raises(ValueError, match="frames must be"):
        A.annotate_frames_device(ring[:, :, ::2], lm)
    with pytest.raises(ValueError, match="contiguous"):
        A.annotate_frames_device(nv[:, :, :PITCH - 8], lm, src=ff)
    with pytest.raises(ValueError, match="regions_out"):
        A.annotate_frames_device(ring, lm, regions_out=torch.zeros((k, 8), dtype=torch.int32, device="cuda")[:, :4])
    with pytest.raises(ValueError, match="frame_index_dev"):
        A.annotate_frames_device(ring, lm, frame_index_dev=torch.zeros(2 * k, dtype=torch.int32, device="cuda")[::2])
    assert torch.equal(ring, before)                                   # nothing was written on the way
