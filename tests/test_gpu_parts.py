"""Face parts on the GPU (flm_part_affines, flm_warp_parts_frames and their Python wrappers) against tests/parts_ref.py and
against the similarity warp the patches are defined by.

Shapes: a ring of 2 slots of 96x128, BGR24 and NV12 (pitch 160, BT.709); K = 5 and K = 65 faces, among them faces with
rejected points, zero and NaN weights, one participating point, coincident points, a NaN coordinate, the last face in a
ring slot outside the ring and the one before it with an empty box; the default parts and a custom set whose indices
are non-contiguous and out of order; patches of 16x24, 17x23 (odd: ragged waves) and 40x72 (several trips of the
workgroup's pixel loop); samples 1, 2, 4; float32 NHWC BGR, uint8 NCHW RGB and float16 NCHW normalised."""
import numpy as np
import pytest
import torch

import parts_ref as ref

pytestmark = pytest.mark.gpu
FH, FW, NF, PITCH, ROWS = 96, 128, 2, 160, 150
SIZES = [(16, 24), (17, 23), (40, 72)]


@pytest.fixture(scope="module")
def mods():
    import flm_amd  # noqa: F401
    from flm_amd import _lib, alignment, prediction
    _lib.load()
    return _lib, alignment, prediction


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def bits(t):
    """A tensor's raw bits as an integer tensor (device side)."""
    return t.view({4: torch.int32, 2: torch.int16, 1: torch.uint8}[t.element_size()])


@pytest.fixture(scope="module")
def rings(mods):
    _, A, _ = mods
    rng = np.random.default_rng(11)
    return {"bgr": (dev(rng.integers(0, 256, (NF, FH, FW, 3), dtype=np.uint8)), None),
            "nv12": (dev(rng.integers(0, 256, (NF, ROWS, PITCH), dtype=np.uint8)),
                     A.FrameFormat.nv12(FH, FW, matrix="bt709", uv_row=FH + 2))}


def formats(A):
    return {"f32_nhwc": None,
            "u8_nchw_rgb": A.AlignedFormat("nchw", "uint8", "rgb"),
            "f16_nchw_norm": A.AlignedFormat("nchw", "float16", "bgr", (1 / 127.5,) * 3, (-1.0,) * 3)}


_CASES = {}


def case(A, k, kind, size):
    """(FaceParts, [(indices, template)], lm, w, frame_idx, boxes, the reference's aff and ok), computed once."""
    key = (k, kind, size)
    if key not in _CASES:
        if kind == "default":
            parts = A.FaceParts.default(68, size)
        else:
            cp = ref.custom_parts(*size)
            parts = A.FaceParts([i for i, _ in cp], [t for _, t in cp], size)
        plist = [parts.part(r) for r in range(len(parts))]
        lm, w = ref.face_landmarks(k, FH, FW, 3, A.canonical_template(68, FH, FW))
        idx = (np.arange(k) % NF).astype(np.int32)
        idx[k - 1] = 5                                             # a slot outside the ring
        boxes = np.tile(np.array([0, 0, FW, FH], np.int32), (k, 1))
        boxes[k - 2] = [30, 30, 30, 50]                            # an empty box
        _CASES[key] = (parts, plist, lm, w, idx, boxes) + ref.part_affines(lm, w, plist)
    return _CASES[key]


def guarded(shape, dtype, fill):
    """(buffer with one guard row before and after, the view between them)."""
    buf = torch.full((shape[0] + 2,) + tuple(shape[1:]), fill, dtype=dtype, device="cuda")
    return buf, buf[1:-1]


def guards_intact(buf, fill):
    g = torch.stack([buf[0], buf[-1]])
    return bool((g == fill).all())


@pytest.mark.parametrize("kind", ["default", "custom"])
@pytest.mark.parametrize("k", [5, 65])
def test_part_affines_bit_exact(mods, k, kind):
    _, A, _ = mods
    for size in SIZES[:2]:
        parts, plist, lm, w, _, _, aff, ok = case(A, k, kind, size)
        r = len(parts)
        for weights in (None, w):
            want_aff, want_ok = (aff, ok) if weights is not None else ref.part_affines(lm, None, plist)
            abuf, aview = guarded((k, r, 2, 3), torch.float32, -3.0)
            obuf, oview = guarded((k, r), torch.int32, -7)
            got, got_ok = A.part_affines_device(dev(lm), parts, weights=None if weights is None else dev(weights), out=aview,
                                                ok_out=oview)
            assert got.data_ptr() == aview.data_ptr() and tuple(got.shape) == (k, r, 2, 3)
            assert np.array_equal(got.cpu().numpy().view(np.uint32), want_aff.view(np.uint32)), (size, weights is None)
            assert np.array_equal(got_ok.cpu().numpy(), want_ok)
            assert guards_intact(abuf, -3.0) and guards_intact(obuf, -7)
            assert set(want_ok.ravel().tolist()) == {0, 1}
            ident = np.array([[1, 0, 0], [0, 1, 0]], np.float32)
            assert (want_aff[want_ok == 0] == ident).all()
        # landmarks and weights read in place from a record tensor (stride 6)
        rec = torch.full((k, 68, 6), 9.0, dtype=torch.float64, device="cuda")
        rec[..., :2] = dev(lm)
        rec[..., 2] = dev(w)
        got, got_ok = A.part_affines_device(rec[..., :2], parts, weights=rec[..., 2])
        assert np.array_equal(got.cpu().numpy().view(np.uint32), aff.view(np.uint32)) and np.array_equal(got_ok.cpu().numpy(), ok)


@pytest.mark.parametrize("kind", ["default", "custom"])
@pytest.mark.parametrize("source", ["bgr", "nv12"])
@pytest.mark.parametrize("k", [5, 65])
def test_patches_equal_the_affine_warp(mods, rings, k, source, kind):
    """THE CONTRACT: patch (f, r) is what flm_warp_affine_frames_src stores with m = aff[f][r]; a part that is not ok, a
    slot outside the ring and an empty box give that call's zero face; aff_out and part_ok_out hold the reference's bits;
    nothing around the outputs is written."""
    _, A, _ = mods
    ring, ff = rings[source]
    for size in SIZES:
        parts, plist, lm, w, idx, boxes, aff, ok = case(A, k, kind, size)
        r = len(parts)
        lm_d, w_d, idx_d, boxes_d, aff_d = dev(lm), dev(w), dev(idx), dev(boxes), dev(aff)
        ok_d = dev(ok)
        for fmt_name, fmt in formats(A).items():
            ofmt = fmt or A.AlignedFormat()
            face = tuple(ofmt.shape(1, *size)[1:])
            fill = 77 if ofmt.torch_dtype == torch.uint8 else -5.0
            for samples in (1, 2, 4):
                where = dict(frame_index_dev=idx_d, boxes_dev=boxes_d, samples=samples, fmt=fmt, src=ff)
                pbuf, pview = guarded((k, r) + face, ofmt.torch_dtype, fill)
                abuf, aview = guarded((k, r, 2, 3), torch.float32, -3.0)
                obuf, oview = guarded((k, r), torch.int32, -7)
                got = A.warp_parts_frames_device(ring, lm_d, parts, weights=w_d, out=pview, affines_out=aview, ok_out=oview,
                                                 **where)
                tag = (size, fmt_name, samples)
                assert got.data_ptr() == pview.data_ptr() and tuple(got.shape) == (k, r) + face, tag
                assert torch.equal(bits(aview), bits(aff_d)) and torch.equal(oview, ok_d), tag
                assert guards_intact(pbuf, fill) and guards_intact(abuf, -3.0) and guards_intact(obuf, -7), tag
                for j in range(r):
                    want = A.warp_frames_device(ring, aff_d[:, j].contiguous(), size[0], size[1], **where)
                    zero = want[k - 1]                                  # the face of the slot outside the ring
                    not_ok = (ok_d[:, j] == 0).view((k,) + (1,) * len(face))
                    want = torch.where(not_ok, zero[None], want)
                    assert torch.equal(bits(got[:, j]), bits(want)), tag + (j,)
                    assert torch.equal(bits(got[k - 2, j]), bits(zero)), tag + (j,)   # the empty box
                # without frame_idx and boxes every face reads slot 0: only the fits that are not ok are zero faces
                if samples == 1 and fmt_name == "f32_nhwc":
                    got0 = A.warp_parts_frames_device(ring, lm_d, parts, weights=w_d, src=ff)
                    for j in range(r):
                        want = A.warp_frames_device(ring, aff_d[:, j].contiguous(), size[0], size[1], src=ff)
                        want = torch.where((ok_d[:, j] == 0).view(k, 1, 1, 1), torch.zeros_like(want), want)
                        assert torch.equal(bits(got0[:, j]), bits(want)), tag + (j, "slot 0")
                    assert bool((got0[ok_d != 0] != 0).any())


def test_prediction_face_parts(mods, rings):
    _, A, P = mods
    ring, _ = rings["bgr"]
    parts, plist, lm, w, idx, _, aff, ok = case(A, 5, "default", (32, 48))
    out, m, good = P.face_parts(ring, dev(lm), weights=dev(w), frame_index=[int(v) for v in idx[:4]] + [1])
    assert tuple(out.shape) == (5, 3, 32, 48, 3) and out.dtype == torch.float32
    assert np.array_equal(m.cpu().numpy().view(np.uint32), aff.view(np.uint32)) and np.array_equal(good.cpu().numpy(), ok)
    want = A.warp_frames_device(ring, m[:, 0].contiguous(), 32, 48, frame_index_dev=dev(np.array(list(idx[:4]) + [1], np.int32)))
    assert torch.equal(bits(out[0, 0]), bits(want[0]))
    with pytest.raises(ValueError):
        P.face_parts(ring, dev(lm), parts="eyes")
    with pytest.raises(ValueError):
        P.face_parts(ring, dev(lm[:, :5]))
