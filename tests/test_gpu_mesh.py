"""The piecewise-affine warp over the landmark mesh on the GPU (flm_mesh_map, flm_mesh_affines, flm_warp_mesh_frames and
their Python wrappers) against tests/mesh_ref.py and against the similarity warp it is defined by.

Shapes: a ring of 2 slots of 64x96, BGR24 and NV12 (pitch 128); K = 3 faces, one in ring slot 5 and one with an empty
box (and the same three with every face in the ring, so that the face with two coincident landmarks and the face with a
NaN landmark are warped too); a tiny mesh (4 landmarks on the edge midpoints + 4 corner anchors, 6 triangles) and the
default 68 + 8; aligned faces of 24x20, and 112x112 once."""
import numpy as np
import pytest
import torch

import aligned_format_ref as fref
import mesh_ref

pytestmark = pytest.mark.gpu
f32 = np.float32
FH, FW, NF, PITCH, UV_ROW, ROWS = 64, 96, 2, 128, 64, 96
K = 3
IDX = np.array([1, 5, 0], np.int32)                                   # face 1: a slot outside the ring
BOXES = np.array([[8, 6, 80, 60], [8, 6, 80, 60], [30, 30, 30, 50]], np.int32)     # face 2: an empty box


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


def tiny_mesh(A, h, w):
    """4 landmarks on the edge midpoints of [0,w-1] x [0,h-1] + 4 corner anchors: the four corner triangles and the inner
    diamond cut in two -- 6 triangles, every point on the border."""
    x1, y1 = w - 1.0, h - 1.0
    pts = np.array([[x1 / 2, 0], [x1, y1 / 2], [x1 / 2, y1], [0, y1 / 2], [0, 0], [x1, 0], [x1, y1], [0, y1]], np.float64)
    tris = np.array([[0, 1, 2], [0, 2, 3], [4, 0, 3], [5, 1, 0], [6, 2, 1], [7, 3, 2]], np.int32)
    return A.FaceMesh(pts, tris, 4)


def get_mesh(A, name, h, w):
    return tiny_mesh(A, h, w) if name == "tiny" else A.FaceMesh.default(68, h, w)


def similarities(h, w):
    """Three similarities frame px -> aligned px: faces of about 40, 30 and 56 frame px, rotated."""
    out = np.zeros((K, 2, 3), f32)
    for i, (s, th, cx, cy) in enumerate([(0.5, 0.2, 46.0, 30.0), (0.7, -0.4, 30.0, 34.0), (0.36, 0.05, 50.0, 32.0)]):
        s = s * h / 24.0
        a, b = s * np.cos(th), s * np.sin(th)
        out[i] = [[a, -b, (w - 1) / 2 - (a * cx - b * cy)], [b, a, (h - 1) / 2 - (b * cx + a * cy)]]
    return out


def faces_for(mesh, h, w, seed=3):
    """(lm float64 [K,C,2], m float32 [K,2,3]): the landmarks are M^-1 of the template moved by up to 1.5 frame px; face 1
    has two coincident landmarks, face 2 a NaN coordinate."""
    rng = np.random.default_rng(seed)
    m = similarities(h, w)
    c = mesh.n_landmarks
    lm = mesh_ref.anchor_source_ref(m, mesh.points[:c]) + rng.uniform(-1.5, 1.5, (K, c, 2))
    lm[1, 1] = lm[1, 0]
    lm[2, c - 1, 1] = np.nan
    return lm, m


@pytest.fixture(scope="module")
def rings(mods):
    _, A, _ = mods
    rng = np.random.default_rng(11)
    return {"bgr": (dev(rng.integers(0, 256, (NF, FH, FW, 3), dtype=np.uint8)), None),
            "nv12": (dev(rng.integers(0, 256, (NF, ROWS, PITCH), dtype=np.uint8)),
                     A.FrameFormat.nv12(FH, FW, matrix="bt709", uv_row=UV_ROW))}


def formats(A):
    return {"f32_nhwc": None,
            "f16_nchw_rgb": A.AlignedFormat("nchw", "float16", "rgb", (1 / 127.5,) * 3, (-1.0,) * 3),
            "u8_nchw": A.AlignedFormat("nchw", "uint8"),
            "u8_nhwc": A.AlignedFormat("nhwc", "uint8")}


# ---- the map and the affines ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(24, 20), (112, 112)])
@pytest.mark.parametrize("name", ["tiny", "default"])
def test_mesh_map_bit_exact(mods, name, hw):
    _, A, _ = mods
    mesh = get_mesh(A, name, *hw)
    got = A.mesh_map_device(mesh, *hw).cpu().numpy()
    want = mesh_ref.mesh_map_ref(mesh.points, mesh.triangles, *hw)
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    assert (got != 255).all()
    assert mesh.map("cuda", *hw) is mesh.map("cuda", *hw) and np.array_equal(mesh.map("cuda", *hw).cpu().numpy(), want)
    if name == "tiny":            # with a hole, and in index order: the first triangle's pixels are the fourth's or nobody's
        holed = A.FaceMesh(mesh.points, mesh.triangles[1:], 4)
        got_h = A.mesh_map_device(holed, *hw).cpu().numpy()
        assert np.array_equal(got_h, mesh_ref.mesh_map_ref(holed.points, holed.triangles, *hw)) and (got_h == 255).any()


@pytest.mark.parametrize("name", ["tiny", "default"])
def test_mesh_affines_bit_exact(mods, rings, name):
    _, A, _ = mods
    h, w = 24, 20
    mesh = get_mesh(A, name, h, w)
    lm, m = faces_for(mesh, h, w)
    want = mesh_ref.mesh_affines_ref(lm, m, mesh.points, mesh.triangles, mesh.n_anchors)
    got = A.mesh_affines_device(dev(lm), dev(m), mesh)
    assert got.dtype == torch.float32 and tuple(got.shape) == (K, mesh.n_triangles, 2, 3)
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
    # the fallback is taken where it must be: the triangles of the coincident pair and of the NaN landmark hold M's bits
    tri = mesh.triangles
    c = mesh.n_landmarks
    pair = ((tri == 0).any(1) & (tri == 1).any(1))
    nan = (tri == c - 1).any(1)
    assert pair.any() and nan.any()
    g = got.cpu().numpy().view(np.uint32)
    assert (g[1, pair] == m[1].view(np.uint32)).all() and (g[2, nan] == m[2].view(np.uint32)).all()
    assert not (g[0] == m[0].view(np.uint32)).all(axis=(1, 2)).any()
    # aff_out of the warp: the same bits, zero faces included, from both sources; landmarks read in place from a record
    rec = torch.full((K, c, 6), 7.0, dtype=torch.float64, device="cuda")
    rec[..., :2] = dev(lm)
    for src_name, (ring, ff) in rings.items():
        for lm_dev in (dev(lm), rec[..., :2]):
            aff = torch.full((K, mesh.n_triangles, 2, 3), -3.0, dtype=torch.float32, device="cuda")
            A.warp_mesh_frames_device(ring, lm_dev, dev(m), mesh, h, w, frame_index_dev=dev(IDX), boxes_dev=dev(BOXES), src=ff,
                                      affines_out=aff)
            assert torch.equal(bits(aff), bits(got)), src_name
    assert torch.equal(bits(A.mesh_affines_device(rec[..., :2], dev(m), mesh)), bits(got))
    # min_det is the call's: with a huge one every triangle takes M
    allm = A.mesh_affines_device(dev(lm), dev(m), mesh, min_det=1e30).cpu().numpy()
    assert (allm.view(np.uint32) == m.view(np.uint32)[:, None]).all()


# ---- the contract ------------------------------------------------------------------------------------------------------
def contract(A, ring, ff, fmt, mesh, h, w, lm, m, idx, boxes, samples):
    """(mesh faces, the faces assembled from flm_warp_affine_frames_src with m = aff[:, t] on the pixels of triangle t)."""
    lm_d, m_d = dev(lm), dev(m)
    where = dict(frame_index_dev=None if idx is None else dev(idx), boxes_dev=None if boxes is None else dev(boxes),
                 samples=samples, fmt=fmt, src=ff)
    aff = torch.empty((K, mesh.n_triangles, 2, 3), dtype=torch.float32, device="cuda")
    got = A.warp_mesh_frames_device(ring, lm_d, m_d, mesh, h, w, affines_out=aff, **where)
    assert torch.equal(bits(aff), bits(A.mesh_affines_device(lm_d, m_d, mesh)))
    tmap = mesh.map("cuda", h, w)
    assert bool((tmap != 255).all())                                   # no pixel is left out of the comparison
    nchw = fmt is not None and fmt.layout == "nchw"
    want = torch.zeros_like(got)
    covered = torch.zeros((h, w), dtype=torch.bool, device="cuda")
    for t in torch.unique(tmap).tolist():
        face_t = A.warp_frames_device(ring, aff[:, t].contiguous(), h, w, **where)
        mask = tmap == t
        covered |= mask
        want = torch.where(mask[None, None] if nchw else mask[None, :, :, None], face_t, want)
    assert bool(covered.all())
    return got, want


@pytest.mark.parametrize("fmt_name", ["f32_nhwc", "f16_nchw_rgb", "u8_nchw", "u8_nhwc"])
@pytest.mark.parametrize("source", ["bgr", "nv12"])
@pytest.mark.parametrize("name", ["tiny", "default"])
def test_contract_pixels_equal_the_affine_warp(mods, rings, name, source, fmt_name):
    _, A, _ = mods
    h, w = 24, 20
    ring, ff = rings[source]
    fmt = formats(A)[fmt_name]
    mesh = get_mesh(A, name, h, w)
    lm, m = faces_for(mesh, h, w)
    for samples in (1, 2, 4):
        for idx, boxes in ((IDX, BOXES), (None, None)):
            got, want = contract(A, ring, ff, fmt, mesh, h, w, lm, m, idx, boxes, samples)
            assert torch.equal(bits(got), bits(want)), (samples, idx is None)
            if idx is not None:    # faces 1 and 2 are zero faces, equal to the affine call's; face 0 is not
                zero = A.warp_frames_device(ring, dev(m), h, w, frame_index_dev=dev(idx), boxes_dev=dev(boxes), samples=samples,
                                            fmt=fmt, src=ff)
                assert torch.equal(bits(got[1:]), bits(zero[1:])) and not torch.equal(bits(got[0]), bits(got[1]))
                assert torch.equal(bits(got[1]), bits(got[2]))


@pytest.mark.parametrize("source,samples,fmt_name", [("bgr", 1, "u8_nchw"), ("nv12", 4, "f32_nhwc")])
def test_contract_at_112(mods, rings, source, samples, fmt_name):
    """112 x 112: several workgroups per face (13 at samples = 1, 49 at samples = 4), whole and ragged waves."""
    _, A, _ = mods
    h, w = 112, 112
    ring, ff = rings[source]
    mesh = get_mesh(A, "default", h, w)
    lm, m = faces_for(mesh, h, w)
    got, want = contract(A, ring, ff, formats(A)[fmt_name], mesh, h, w, lm, m, None, None, samples)
    assert torch.equal(bits(got), bits(want))


@pytest.mark.parametrize("k,groups", [(330, 4), (700, 2), (1100, 1)])
def test_contract_many_faces_several_trips_per_workgroup(mods, rings, k, groups):
    """Past 1024 workgroups the launcher gives a workgroup several trips of the pixel loop: 330 faces of 112 x 112 at
    samples = 1 are 13 trips in 4 workgroups per face, 700 faces 13 trips in 2, 1100 faces in one.  The tiny mesh, so
    that the comparison is six affine warps."""
    _, A, _ = mods
    h, w = 112, 112
    assert -(-h * w // 1024) == 13 and -(-13 // min(13, k * 13 // 1024)) == groups
    ring, ff = rings["bgr"]
    mesh = tiny_mesh(A, h, w)
    rng = np.random.default_rng(k)
    m = np.tile(similarities(h, w), (k // 3 + 1, 1, 1))[:k].copy()
    m[:, :, 2] += rng.uniform(-4, 4, (k, 2)).astype(f32)
    lm = mesh_ref.anchor_source_ref(m, mesh.points[:4]) + rng.uniform(-1.5, 1.5, (k, 4, 2))
    fmt = formats(A)["u8_nchw"]
    idx = dev(rng.integers(0, NF, k).astype(np.int32))
    aff = torch.empty((k, 6, 2, 3), dtype=torch.float32, device="cuda")
    got = A.warp_mesh_frames_device(ring, dev(lm), dev(m), mesh, h, w, frame_index_dev=idx, fmt=fmt, affines_out=aff)
    tmap = mesh.map("cuda", h, w)
    want = torch.zeros_like(got)
    for t in range(6):
        face_t = A.warp_frames_device(ring, aff[:, t].contiguous(), h, w, frame_index_dev=idx, fmt=fmt)
        want = torch.where((tmap == t)[None, None], face_t, want)
    assert bool((tmap < 6).all()) and torch.equal(got, want)
    assert np.array_equal(aff.cpu().numpy().view(np.uint32),
                          mesh_ref.mesh_affines_ref(lm, m, mesh.points, mesh.triangles, 4).view(np.uint32))


# ---- a hole, a canary, and what the buffers held before ---------------------------------------------------------------
@pytest.mark.parametrize("fmt_name", ["f32_nhwc", "f16_nchw_rgb", "u8_nhwc"])
def test_hole_stores_zero_and_nothing_outside_the_faces(mods, rings, fmt_name):
    _, A, _ = mods
    h, w = 24, 20
    ring, ff = rings["bgr"]
    fmt = formats(A)[fmt_name]
    plain = fmt or A.AlignedFormat()
    full = tiny_mesh(A, h, w)
    holed = A.FaceMesh(full.points, full.triangles[1:], 4)
    lm, m = faces_for(full, h, w)
    tmap = mesh_ref.mesh_map_ref(holed.points, holed.triangles, h, w)
    hole = tmap == 255
    assert hole.any() and not hole.all()
    # K faces inside K + 2, the neighbours and the rest of the buffer a canary; the slice starts where its element does
    # and nowhere rounder (f16: 2 bytes past a 16-byte boundary is reached by the face size 24*20*3*2 = 2880 = 16*180,
    # so the first face is shifted by one element through a flat view)
    esize = plain.itemsize
    n_el = K * h * w * 3
    flat = torch.full(((K + 2) * h * w * 3 * esize,), 0xA5, dtype=torch.uint8, device="cuda")
    for shift in (0, 1):
        flat.fill_(0xA5)
        start = (h * w * 3 + shift) * esize
        out = flat[start:start + n_el * esize].view(plain.torch_dtype).view(plain.shape(K, h, w))
        res = A.warp_mesh_frames_device(ring, dev(lm), dev(m), holed, h, w, fmt=fmt, out=out, samples=2)
        assert res.data_ptr() == out.data_ptr()
        host = flat.cpu().numpy()
        assert (host[:start] == 0xA5).all() and (host[start + n_el * esize:] == 0xA5).all()
        got = out.cpu().numpy()
        zero_img = fref.convert(np.zeros((K, h, w, 3), f32), plain)     # the format's image of 0
        ref = A.warp_mesh_frames_device(ring, dev(lm), dev(m), full, h, w, fmt=fmt, samples=2).cpu().numpy()
        sel = np.broadcast_to(hole[None, None] if plain.layout == "nchw" else hole[None, :, :, None], got.shape)
        assert np.array_equal(fref.bits(got)[sel], fref.bits(zero_img)[sel])
        # outside the hole: the triangles that remain keep their pixels, except where the dropped triangle's edge
        # pixels pass to the next triangle that holds them -- those follow the map, which the contract test pins
        same_tri = ~hole & (mesh_ref.mesh_map_ref(full.points, full.triangles, h, w).astype(np.int64) == tmap.astype(np.int64) + 1)
        keep = np.broadcast_to(same_tri[None, None] if plain.layout == "nchw" else same_tri[None, :, :, None], got.shape)
        assert np.array_equal(fref.bits(got)[keep], fref.bits(ref)[keep]) and same_tri.sum() > hole.sum()


@pytest.mark.parametrize("source", ["bgr", "nv12"])
def test_buffer_independence(mods, rings, source):
    """The same call into buffers that held 0x00 and 0xFF gives equal bytes: faces, aff_out and the map."""
    _, A, _ = mods
    h, w = 24, 20
    ring, ff = rings[source]
    mesh = get_mesh(A, "default", h, w)
    lm, m = faces_for(mesh, h, w)
    fmt = formats(A)["f16_nchw_rgb"]
    results = []
    for fill in (0x00, 0xFF):
        out = torch.full((K * 3 * h * w * 2,), fill, dtype=torch.uint8, device="cuda").view(torch.float16).view(fmt.shape(K, h, w))
        aff = torch.full((K, mesh.n_triangles, 2, 3 * 4), fill, dtype=torch.uint8, device="cuda").view(torch.float32)
        tmap = torch.full((h, w), fill, dtype=torch.uint8, device="cuda")
        A.mesh_map_device(mesh, h, w, out=tmap)
        for samples in (1, 4):
            A.warp_mesh_frames_device(ring, dev(lm), dev(m), mesh, h, w, frame_index_dev=dev(IDX), boxes_dev=dev(BOXES),
                                      samples=samples, fmt=fmt, src=ff, out=out, affines_out=aff)
            results.append((fill, samples, bits(out).clone(), bits(aff).clone(), tmap.clone()))
    for a, b in zip(results[:2], results[2:]):
        assert a[1] == b[1] and all(torch.equal(x, y) for x, y in zip(a[2:], b[2:])), a[1]


# ---- a rigid face: every triangle's affine is M ---------------------------------------------------------------------------
def ramp_frame():
    """A frame whose three channels are integer-linear in (x, y) and stay inside uint8: bilinear interpolation of it is
    exactly B = x + 2y, G = 2x + y, R = 255 - (x + y) at every position inside the frame, so a position error of
    (dx, dy) moves no channel by more than 2*max(|dx|,|dy|) + min(...) <= 3*max(|dx|,|dy|)."""
    y, x = np.mgrid[0:FH, 0:FW]
    fr = np.stack([x + 2 * y, 2 * x + y, 255 - (x + y)], -1)
    assert fr.min() >= 0 and fr.max() <= 255
    return fr.astype(np.uint8)


def test_rigid_face_takes_the_similarity(mods):
    """The landmarks are exactly M^-1 of the template (float64, from the float32 M), so every triangle's affine is M up to
    rounding, and the mesh faces are the similarity-aligned faces up to the gradient of the frame times that.

    The tolerance, derived (u = 2^-24, e = 2^-53; S = 96 bounds every frame coordinate; s = the scale of M; L = the
    longest template edge and a2 = the smallest doubled template area of the mesh; amax, tmax = the largest linear and
    translation element of M):
      * a source vertex is M^-1 d through one determinant, four quotients, two differences, four products and two sums:
        at most 8 roundings on terms of magnitude <= 2S, so it is off by delta <= 16*e*S;
      * the solve divides numerators g*e - g*e, |g| <= L, |e| <= L/s, by det = a2_src >= a2/s^2.  Source errors of delta
        in both ends of an edge move a numerator by <= 4*L*delta, its own three roundings by <= 6*e*L*L/s:
          dA_lin <= (4*L*delta + 6*e*L*L/s) * s^2/a2             (the condition number of the smallest triangle)
        and the translation a02 = d0 - (a00*s0x + a01*s0y) by dA_tr <= 2*S*dA_lin + 6*e*amax*S;
      * rounding to float32 adds u*|a|:   tol_lin = dA_lin + u*(amax + dA_lin),   tol_tr = dA_tr + u*(tmax + dA_tr).
    For the pixels: two affine maps that differ by (tol_lin, tol_tr) send an aligned pixel to source positions
      dp_exact <= ||M^-1|| * (||dA|| * |p| + |da|) <= (2/s) * (2*tol_lin*P + tol_tr),     P = the largest |M^-1 q| over
    the aligned rectangle, and each of the two float32 evaluations (warp_inverse: det 2 roundings, 1/det 2, a product 1,
    so 6u on the linear part and 16u*|i|*tmax on the translation; warp_position: two fmas on values <= P) is off by
      dp_f32 <= u * ((2/s) * (6*(W+H) + 16*tmax) + 2*P).
    On the ramp frame a position error dp moves a channel by <= 3*dp, and the three fmas of each blend round values
    below 256 by <= 2^-17 each: |mesh - similarity| <= 3*(dp_exact + 2*dp_f32) + 6*2^-17."""
    _, A, _ = mods
    h, w = 24, 20
    mesh = A.FaceMesh.default(68, h, w)
    m = similarities(h, w)
    lm = mesh_ref.anchor_source_ref(m, mesh.points[:68])
    ring = dev(np.stack([ramp_frame(), ramp_frame()[::-1].copy()]))
    idx = dev(np.array([0, 1, 0], np.int32))
    aff = torch.empty((K, mesh.n_triangles, 2, 3), dtype=torch.float32, device="cuda")
    got = A.warp_mesh_frames_device(ring, dev(lm), dev(m), mesh, h, w, frame_index_dev=idx, affines_out=aff).cpu().numpy()
    sim = A.warp_frames_device(ring, dev(m), h, w, frame_index_dev=idx).cpu().numpy()
    aff = aff.cpu().numpy().astype(np.float64)
    u, e, S = 2.0 ** -24, 2.0 ** -53, 96.0
    pts, tri = mesh.points, mesh.triangles
    a, b, c = pts[tri[:, 0]], pts[tri[:, 1]], pts[tri[:, 2]]
    a2 = ((b[:, 0] - a[:, 0]) * (c[:, 1] - a[:, 1]) - (b[:, 1] - a[:, 1]) * (c[:, 0] - a[:, 0])).min()
    L = max(np.abs(b - a).max(), np.abs(c - a).max(), np.abs(c - b).max()) * np.sqrt(2.0)
    corners = np.array([[0, 0], [w - 1, 0], [w - 1, h - 1], [0, h - 1]], np.float64)
    worst = 0.0
    for f in range(K):
        mf = m[f].astype(np.float64)
        s = np.sqrt(mf[0, 0] ** 2 + mf[1, 0] ** 2)
        amax, tmax = np.abs(mf[:, :2]).max(), np.abs(mf[:, 2]).max()
        delta = 16 * e * S
        da_lin = (4 * L * delta + 6 * e * L * L / s) * s * s / a2
        da_tr = 2 * S * da_lin + 6 * e * amax * S
        tol_lin, tol_tr = da_lin + u * (amax + da_lin), da_tr + u * (tmax + da_tr)
        d = np.abs(aff[f] - mf[None])
        print("face %d: |aff - M| linear %.3g (tol %.3g), translation %.3g (tol %.3g)"
              % (f, d[:, :, :2].max(), tol_lin, d[:, :, 2].max(), tol_tr))
        assert d[:, :, :2].max() <= tol_lin and d[:, :, 2].max() <= tol_tr
        P = np.abs(mesh_ref.anchor_source_ref(m[f:f + 1], corners)).max()
        dp_exact = (2 / s) * (2 * tol_lin * P + tol_tr)
        dp_f32 = u * ((2 / s) * (6 * (w + h) + 16 * tmax) + 2 * P)
        bound = 3 * (dp_exact + 2 * dp_f32) + 6 * 2.0 ** -17
        diff = np.abs(got[f].astype(np.float64) - sim[f].astype(np.float64)).max()
        print("face %d: |mesh - similarity| %.3g (bound %.3g)" % (f, diff, bound))
        assert diff <= bound
        worst = max(worst, bound)
    assert worst < 0.02                                               # the bound is a number, and a small one
    assert got.std() > 10                                             # and the faces are not flat


# ---- the capability: every landmark's texture on its template pixel --------------------------------------------------------
def centroids(face, points, radius=3.0):
    """The intensity centroid of `face` [h,w] inside a disc around each of `points`."""
    h, w = face.shape
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    out = []
    for px, py in points:
        wgt = face.astype(np.float64) * (((x - px) ** 2 + (y - py) ** 2) <= radius ** 2)
        assert wgt.sum() > 0
        out.append([(wgt * x).sum() / wgt.sum(), (wgt * y).sum() / wgt.sum()])
    return np.array(out)


def test_shape_normalisation_puts_every_landmark_on_its_template_pixel(mods):
    """A frame with a dot at every landmark, the landmarks 2 to 4 frame px off the similarity image of the template.  In
    the mesh faces every dot's centroid is within 0.5 px of its template point; in the similarity-aligned faces none is
    -- on the device, and in the numpy restatement of both warps, so that neither half can pass vacuously.

    The shapes: a dot's centroid is the image of its centre only to first order in (dot size) x (offset / landmark
    spacing) -- the dot is stretched differently in each triangle around its vertex -- so the dots (sigma 2 px) and the
    offsets are small beside the triangles: five landmarks 65 frame px apart in a 176 x 176 frame, aligned at a scale of
    0.7 to 112 x 112, where the offsets are 1.4 to 2.8 aligned px."""
    _, A, _ = mods
    fh = fw = 176
    h = w = 112
    mesh = A.FaceMesh.default(5, h, w)
    tmpl = mesh.points[:5]
    th, s, cx, cy = 0.15, 0.7, 88.0, 87.0
    a, b = s * np.cos(th), s * np.sin(th)
    m = np.array([[[a, -b, (w - 1) / 2 - (a * cx - b * cy)], [b, a, (h - 1) / 2 - (b * cx + a * cy)]]], f32)
    rng = np.random.default_rng(5)
    ang, rad = rng.uniform(0, 2 * np.pi, 5), rng.uniform(2.0, 4.0, 5)
    lm = mesh_ref.anchor_source_ref(m, tmpl) + np.stack([rad * np.cos(ang), rad * np.sin(ang)], -1)[None]
    y, x = np.mgrid[0:fh, 0:fw].astype(np.float64)
    tex = np.zeros((fh, fw))
    for px, py in lm[0]:
        tex += 255.0 * np.exp(-((x - px) ** 2 + (y - py) ** 2) / (2 * 2.0 ** 2))
    frame = np.repeat(np.clip(np.rint(tex), 0, 255).astype(np.uint8)[..., None], 3, -1)
    ring = dev(frame[None])
    got = A.warp_mesh_frames_device(ring, dev(lm), dev(m), mesh, h, w).cpu().numpy()[0, ..., 0]
    sim = A.warp_frames_device(ring, dev(m), h, w).cpu().numpy()[0, ..., 0]
    ref_mesh = mesh_ref.warp_mesh_ref(frame, lm[0], m[0], mesh.points, mesh.triangles, 8, h, w)[..., 0]
    ref_sim = mesh_ref.warp_affine_frame_ref(frame, m[0], h, w)[..., 0]
    err = {name: np.linalg.norm(centroids(face, tmpl, radius=6.0) - tmpl, axis=1)
           for name, face in (("mesh", got), ("similarity", sim), ("mesh_ref", ref_mesh), ("similarity_ref", ref_sim))}
    print({k: np.round(v, 3).tolist() for k, v in err.items()})
    assert (err["mesh"] <= 0.5).all() and (err["mesh_ref"] <= 0.5).all()
    assert (err["similarity"] > 0.5).all() and (err["similarity_ref"] > 0.5).all()


def test_normalize_frames_is_the_mesh_warp_of_align_frames_results(mods, rings):
    _, A, P = mods
    h, w = 24, 20
    ring, ff = rings["nv12"]
    mesh = A.FaceMesh.default(68, h, w)
    lm, m = faces_for(mesh, h, w)
    fmt = A.AlignedFormat.matcher()
    got = P.normalize_frames(ring, dev(lm), dev(m), out_size=(h, w), frame_index=[1, 0, 1], samples=2, aligned_format=fmt,
                             frame_format=ff)
    want = A.warp_mesh_frames_device(ring, dev(lm), dev(m), mesh, h, w, frame_index_dev=dev(np.array([1, 0, 1], np.int32)),
                                     samples=2, fmt=fmt, src=ff)
    assert got.dtype == torch.float16 and tuple(got.shape) == (K, 3, h, w) and torch.equal(bits(got), bits(want))
