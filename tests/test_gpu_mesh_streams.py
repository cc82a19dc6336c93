"""The mesh warp under the library's reentrancy rule (calls on different streams run concurrently, cached
scratch is per stream, only FINISHED read-only data is shared): a FaceMesh caches its device tensors and its triangle map
for the callers of every stream, so the first call -- which uploads the points and launches flm_mesh_map on ITS stream --
must leave finished data behind.  Cold caches, two streams, in the style of tests/test_gpu_reentrancy.py's
test_align_frames_from_two_threads and test_shared_model_two_streams_one_thread:

  * one thread: stream A is given a queue of work, then the first warp_mesh_frames_device of a new mesh (its map kernel
    waits behind that queue); at once, without a synchronise of the test's own, stream B warps with the same mesh and
    finds the map in the cache;
  * two threads on two streams make their first prediction.normalize_frames call (the module's shared default mesh,
    evicted first) together.

Every result equals the serial call's, made afterwards with a mesh of its own."""
import threading

import numpy as np
import pytest
import torch

import mesh_ref

pytestmark = pytest.mark.gpu
f32 = np.float32
FH, FW, K = 64, 96, 3


@pytest.fixture(scope="module")
def mods():
    import flm_amd  # noqa: F401
    from flm_amd import _lib, alignment, prediction
    _lib.load()
    return alignment, prediction


def faces(mesh, h, w, seed):
    rng = np.random.default_rng(seed)
    m = np.zeros((K, 2, 3), f32)
    for i in range(K):
        s, th = rng.uniform(0.3, 0.7) * h / 24.0, rng.uniform(-0.4, 0.4)
        cx, cy = rng.uniform(30, 66), rng.uniform(24, 40)
        a, b = s * np.cos(th), s * np.sin(th)
        m[i] = [[a, -b, (w - 1) / 2 - (a * cx - b * cy)], [b, a, (h - 1) / 2 - (b * cx + a * cy)]]
    lm = mesh_ref.anchor_source_ref(m, mesh.points[:mesh.n_landmarks]) + rng.uniform(-1.5, 1.5, (K, mesh.n_landmarks, 2))
    return torch.from_numpy(lm).cuda(), torch.from_numpy(m).cuda()


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_cold_map_made_on_one_stream_read_on_another(mods):
    A, _ = mods
    h, w = 40, 36
    ring = torch.from_numpy(np.random.default_rng(1).integers(0, 256, (2, FH, FW, 3), dtype=np.uint8)).cuda()
    busy = torch.randn((2048, 2048), device="cuda")
    for rep in range(3):
        mesh = A.FaceMesh.default(68, h, w)                    # new: no tensors, no map
        lm_a, m_a = faces(mesh, h, w, 10 + rep)
        lm_b, m_b = faces(mesh, h, w, 20 + rep)
        sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(sa):
            for _ in range(40):                                 # some milliseconds of queue in front of the map kernel
                busy = busy @ busy * 1e-3
            got_a = A.warp_mesh_frames_device(ring, lm_a, m_a, mesh, h, w)
        with torch.cuda.stream(sb):
            got_b = A.warp_mesh_frames_device(ring, lm_b, m_b, mesh, h, w)
            map_b = mesh.map("cuda", h, w).clone()              # what stream B read, as stream B sees it
        torch.cuda.synchronize()
        fresh = A.FaceMesh.default(68, h, w)
        assert same(got_a, A.warp_mesh_frames_device(ring, lm_a, m_a, fresh, h, w)), rep
        assert same(got_b, A.warp_mesh_frames_device(ring, lm_b, m_b, fresh, h, w)), rep
        assert np.array_equal(map_b.cpu().numpy(), mesh_ref.mesh_map_ref(mesh.points, mesh.triangles, h, w)), rep
        assert mesh.map("cuda", h, w) is mesh.map("cuda:%d" % torch.cuda.current_device(), h, w)     # one entry per device


def test_first_normalize_frames_from_two_threads(mods):
    A, P = mods
    h, w = 44, 40
    rng = np.random.default_rng(2)
    rings = [torch.from_numpy(rng.integers(0, 256, (2, FH, FW, 3), dtype=np.uint8)).cuda() for _ in range(2)]
    proto = A.FaceMesh.default(68, h, w)
    args = [faces(proto, h, w, 30 + i) for i in range(2)]
    busy = [torch.randn((2048, 2048), device="cuda") for _ in range(2)]
    for rep in range(3):
        P._MESHES.pop((68, h, w), None)                          # the module's shared default mesh: cold
        torch.cuda.synchronize()
        start = threading.Barrier(2)
        got, errors = [None, None], []

        def caller(i):
            try:
                with torch.cuda.stream(torch.cuda.Stream()):
                    x = busy[i]
                    start.wait(timeout=30)
                    for _ in range(20 if i == 0 else 1):        # thread 0's first call queues behind more work
                        x = x @ x * 1e-3
                    got[i] = P.normalize_frames(rings[i], args[i][0], args[i][1], out_size=(h, w), frame_index=[0, 1, 0])
                    torch.cuda.current_stream().synchronize()
            except BaseException as e:                           # noqa: BLE001 -- reported by the main thread
                errors.append(repr(e))

        threads = [threading.Thread(target=caller, args=(i,)) for i in range(2)]
        for t in threads:
            t.start()
        for t in threads:
            t.join(60)
        assert not errors and not any(t.is_alive() for t in threads), errors
        idx = torch.tensor([0, 1, 0], dtype=torch.int32, device="cuda")
        for i in range(2):
            want = A.warp_mesh_frames_device(rings[i], args[i][0], args[i][1], proto, h, w, frame_index_dev=idx)
            assert same(got[i], want), (rep, i)
