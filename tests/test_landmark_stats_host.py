"""CPU-side checks of the landmark records and the weighted fit (flm_decode_stats, FLM_OUT_LANDMARKS_STATS,
flm_similarity_from_landmarks_weighted): the symbols exist, the size queries and every argument check answer before any
launch (so without a GPU), and the Python wrappers reject what they cannot run."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import flm_amd  # noqa: F401
from flm_amd import _lib, alignment, prediction
from flm_amd.networks import fcn

import stats_ref


def test_enum_and_symbols():
    assert _lib.OUT_LANDMARKS_STATS == 4 and _lib.LANDMARK_REC == 6
    assert fcn._OUT["landmark_stats"] == 4
    lib = C.CDLL(_lib.LIB_PATH)
    for name in ("flm_decode_stats_workspace_bytes", "flm_decode_stats", "flm_similarity_from_landmarks_weighted"):
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTS
    assert _lib.load().flm_abi_version() == 2          # purely additive


def test_argument_checks_answer_without_a_gpu():
    lib = _lib.load()
    p = C.c_void_p(0x1000)        # never dereferenced: every call below is rejected before a launch
    assert lib.flm_decode_stats(None, None, 1, 8, 8, 1, 0, 0, 0.0, None, None, 0) == -1
    assert lib.flm_decode_stats(None, p, 1, 8, 8, 1, 0, 0, 0.0, None, p, 0) == -1
    assert lib.flm_decode_stats(None, p, 1, 8, 8, 97, 1, 4, 0.0, p, p, 1 << 20) == -2          # as flm_decode: L <= 96
    assert lib.flm_decode_stats(None, p, 1, 8, 8, 68, 1, 129, 0.0, p, p, 1 << 20) == -5        # n_points <= 128
    assert lib.flm_decode_stats(None, p, 1, 8, 8, 68, 1, 4, 0.0, p, p, 0) == -3                # workspace too small
    w = lib.flm_similarity_from_landmarks_weighted
    assert w(None, p, 1, p, 1, p, 7, 68, 1.0, 1.0, p) == -2 and b"lm_stride" in lib.flm_last_error()
    assert w(None, p, 2, p, 0, p, 7, 68, 1.0, 1.0, p) == -2 and b"w_stride" in lib.flm_last_error()
    assert w(None, p, 6, p, 6, p, 0, 68, 1.0, 1.0, p) == -2
    assert w(None, p, 6, p, 6, p, 7, 1025, 1.0, 1.0, p) == -2
    assert w(None, None, 2, p, 1, p, 7, 68, 1.0, 1.0, p) == -1
    assert w(None, p, 2, p, 1, None, 7, 68, 1.0, 1.0, p) == -1
    assert w(None, p, 2, p, 1, p, 7, 68, 1.0, 1.0, None) == -1
    # out mode 4 is known, 9 is not (the null workspace answers first for a known mode, the enum check for an unknown one)
    assert lib.flm_fcn8_forward(None, p, p, 0, 1, 32, 32, 68, 0, 9, 1, 4, 0.0, p, p, 0) == -1
    assert b"output mode" in lib.flm_last_error()
    assert lib.flm_fcn8_forward(None, p, p, 0, 1, 32, 32, 68, 0, 4, 1, 4, 0.0, p, p, 0) == -3


def test_size_queries():
    lib = _lib.load()
    for dt in (_lib.FLM_F32, _lib.FLM_BF16):
        for arch in (_lib.ARCH_FCN8, _lib.ARCH_FCN32):
            a = (arch, 8, 256, 256, 68, dt)
            for npts in (4, 64):      # candidate path and materialised top-n: the records cost no workspace
                assert lib.flm_fcn_workspace_bytes(*a, 4, _lib.DECODE_TOPN, npts) == \
                    lib.flm_fcn_workspace_bytes(*a, 2, _lib.DECODE_TOPN, npts) > 0
            allpix = lib.flm_fcn_workspace_bytes(*a, 4, _lib.DECODE_ALL, 0)
            assert allpix >= lib.flm_fcn_workspace_bytes(*a, 2, _lib.DECODE_ALL, 0) > 0
    q = lib.flm_decode_stats_workspace_bytes
    assert q(2, 64, 64, 97, _lib.DECODE_TOPN, 4) == 0
    assert q(2, 64, 64, 68, _lib.DECODE_TOPN, 129) == 0
    assert q(2, 64, 64, 68, _lib.DECODE_TOPN, 0) == 0
    assert q(2, 64, 64, 68, 7, 4) == 0
    assert q(2, 64, 64, 68, _lib.DECODE_TOPN, 4) == lib.flm_decode_workspace_bytes(2, 64, 64, 68, _lib.DECODE_TOPN, 4) > 0
    # all-pixel: six partial sums per (chunk, landmark) instead of three
    assert lib.flm_decode_workspace_bytes(2, 64, 64, 68, _lib.DECODE_ALL, 0) < q(2, 64, 64, 68, _lib.DECODE_ALL, 0) \
        <= 2 * lib.flm_decode_workspace_bytes(2, 64, 64, 68, _lib.DECODE_ALL, 0)


def test_stats_source_compiles_without_scratch(tmp_path):
    """Same method as tests/test_build_hygiene.py, for the source that file's fixed list does not name: no kernel of
    flm_decode_stats.hip has a private segment (the all-pixel kernels hold six float64 lane sums for each of up to 24
    channels: 288 register pairs, which only fit because a 256-thread workgroup may take the whole register file)."""
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "face-landmark-detector_amd", "csrc")
    spec = importlib.util.spec_from_file_location("_flm_build", os.path.join(root, "face-landmark-detector_amd", "build.py"))
    bld = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bld)
    assert "flm_decode_stats.hip" in bld.SOURCES
    out = str(tmp_path / "flm_decode_stats.s")
    cmd = [bld._hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off",
           *bld.FILE_FLAGS.get("flm_decode_stats.hip", []), "-I", os.path.join(root, "include"), "-I", csrc, "-S",
           "--cuda-device-only", os.path.join(csrc, "flm_decode_stats.hip"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels = {m.group(1): int(m.group(2)) for m in re.finditer(
        r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n", open(out).read())}
    print(kernels)
    for name in ("decode_merge_stats_kernelILb0E", "decode_merge_stats_kernelILb1E", "decode_partial_all_stats_kernelILi17E",
                 "decode_partial_all_stats_kernelILi24E", "decode_partial_all_dma_stats_kernel", "decode_merge_all_stats_kernel"):
        assert any(name in k for k in kernels), name
    bad = {k: v for k, v in kernels.items() if v != 0}
    assert not bad, "kernels with a private segment (scratch): %s" % bad


class _Model:
    n_classes, input_height, input_width, output_height, output_width = 68, 256, 256, 264, 264


def test_python_wrappers_reject_bad_arguments_on_the_host():
    crops = np.zeros((2, 256, 256, 3), np.uint8)
    with pytest.raises(ValueError):      # not [N,H,W,3]
        prediction.predict(crops[0], _Model(), return_stats=True)
    with pytest.raises(ValueError):
        prediction.predict(np.zeros((2, 256, 256, 4), np.uint8), _Model(), return_stats=True)
    with pytest.raises(ValueError):
        prediction.predict(crops, _Model(), return_stats="yes")
    with pytest.raises(ValueError):
        prediction.align(crops, _Model(), weights="nonsense")
    with pytest.raises(ValueError):      # scores come from the model's forward, not from given landmarks
        prediction.align(crops, _Model(), landmarks=np.zeros((2, 68, 2)), weights="score")
    with pytest.raises(ValueError):      # [N,C] wanted
        prediction.align(crops, _Model(), weights=np.ones((2, 68, 1)))
    ring = torch.zeros((2, 64, 96, 3), dtype=torch.uint8)
    with pytest.raises(ValueError):
        prediction.align_frames(ring, [[(10, 10, 60, 60)], []], _Model(), weights="nonsense")
    lm = torch.zeros((2, 68, 2), dtype=torch.float64)
    tm = torch.zeros((68, 2), dtype=torch.float64)
    with pytest.raises(ValueError):      # float32 weights
        alignment.similarity_device(lm, tm, weights=torch.ones((2, 68)))
    with pytest.raises(ValueError):      # wrong shape
        alignment.similarity_device(lm, tm, weights=torch.ones((2, 67), dtype=torch.float64))
    from flm_amd.utils import metrics
    with pytest.raises(ValueError):      # host memory
        metrics.decode_stats_device(torch.zeros((1, 8, 8, 2)))


def test_views_of_a_record_tensor_pass_their_strides():
    rec = torch.zeros((3, 68, 6), dtype=torch.float64)
    assert alignment._uniform_stride(rec[..., :2], 2) == 6 and alignment._uniform_stride(rec[..., 2], 1) == 6
    assert alignment._uniform_stride(rec[..., :2].contiguous(), 2) == 2
    assert alignment._uniform_stride(rec[:, ::2, :2], 2) == 12             # every other landmark: still one stride
    assert alignment._uniform_stride(rec[:, :67, :2], 2) is None          # face stride is not K * point stride
    assert alignment._uniform_stride(rec.transpose(1, 2)[:, :2, :].transpose(1, 2), 2) == 6
    assert alignment._uniform_stride(torch.zeros((3, 2, 68), dtype=torch.float64).transpose(1, 2), 2) is None


def test_meaning_check_figures_on_the_restatement():
    """The figures tests/test_gpu_landmark_stats.py asserts on the device, on the numpy restatement: 10 of 68 landmarks
    displaced by 40 px pull the unweighted fit off by more than a pixel; with weight 1e-6 on them the fit is the true
    transform within 1e-3."""
    from oracle import warp_ref
    lm, tm, w, m = stats_ref.similarity_case()
    mw = stats_ref.weighted_similarity_ref(lm, tm, w)[0].astype(np.float64)
    mu = stats_ref.weighted_similarity_ref(lm, tm, None)
    assert np.array_equal(mu, warp_ref.similarity_ref(lm, tm))            # unit weights: the unweighted oracle's bits
    assert np.abs(mw - m).max() < 1e-3
    assert np.hypot(*(mu[0].astype(np.float64) - m)[:, 2]) > 1.0
