"""The VGG, MobileNet and ResNet50 encoders of fcn_8_vgg / fcn_8_mobilenet / fcn_8_resnet50, layer by layer, in both types.

Before this module these 13 / 27 / 54 layers were seen only through the softmax at the far end of the network (fp32: 1e-5
on probabilities near 1 / 68; bf16: four times the distance between two free-running oracles, tests/test_gpu_forward.py).
Here every layer is teacher-forced (tests/bf16_gate.py check_layers with `encoder=`): layer i gets the DEVICE's own input --
model.intermediate("act<src>"), every encoder layer has a workspace region of its own -- and its device output
intermediate("act<i>") is held against the float64 evaluation of that input by one step of the oracle's chain
(oracle/fcn_bf16_ref.py ENCODER_CHAINS, encoder_layer_ref), under the project's criteria as they stand:

  bf16-stored (every encoder layer, fc6, fc7 in bf16):   |got - exact64| <= ulp_bf16(exact64) / 2 + slack * max|exact64|
                                                         flips (got != round_bf16(exact64)) <= max(4 x the float32 evaluation's, 8)
  fp32-stored (everything in fp32; score5 .. logits):    |got - exact64| <= slack * max|exact64|
  slack = min(2e-5, max(4 x e32, 2^-23)), e32 measured per layer and input on the reference alone
  ResNet50's max-pool: the 3x3 stride-2 maximum of the device's own input, bit for bit, in both types
  class pad columns exact zeros; probabilities within 1e-5 of the softmax of the oracle's logits from the device's seg_feats

The library's layer table (flm_fcn_encoder_layer) only locates the buffers; every case first asserts that its names,
sources, shortcuts, strides, kernel sizes, activations and widths are the chain's (which was written from the reference's
network files, tests/test_oracle_encoder_chains.py).  Non-vacuity, asserted on the oracle's tensors: no layer is skipped;
every conv layer's exact output has at least 25 % non-zero elements (measured minimum 0.404, res2a_branch2b); at 3 x 64 x 96
every ReLU6 layer of MobileNet has elements clamped at 6 (0.37 % .. 6.4 % per layer).

Cases, 68 classes, uint8 BGR input from default_rng(7), synthetic weights (VGG seed 4, MobileNet 5, ResNet50 6):
  1 x 32 x 32   a 1 x 1 f5; MobileNet's last stride-2 depthwise takes 2 x 2 to 1 x 1; ResNet50 runs 16 x 16 -> max-pool 7 x 7 ->
                4 x 4 -> 2 x 2 -> 1 x 1 with 3x3 convs whose only real tap is the centre.  Encoder layers only.
  3 x 64 x 96   an odd face count, ragged tiles in every layer, ResNet50's odd 15 x 23 grid under the strided 1x1 convs and
                both residual epilogues, the pixel-pair pointwise conv on a 32 x 48 grid; here also the head and decoder
                (fc6 at K = 49 x 512 | 1024 | 2048, fc7, score5, fuse4, seg_feats, logits, probs), once per encoder and type.
  float32 RGB input, 1 x 32 x 32, fp32: the second template of mb_conv1_kernel / rn_conv1_kernel and VGG's first conv.
  f32_lean_tile = 0 on MobileNet and ResNet50 at 3 x 64 x 96: every act tensor and the probabilities bit for bit the
                default's (include/flm.h promises "same bits"; the strided and residual launches were where nothing checked it).

Measured on an MI355X (one run; the bars are the formulas above, not these figures).  Per encoder, type and layer group: the
reference-side e32 range over the group's layers and both shapes; the kernels' largest error (bf16: beyond the half step)
against the slack it was gated with, at the layer and shape where the two came closest; for bf16 the flip count against
its allowance where that came closest.

    encoder   type layer group                        e32 (reference)        error / slack (kernels)
    vgg       f32  block1_conv1 (first conv, no pool) 2.1e-07 .. 2.2e-07    2.5e-07 / 8.7e-07  (block1_conv1, 3x64x96)
    vgg       f32  3x3 <= 256 ch + pool               1.8e-07 .. 2.9e-07    1.7e-07 / 9.4e-07  (block3_conv3, 3x64x96)
    vgg       f32  3x3 <= 256 ch                      2.1e-07 .. 4.8e-07    1.4e-07 / 8.5e-07  (block3_conv2, 1x32x32)
    vgg       f32  3x3 512 ch                         2.3e-07 .. 1.7e-06    1.9e-07 / 9.3e-07  (block4_conv1, 1x32x32)
    vgg       f32  3x3 512 ch + pool                  2.1e-07 .. 9.3e-07    1.7e-07 / 9.5e-07  (block5_conv3, 3x64x96)
    vgg       f32  fc6                                2.3e-07 .. 2.3e-07    1.5e-07 / 9.2e-07  (fc6, 3x64x96)
    vgg       f32  fc7                                2.9e-07 .. 2.9e-07    1.6e-07 / 1.1e-06  (fc7, 3x64x96)
    vgg       f32  score5                             2.7e-07 .. 2.7e-07    2.6e-07 / 1.1e-06  (score5, 3x64x96)
    vgg       f32  fuse4                              3.3e-07 .. 3.3e-07    1.4e-07 / 1.3e-06  (fuse4, 3x64x96)
    vgg       f32  seg_feats                          3.9e-07 .. 3.9e-07    3.1e-07 / 1.6e-06  (seg_feats, 3x64x96)
    vgg       f32  logits                             4.0e-07 .. 4.0e-07    3.4e-07 / 1.6e-06  (logits, 3x64x96)
    vgg       bf16 block1_conv1 (first conv, no pool) 8.0e-08 .. 1.4e-07    9.2e-09 / 5.7e-07  (block1_conv1, 3x64x96)  flips 8 / 28 allowed of 1179648 (block1_conv1, 3x64x96)
    vgg       bf16 3x3 <= 256 ch + pool               1.0e-07 .. 2.1e-07    6.6e-08 / 5.7e-07  (block1_conv2, 3x64x96)  flips 5 / 16 allowed of 147456 (block2_conv2, 3x64x96)
    vgg       bf16 3x3 <= 256 ch                      1.3e-07 .. 2.0e-07    3.7e-08 / 7.4e-07  (block3_conv1, 3x64x96)  flips 22 / 68 allowed of 294912 (block3_conv2, 3x64x96)
    vgg       bf16 3x3 512 ch                         1.4e-07 .. 7.3e-07    4.3e-08 / 9.3e-07  (block4_conv1, 3x64x96)  flips 4 / 12 allowed of 36864 (block5_conv2, 3x64x96)
    vgg       bf16 3x3 512 ch + pool                  1.3e-07 .. 4.7e-07    1.2e-08 / 8.6e-07  (block4_conv3, 3x64x96)  flips 2 / 8 allowed of 36864 (block4_conv3, 3x64x96)
    vgg       bf16 fc6                                2.5e-07 .. 2.5e-07    3.8e-08 / 1.0e-06  (fc6, 3x64x96)  flips 4 / 12 allowed of 73728 (fc6, 3x64x96)
    vgg       bf16 fc7                                2.0e-07 .. 2.0e-07    5.2e-08 / 8.0e-07  (fc7, 3x64x96)  flips 11 / 32 allowed of 73728 (fc7, 3x64x96)
    vgg       bf16 score5                             1.8e-07 .. 1.8e-07    1.8e-07 / 7.1e-07  (score5, 3x64x96)
    vgg       bf16 fuse4                              2.0e-07 .. 2.0e-07    2.0e-07 / 8.1e-07  (fuse4, 3x64x96)
    vgg       bf16 seg_feats                          1.4e-07 .. 1.4e-07    1.5e-07 / 5.6e-07  (seg_feats, 3x64x96)
    vgg       bf16 logits                             2.1e-07 .. 2.1e-07    2.7e-07 / 8.3e-07  (logits, 3x64x96)
    mobilenet f32  conv1 (3x3 s2)                     3.2e-07 .. 3.7e-07    3.7e-07 / 1.5e-06  (conv1, 3x64x96)
    mobilenet f32  depthwise s1                       4.9e-08 .. 2.7e-07    2.6e-07 / 1.0e-06  (conv_dw_5, 3x64x96)
    mobilenet f32  pointwise 1 (pixel pairs)          2.8e-07 .. 3.4e-07    3.4e-07 / 1.4e-06  (conv_pw_1, 3x64x96)
    mobilenet f32  depthwise s2                       5.7e-08 .. 3.4e-07    2.1e-07 / 5.3e-07  (conv_dw_12, 3x64x96)
    mobilenet f32  pointwise 2..13                    2.4e-07 .. 9.3e-07    4.2e-07 / 1.6e-06  (conv_pw_2, 3x64x96)
    mobilenet f32  fc6                                2.7e-07 .. 2.7e-07    1.5e-07 / 1.1e-06  (fc6, 3x64x96)
    mobilenet f32  fc7                                2.6e-07 .. 2.6e-07    1.5e-07 / 1.0e-06  (fc7, 3x64x96)
    mobilenet f32  score5                             2.5e-07 .. 2.5e-07    1.2e-07 / 9.9e-07  (score5, 3x64x96)
    mobilenet f32  fuse4                              4.5e-07 .. 4.5e-07    2.1e-07 / 1.8e-06  (fuse4, 3x64x96)
    mobilenet f32  seg_feats                          3.6e-07 .. 3.6e-07    2.1e-07 / 1.4e-06  (seg_feats, 3x64x96)
    mobilenet f32  logits                             4.2e-07 .. 4.2e-07    3.0e-07 / 1.7e-06  (logits, 3x64x96)
    mobilenet bf16 conv1 (3x3 s2)                     3.2e-07 .. 3.7e-07    3.8e-08 / 1.5e-06  (conv1, 3x64x96)  flips 9 / 36 allowed of 147456 (conv1, 3x64x96)
    mobilenet bf16 depthwise s1                       3.8e-08 .. 3.0e-07    7.1e-09 / 8.9e-07  (conv_dw_5, 3x64x96)  flips 2 / 8 allowed of 147456 (conv_dw_3, 3x64x96)
    mobilenet bf16 pointwise 1 (pixel pairs)          1.2e-07 .. 1.7e-07    0.0e+00 / 6.9e-07  (conv_pw_1, 3x64x96)  flips 0 / 8 allowed of 16384 (conv_pw_1, 1x32x32)
    mobilenet bf16 depthwise s2                       8.2e-08 .. 3.3e-07    4.3e-09 / 1.0e-06  (conv_dw_2, 3x64x96)  flips 1 / 8 allowed of 73728 (conv_dw_2, 3x64x96)
    mobilenet bf16 pointwise 2..13                    8.7e-08 .. 5.2e-07    1.0e-07 / 1.2e-06  (conv_pw_11, 3x64x96)  flips 2 / 8 allowed of 147456 (conv_pw_2, 3x64x96)
    mobilenet bf16 fc6                                3.3e-07 .. 3.3e-07    2.5e-08 / 1.3e-06  (fc6, 3x64x96)  flips 6 / 12 allowed of 73728 (fc6, 3x64x96)
    mobilenet bf16 fc7                                1.5e-07 .. 1.5e-07    2.5e-08 / 6.0e-07  (fc7, 3x64x96)  flips 7 / 20 allowed of 73728 (fc7, 3x64x96)
    mobilenet bf16 score5                             1.0e-07 .. 1.0e-07    1.1e-07 / 4.1e-07  (score5, 3x64x96)
    mobilenet bf16 fuse4                              2.3e-07 .. 2.3e-07    3.3e-07 / 9.0e-07  (fuse4, 3x64x96)
    mobilenet bf16 seg_feats                          1.6e-07 .. 1.6e-07    1.3e-07 / 6.3e-07  (seg_feats, 3x64x96)
    mobilenet bf16 logits                             1.8e-07 .. 1.8e-07    2.2e-07 / 7.3e-07  (logits, 3x64x96)
    resnet50  f32  conv1 (7x7 s2)                     4.3e-07 .. 4.7e-07    4.7e-07 / 1.9e-06  (conv1, 1x32x32)
    resnet50  f32  branch1 (shortcut 1x1, no ReLU)    3.3e-07 .. 4.0e-07    1.9e-07 / 1.3e-06  (res2a_branch1, 1x32x32)
    resnet50  f32  branch2a 1x1                       1.9e-07 .. 9.5e-07    2.0e-07 / 1.0e-06  (res2c_branch2a, 3x64x96)
    resnet50  f32  branch2b 3x3                       1.4e-07 .. 9.9e-07    2.0e-07 / 9.0e-07  (res4b_branch2b, 3x64x96)
    resnet50  f32  branch2c 1x1 + residual            3.6e-08 .. 2.3e-07    3.8e-08 / 1.4e-07  (res5a_branch2c, 1x32x32)
    resnet50  f32  branch1 (shortcut 1x1, no ReLU) s2 2.4e-07 .. 5.6e-07    2.2e-07 / 9.8e-07  (res3a_branch1, 3x64x96)
    resnet50  f32  branch2a 1x1 s2                    1.7e-07 .. 5.7e-07    1.4e-07 / 6.9e-07  (res3a_branch2a, 3x64x96)
    resnet50  f32  fc6                                4.2e-07 .. 4.2e-07    1.7e-07 / 1.7e-06  (fc6, 3x64x96)
    resnet50  f32  fc7                                2.8e-07 .. 2.8e-07    1.8e-07 / 1.1e-06  (fc7, 3x64x96)
    resnet50  f32  score5                             1.9e-07 .. 1.9e-07    1.5e-07 / 7.7e-07  (score5, 3x64x96)
    resnet50  f32  fuse4                              2.8e-07 .. 2.8e-07    1.5e-07 / 1.1e-06  (fuse4, 3x64x96)
    resnet50  f32  seg_feats                          3.5e-07 .. 3.5e-07    2.3e-07 / 1.4e-06  (seg_feats, 3x64x96)
    resnet50  f32  logits                             3.9e-07 .. 3.9e-07    2.7e-07 / 1.6e-06  (logits, 3x64x96)
    resnet50  bf16 conv1 (7x7 s2)                     4.3e-07 .. 4.7e-07    8.8e-08 / 1.7e-06  (conv1, 3x64x96)  flips 23 / 92 allowed of 294912 (conv1, 3x64x96)
    resnet50  bf16 branch1 (shortcut 1x1, no ReLU)    1.0e-07 .. 1.6e-07    1.2e-08 / 6.6e-07  (res2a_branch1, 3x64x96)  flips 6 / 32 allowed of 264960 (res2a_branch1, 3x64x96)
    resnet50  bf16 branch2a 1x1                       9.0e-08 .. 5.0e-07    8.8e-08 / 7.4e-07  (res4e_branch2a, 3x64x96)  flips 3 / 12 allowed of 18432 (res4c_branch2a, 3x64x96)
    resnet50  bf16 branch2b 3x3                       7.8e-08 .. 4.3e-07    1.1e-07 / 1.0e-06  (res5c_branch2b, 3x64x96)  flips 5 / 8 allowed of 36864 (res3c_branch2b, 3x64x96)
    resnet50  bf16 branch2c 1x1 + residual            3.5e-08 .. 1.3e-07    2.0e-08 / 2.4e-07  (res2c_branch2c, 3x64x96)  flips 6 / 16 allowed of 264960 (res2c_branch2c, 3x64x96)
    resnet50  bf16 branch1 (shortcut 1x1, no ReLU) s2 1.6e-07 .. 2.5e-07    6.2e-08 / 7.4e-07  (res5a_branch1, 3x64x96)  flips 5 / 16 allowed of 36864 (res5a_branch1, 3x64x96)
    resnet50  bf16 branch2a 1x1 s2                    8.1e-08 .. 3.5e-07    7.3e-09 / 8.1e-07  (res4a_branch2a, 3x64x96)  flips 1 / 8 allowed of 18432 (res4a_branch2a, 3x64x96)
    resnet50  bf16 fc6                                5.0e-07 .. 5.0e-07    5.0e-08 / 2.0e-06  (fc6, 3x64x96)  flips 10 / 16 allowed of 73728 (fc6, 3x64x96)
    resnet50  bf16 fc7                                1.7e-07 .. 1.7e-07    3.3e-08 / 6.8e-07  (fc7, 3x64x96)  flips 4 / 24 allowed of 73728 (fc7, 3x64x96)
    resnet50  bf16 score5                             1.2e-07 .. 1.2e-07    1.7e-07 / 4.9e-07  (score5, 3x64x96)
    resnet50  bf16 fuse4                              1.2e-07 .. 1.2e-07    2.5e-07 / 4.9e-07  (fuse4, 3x64x96)
    resnet50  bf16 seg_feats                          1.7e-07 .. 1.7e-07    1.7e-07 / 7.0e-07  (seg_feats, 3x64x96)
    resnet50  bf16 logits                             1.9e-07 .. 1.9e-07    2.5e-07 / 7.6e-07  (logits, 3x64x96)
    probs     max-abs error against the bar of 1e-5: VGG 1.6e-07 (bf16 1.2e-07), MobileNet 4.5e-08 (6.2e-08), ResNet50 4.5e-07 (4.2e-07)

Every layer of every case passes on the unmodified kernels: the largest share of an allowance used is 0.52 (bf16 ResNet50,
fuse4), 0.40 among encoder layers (fp32 MobileNet conv1, whose fmaf chain is the reference's own order: error = e32); the
2e-5 cap never binds; the max-pool is bit-exact in all five ResNet50 cases; f32_lean_tile = 0 changes no bit of any of the
27 / 54 act tensors or of the probabilities.  Nothing to fix in a kernel or in the oracle.

(A negative "error" beyond the half step means every element lay inside it; it is printed as 0.)

Fault injection (scratch builds, not committed; wrong values only, no address or bound touched; each build run once).  For
each: the tests of the suite as it stood before this module that reach the faulted kernel (every MobileNet / ResNet50 test of
tests/test_gpu_forward.py and tests/test_gpu_igemm_lean_tile.py, 12 tests; no other module runs these encoders), then
this module.  THE OLD SUITE CATCHES ALL THREE -- at the probabilities, at its 224 x 224 / 256 x 256 shapes; what this module
adds is the layer, the size of the error at that layer, and the small shapes.
(a) mb_depthwise_kernel treats the last input column as padding when stride == 2.  Old suite: test_mobilenet_variants fails
    (fp32 probabilities 3.8e-2 from the oracle against 1e-5) and test_mobilenet_bf16_close_to_fp32 fails (mean distance to the
    rounding oracle 8.4e-4 against 4 x 7.7e-5); 10 pass.  Here: all 5 gated MobileNet cases fail, and in each exactly
    conv_dw_2, conv_dw_4, conv_dw_6 and conv_dw_12 -- the four stride-2 layers -- with an error of 0.997 .. 1.0 of the tensor's maximum
    against slacks near 1e-6 (bf16: 1.8 % .. 41 % of the elements flipped against an allowance of 8); every other layer, handed
    the device's wrong input, passes.  The f32_lean_tile = 0 case passes: both of its forwards run the same depthwise kernel.
(b) The guarded epilogue of the implicit GEMM skips the residual add.  Old suite: test_resnet50_variants fails (fp32
    probabilities 0.81 off), test_resnet50_bf16_close_to_fp32 fails, test_other_encoders_f32_lean_tile_keeps_every_bit
    [fcn_8_resnet50] fails; 9 pass.  Here: all 6 ResNet50 cases fail; in the gated ones exactly the 16 `2c` convs, 0.16 .. 1.0
    of the maximum (bf16: 35 % .. 69 % flipped), at 1 x 32 x 32 too; with f32_lean_tile = 0, 49 of the 54 act tensors and the
    probabilities differ from the default's (the default's whole tiles take the fast epilogue, which still adds).
(c) pack_bf16x2 truncates instead of rounding to nearest even.  Old suite: test_mobilenet_bf16_close_to_fp32 fails (mean distance
    5.5e-4 against 4 x 7.7e-5) and test_resnet50_bf16_close_to_fp32 fails BY A HAIR on its second criterion only (mean distance
    to the bf16 oracle 1.91e-4 against 1.76e-4 to the fp32 oracle; its 4 x bars hold: 1.9e-4 against 6.2e-4); 10 pass.  Here: the 4
    bf16 MobileNet / ResNet50 cases fail, in exactly the layers that store through store4<true>: MobileNet's conv1 and all 13
    depthwise layers, ResNet50's conv1 -- 1.2e-3 .. 3.6e-3 of the maximum beyond the half step, 22 % .. 27 % of the elements flipped
    against allowances of 8 .. 92.  The pointwise and bottleneck convs (another store) pass, the max-pool stays bit-exact
    (a maximum of bf16 values needs no rounding).
"""
import json

import numpy as np
import pytest
import torch

import enc_chain_cases as cases
from bf16_gate import check_layers

pytestmark = pytest.mark.gpu

MODELS = {"vgg": "fcn_8_vgg", "mobilenet": "fcn_8_mobilenet", "resnet50": "fcn_8_resnet50"}
SMALL, LARGE = (1, 32, 32), (3, 64, 96)
# (encoder, type, shape, variant), one encoder's cases together: its weights (ResNet50: 1.7 GB) and the float64 operand of
# its fc6 (3 GB) are built once
CASES = [(enc, dtype, shape, None) for enc in MODELS for dtype in ("f32", "bf16") for shape in (SMALL, LARGE)]
CASES += [(enc, "f32", SMALL, "f32_rgb") for enc in MODELS]
CASES += [(enc, "f32", LARGE, "f32_lean_tile=0") for enc in ("mobilenet", "resnet50")]
CASES.sort(key=lambda c: list(MODELS).index(c[0]))


@pytest.fixture(scope="module")
def flm():
    import flm_amd
    from flm_amd import _lib
    _lib.load()
    yield flm_amd
    _MODEL.clear()
    _ORACLE_CACHE.clear()


_MODEL = {}
_ORACLE_CACHE = {}   # the oracle's float64 fc6 operands of the current encoder (check_layers cache=)


def _model(enc, dtype, h, w):
    from flm_amd.networks import LANDMARKS_MODELS
    key = (enc, dtype, h, w)
    if key not in _MODEL:
        if _MODEL and next(iter(_MODEL))[0] != enc:
            _ORACLE_CACHE.clear()                # the previous encoder's fc6 operands
        _MODEL.clear()
        model = LANDMARKS_MODELS[MODELS[enc]](68, input_height=h, input_width=w, dtype=dtype)
        model.load_weights(cases.encoder_params(enc))
        _MODEL[key] = model
    return _MODEL[key]


def _acts(model, n):
    return [model.intermediate("act%d" % i, n, "probs").clone() for i in range(len(model.encoder_layer_names()))]


@pytest.mark.parametrize("enc,dtype,shape,variant", CASES,
                         ids=["%s-%s-%dx%dx%d%s" % (e, d, *s, "-" + v if v else "") for e, d, s, v in CASES])
def test_encoder_layers_teacher_forced(flm, enc, dtype, shape, variant):
    from flm_amd import _lib
    from oracle import fcn_ref
    n, h, w = shape
    params = cases.encoder_params(enc)
    model = _model(enc, dtype, h, w)
    cases.check_chain_against_table(model, enc)        # the table only locates buffers: its wiring must be the oracle's
    crops = cases.crops(n, h, w)
    label = "%s %s %dx%dx%d%s" % (MODELS[enc], dtype, n, h, w, " " + variant if variant else "")
    if variant == "f32_lean_tile=0":             # "same bits" (include/flm.h) under the strided and the residual launches
        xd = torch.from_numpy(crops).cuda()
        p0 = model.forward_device(xd, "probs").clone()
        a0 = _acts(model, n)
        with _lib.tuning(f32_lean_tile=0):
            p1 = model.forward_device(xd, "probs").clone()
            a1 = _acts(model, n)
        torch.cuda.synchronize()
        diff = [model.encoder_layer_names()[i] for i, (u, v) in enumerate(zip(a0, a1)) if not torch.equal(u, v)]
        print("%s: %d of %d act tensors differ from the default's%s" % (label, len(diff), len(a0), ", probabilities too" if not torch.equal(p0, p1) else ""))
        assert not diff and torch.equal(p0, p1), diff
        assert all(np.isfinite(a.cpu().numpy()).all() and a.abs().max() > 0 for a in a0)
        return
    x = np.stack([fcn_ref.get_image_array_ref(c) for c in crops]) if variant == "f32_rgb" else crops
    xd = torch.from_numpy(x).cuda()
    head = shape == LARGE and variant is None    # fc6 .. logits, probs: once per encoder and type
    probs = model.forward_device(xd, "probs").cpu().numpy()
    lg = model.forward_device(xd, "logits").cpu().numpy() if head else None
    torch.cuda.synchronize()
    for bad in ("act%d" % len(model.encoder_layer_names()), "act", "nonsense"):
        with pytest.raises(KeyError):
            model.intermediate(bad, n, "probs")
    if head:
        for k in ("act0", "f5", "fc7", "seg_feats"):   # the two forwards wrote the same bits into their workspaces
            assert torch.equal(model.intermediate(k, n, "probs"), model.intermediate(k, n, "logits")), k
    reports = check_layers(model, params, x, n, "probs", logits=lg, probs=probs if head else None, label=label, dtype=dtype,
                           encoder=enc, head=head, cache=_ORACLE_CACHE)
    from oracle import fcn_bf16_ref as B
    chain = B.ENCODER_CHAINS[enc]
    # no layer skipped, and the gate is not vacuous: live outputs everywhere, ReLU6 clamps reached at the larger shape
    assert [st.name for st in chain] == [k for k in reports if k in {st.name for st in chain}] and len(chain) in (13, 27, 54)
    if head:
        assert list(reports)[len(chain):] == ["fc6", "fc7", "score5", "fuse4", "seg_feats", "logits", "probs"]
    else:
        assert len(reports) == len(chain)
    for st in chain:
        if st.op == "conv":
            assert reports[st.name]["nonzero"] >= 0.25, (st.name, reports[st.name]["nonzero"])
        if st.relu == 2 and shape == LARGE:
            assert reports[st.name]["at6"] > 0, st.name
    print("ENCGATE " + json.dumps(dict(case=label, reports={k: {a: b for a, b in r.items() if a != "ok"} for k, r in reports.items()})))
