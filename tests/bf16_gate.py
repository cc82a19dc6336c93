"""Teacher-forced layer checks of the bf16 configuration (vanilla fcn_8), shared by the GPU test modules.

Every layer is handed the DEVICE's own input, read back exactly through model.intermediate, and its device output is
held against the float64 evaluation of that input by oracle/fcn_bf16_ref.py:

  bf16-stored (f1..f5, fc6, fc7):            |got - exact64| <= ulp_bf16(exact64) / 2 + slack * max|exact64|
  fp32-stored (score5, fuse4, seg_feats,
               logits):                      |got - exact64| <=                        slack * max|exact64|
  flips (bf16-stored):  elements with got != round_bf16(exact64)  <=  max(4 x the float32 evaluation's, 8)

slack is measured on the reference side, per layer and input: 4 x the largest error of torch's float32 evaluation of
the same rounded operands against float64, capped at the fp32 suite's 2e-5 (never below one float32 step, 2^-23).

dtype="f32" gates the exact-fp32 configuration the same way against the oracle's fp32 arithmetic (layer_f32_ref: the
packer's folded float32 scale / shift, nothing rounded to bf16): every layer is fp32-stored, so the criterion is
|got - exact64| <= slack * max|exact64| with e32 from the float32-accumulating evaluation of the same input, and there
is no flip count.  Class pad columns of score5 / fuse4 / seg_feats must be exact zeros in both configurations.

encoder="vgg" | "mobilenet" | "resnet50" gates the fcn_8 model on that encoder the same way, one step of the oracle's chain
(oracle/fcn_bf16_ref.py ENCODER_CHAINS) per encoder layer: the device's output of layer i is model.intermediate("act<i>"),
its input the device's output of the step's source (and shortcut), its reference encoder_layer_ref of that input.  Every
encoder layer is stored in the operand type, so in bf16 each gets the half step and the flip count.  ResNet50's max-pool
has no arithmetic: it must be the 3x3 stride-2 maximum of the device's own input bit for bit.  The head (fc6 .. seg_feats,
logits, probs; `head=False` leaves it out) reads f3 / f4 / f5 = the chain's levels.  Each report also carries `nonzero`,
the share of non-zero elements of the exact output, and for ReLU6 layers `at6`, the share clamped at 6.
"""
import numpy as np
import torch

from oracle import fcn_bf16_ref as B
from oracle import fcn_ref

STORED_BF16 = ("f1", "f2", "f3", "f4", "f5", "fc6", "fc7")
CHAIN = (("f1", "enc1", ("x",)), ("f2", "enc2", ("f1",)), ("f3", "enc3", ("f2",)), ("f4", "enc4", ("f3",)),
         ("f5", "enc5", ("f4",)), ("fc6", "fc6", ("f5",)), ("fc7", "fc7", ("fc6",)), ("score5", "score5", ("fc7",)),
         ("fuse4", "fuse4", ("score5", "f4")), ("seg_feats", "seg_feats", ("fuse4", "f3")))


def check_layers(model, params, crops_u8, n, out, faces=None, logits=None, probs=None, label="", dtype="bf16",
                 encoder=None, head=True, cache=None):
    """Gate every layer of the last forward (n faces, output mode `out`) on `faces` (default: all).  `logits` / `probs`:
    device outputs of forwards of the SAME faces (numpy, [F,H',W',C] / [F,H'*W',C]) whose workspaces hold the seg_feats
    they were computed from.  `crops_u8` may also be the float32 preprocessed input the forward was given.  Prints one
    line per layer, then asserts.  Returns {name: report}.  `cache`: a dict of the caller's for the oracle's large float64
    operands (oracle/fcn_bf16_ref.py _weight; fc6 on a 2048-channel f5 is 3 GB)."""
    assert dtype in ("bf16", "f32") and model.dtype == dtype, (dtype, model.dtype)
    f32 = dtype == "f32"
    crops_u8 = np.asarray(crops_u8)
    faces = list(range(n)) if faces is None else list(faces)
    dev = {"x": np.stack([fcn_ref.get_image_array_ref(crops_u8[f]) if crops_u8.dtype == np.uint8 else crops_u8[f] for f in faces])}
    steps = () if encoder is None else B.ENCODER_CHAINS[encoder]
    tail = CHAIN if encoder is None else (CHAIN[5:] if head else ())
    for i, st in enumerate(steps):
        dev[st.name] = model.intermediate("act%d" % i, n, out)[faces].cpu().numpy().astype(np.float64)
    for name, _, _ in tail:
        dev[name] = model.intermediate(name, n, out)[faces].cpu().numpy().astype(np.float64)
    if steps and head:   # the head reads the chain's levels
        for k in (3, 4, 5):
            dev["f%d" % k] = dev[B.ENCODER_LEVELS[encoder][k - 1]]
            assert np.array_equal(dev["f%d" % k], model.intermediate("f%d" % k, n, out)[faces].cpu().numpy()), k
    reports, bad = {}, []

    def gate(name, layer, xin, got, enc=None):
        ref = (lambda **kw: B.layer_bf16_ref(layer, xin, params, fp32=f32, cache=cache, **kw)) if enc is None else \
            (lambda **kw: B.encoder_layer_ref(enc, layer, xin, params, fp32=f32, **kw))
        exact, _ = ref()
        e32, s32 = ref(accum=torch.float32)
        rep = B.gate_layer(got, exact, e32, s32, (name in STORED_BF16 or enc is not None) and not f32)   # class pad columns: exact zeros
        rep["nonzero"] = float((exact != 0).mean())
        line = B.format_report(name, rep)
        if f32:   # nothing is stored rounded: `over` is the whole error
            line = line.replace("over-half-step", "error")
        print("%s %s" % (label, line) + (" pad columns not zero: %g" % rep["pad"] if "pad" in rep else ""))
        reports[name] = rep
        if not rep["ok"]:
            bad.append(name)
        return exact

    for st in steps:
        xin = dev[st.inputs[0]] if len(st.inputs) == 1 else tuple(dev[s] for s in st.inputs)
        if st.op == "maxpool3":   # no arithmetic: the maximum of the device's own input, bit for bit
            exp = B.encoder_layer_ref(encoder, st.name, xin, params, fp32=f32)[1]
            same = exp.shape == dev[st.name].shape and np.array_equal(exp, dev[st.name])
            print("%s %-9s 3x3 stride-2 maximum of the device's input: %s" % (label, st.name, "bit for bit" if same else "DIFFERS   <-- FAILS"))
            reports[st.name] = dict(ok=same, nonzero=float((exp != 0).mean()))
            if not same:
                bad.append(st.name)
            continue
        exact = gate(st.name, st.name, xin, dev[st.name], enc=encoder)
        if st.relu == 2:
            reports[st.name]["at6"] = float((exact == 6.0).mean())
    for name, layer, srcs in tail:
        xin = dev[srcs[0]] if len(srcs) == 1 else tuple(dev[s] for s in srcs)
        gate(name, layer, xin, dev[name])
    for what, arr, mode in (("logits", logits, "logits"), ("probs", probs, "probs")):
        if arr is None:
            continue
        seg = model.intermediate("seg_feats", len(faces) if mode != out else n, mode)
        seg = (seg[faces] if mode == out else seg).cpu().numpy().astype(np.float64)
        if what == "logits":
            gate("logits", "logits", seg, np.asarray(arr, np.float64))
        else:   # the fp32 suite's bar, against the softmax of the oracle's logits FROM THE DEVICE'S seg_feats
            d = B.probs_report(arr, B.layer_bf16_ref("logits", seg, params, fp32=f32, cache=cache)[0])["err"]
            print("%s probs     max-abs error %.3g (bar 1e-5), rows sum to 1 within %.3g" % (label, d, np.abs(arr.sum(-1) - 1).max()))
            reports["probs"] = dict(err=d, ok=d <= 1e-5)
            if d > 1e-5:
                bad.append("probs")
    assert not bad, (label, {k: reports[k] for k in bad})
    return reports
