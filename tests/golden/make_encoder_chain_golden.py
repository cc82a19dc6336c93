"""Generate tests/golden/encoder_chain_golden.npz: the five levels of oracle/fcn_bf16_ref.py's free-running VGG, MobileNet
and ResNet50 encoders in every arithmetic, RECORDED AT THE COMMIT BEFORE THE ENCODERS WERE RESTATED AS CHAINS.

    python tests/golden/make_encoder_chain_golden.py

Run it at a commit whose encoders are trusted (it only needs `_ENCODERS[name](Arith, x_nchw, params) -> [(exact, stored)]`);
tests/test_oracle_encoder_chains.py then holds every later statement of the encoders to what that commit computed.  Per
encoder, shape (tests/enc_chain_cases.py) and arithmetic: 256 sampled values of each stored level (float64) and the
digest of the whole level, exact and stored; plus the platform probe of the machine that made them.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
import flm_amd  # noqa: E402,F401
import enc_chain_cases as cases  # noqa: E402
from oracle import fcn_bf16_ref as B  # noqa: E402
from oracle import fcn_ref  # noqa: E402

out, digests = {}, []
for enc, _, _ in cases.ENCODERS:
    p = cases.encoder_params(enc)
    for n, h, w in cases.CPU_SHAPES:
        x = np.stack([fcn_ref.get_image_array_ref(c) for c in cases.crops(n, h, w)])
        for name, kw in cases.ARITHS.items():
            levels = B._ENCODERS[enc](B.Arith(**kw), B._nchw(x), p)
            for k, (e, s) in enumerate(levels):
                key = "%s/%dx%dx%d/%s/f%d" % (enc, n, h, w, name, k + 1)
                out[key] = cases.sample(B._nhwc(s))
                digests.append("%s=%s,%s" % (key, cases.digest(B._nhwc(e)), cases.digest(B._nhwc(s))))
            print(enc, (n, h, w), name, "done")
out["digests"] = np.array(digests)
out["probe"] = np.array(cases.platform_probe())
dst = os.path.join(HERE, "encoder_chain_golden.npz")
np.savez_compressed(dst, **out)
print("wrote", dst, os.path.getsize(dst), "bytes")
