"""flm_track_associate_streams as include/flm.h states it: a loop over the streams around track_assoc_ref.associate on
each stream's own slices, the i*K offset on det_slot where it names a slot, and the skip rule (n_det[i] < 0: nothing of
the stream's state is read or written, det_slot = -1, slot_det = -1, counts = 0).  What the kernel must equal bit for bit
on all eight tensors.
"""
import numpy as np

import track_assoc_ref

NAMES = ("m_crop", "boxes", "status", "misses", "state", "det_slot", "slot_det", "counts")


def associate_streams(det, n_det, m_crop, boxes, status, misses, state, k, in_h, in_w, fh, fw, **opts):
    """det int32 [S,D,4]; n_det None or S integers; m_crop [S*K,2,3], boxes [S*K,4], status, misses [S*K], state None or
    float64 [S*K,C,6]; k slots per stream -> dict of the eight tensors after the call; the inputs are not changed."""
    det = np.asarray(det, np.int32)
    s, d = det.shape[:2]
    n = s * k
    out = dict(m_crop=np.array(m_crop, np.float32).reshape(n, 2, 3).copy(), boxes=np.array(boxes, np.int32).reshape(n, 4).copy(),
               status=np.array(status, np.int32).reshape(n).copy(), misses=np.array(misses, np.int32).reshape(n).copy(),
               state=None if state is None else np.array(state, np.float64).copy(),
               det_slot=np.full((s, d), -1, np.int32), slot_det=np.full(n, -1, np.int32), counts=np.zeros((s, 8), np.int32))
    for i in range(s):
        if n_det is not None and int(n_det[i]) < 0:
            continue                                             # skipped: the copies above are the stream's result
        sl = slice(i * k, (i + 1) * k)
        r = track_assoc_ref.associate(det[i], None if n_det is None else int(n_det[i]), out["m_crop"][sl], out["boxes"][sl],
                                      out["status"][sl], out["misses"][sl], None if state is None else out["state"][sl],
                                      in_h, in_w, fh, fw, **opts)
        for name in ("m_crop", "boxes", "status", "misses", "slot_det"):
            out[name][sl] = r[name]
        if state is not None:
            out["state"][sl] = r["state"]
        ds = r["det_slot"].copy()
        ds[ds >= 0] += i * k                                     # a slot's name is global; -1 and -2 keep their meaning
        out["det_slot"][i] = ds
        out["counts"][i] = r["counts"]
    return out
