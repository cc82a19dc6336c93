"""flm_track_retire of include/flm.h in plain numpy: one loop over the slots per numbered step of the contract, nothing
taken from the kernel.  `retire` works in place on a dict of arrays named as the header names them."""
import numpy as np

EXIT_META = 8


def live_of(boxes, fh, fw):
    """Step 1: the clipped box is not empty (the clip of the tracking section)."""
    b = np.asarray(boxes, np.int64)
    cx0, cx1 = np.clip(b[:, 0], 0, fw), np.clip(b[:, 2], 0, fw)
    cy0, cy1 = np.clip(b[:, 1], 0, fh), np.clip(b[:, 3], 0, fh)
    return ~((cx1 - cx0 <= 0) | (cy1 - cy0 <= 0))


def new_state(k, q, face_bytes, c, optional=True, rng=None):
    """Tracker-side state and an exit ring, ring and exit_row filled with a sentinel pattern (or noise from `rng`)."""
    def fill(shape, dtype, value):
        if rng is None:
            return np.full(shape, value, dtype)
        if np.dtype(dtype).kind == "f":
            return rng.standard_normal(shape).astype(dtype)
        return rng.integers(0, 200, size=shape).astype(dtype)
    s = dict(
        boxes=np.zeros((k, 4), np.int32), status=np.ones((k,), np.int32), best_q=np.full((k,), -1.0),
        gallery=np.zeros((k, face_bytes), np.uint8), best_frame=np.full((k,), -1, np.int64),
        born=np.zeros((k,), np.int32), track_id=np.full((k,), -1, np.int64), born_frame=np.full((k,), -1, np.int64),
        head=np.zeros((4,), np.int64),
        x_gallery=fill((q, face_bytes), np.uint8, 0xA5), x_meta=fill((q, EXIT_META), np.int64, -77),
        x_q=fill((q,), np.float64, -7.5), exit_row=np.full((k,), -9, np.int32))
    if optional:
        s.update(best_m=np.zeros((k, 2, 3), np.float32), best_lm=np.full((k, c, 2), -1.0), best_rec=np.zeros((k, 8), np.int64),
                 x_m=fill((q, 2, 3), np.float32, -3.0), x_lm=fill((q, c, 2), np.float64, -5.0), x_rec=fill((q, 8), np.int64, -11))
    return s


def retire(s, fh, fw, frame_id, flush=False, min_q=0.0):
    """One flm_track_retire on `s`, in place.  Returns a dict of what the call decided: ends, emitted, written, births
    (bool [K]) and E, B."""
    k, q = len(s["track_id"]), len(s["x_q"])
    live = live_of(s["boxes"], fh, fw)                                   # 1
    born = s["born"] != 0
    held = s["track_id"] >= 0
    ends = held & (born | ~live | bool(flush))                           # 2
    with np.errstate(invalid="ignore"):
        emitted = ends & (s["best_q"] >= min_q)                          # 3 (false for a NaN)
    discarded = ends & ~emitted
    seq0, next_id = int(s["head"][0]), int(s["head"][1])
    e_slots = np.flatnonzero(emitted)                                    # 4: ranked by ascending slot
    e = len(e_slots)
    exit_row = np.full((k,), -1, np.int32)
    exit_row[discarded] = -2
    written = np.zeros((k,), bool)
    for r, t in enumerate(e_slots):
        if r >= e - q:
            row = (seq0 + r) % q
            exit_row[t] = row
            written[t] = True
            s["x_gallery"][row] = s["gallery"][t]                        # 5
            s["x_q"][row] = s["best_q"][t]
            for src, dst in (("best_m", "x_m"), ("best_lm", "x_lm"), ("best_rec", "x_rec")):
                if src in s:
                    s[dst][row] = s[src][t]
            end = -1 if born[t] else int(s["status"][t]) if not live[t] else -2
            s["x_meta"][row] = [s["track_id"][t], t, s["born_frame"][t], frame_id, s["best_frame"][t], end, seq0 + r, 0]
        else:
            exit_row[t] = -3
    births = born & live                                                 # 6
    b_slots = np.flatnonzero(births)
    for t in range(k):
        if not births[t] and (ends[t] or born[t]):
            s["track_id"][t] = -1
    for b, t in enumerate(b_slots):
        s["track_id"][t] = next_id + b
        s["born_frame"][t] = frame_id
    s["born"][:] = 0
    s["exit_row"][:] = exit_row
    s["head"][0] = seq0 + e
    s["head"][1] = next_id + len(b_slots)
    s["head"][2] += int(discarded.sum())
    s["head"][3] += max(e - q, 0)
    return dict(ends=ends, emitted=emitted, written=written, births=births, discarded=discarded, E=e, B=len(b_slots),
                held=held, born=born, live=live)


def exit_rows_brute(seq, cursor, capacity):
    """alignment.exit_rows by replaying the ring: which sequence number each row holds after `seq` exits."""
    holds = {}
    for s in range(seq):
        holds[s % capacity] = s
    rows = [s % capacity for s in range(cursor, seq) if holds[s % capacity] == s]
    return rows, (seq - cursor) - len(rows)
