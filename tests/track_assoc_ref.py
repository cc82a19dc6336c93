"""flm_track_associate as include/flm.h ("association") states it, in numpy and Python integers, serially and in the
plainest way: the box maths, the clip, int64 areas, the one float64 multiplication of the threshold test, the exact
order of pairs, and the true greedy loop.  What the kernel must equal bit for bit on all eight tensors.  Builds on
track_ref.seed for the matrices of restarted and born slots.
"""
import functools

import numpy as np

import track_ref

DUPLICATE, UNCONFIRMED = 32, 64
LIM = 2 ** 28
COUNTS = ("matched", "born", "refreshed", "duplicates", "unconfirmed", "dropped", "void", "zero")


def square_box(box):
    """Item 2 of the contract: the box maths of the reference's detect_marks, in the header's form."""
    x0, y0, x1, y1 = [int(v) for v in box]
    off = int(abs(float(y1 - y0) * 0.1))
    y0 += off
    y1 += off
    diff = (y1 - y0) - (x1 - x0)
    delta, odd = abs(diff) >> 1, abs(diff) & 1
    if diff > 0:
        x0 -= delta
        x1 += delta + odd
    elif diff < 0:
        y0 -= delta
        y1 += delta + odd
    return [x0, y0, x1, y1]


def clip(box, fh, fw):
    x0, y0, x1, y1 = [int(v) for v in box]
    return [min(max(x0, 0), fw), min(max(y0, 0), fh), min(max(x1, 0), fw), min(max(y1, 0), fh)]


def empty(c):
    return c[2] - c[0] <= 0 or c[3] - c[1] <= 0


def area(c):
    return (c[2] - c[0]) * (c[3] - c[1])


def inter(a, b):
    w = min(a[2], b[2]) - max(a[0], b[0])
    h = min(a[3], b[3]) - max(a[1], b[1])
    return 0 if w <= 0 or h <= 0 else w * h


def iou_ge(i, u, t):
    return i > 0 and float(i) >= float(t) * float(u)


def before(p, q):
    """p, q = (inter, uni, slot, det): the strict order of item 3, exact in Python integers."""
    l, r = p[0] * q[1], q[0] * p[1]
    if l != r:
        return l > r
    if p[2] != q[2]:
        return p[2] < q[2]
    return p[3] < q[3]


def _wrap32(v):
    return (int(v) + 2 ** 31) % 2 ** 32 - 2 ** 31


def associate(det, n_det, m_crop, boxes, status, misses, state, in_h, in_w, fh, fw, match_iou=0.3, dup_iou=0.7,
              refresh_iou=0.0, max_misses=0, square=True):
    """-> dict of the eight tensors after the call; the inputs are not changed.  det int32 [D,4], n_det None or an int,
    state None or float64 [K,C,6]."""
    det = np.asarray(det, np.int32).reshape(-1, 4)
    d, k = len(det), len(boxes)
    m_crop = np.array(m_crop, np.float32).reshape(k, 2, 3).copy()
    boxes = np.array(boxes, np.int32).reshape(k, 4).copy()
    status = np.array(status, np.int32).copy()
    misses = np.array(misses, np.int32).copy()
    state = None if state is None else np.array(state, np.float64).copy()
    det_slot = np.full(d, -1, np.int32)
    slot_det = np.full(k, -1, np.int32)
    cnt = dict.fromkeys(COUNTS, 0)
    nd = d if n_det is None else min(max(int(n_det), 0), d)

    # 2. the detections
    dbox, dclip = [None] * d, [None] * d            # None = void or unread
    for j in range(nd):
        b = [int(v) for v in det[j]]
        if any(v < -LIM or v > LIM for v in b):
            cnt["void"] += 1
            continue
        if square:
            b = square_box(b)
        c = clip(b, fh, fw)
        if empty(c):
            cnt["void"] += 1
            continue
        dbox[j], dclip[j] = b, c
    # 4. the slots
    tclip = [clip(boxes[t], fh, fw) for t in range(k)]
    live = [not empty(c) for c in tclip]

    def kill(t, bit):
        boxes[t] = 0
        m_crop[t] = track_ref.IDENTITY
        status[t] |= bit
        misses[t] = 0

    def restart(t, j):
        m, st = track_ref.seed([dbox[j]], in_h, in_w, fh, fw)
        m_crop[t], status[t], boxes[t], misses[t] = m[0], st[0], dbox[j], 0
        if state is not None:
            state[t] = -1.0

    # 5. duplicates
    dup = [False] * k
    for t in range(k):
        if not live[t]:
            continue
        for s in range(t):
            if live[s]:
                i = inter(tclip[s], tclip[t])
                if iou_ge(i, area(tclip[s]) + area(tclip[t]) - i, dup_iou):
                    dup[t] = True
                    break
    surv = [live[t] and not dup[t] for t in range(k)]
    # 6. greedy matching: the pairs in order; a pair is taken when its slot and its detection are both still there --
    # which is "take the first pair, remove its slot and its detection, repeat"
    pairs = []
    for t in range(k):
        if not surv[t]:
            continue
        at = area(tclip[t])
        for j in range(nd):
            if dclip[j] is None:
                continue
            i = inter(tclip[t], dclip[j])
            if i == 0:
                continue
            u = at + area(dclip[j]) - i
            if iou_ge(i, u, match_iou):
                pairs.append((i, u, t, j))
    pairs.sort(key=functools.cmp_to_key(lambda p, q: -1 if before(p, q) else 1))
    match = {}
    taken = set()
    for i, u, t, j in pairs:
        if t in match or j in taken:
            continue
        match[t] = (j, i, u)
        taken.add(j)
    # 5, 7, 8: the slots that were live
    for t in range(k):
        if dup[t]:
            kill(t, DUPLICATE)
            cnt["duplicates"] += 1
        elif t in match:
            j, i, u = match[t]
            slot_det[t], det_slot[j] = j, t
            cnt["matched"] += 1
            if refresh_iou > 0 and not iou_ge(i, u, refresh_iou):
                restart(t, j)
                cnt["refreshed"] += 1
            else:
                misses[t] = 0
        elif surv[t]:
            misses[t] = _wrap32(int(misses[t]) + 1)
            if max_misses > 0 and misses[t] >= max_misses:
                kill(t, UNCONFIRMED)
                cnt["unconfirmed"] += 1
    # 9. births
    free = [t for t in range(k) if not live[t]]
    for j in range(nd):
        if dclip[j] is None or j in taken:
            continue
        if free:
            t = free.pop(0)
            restart(t, j)
            slot_det[t], det_slot[j] = j, t
            cnt["born"] += 1
        else:
            det_slot[j] = -2
            cnt["dropped"] += 1
    counts = np.array([cnt[n] for n in COUNTS], np.int32)
    return dict(m_crop=m_crop, boxes=boxes, status=status, misses=misses, state=state, det_slot=det_slot,
                slot_det=slot_det, counts=counts)
