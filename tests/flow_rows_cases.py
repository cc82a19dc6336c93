"""The cases tests/test_flow_rows_native_host.py and tests/test_gpu_flow_rows.py run against tests/flow_rows_ref.py: rows of
crop pairs with their matrices and slot map over a history store, for flm_landmark_flow_rows; states and streams for
flm_track_gather_flow; rows and stores for flm_track_flow_history_put.  Every case is built from a seed; the reference
answer of a case is computed once (`expected`, `gather_expected`, `put_expected`) and shared."""
import functools

import numpy as np

import flow_cases
import flow_ref
import flow_rows_ref


def make(name, n, n_slots, slot, max_fb, **kw):
    """A case of tests/flow_cases.py with n faces turned into rows: face r is row r, its previous landmarks (and weights)
    lie at slot[r] of a store of n_slots entries whose other entries hold valid points of their own -- a kernel that reads
    the store at the row, or at another row's slot, gets another answer.  slot[r] < 0: the row is inert."""
    c = flow_cases.make(name, n, **kw)
    rng = np.random.default_rng(kw["seed"] + 1000)
    h, w = c["hw"]
    cc = c["lm"].shape[1]
    store = np.stack([rng.uniform(8.0, min(h, w) - 9.0, (cc, 2)) for _ in range(n_slots)])
    wstore = rng.uniform(0.05, 1.0, (n_slots, cc)) if c["w"] is not None else None
    slot = np.asarray(slot, np.int32)
    assert len(slot) == n and len(set(v for v in slot if v >= 0)) == (slot >= 0).sum() and slot.max() < n_slots
    for r, g in enumerate(slot):
        if g >= 0:
            store[g] = c["lm"][r]
            if wstore is not None:
                wstore[g] = c["w"][r]
    c.update(slot=slot, lm=np.ascontiguousarray(store), w=wstore, max_fb=float(max_fb), n_slots=n_slots)
    return c


def occlusion(name, seed, other, max_fb=1.0, shift=(1.25, -0.75)):
    """The case only the backward pass can judge: `cur` is `prev` shifted, with its upper left quadrant replaced by the
    texture of another seed, and max_err opened to 255 -- the forward pass accepts points there."""
    c = make(name, 1, 4, [2], max_fb, c=68, h=64, w=64, ch=1, levels=3, radius=7, seed=seed, shift=shift, rejected=False,
             max_err=255.0)
    cur = c["cur"].copy()
    cur[0, :32, :32] = flow_ref.shifted(flow_ref.texture(64, 64, other), 0.0, 0.0)[:32, :32]
    c["cur"] = np.ascontiguousarray(cur)
    return c


OCCLUSION = 6       # the index of the occlusion case below


@functools.lru_cache(maxsize=None)
def cases():
    rot = lambda f: flow_cases._rot(7.0 + 3 * f, 0.5 + 0.05 * f, 9.0 - f, 4.0 + 2 * f)
    return (
        make("n1_c5_over_4_slots", 1, 4, [2], 0.0, c=5, h=64, w=64, ch=1, levels=3, radius=7, seed=11),
        make("n3_c68_permuted_bgr_weights_fb", 3, 6, [4, 0, 3], 1.0, c=68, h=64, w=64, ch=3, levels=3, radius=7, seed=12,
             weights=True, zero=1),
        make("n9_c68_r3_inert_rows_fb", 9, 12, [7, 2, -1, 11, 0, 5, 9, 3, -1], 0.5, c=68, h=64, w=64, ch=1, levels=3,
             radius=3, seed=13, shift=(3.3, -2.6), zero=4, coarse_flat=7),
        make("n3_c5_32x48_two_levels_fb", 3, 4, [3, 1, 0], 1.0, c=5, h=32, w=48, ch=3, levels=2, radius=7, seed=14,
             shift=(-0.5, 1.0)),
        make("n3_c68_rotated_weights_off", 3, 5, [1, 4, 2], 0.0, c=68, h=64, w=64, ch=1, levels=3, radius=7, seed=15, m=rot,
             weights=True),
        make("n2_c5_r3_tight_fb", 2, 4, [0, 3], 0.25, c=5, h=64, w=64, ch=1, levels=3, radius=3, seed=16,
             shift=(3.3, -2.6), max_move=6.0, min_eig=0.0),
        occlusion("n1_c68_occluded_quadrant", 17, 170),
    )


@functools.lru_cache(maxsize=None)
def expected(i):
    """(lm, w, err, fb, flags) of case i by flow_rows_ref, computed once."""
    c = cases()[i]
    return flow_rows_ref.landmark_flow_rows(c["prev"], c["cur"], c["slot"], c["lm"], c["m"], c["opts"], c["max_fb"], c["w"])


def occlusion_holds():
    """The condition of the occlusion case, on the reference alone: at least 5 points carry FLOW_FB and no other flag, and
    at least 5 points of the shifted part pass with fb2 below max_fb^2.  Returns (points with FB alone, points of the
    shifted part that pass)."""
    c = cases()[OCCLUSION]
    lm, _, _, fb, flags = expected(OCCLUSION)
    start = c["lm"][c["slot"][0]]                       # identity matrix: frame px are crop px
    moved = ~((start[:, 0] < 32 + 8) & (start[:, 1] < 32 + 8))     # clear of the replaced quadrant by a window's radius
    only_fb = int((flags[0] == flow_rows_ref.FB).sum())
    passed = int(((flags[0] == 0) & moved & (fb[0] >= 0.0) & (fb[0] < c["max_fb"] ** 2)).sum())
    return only_fb, passed


# ---- flm_track_gather_flow ------------------------------------------------------------------------------------------------
def _gather(name, s, k, n, seed, live, ready, on=None, cursor=0, age=None, dt=None, dt_stream=None, best=True, reset=True,
            frames=True):
    """live, ready: 0/1 lists over the s*k slots."""
    rng = np.random.default_rng(seed)
    ns = s * k
    boxes = np.zeros((ns, 4), np.int32)
    for g in range(ns):
        if live[g]:
            x0, y0 = rng.integers(0, 1500), rng.integers(0, 800)
            boxes[g] = (x0, y0, x0 + rng.integers(40, 300), y0 + rng.integers(40, 200))
        elif g % 3 == 0:
            boxes[g] = (2000, 50, 2100, 150)        # not empty as numbers, empty once clipped to the frame
    a = dict(name=name, s=s, k=k, fh=1080, fw=1920, n=n, dt=0.0 if dt is None else dt,
             m_crop=rng.standard_normal((ns, 2, 3)).astype(np.float32), boxes=boxes,
             flow_frame=rng.integers(0, 7, ns).astype(np.int32), flow_ready=(np.asarray(ready, np.int32) * (1 + np.arange(ns) % 2)).astype(np.int32),
             stream_on=None if on is None else np.asarray(on, np.int32),
             frame_idx_stream=rng.integers(0, 7, s).astype(np.int32) if frames else None,
             dt_stream=None if dt_stream is None else np.asarray(dt_stream, np.float64),
             best_q=rng.uniform(0, 1, ns) if best else None, reset=rng.integers(0, 2, ns).astype(np.int32) if reset else None,
             age=None if age is None else np.asarray(age, np.float64),
             cursor=None if cursor is None else np.asarray([cursor], np.int32))
    return a


@functools.lru_cache(maxsize=None)
def gather_cases():
    nan = float("nan")
    all8 = [1] * 8
    return (
        _gather("all_served", 2, 4, 8, 21, [1, 1, 0, 1, 0, 1, 1, 0], [1, 1, 1, 0, 1, 1, 0, 0], age=[0.0] * 8, dt=0.04),
        _gather("wrap_around_e_over_n", 2, 4, 3, 22, all8, [1, 1, 1, 1, 0, 1, 1, 1], cursor=6, age=np.arange(8) * 0.01, dt=0.04),
        _gather("last_row_is_last_slot", 2, 4, 2, 23, all8, [0, 1, 0, 0, 0, 0, 1, 1], cursor=6, age=[0.0] * 8,
                dt_stream=[0.04, 0.02]),
        _gather("off_stream", 3, 3, 4, 24, [1] * 9, [1] * 9, on=[1, 0, 2], cursor=2, age=np.arange(9) * 0.5, dt_stream=[0.1, 0.2, 0.3]),
        _gather("nan_ages_and_bad_dt", 2, 4, 2, 25, all8, [1, 0, 1, 1, 1, 1, 0, 1], cursor=1,
                age=[nan, 0.5, 0.25, nan, 1.0, 0.0, nan, 2.0], dt_stream=[0.04, -1.0]),
        _gather("no_optional_groups", 1, 5, 3, 26, [1, 0, 1, 1, 1], [1, 1, 0, 1, 1], cursor=None, best=False, reset=False,
                frames=False),
        _gather("cursor_outside", 2, 2, 1, 27, [1, 1, 1, 1], [1, 1, 1, 1], cursor=9, age=[0.0] * 4, dt=0.04),
        _gather("nobody_has_history", 1, 4, 4, 28, [1, 1, 0, 1], [0, 0, 0, 0], age=[0.0, 1.0, 3.0, nan], dt=0.04),
        _gather("more_than_one_chunk", 70, 16, 64, 29, list(np.random.default_rng(290).integers(0, 2, 1120)),
                list(np.random.default_rng(291).integers(0, 2, 1120)), cursor=1100, age=np.zeros(1120), dt=0.04,
                on=list(np.random.default_rng(292).integers(0, 2, 70))),
    )


@functools.lru_cache(maxsize=None)
def gather_expected(i):
    return flow_rows_ref.gather_flow(gather_cases()[i])


# ---- flm_track_flow_history_put ---------------------------------------------------------------------------------------------
def _put(name, n, n_slots, c, seed, slot, status, lm=True, w=True):
    rng = np.random.default_rng(seed)
    return dict(name=name, slot=np.asarray(slot, np.int32), status_rows=np.asarray(status, np.int32),
                frame_idx_c=rng.integers(0, 9, n).astype(np.int32), lm_rows=rng.uniform(-1, 1900, (n, c, 2)) if lm else None,
                w_rows=rng.uniform(0, 1, (n, c)) if lm and w else None, hist_lm=rng.uniform(0, 1900, (n_slots, c, 2)) if lm else None,
                hist_w=rng.uniform(0, 1, (n_slots, c)) if lm and w else None, flow_frame=rng.integers(0, 9, n_slots).astype(np.int32),
                flow_ready=rng.integers(0, 2, n_slots).astype(np.int32), c=c)


@functools.lru_cache(maxsize=None)
def put_cases():
    return (
        _put("rows_to_slots", 5, 8, 68, 31, [6, -1, 0, 3, 7], [0, 0, 4, 0, 1]),
        _put("no_weights", 3, 4, 5, 32, [2, 1, -1], [0, 64, 0], w=False),
        _put("flags_alone_slot_is_row", 6, 7, 1, 33, list(range(6)), [0, 1, 0, 0, 2, 0], lm=False),
        _put("slot_past_the_store_is_inert", 2, 3, 70, 34, [3, 1], [0, 0]),
    )


@functools.lru_cache(maxsize=None)
def put_expected(i):
    a = put_cases()[i]
    return flow_rows_ref.history_put(a["slot"], a["status_rows"], a["frame_idx_c"], a["flow_frame"], a["flow_ready"],
                                     a["lm_rows"], a["hist_lm"], a["w_rows"], a["hist_w"])
