"""The reentrancy contract of include/flm.h on the device: "calls on different streams may run concurrently from different
threads", and a knob setter beside launches on other threads "takes effect between launches, never inside one".

Every concurrent call runs in a fresh child process (tests/reentrancy_child.py, started as tests/test_gpu_rccl.py starts
its child): a cold first call exists once per process, and a child that hangs is ended by its time limit without taking
the suite's process with it.  A child prints one JSON line; if one times out or dies on a signal, the remaining tests of
this module skip -- nothing more is started on the card after trouble.  The reference of every comparison is the same
call made serially, alone, on the default stream of the same child, with the knobs at their defaults; concurrent results
equal it BIT FOR BIT (arena.same_bits; no tolerance anywhere).  The values themselves are pinned by the other modules at
these shapes.  The host side of the same contract runs under ThreadSanitizer in tests/test_reentrancy_native_host.py.

Audit by reading, before the first run: every piece of state that outlives a call, and who may touch it.

    state                                   where                              who may touch it, and how it is kept safe
    knob table g_knobs[17]                  csrc/flm_api.hip                   any thread: std::atomic<int> each, relaxed store in
                                                                               flm_set_tuning, relaxed load in tuning(); a launcher
                                                                               loads a knob ONCE per launch into a local (read: every
                                                                               tuning(KNOB_*) site is a single load -- posmajor_rows_for,
                                                                               dispatch, launch_big, conv3_halo, score1x1, the tail,
                                                                               up3_wreg, the candidate launch (two knobs, one load each),
                                                                               launch_warp, use_dma, posmajor_fill_perm)
    error string g_err[512]                 csrc/flm_api.hip                   thread_local: the calling thread alone
    g_posperm_cache (<= 64 entries)         csrc/flm_igemm.hip                 any launching thread, under g_posperm_mu; entries are
                                                                               copied out under the lock; past the cap the search runs
                                                                               again every launch and gives the same table
    g_rows_cache (<= 256), g_rows_last      csrc/flm_igemm.hip                 under g_rows_mu (the occupancy queries included);
                                                                               g_rows_last is an atomic that only flm_debug_query reads
    FuncAttrOnce, ten function-local        flm_igemm, flm_igemm_bf16,         one bit per device, double-checked under the flag's own
    statics (one per kernel template        flm_conv3_halo, flm_convt (2),     mutex: hipFuncSetAttribute runs once, before the first
    instantiation)                          flm_decode (2), flm_decode_stats,  launch of that instantiation by any thread
                                            flm_tail_bf16, flm_up3_wreg
    g_prof* (the measurement hook)          csrc/flm_api.hip                   declared NOT thread-safe; off here (a null pointer that
                                                                               every forward reads and nobody writes)
    prediction._TEMPLATES                   prediction.py                      any thread: the tensor is complete before it enters the
                                                                               dict (a blocking upload), two first callers both upload
                                                                               and one entry stays; never freed
    Fcn8Model._ws                           networks/fcn.py                    any thread: keyed by (stream, call), under _ws_lock

No other file-static, counter or handle exists in csrc/ (the kernels' counters live in the caller's workspace or in LDS).

Result on an MI355X, unmodified kernels and launchers: all 8 tests pass -- in the C ABI no output, no named intermediate
(fc6, fc7, score5, fuse4, seg_feats), no guard byte and no input differs between the concurrent and the serial runs, cold
or warm, with the flipper making some 2 000 - 8 000 knob stores beside 192 worker calls and 6 144 burst decodes.  Nothing to
fix in a kernel or a launcher.  The one real finding is in the Python layer:

The shared-model tests on the parent commit's networks/fcn.py (workspaces cached by (n, out, decode, n_points, opts), no
stream in the key, no lock), run once: they FAIL.  Four threads at one batch size: 2 of the 12 calls return landmarks that
differ from the serial call in all 4352 coordinates.  Batch sizes in rotation: 8 of the 56 calls wrong in every coordinate
(136 - 4352 of them).  No thread, stream A then stream B: 4351 and 4350 of 4352 coordinates wrong -- both callers, every
time, since the second forward rewrites every intermediate under the first.  intermediate("fc6") after another stream's
forward: 249421 of 393216 elements are the other stream's.  align_frames from two threads: aligned 183225 of 188160
elements, all 30 matrix entries, all 680 landmark coordinates and all 340 weights wrong for caller 0, the same for caller 1.
Caller-owned workspaces: correct there too, as expected.  With the cache keyed by the current stream and guarded by a lock
all of these pass; the cap of four holds per stream (20 entries after four streams and the default one had their turn).

Fault injection (scratch builds, not committed; wrong values only -- no pointer, count, length or index touched).
 1. decode_run stores `thresh` in a file-static at entry and reads it back a few statements later, when it fills
    DecodeArgs.  NOT SEEN: 0 cases fail, also with the bursts (6 144 coinciding decodes with three reject levels).  Two
    entries into the library from Python threads are never closer than a hand-over of the interpreter lock plus the
    argument conversion (microseconds), so a window of some tens of nanoseconds inside one launcher cannot be hit from
    here.  That class belongs to the ThreadSanitizer program, which needs no coincidence: with posperm_cache_get reading
    the cache without its lock (values still right, "0 failures") it reports 14 data races on g_posperm_cache and exits 66.
 2. The same static read back AFTER decode_run's first launch, for the merge launch (a window of one kernel launch, the
    shape of a "current call" global).  SEEN: test_warm_mixed_work_beside_a_knob_flipper fails, at least 8 of its 24 burst
    checks (3 workers x 8 rounds), e.g. worker 0 round 0: 808 of 104448 output elements differ (it rejects nothing; it got
    other workers' levels in about five of its 256 calls), worker 1 round 2: 24336 of 104448.  Guards intact: values only.
So this module sees process state that lives across a launch or longer -- which is also the only kind the Python layer
itself can create (_ws, _TEMPLATES) --, and the host program sees the rest.
"""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = ("import sys; sys.path[:0] = [%r, %r]; import reentrancy_child; reentrancy_child.main(%%r)"
         % (ROOT, os.path.join(ROOT, "tests")))
CHILD_S = 120          # import and initialisation, packing two blobs, a few seconds of work

_trouble = []          # why a child was ended or died: the tests after it skip
_results = {}


def _child(part):
    """The result dict of one part, run once per session."""
    if part in _results:
        return _results[part]
    if _trouble:
        pytest.skip("an earlier child of this module %s: nothing more is started on the card" % _trouble[0])
    try:
        r = subprocess.run([sys.executable, "-c", CHILD % part], capture_output=True, text=True, timeout=CHILD_S)
    except subprocess.TimeoutExpired as e:
        _trouble.append("was ended after %d s (part %r)" % (CHILD_S, part))
        pytest.fail("the child of part %r was ended after %d s: %s" % (part, CHILD_S, (e.stderr or "")[-2000:]))
    if r.returncode < 0:
        _trouble.append("died on signal %d (part %r)" % (-r.returncode, part))
    elif r.returncode == 3:
        _trouble.append("had a thread that did not finish (part %r)" % part)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    assert r.returncode == 0 and len(lines) == 1, (part, r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    _results[part] = json.loads(lines[0][len("RESULT "):])
    print(part, {k: v if not isinstance(v, list) or len(v) < 8 else "%d entries" % len(v) for k, v in _results[part].items()})
    return _results[part]


def test_cold_first_calls_from_four_threads():
    """The first forward of the process by four threads at once: fp32 32 x 128 x 128 (the smallest shape with two positions
    per fc6 tile: every FuncAttrOnce of the fp32 path and posperm_cache_put raced cold on one key), then the four threads'
    first calls of 64 x 64 x 64 (the rows-per-tile model and its cache), of the bf16 model at 3 x 96 x 160, of flm_decode at
    68 landmarks (the LDS-DMA form and its FuncAttrOnce) and of flm_decode_stats.  Landmarks, fc6, fc7, score5, fuse4 and
    seg_feats of every caller equal the serial run made afterwards; guards intact, inputs unchanged."""
    res = _child("cold")
    assert not res["fails"], res["fails"]
    assert res["compared"] == 4 * (3 * 6 + 2) and res["distinct"]
    assert res["igemm_posmajor_rows"] in (64, 128)          # (information: the form the last fp32 fc6 launch took)


def test_warm_mixed_work_beside_a_knob_flipper():
    """Three workers, 8 rounds each.  A round opens with a burst that the three start together: 256 flm_decode calls back to
    back per worker, each into a slot of its own, each worker with its own reject level.  Then 7 different calls per worker --
    fp32 and bf16 forwards at 1 x 32 x 32 (split-K everywhere), 3 x 96 x 160 (ragged tiles) and 20 x 64 x 64 with probs, classmap,
    landmarks n = 4 and 25 (the candidate path, its counters in the caller's own workspace), landmark_stats and the overflow
    fallback (candidate_cap_div = 4096); flm_decode_sweep, flm_warp_affine_fmt, flm_crop_resize_frames, flm_face_quality,
    flm_track_step -- while a fourth thread cycles every bit-neutral knob through its legal values.  Every result of every
    round equals the serial, default-knob one; one worker makes an argument error every round and reads its own message."""
    res = _child("mixed")
    assert not res["fails"], res["fails"][:10]
    assert res["calls"] == res["rounds"] * res["jobs"] and res["flips"] >= 16
    assert len(set(res["rejected_per_worker"])) == 3, res["rejected_per_worker"]   # the reject levels really differ in effect


def test_shared_model_same_key_from_four_threads():
    """Four threads under their own streams share one model and call forward_device at one batch size (fp32 32 x 128 x 128,
    cached workspaces): the cache key without the stream is the same for all four."""
    res = _child("model")
    assert not res["fails"] and not res["same_key"], (res["fails"], res["same_key"][:6])


def test_shared_model_two_streams_one_thread():
    """No thread: the forward is enqueued on stream A and at once, without a sync, on stream B -- same key, other input."""
    res = _child("model")
    assert not res["two_streams"], res["two_streams"]
    assert not res["intermediate"], res["intermediate"]     # intermediate() reads the current stream's workspace


def test_shared_model_evictions_while_other_streams_run():
    """Batch sizes in rotation over more keys than _ws_cap, from four threads: workspaces are evicted while others run."""
    res = _child("model")
    assert not res["rotate"], res["rotate"][:6]
    assert res["cached_workspaces"] <= 5 * res["ws_cap"]    # the cap holds per stream (four here, and the default stream)


def test_caller_owned_workspaces_from_four_threads():
    """workspace=model.new_workspace(...) and out_tensor= per thread: independent of the cache."""
    res = _child("model")
    assert not res["caller_owned"], res["caller_owned"]


def test_align_frames_from_two_threads():
    """prediction.align_frames(weights="score") from two threads on two streams with the default template, whose upload
    into the module's _TEMPLATES is made by whichever thread comes first and read by both: all five returned tensors
    equal the serial call's."""
    res = _child("align")
    assert not res["fails"], res["fails"]
    assert res["faces"] == [5, 5]


def test_captured_pipelines_replayed_concurrently():
    """Two graphs.CapturedPipeline (1 and 5 faces), captured one after the other on the main thread, each replayed three
    times from its own thread on its own stream: landmarks, matrices and aligned crops equal the eager serial sequence.
    Replay only: nothing captures while another thread launches."""
    res = _child("graphs")
    assert not res["fails"], res["fails"]
    assert res["replays"] == 6
