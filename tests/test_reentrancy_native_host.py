"""The host side of libflm_hip.so under ThreadSanitizer (CPU only, a stand-alone program: nothing is loaded into Python
and nothing is preloaded).  Every source is rebuilt with `-fsanitize=thread` into csrc/build_tsan/, by the recipe of
tests/test_abi_sanitized.py with the sanitizer swapped (device code is compiled as usual and never runs here: host-only
objects do not link, each refers to the fat binary its device pass would have made), and
tests/native/reentrancy_host.cpp is linked against that library.
The program runs eight threads through the position-permutation cache, the knob table and the thread-local error
string (see its header comment) and must exit 0, print "0 failures" and leave no ThreadSanitizer report.

Fault injection (a scratch build, not committed, run once): posperm_cache_get reading g_posperm_cache without its lock.
Every table still comes out right ("0 failures"), and ThreadSanitizer reports 14 data races between the unlocked read
and posperm_cache_put's push_back and ends the program with status 66: this test fails on the status and on the report."""
import importlib
import os
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=thread", "-fno-omit-frame-pointer", "-O1", "-g"]
HOST = ["-x", "hip", "--cuda-host-only"]   # the program itself: it has no kernel, only the launchers' host headers
PROGRAM = os.path.join(ROOT, "tests", "native", "reentrancy_host.cpp")


def _build():
    sys.path.insert(0, ROOT)
    bld = importlib.import_module("face-landmark-detector_amd.build")
    out = os.path.join(bld.CSRC, "build_tsan")
    os.makedirs(out, exist_ok=True)
    hipcc = bld._hipcc()
    srcs = [os.path.join(bld.CSRC, s) for s in bld.SOURCES]
    hdrs = [os.path.join(bld.CSRC, f) for f in os.listdir(bld.CSRC) if f.endswith(".h")] + \
           [os.path.join(bld.INCLUDE, "flm.h"), PROGRAM]
    stamp = bld._stamp(srcs + hdrs) + " ".join(SAN)
    exe = os.path.join(out, "reentrancy_host")
    sf = os.path.join(out, "stamp.txt")
    if os.path.exists(exe) and os.path.exists(sf) and open(sf).read() == stamp:
        return exe
    flags = [f for f in bld.FLAGS if f != "-O3"] + SAN

    def cc(src):
        obj = os.path.join(out, os.path.basename(src) + ".o")
        r = subprocess.run([hipcc, *flags, "-c", src, "-o", obj], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        return obj

    with ThreadPoolExecutor(max_workers=6) as ex:
        objs = list(ex.map(cc, srcs))
    lib = os.path.join(out, "libflm_hip_tsan.so")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", *SAN, "-o", lib, *objs], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([hipcc, *HOST, "--offload-arch=gfx950", *SAN, "-std=c++17", "-I", bld.INCLUDE, "-I", bld.CSRC, PROGRAM,
                        "-o", exe, "-L", out, "-lflm_hip_tsan", "-Wl,-rpath," + out, "-pthread"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    with open(sf, "w") as f:
        f.write(stamp)
    return exe


def test_host_state_is_race_free_under_thread_sanitizer():
    if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not available")
    exe = _build()
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=0:second_deadlock_stack=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert " 0 failures" in r.stdout and "ThreadSanitizer" not in r.stderr, (r.stdout[-2000:], r.stderr[-4000:])
