"""StreamPool<T> (csrc/avr_internal.h) -- what the library keeps per (device, stream): the renumbering's scratch, K2p's side stream
and events, the part streams -- from eight host threads at once: tests/stream_pool_check.cpp, a stand-alone program built once with
ThreadSanitizer and once with AddressSanitizer + UBSan and started as a child process (nothing sanitised is loaded into this process,
nothing is preloaded into that one).  The program defines hipGetDevice itself and links no HIP library; what it holds the pool to is
listed at its top.  It exits non-zero on any violated count; the sanitizers' reports are looked for in what it writes.

That the ThreadSanitizer build can report was shown once on a copy of the header with the lock_guard taken out of StreamPool::get:
ThreadSanitizer reports data races in get() (and the program counts lost writes and second makes)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "avrecode-ms_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "stream_pool_check.cpp")
ROUNDS = 4000
BUILDS = {"tsan": ["-fsanitize=thread"], "asan-ubsan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]}
REPORTS = ("ThreadSanitizer", "AddressSanitizer", "LeakSanitizer", "runtime error")


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_the_pool_from_eight_threads(tmp_path, build):
    program = str(tmp_path / ("stream_pool_" + build))
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-pthread"] + BUILDS[build] + ["-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + CSRC,
                    "-o", program, SRC], check=True)
    r = subprocess.run([program, str(ROUNDS)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert not any(word in r.stderr for word in REPORTS), r.stderr[-4000:]
    assert r.stdout.split() == ("8 threads, %d rounds: 0 violations" % ROUNDS).split(), r.stdout
