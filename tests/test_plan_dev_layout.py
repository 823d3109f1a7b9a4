"""The host arithmetic of the device planner without a device: scan_levels, sort_shape, the three workspace layouts and the quote of
csrc/avr_plan_dev.h, in a stand-alone program (tests/plan_dev_layout_check.cpp) built by g++ under AddressSanitizer and UBSan and
started as a child process.  It covers every n in 0..5000, every n within two of a power of two up to 2^31, and 2^31 - 1 -- the
three-level scan (n > 2^30) among them, which no GPU test of seconds can run.  Nothing sanitised is loaded into this process and
nothing is preloaded into that one."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "avrecode-ms_amd", "csrc")
CHECK_SRC = os.path.join(ROOT, "tests", "plan_dev_layout_check.cpp")
CHECK_BIN = os.path.join(ROOT, "tests", "_plan_dev_layout_check")
DEPS = [os.path.join(CSRC, h) for h in ("avr_plan_dev.h", "avr_layout.h", "avr_k1p.h", "avr_chunk.h")] + [os.path.join(ROOT, "include", "avrecode_ms_amd.h")]


def _stale(target, sources):
    return not os.path.exists(target) or any(os.path.getmtime(s) > os.path.getmtime(target) for s in sources)


def test_the_sanitized_stand_alone_program():
    if _stale(CHECK_BIN, [CHECK_SRC] + DEPS):
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + CSRC,
                        "-o", CHECK_BIN, CHECK_SRC], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0")
    r = subprocess.run([CHECK_BIN], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.split() == ["ok", str(5001 + 5 * len(range(13, 32))), "cases"]      # 0..5000, then 2^13 .. 2^31, five around each
