"""One bin of the K2 coders at chosen ranges, against plain 64-bit integers (tests/k2_steps_cases.h): every record the ABI accepts
(pos, neg 0 .. 127) at about 130 ranges each -- the ends of every binade from 2^51 to 2^63 and the ranges at which range / total is
one unit from changing -- through range_step with avr_div.h's quotient, bin<true> from three values of low, one step of the
double-precision form, and chains of eight steps.  Here the host side of csrc/avr_div.h and csrc/avr_k2p.h runs them, as a stand-alone
program under the address and undefined-behaviour sanitizers; tests/test_gpu_k2_steps.py runs the device side on the GPU, and this
module proves that its program builds for gfx950 before anyone takes it there."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")
CSRC = os.path.join(ROOT, "avrecode-ms_amd", "csrc")
DEPS = [os.path.join(TESTS, f) for f in ("k2_steps_cases.h", "k2_steps_run.h")] + [os.path.join(CSRC, f) for f in ("avr_div.h", "avr_k2p.h", "avr_chunk.h")]
HOST_SRC, HOST_BIN = os.path.join(TESTS, "k2_steps_host.cpp"), os.path.join(TESTS, "_k2_steps_host")
DEV_SRC, DEV_BIN = os.path.join(TESTS, "k2_steps_dev.hip"), os.path.join(TESTS, "_k2_steps_dev")
CHECKS = 5


def stale(target, src):
    return not os.path.exists(target) or any(os.path.getmtime(d) > os.path.getmtime(target) for d in [src] + DEPS)


def build_dev():
    """tests/_k2_steps_dev with the library's own flags (build_native)."""
    if stale(DEV_BIN, DEV_SRC):
        hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
        subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wall", "-I" + CSRC, "-I" + TESTS, "-o", DEV_BIN + ".tmp", DEV_SRC], check=True)
        os.replace(DEV_BIN + ".tmp", DEV_BIN)
    return DEV_BIN


def verdict(stdout):
    """The program's report: ({check: (cases, mismatches)}, total mismatches)."""
    checks = {int(m[1]): (int(m[2]), int(m[3])) for m in re.finditer(r"^check (\d) [^:]*: (\d+) cases, (\d+) mismatches$", stdout, re.M)}
    total = re.search(r"^k2_steps: (\d+) mismatches$", stdout, re.M)
    assert total and sorted(checks) == list(range(1, CHECKS + 1)), stdout[-3000:]
    return checks, int(total[1])


def assert_clean(child):
    print(child.stdout)
    checks, total = verdict(child.stdout)
    assert child.returncode == 0 and total == 0 and all(bad == 0 for _, bad in checks.values()), child.stdout[-3000:] + child.stderr[-3000:]
    # 256 divisors; 32 766 records of a total above 0 at 133 ranges and the two of total 0 at 61; three lows a case; the chains
    cases = 32766 * 133 + 2 * 61
    assert [checks[k][0] for k in range(1, CHECKS + 1)] == [256, cases, 3 * cases, cases, 250000]


def test_host_side_is_exact_under_sanitizers():
    if stale(HOST_BIN, HOST_SRC):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + CSRC, "-I" + TESTS,
                        "-o", HOST_BIN + ".tmp", HOST_SRC], check=True)
        os.replace(HOST_BIN + ".tmp", HOST_BIN)
    assert_clean(subprocess.run([HOST_BIN], capture_output=True, text=True, timeout=600,
                                env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0")))


def test_device_program_builds_for_gfx950():
    assert os.path.getsize(build_dev()) > 0
