"""avr_multi (csrc/avr_multi.cpp) on the CPU stand-in for the batch calls: the layer that shards, held to one batch given the same calls.

tests/multi_check.cpp (its own main) is linked with csrc/avr_multi.cpp, tests/cpu_batch.cpp as it stands and the oracle, the way
tests/cpu_recode.py builds its sanitized programs, and run directly as a child process, nothing preloaded: once under ASan + UBSan and
once under ThreadSanitizer.  The program drives a multi over 1, 3 and 4 entries and one stand-in avr_batch with the same calls and
compares everything in the equivalence rule; with AVR_CPU_BATCH_FAULT set it holds the multi to one stand-in batch per entry (the
stand-in's fault points address each sub-batch's own slice K - 1, which the program finds among the caller's slices through
avr_multi_placement).  What it covers is listed at the top of the program.

Under ThreadSanitizer the multi runs as it ships, one host thread per entry: the stand-in showed no race of its own there."""
import os
import subprocess

import pytest

import cpu_recode

ROOT = cpu_recode.ROOT
SOURCES = [os.path.join(ROOT, "tests", "multi_check.cpp"), os.path.join(cpu_recode.CSRC, "avr_multi.cpp"), os.path.join(ROOT, "tests", "cpu_batch.cpp")]
FAULTS = ("verify_flip=2", "est_flip=2,est_flip_bin=5", "restore_flip=2", "verify_flip=1", "restore_flip=3")


@pytest.fixture(scope="module")
def asan(tmp_path_factory):
    return cpu_recode._compile(str(tmp_path_factory.mktemp("multi_asan") / "multi_check_asan"), cpu_recode.SANITIZE, SOURCES)


@pytest.fixture(scope="module")
def tsan(tmp_path_factory):
    return cpu_recode._compile(str(tmp_path_factory.mktemp("multi_tsan") / "multi_check_tsan"), ["-O1", "-g", "-fsanitize=thread"], SOURCES)


def run(exe, mode, fault=None):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", TSAN_OPTIONS="halt_on_error=1")
    env.pop("AVR_CPU_BATCH_FAULT", None)
    for k in ("AVR_CPU_BATCH_REPORT", "AVR_CPU_BATCH_DUMP"):
        env.pop(k, None)
    if fault:
        env["AVR_CPU_BATCH_FAULT"] = fault
    p = subprocess.run([exe, mode], capture_output=True, text=True, env=env, timeout=cpu_recode.TIMEOUT)
    assert p.returncode == 0 and p.stdout.startswith("multi_check ok: " + mode), p.stdout + p.stderr
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr
    return p.stdout


def test_the_multi_gives_what_one_batch_gives_under_asan_and_ubsan(asan):
    run(asan, "rule")


def test_the_multi_gives_what_one_batch_gives_under_tsan(tsan):
    run(tsan, "rule")


@pytest.mark.parametrize("fault", FAULTS)
def test_a_fault_hits_local_slice_k_of_every_entry_and_no_other(asan, fault):
    run(asan, "fault", fault)


def test_the_faults_under_tsan(tsan):
    for fault in FAULTS[:3]:
        run(tsan, "fault", fault)


def test_a_run_without_a_fault_point_named_is_refused(asan):
    """The fault mode must not pass for a sound run because a name was mistyped: the program wants one of the three, and the stand-in
    itself ends on an unknown name."""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    env.pop("AVR_CPU_BATCH_FAULT", None)
    assert subprocess.run([asan, "fault"], capture_output=True, env=env, timeout=cpu_recode.TIMEOUT).returncode == 1
    env["AVR_CPU_BATCH_FAULT"] = "verify_flop=2"
    assert subprocess.run([asan, "fault"], capture_output=True, env=env, timeout=cpu_recode.TIMEOUT).returncode != 0
