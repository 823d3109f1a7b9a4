"""The `recode` command line on the CPU stand-in for the batch calls (tests/cpu_batch.cpp, coded by oracle/): how the tests
build it and start it.  Stand-alone programs started as child processes, nothing preloaded."""
import collections
import hashlib
import os
import shutil
import subprocess
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "avrecode-ms_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden")
SANITIZE = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
TIMEOUT = 120                                            # a hang detector, not a measurement: the short clip takes a fraction of a second


def _compile(out, flags, sources):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++")
    # the oracle is C: -x c behind the C++ sources (the driver warns that -std=c++17 is not for C; nothing else)
    cmd = [cxx] + flags + ["-pthread", "-std=c++17", "-w", "-I" + CSRC, "-o", out] + sources + \
          ["-x", "c", os.path.join(ROOT, "oracle", "avr_oracle.c"), os.path.join(ROOT, "oracle", "spec_cabac.c")]
    subprocess.run(cmd, check=True)
    return out


def build(directory, sanitize):
    """recode_main.cpp + the stand-in + the oracle: a CLI that runs both directions without a GPU."""
    return _compile(os.path.join(str(directory), "recode_cpu_asan" if sanitize else "recode_cpu"), SANITIZE if sanitize else ["-O2"],
                    [os.path.join(CSRC, "host", "recode_main.cpp"), os.path.join(ROOT, "tests", "cpu_batch.cpp")])


def build_cached():
    """The plain stand-in CLI kept beside the tests (tests/_recode_cpu, not in git), rebuilt when a source is newer: for the GPU
    tests, which compare the product with it and have no use for a build per session."""
    out = os.path.join(ROOT, "tests", "_recode_cpu")
    host = os.path.join(CSRC, "host")
    deps = [os.path.join(host, f) for f in os.listdir(host)] + [os.path.join(ROOT, "include", "avrecode_ms_amd.h"), os.path.join(ROOT, "tests", "cpu_batch.cpp"), os.path.join(ROOT, "tests", "est_plain.cpp")]
    deps += [os.path.join(ROOT, "oracle", f) for f in ("avr_oracle.c", "avr_oracle.h", "avr_oracle_coder.inc", "avr_oracle_tables.h", "spec_cabac.c")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        _compile(out + ".tmp", ["-O2"], [os.path.join(host, "recode_main.cpp"), os.path.join(ROOT, "tests", "cpu_batch.cpp")])
        os.replace(out + ".tmp", out)
    return out


def build_program(directory, name, source, sanitize=True):
    """A stand-alone program of the tests (its own main) on the host headers and the stand-in."""
    return _compile(os.path.join(str(directory), name), SANITIZE if sanitize else ["-O2"], [source, os.path.join(ROOT, "tests", "cpu_batch.cpp")])


Outcome = collections.namedtuple("Outcome", "status messages stderr seconds pending")


def run(exe, command, src, dst, model_hooks, env=None, limit_address_space=None):
    """One child process.  status: the exit status (negative: ended by that signal); messages: the `Exception (` lines of stderr;
    pending: what the stand-in's avr_batch_run was given ("N slices, M bins"), None where the run did not get that far or the
    program is not the stand-in.  TimeoutExpired is the caller's to see."""
    e = dict(os.environ, AVR_MODEL_HOOKS=str(int(model_hooks)), AVR_CPU_BATCH_REPORT="1", ASAN_OPTIONS="detect_leaks=0:abort_on_error=0")
    for k in ("AVR_VERIFY", "AVR_VERIFY_K1", "AVR_VERIFY_RESTORE", "AVR_DEVICE_ESTIMATORS", "AVR_TIMING"):
        e.pop(k, None)
    e.update(env or {})
    limit = None
    if limit_address_space:
        def limit():
            import resource
            resource.setrlimit(resource.RLIMIT_AS, (limit_address_space, limit_address_space))
    t0 = time.perf_counter()
    p = subprocess.run([exe, command, str(src), str(dst)], capture_output=True, env=e, timeout=TIMEOUT, preexec_fn=limit)
    seconds = time.perf_counter() - t0
    stderr = p.stderr.decode("utf-8", "replace")
    lines = stderr.splitlines()
    pending = [l[len("[cpu_batch] "):] for l in lines if l.startswith("[cpu_batch] ")]
    return Outcome(p.returncode, [l for l in lines if l.startswith("Exception (")], stderr, seconds, pending[-1] if pending else None)


def digest(path):
    with open(str(path), "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def golden(name):
    with open(os.path.join(GOLDEN, name + ".mp4"), "rb") as f:
        return f.read()
