"""What the command line does when a verify switch finds a fault: the cases and their expected ends, for
tests/test_cli_verify_faults.py (the CPU stand-in, tests/cpu_batch.cpp, under sanitizers) and tests/test_gpu_cli_verify_faults.py (the
product and the hooked test build of the command line, tests/recode_hooked.cpp, on the device).

A fault is one of the four fault points the device's test build has (csrc/avr_internal.h) and the stand-in repeats
(AVR_CPU_BATCH_FAULT): it addresses slice K - 1 of a BATCH.  What the README promises is about a FILE: `Verify error: ... (slice N,
bin M)` with N the index among the file's own coded slices, exit status 1, nothing written -- and in `recode test <dir>`, where the
files of a window share a batch, only the owning file lost.

The expected bin is worked out here, from the oracle alone: the stand-in's AVR_CPU_BATCH_DUMP gives what a sound run handed to the
coder and what came back (records or codes, coded bytes, expectations), the byte is flipped here and decoded here."""
import os
import shutil
import struct
import subprocess

import numpy as np

import cpu_recode
import oracle_lib
import restore_ref
import verify_streams

ROOT = cpu_recode.ROOT
VERIFY_NONE = 0xFFFFFFFF
KIND_RANGE, KIND_CODES, KIND_KEYS = 1, 2, 4
SWITCHES = ("AVR_DEVICE_ESTIMATORS", "AVR_VERIFY", "AVR_VERIFY_RESTORE")

# The README's sentence for each check, the switches that turn the check on, the command that runs it on one file (every one of them
# also through `roundtrip` and `test <dir>`), the fault point, and the `[timing]` lines the README names for the switch.
KINDS = {
    "k2": dict(sentence="Verify error: recoded block does not decode to its bins (slice %d, bin %d)", env={"AVR_VERIFY": "1"},
               command="compress", point="verify_flip"),
    "est": dict(sentence="Verify error: resolved estimators do not follow the model (slice %d, bin %d)",
                env={"AVR_DEVICE_ESTIMATORS": "1", "AVR_VERIFY": "1"}, command="compress", point="est_flip"),
    "k1": dict(sentence="Verify error: coded slice does not decode to its bins (slice %d, bin %d)", env={"AVR_VERIFY_K1": "1"},
               command="decompress", point="verify_flip"),
    "restore": dict(sentence="Verify error: coded slice does not restore its payload (slice %d, byte %d)", env={"AVR_VERIFY_RESTORE": "1"},
                    command="compress", point="restore_flip"),
}
TIMING_LINES = {"AVR_VERIFY": ("compress: GPU verify (a5)",), "AVR_VERIFY_RESTORE": ("compress: GPU restore check (K1)", "compress: restore check kernel"),
                "AVR_VERIFY_K1": ("decompress: GPU verify (K1)",)}
EST_TIMING_LINE = "compress: GPU verify estimators"      # AVR_VERIFY and AVR_DEVICE_ESTIMATORS both on (and the residual hooks off)
EXCEPTION = "Exception (St13runtime_error): "


def switch_subsets():
    return [tuple(s for k, s in enumerate(SWITCHES) if m >> k & 1) for m in range(8)]


# ------------------------------------------------------------------------------------------------ builds
def build_tsan(directory):
    """The stand-in command line under ThreadSanitizer: a stand-alone program, nothing preloaded."""
    return cpu_recode._compile(os.path.join(str(directory), "recode_cpu_tsan"), ["-O1", "-g", "-fsanitize=thread"],
                               [os.path.join(cpu_recode.CSRC, "host", "recode_main.cpp"), os.path.join(ROOT, "tests", "cpu_batch.cpp")])


def build_hooked(avr):
    """tests/recode_hooked.cpp against libavrecode_hip_hooks.so, kept beside the tests (tests/_recode_hooked, not in git) and rebuilt
    when a source is newer.  The product's own command line (avr.build_recode) is another program and has no hooks."""
    import pytest
    out = os.path.join(ROOT, "tests", "_recode_hooked")
    host = os.path.join(cpu_recode.CSRC, "host")
    deps = [os.path.join(host, f) for f in os.listdir(host)] + [avr.HEADER_PATH, avr.HOOKS_LIB_PATH, os.path.join(ROOT, "tests", "recode_hooked.cpp")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        cxx = shutil.which("g++")
        if not cxx:
            pytest.skip("no g++")
        package = os.path.dirname(avr.HOOKS_LIB_PATH)
        subprocess.run([cxx, "-O2", "-pthread", "-std=c++17", "-w", "-I" + cpu_recode.CSRC, "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__", "-o", out + ".tmp",
                        os.path.join(ROOT, "tests", "recode_hooked.cpp"), "-L" + package, "-lavrecode_hip_hooks",
                        "-Wl,-rpath,$ORIGIN/../" + os.path.basename(package)], check=True)
        os.replace(out + ".tmp", out)
    return out


# ------------------------------------------------------------------------------------------------ what a sound run codes
def read_dump(path):
    """AVR_CPU_BATCH_DUMP's file: [(kind, [slice])], a slice being dict(status, data = its records (uint16) or codes (uint8), out =
    its coded bytes, expect = its expectation or None)."""
    with open(str(path), "rb") as f:
        raw = f.read()
    at, batches = 0, []

    def u32():
        nonlocal at
        at += 4
        return struct.unpack_from("<I", raw, at - 4)[0]

    def take(n):
        nonlocal at
        at += n
        return raw[at - n:at]
    while at < len(raw):
        assert u32() == 0x42525641
        kind, n = u32(), u32()
        slices = []
        for _ in range(n):
            status, count = u32(), u32()
            data = np.frombuffer(take(count), np.uint8) if kind == KIND_CODES else np.frombuffer(take(2 * count), np.uint16)
            out = take(u32())
            e = u32()
            slices.append(dict(status=status, data=data, out=out, expect=None if e == VERIFY_NONE else take(e)))
        batches.append((kind, slices))
    return batches


class Sound:
    """One clip through the stand-in with no switch (and once with the restore check, for its batch): the container, and per check the
    slices of the batch it looks at.  k2 / est: the K2 batch of compress (range records; with AVR_DEVICE_ESTIMATORS=1 the resolver
    gives these very records -- the .recode bytes are the same either way); restore: the restore batch; k1: the K1 batch of decompress."""

    def __init__(self, exe, work, clip, model_hooks=0):
        self.clip, self.model_hooks = clip, model_hooks
        src = os.path.join(cpu_recode.GOLDEN, clip + ".mp4")
        tag = "%s.%d" % (clip, model_hooks)
        self.path, dump_c, dump_d = work / (tag + ".recode"), work / (tag + ".compress.dump"), work / (tag + ".decompress.dump")
        c = cpu_recode.run(exe, "compress", src, self.path, model_hooks, env={"AVR_CPU_BATCH_DUMP": str(dump_c), "AVR_VERIFY_RESTORE": "1"})
        assert c.status == 0, c.stderr[-2000:]
        d = cpu_recode.run(exe, "decompress", self.path, work / (tag + ".back"), model_hooks, env={"AVR_CPU_BATCH_DUMP": str(dump_d)})
        assert d.status == 0 and (work / (tag + ".back")).read_bytes() == cpu_recode.golden(clip), d.stderr[-2000:]
        self.container = self.path.read_bytes()
        (k2_kind, k2), (r_kind, restore) = read_dump(dump_c)
        ((k1_kind, k1),) = read_dump(dump_d)
        assert (k2_kind, r_kind, k1_kind) == (KIND_RANGE, KIND_CODES, KIND_CODES) and len(k2) == len(restore) == len(k1)
        assert all(s["status"] == 0 for s in k2 + restore + k1)
        self.slices = {"k2": k2, "est": k2, "restore": restore, "k1": k1}
        self.n = len(k2)

    def places(self, kind):
        """The first, a middle and the last of the file's coded slices with coded bytes (and, for est, bins)."""
        usable = [j for j, s in enumerate(self.slices[kind]) if len(s["out"]) > 0 and s["data"].size > 0]
        assert len(usable) >= 3
        return usable[0], usable[len(usable) // 2], usable[-1]

    def est_bin(self, j):
        """Which bin of slice j est_flip bumps: not always the first, never past the end."""
        return min(int(self.slices["est"][j]["data"].size) - 1, 7 * j + 1)

    def expected(self, kind, j):
        """The M of the message for a fault at the file's slice j, from the oracle: None where the check would find nothing."""
        oracle = oracle_lib.load_oracle()
        s = self.slices[kind][j]
        if kind == "est":
            return self.est_bin(j)
        flipped = bytes([s["out"][0] ^ 0x80]) + s["out"][1:]
        if kind == "k2":
            m = verify_streams.first_bad(oracle, flipped, s["data"])
        elif kind == "k1":
            m = first_bad_codes(oracle, flipped, s["data"])
        else:
            m = restore_ref.first_diff(oracle, flipped, s["expect"])
        return None if m == VERIFY_NONE else m

    def message(self, kind, j):
        m = self.expected(kind, j)
        assert m is not None, "the flipped byte of slice %d is not found by the oracle's decoder: choose another slice" % j
        return EXCEPTION + KINDS[kind]["sentence"] % (j, m)


def first_bad_codes(oracle, data, codes):
    """Index of the first bin oracle/spec_cabac.c's decoder (H.264 9.3.3.2, from resolved codes) decodes differently from the codes."""
    import ctypes
    codes = np.ascontiguousarray(codes, np.uint8)
    buf = np.frombuffer(bytes(data) + b"\0", np.uint8).copy()
    bins = np.zeros(codes.size, np.uint8)
    rc = oracle.L.avr_spec_cabac_decode_codes(oracle_lib.ptr(buf), ctypes.c_size_t(len(data)), oracle_lib.ptr(codes), ctypes.c_size_t(codes.size), oracle_lib.ptr(bins))
    assert rc == 0
    diff = np.nonzero(bins != (codes & 1))[0]
    return int(diff[0]) if diff.size else VERIFY_NONE


# ------------------------------------------------------------------------------------------------ a fault, for either build
def fault_env(kind, k, est_bin=0, hooked=False, more_hooks=None, both=False):
    """The environment of a run with kind's switches on and its fault point aimed at batch slice k - 1.  hooked: for
    tests/recode_hooked.cpp (AVR_TEST_HOOKS_SET), else for the stand-in (AVR_CPU_BATCH_FAULT).  both: verify_flip beside est_flip."""
    point = KINDS[kind]["point"]
    pairs = ["%s=%d" % (point, k)]
    if point == "est_flip":
        pairs.append("est_flip_bin=%d" % est_bin)
        if both:
            pairs.append("verify_flip=%d" % k)
    pairs += ["%s=%d" % kv for kv in (more_hooks or {}).items()]
    env = dict(KINDS[kind]["env"])
    env["AVR_TEST_HOOKS_SET" if hooked else "AVR_CPU_BATCH_FAULT"] = ",".join(pairs)
    return env


def without_switches(env):
    return {k: v for k, v in env.items() if not k.startswith("AVR_VERIFY") and k != "AVR_DEVICE_ESTIMATORS"}


# ------------------------------------------------------------------------------------------------ recode test <dir>
COPIES = ("a.mp4", "b.mp4", "c.mp4", "d.mp4", "e.mp4")


def make_directory(path, clip="realshort"):
    os.makedirs(str(path))
    for name in COPIES:
        shutil.copyfile(os.path.join(cpu_recode.GOLDEN, clip + ".mp4"), os.path.join(str(path), name))
    return path


def owners(k, window, slices_per_file, n_files=len(COPIES)):
    """Which files a fault at batch slice k - 1 hits, and at which of their own slices: every window has a batch of its own, its files'
    slices one after the other.  {file index: file-local slice index}."""
    hit = {}
    for base in range(0, n_files, window):
        files = min(window, n_files - base)
        if 1 <= k <= files * slices_per_file:
            hit[base + (k - 1) // slices_per_file] = (k - 1) % slices_per_file
    return hit


def run_test(exe, directory, env):
    """`recode test <dir>`: (status, stdout, stderr, the log's text per file, the rows of metrics.csv, {name: bytes} of output/)."""
    e = dict(os.environ, AVR_MODEL_HOOKS="0", ASAN_OPTIONS="detect_leaks=0:abort_on_error=0")
    for k in ("AVR_VERIFY", "AVR_VERIFY_K1", "AVR_VERIFY_RESTORE", "AVR_DEVICE_ESTIMATORS", "AVR_TIMING", "AVR_TEST_WINDOW", "AVR_TEST_SEQUENTIAL"):
        e.pop(k, None)
    e.update(env)
    p = subprocess.run([exe, "test", str(directory)], capture_output=True, env=e, timeout=cpu_recode.TIMEOUT)
    out = os.path.join(str(directory), "output")
    with open(os.path.join(out, "log.txt")) as f:
        log = f.read()
    per_file = ["Input #" + t for t in log.split("Input #")[1:]]
    with open(os.path.join(out, "metrics.csv")) as f:
        rows = [l for l in f.read().splitlines()[1:] if l]
    files = {}
    for name in COPIES:
        if os.path.exists(os.path.join(out, name)):
            with open(os.path.join(out, name), "rb") as f:
                files[name] = f.read()
    return p.returncode, p.stdout.decode("utf-8", "replace"), p.stderr.decode("utf-8", "replace"), per_file, rows, files


def exception_lines(text):
    return [l for l in text.splitlines() if l.startswith("Exception (")]
