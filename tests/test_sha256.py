"""csrc/host/avr_sha256.h against hashlib.sha256: tests/sha256_check.cpp, a stand-alone program built with AddressSanitizer and
UBSan and started as a child process (nothing sanitised is loaded into this process, nothing is preloaded into that one).

The lengths are the ones at which the padding of FIPS 180-4 5.1.1 changes shape -- the empty message, one byte, 55 / 56 / 57 (the
length field just fits, just does not), 63 / 64 / 65 (a block's end), the same one block on (119, 120, 127, 128) -- and 1 000 003
bytes, many blocks and an odd rest.  Each is hashed in one update() call, once more by an object reset() after a message, and in
SPLITS seeded random splits of update()."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "avrecode-ms_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "sha256_check.cpp")
BIN = os.path.join(ROOT, "tests", "_sha256_check")
DEPS = [SRC, os.path.join(CSRC, "host", "avr_sha256.h")]
LENGTHS = (0, 1, 55, 56, 57, 63, 64, 65, 119, 120, 127, 128, 1000003)
SPLITS = 6


@pytest.fixture(scope="module")
def program():
    if not os.path.exists(BIN) or any(os.path.getmtime(s) > os.path.getmtime(BIN) for s in DEPS):
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + CSRC,
                        "-o", BIN + ".tmp", SRC], check=True)
        os.replace(BIN + ".tmp", BIN)
    return BIN


@pytest.mark.parametrize("length", LENGTHS)
def test_sha256_equals_hashlib_in_one_call_and_in_any_split(program, tmp_path, length):
    data = np.random.default_rng(length).integers(0, 256, length, dtype=np.uint8).tobytes()
    path = tmp_path / "message"
    path.write_bytes(data)
    r = subprocess.run([program, str(path), str(SPLITS)], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0"))
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and r.returncode == 0, r.stderr[-4000:]
    assert r.stdout.split() == [hashlib.sha256(data).hexdigest()] * (2 + SPLITS), (length, r.stdout)


def test_the_standard_vectors(program, tmp_path):
    """FIPS 180-4's own examples ("abc" and the 448-bit message), stated here as the hex strings of the standard's appendix, so that the
    test does not rest on hashlib alone."""
    for message, want in ((b"abc", "ba7816bf8f01cfea414140de5dae2223b00361a396177a9cb410ff61f20015ad"),
                          (b"abcdbcdecdefdefgefghfghighijhijkijkljklmklmnlmnomnopnopq", "248d6a61d20638b8e5c026930c3e6039a33ce45964ff2167f6ecedd419db06c1")):
        path = tmp_path / "message"
        path.write_bytes(message)
        r = subprocess.run([program, str(path), "2"], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0"))
        assert r.returncode == 0 and r.stdout.split() == [want] * 4, r.stdout + r.stderr[-2000:]
