"""The restore check on the CPU: the per-word functions of csrc/avr_restore.h -- the functions k_restore_check runs -- compiled by g++
(tests/restore_emul.cpp), one emulated wave per slice, held to the plain-Python reference of tests/restore_ref.py (avr.drop_stop_byte,
avr.tail_patch, a first-difference loop) over the table of cases there: arbitrary byte strings, each in a region and an expectation
buffer of exactly the stated size with 0xFF behind the lengths.  Exact equality in every case.

The same functions run once more under AddressSanitizer and UBSan in a stand-alone program of their own (tests/restore_check.cpp),
started as a child process."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import restore_ref
from restore_ref import VERIFY_NONE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "avrecode-ms_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "restore_emul.cpp")
SO = os.path.join(ROOT, "tests", "_restore_emul.so")
CHECK_SRC = os.path.join(ROOT, "tests", "restore_check.cpp")
CHECK_BIN = os.path.join(ROOT, "tests", "_restore_check")
DEPS = [os.path.join(CSRC, h) for h in ("avr_restore.h", "avr_div.h")]


def _stale(target, sources):
    return not os.path.exists(target) or any(os.path.getmtime(s) > os.path.getmtime(target) for s in sources)


@pytest.fixture(scope="module")
def emul():
    if _stale(SO, [SRC] + DEPS):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I" + CSRC, "-o", SO, SRC], check=True)
    lib = ctypes.CDLL(SO)
    lib.restore_emul.restype = ctypes.c_uint32
    lib.restore_emul.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32]
    return lib


@pytest.fixture(scope="module")
def cases():
    return restore_ref.table()


def emulate(emul, c, fill=restore_ref.FILL):
    cap, e8 = (len(c.out) + 7) // 8 * 8, (len(c.expect) + 7) // 8 * 8
    region, expect = np.full(max(cap, 8), fill, np.uint8), np.full(max(e8, 8), fill, np.uint8)
    region[:len(c.out)] = np.frombuffer(c.out, np.uint8)
    expect[:len(c.expect)] = np.frombuffer(c.expect, np.uint8)
    assert region.ctypes.data % 8 == 0 and expect.ctypes.data % 8 == 0
    return emul.restore_emul(region.ctypes.data, cap, c.out_len, expect.ctypes.data, len(c.expect))


def test_the_table_covers_what_it_says(cases):
    names = {c.name for c in cases}
    assert len(names) == len(cases)
    for L in restore_ref.LENGTHS:
        for tail in restore_ref.TAILS:
            if L >= {"80": 1, "8080": 2, "none": 0}[tail]:
                assert any(n.startswith(f"L{L}-{tail}-") for n in names), (L, tail)
    assert any("+" in n for n in names) and any("-out@" in n for n in names) and any("claimed" in n for n in names)


def test_every_case_equals_the_reference(avr, emul, cases):
    answers = set()
    for c in cases:
        want = restore_ref.first_diff(avr, c.out, c.expect)
        assert emulate(emul, c) == want, c.name
        answers.add(want == VERIFY_NONE)
    assert answers == {True, False}


def test_what_lies_past_the_lengths_changes_nothing(avr, emul, cases):
    for c in cases[::3]:
        assert emulate(emul, c, fill=0x00) == emulate(emul, c, fill=0x80) == restore_ref.first_diff(avr, c.out, c.expect), c.name


def test_the_rule_in_words(avr, emul):
    """A handful of cases spelled out, so that the reference itself is read once: one stop byte dropped and never two, the patch in
    place and appended, no patch below two bytes, a length off by two with the right parity and the right last byte."""
    C = restore_ref.Case
    for out, exp, want in (
            (b"\x11\x22\x80", b"\x11\x22", VERIFY_NONE),                   # finish, then the last byte patched over itself
            (b"\x11\x22\x80", b"\x11\x99", VERIFY_NONE),                   # ... over another one: the container carries it
            (b"\x11\x22\x80\x80", b"\x11\x22\x80", VERIFY_NONE),           # only one 0x80 is dropped
            (b"\x11\x22", b"\x11\x22\x33", VERIFY_NONE),                   # parity differs: the last byte appended
            (b"\x11\x22", b"\x11\x22\x33\x22", 2),                         # off by two: right parity, right last byte, two short
            (b"\x11\x22\x33\x44", b"\x11\x22", 2),                         # ... two long
            (b"\x11", b"\x22", 0), (b"\x11", b"\x11", VERIFY_NONE),        # E < 2: nothing patched
            (b"", b"", VERIFY_NONE), (b"\x80", b"", VERIFY_NONE), (b"\x11", b"", 0),
            (b"\x99\x22\x33", b"\x11\x22\x33", 0)):
        assert restore_ref.first_diff(avr, out, exp) == want, (out, exp)
        assert emulate(emul, C("spelled", out, exp)) == want, (out, exp)


def test_the_sanitized_stand_alone_program():
    """tests/restore_check.cpp: the same functions on heap buffers of exactly the stated sizes, under AddressSanitizer and UBSan,
    against a byte-by-byte statement of the rule.  A child process with this one's environment as it is: nothing sanitised is loaded
    into this process and nothing is preloaded into that one by the test."""
    if _stale(CHECK_BIN, [CHECK_SRC, SRC] + DEPS):
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + CSRC,
                        "-I" + os.path.join(ROOT, "tests"), "-o", CHECK_BIN, CHECK_SRC], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0")
    r = subprocess.run([CHECK_BIN], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "ok" in r.stdout
