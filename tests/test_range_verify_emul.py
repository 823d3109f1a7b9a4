"""The K2 verifier on the CPU: RangeDecoder64 and the slice walk of csrc/avr_verify.h -- the functions k_range_verify runs --
compiled by g++ (tests/range_verify_emul.cpp) and held against the oracle's decoder, and against oracle/_ref's (the reference's own
arithmetic_code.h) where that is built.

Corruptions: every byte position p <= len - 2 of every stream under the XOR masks 0x01, 0x80 and 0xff.  The oracle's own decoder
detects every one of those (asserted first); a flip of the LAST byte may go unnoticed by any decoder of this code (the tail holds
finish()'s stop bit and what follows it), so there only equality with the oracle is asked, whichever way it answers."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import oracle_lib
import verify_streams
from verify_streams import MASKS, VERIFY_NONE, first_bad, flipped

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "avrecode-ms_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "range_verify_emul.cpp")
SO = os.path.join(ROOT, "tests", "_range_verify_emul.so")


@pytest.fixture(scope="module")
def emul():
    deps = [SRC, os.path.join(CSRC, "avr_verify.h"), os.path.join(CSRC, "avr_div.h")]
    if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I" + CSRC, "-o", SO, SRC], check=True)
    lib = ctypes.CDLL(SO)
    lib.range_verify_emul.restype = ctypes.c_uint32
    return lib


@pytest.fixture(scope="module")
def slices():
    return verify_streams.seeded_slices()


def verify(emul, recs, data, fill=0x00, out_len=None):
    """The emulated kernel on one slice: the records padded with no-ops to whole chunks, the bytes at the start of a region of the
    batch API's capacity whose rest holds `fill`."""
    recs = np.asarray(recs, np.uint16)
    padded = np.zeros((recs.size + 7) // 8 * 8 + 8, np.uint16)
    padded[:recs.size] = recs
    cap = (recs.size + 16 + 7) // 8 * 8
    region = np.full(cap, fill, np.uint8)
    region[:len(data)] = np.frombuffer(data, np.uint8)
    return emul.range_verify_emul(padded.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint32(recs.size),
                                  region.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint32(cap),
                                  ctypes.c_uint32(len(data) if out_len is None else out_len))


def test_clean_streams_verify(emul, slices, oracle):
    for recs, data in slices:
        assert first_bad(oracle, data, recs) == VERIFY_NONE
        assert verify(emul, recs, data) == VERIFY_NONE, f"n_bins {recs.size}"


def test_bytes_past_the_length_change_nothing(emul, slices):
    for recs, data in slices:
        assert verify(emul, recs, data, fill=0xFF) == VERIFY_NONE, f"n_bins {recs.size}"
        if len(data) >= 2:                                   # and a corrupted slice gives the same index whatever lies behind it
            bad = flipped(data, 0, 0x80)
            assert verify(emul, recs, bad, fill=0xFF) == verify(emul, recs, bad, fill=0x00)


def test_a_length_beyond_the_capacity_is_clamped(emul, slices):
    recs, data = slices[-1]
    assert verify(emul, recs, data, out_len=1 << 30) == VERIFY_NONE     # the rest of the region is zero: what the decoder reads past the end anyway


def test_every_flip_up_to_the_last_byte_but_one(emul, slices, oracle):
    ref = oracle_lib.load_ref()                              # oracle/_ref where the reference is there to build it from, else None
    n_cases = 0
    for recs, data in slices:
        for p in range(len(data) - 1):                       # p <= len - 2; streams shorter than 2 bytes get no flip
            for mask in MASKS:
                bad = flipped(data, p, mask)
                want = first_bad(oracle, bad, recs)
                assert want != VERIFY_NONE, f"the oracle misses n_bins {recs.size} byte {p} mask {mask:#x}"
                assert verify(emul, recs, bad) == want, f"n_bins {recs.size} byte {p} mask {mask:#x}"
                if ref is not None:
                    assert first_bad(ref, bad, recs) == want
                n_cases += 1
    assert n_cases > 1000


def test_last_byte_flips_equal_the_oracle(emul, slices, oracle):
    for recs, data in slices:
        if not data:
            continue
        for mask in MASKS:
            bad = flipped(data, len(data) - 1, mask)
            assert verify(emul, recs, bad) == first_bad(oracle, bad, recs), f"n_bins {recs.size} mask {mask:#x}"


def test_truncated_and_emptied_streams_equal_the_oracle(emul, slices, oracle):
    for recs, data in slices:
        for cut in (0, len(data) // 2, max(len(data) - 1, 0)):
            assert verify(emul, recs, data[:cut]) == first_bad(oracle, data[:cut], recs), f"n_bins {recs.size} cut {cut}"
