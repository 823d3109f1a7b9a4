"""tests/cpu_batch.cpp, the CPU stand-in for the batch calls, on the routes the command line cannot steer from outside: groups of key
records that start from a caller's table or hold a malformed key, avr_batch_get_estimators, the two refusals, the K1 verifier and the
restore check's answers on strings that are not what the coder made.  Against tests/range_keys.py (the estimator rule in Python), the
oracle and tests/restore_ref.py.  (The fault points are read once per process from the environment: tests/test_cli_verify_faults.py
has them, a child process each.)"""
import ctypes
import os
import shutil
import subprocess
from ctypes import POINTER, byref, c_char_p, c_int, c_size_t, c_uint32, c_void_p

import numpy as np
import pytest

import cli_verify_faults as cvf
import oracle_lib
import range_keys
import restore_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, BAD_RECORD, VERIFY_FAILED, NONE = 0, 3, 4, 0xFFFFFFFF


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++")
    so = str(tmp_path_factory.mktemp("cpu_batch") / "cpu_batch.so")
    subprocess.run([cxx, "-O1", "-g", "-shared", "-fPIC", "-std=c++17", "-w", "-o", so, os.path.join(ROOT, "tests", "cpu_batch.cpp"), "-x", "c",
                    os.path.join(ROOT, "oracle", "avr_oracle.c"), os.path.join(ROOT, "oracle", "spec_cabac.c"), "-pthread"], check=True)
    L = ctypes.CDLL(so)
    L.avr_batch_create.restype = c_void_p
    L.avr_last_error.restype = c_char_p
    for name in ("avr_batch_destroy", "avr_batch_reset", "avr_batch_run", "avr_batch_add_slice_range", "avr_batch_add_slice_codes", "avr_batch_begin_group",
                 "avr_batch_add_slice_range_keys", "avr_batch_set_verify", "avr_batch_set_verify_k1", "avr_batch_expect", "avr_batch_get",
                 "avr_batch_get_verify", "avr_batch_get_verify_est", "avr_batch_get_restore", "avr_batch_get_estimators"):
        getattr(L, name).argtypes = {"avr_batch_destroy": [c_void_p], "avr_batch_reset": [c_void_p], "avr_batch_run": [c_void_p],
                                     "avr_batch_add_slice_range": [c_void_p, c_void_p, c_size_t], "avr_batch_add_slice_codes": [c_void_p, c_void_p, c_size_t],
                                     "avr_batch_begin_group": [c_void_p, c_void_p], "avr_batch_add_slice_range_keys": [c_void_p, c_void_p, c_size_t],
                                     "avr_batch_set_verify": [c_void_p, c_int], "avr_batch_set_verify_k1": [c_void_p, c_int],
                                     "avr_batch_expect": [c_void_p, c_size_t, c_void_p, c_size_t],
                                     "avr_batch_get": [c_void_p, c_size_t, POINTER(c_void_p), POINTER(c_size_t), POINTER(c_int)],
                                     "avr_batch_get_verify": [c_void_p, c_size_t, POINTER(c_uint32)], "avr_batch_get_verify_est": [c_void_p, c_size_t, POINTER(c_uint32)],
                                     "avr_batch_get_restore": [c_void_p, c_size_t, POINTER(c_uint32)],
                                     "avr_batch_get_estimators": [c_void_p, c_size_t, POINTER(c_void_p), POINTER(c_size_t)]}[name]
    return L


def get(L, b, i):
    p, n, status = c_void_p(), c_size_t(), c_int()
    assert L.avr_batch_get(b, i, byref(p), byref(n), byref(status)) == 0
    answers = []
    for f in (L.avr_batch_get_verify, L.avr_batch_get_verify_est, L.avr_batch_get_restore):
        v = c_uint32()
        assert f(b, i, byref(v)) == 0
        answers.append(v.value)
    return (ctypes.string_at(p, n.value) if n.value else b""), status.value, answers


@pytest.mark.parametrize("verify", (0, 1))
def test_key_records_are_resolved_per_group_and_a_malformed_key_fails_the_rest_of_its_group(lib, oracle, verify):
    rng = np.random.default_rng(4100)
    slices = [range_keys.random_keys(rng, n, "skew") for n in (300, 0, 2500, 40, 900, 7, 1200, 64)]
    slices[4][500] = np.uint16(1027 << 1)                    # a key above AVR_SEL_TERMINATE, in the second slice of the second group
    group_first, given = [0, 3, 6, 8], range_keys.random_table(rng)
    want, tables = [], []
    for g in range(3):
        recs, table = range_keys.resolve_group(slices[group_first[g]:group_first[g + 1]], given if g == 2 else None)
        want += recs
        tables.append(table)
    b = lib.avr_batch_create(0, 16, 10000)
    try:
        assert lib.avr_batch_set_verify(b, verify) == 0
        for i, s in enumerate(slices):
            if i in group_first:
                g = group_first.index(i)
                assert lib.avr_batch_begin_group(b, oracle_lib.ptr(np.ascontiguousarray(given)) if g == 2 else None) == g
            assert lib.avr_batch_add_slice_range_keys(b, oracle_lib.ptr(s), s.size) == i
        assert lib.avr_batch_run(b) == 0, lib.avr_last_error()
        for i in range(len(slices)):
            data, status, answers = get(lib, b, i)
            if want[i] is None:
                assert i in (4, 5) and (data, status) == (b"", BAD_RECORD)
            else:
                assert (data, status) == oracle.range_encode(want[i], cap=2 * len(want[i]) + 64) and status == OK, i
            assert answers == [NONE, NONE, NONE]
        for g in (0, 2):                                     # (undefined for the group with the malformed record)
            p, n = c_void_p(), c_size_t()
            assert lib.avr_batch_get_estimators(b, g, byref(p), byref(n)) == 0 and n.value == range_keys.N_KEYS
            assert ctypes.string_at(p, 2 * n.value) == np.asarray(tables[g], np.uint8).tobytes()
        bad = np.ones((range_keys.N_KEYS, 2), np.uint8)
        bad[77] = (0x30, 0x31)                               # pos + neg above 0x60
        assert lib.avr_batch_reset(b) == 0 and lib.avr_batch_begin_group(b, oracle_lib.ptr(bad)) == -1
    finally:
        lib.avr_batch_destroy(b)


def test_each_verifier_is_refused_on_the_other_directions_batch(lib):
    rng = np.random.default_rng(4101)
    recs = oracle_lib.random_range_stream(rng, 300, adaptive=False)
    codes = rng.integers(0, 252, 200).astype(np.uint8)
    b = lib.avr_batch_create(0, 4, 4096)
    try:
        assert lib.avr_batch_set_verify(b, 1) == 0 and lib.avr_batch_add_slice_codes(b, oracle_lib.ptr(codes), codes.size) == 0
        assert lib.avr_batch_run(b) == -1 and b"compress direction" in lib.avr_last_error()
        assert lib.avr_batch_set_verify(b, 0) == 0 and lib.avr_batch_run(b) == 0
        assert lib.avr_batch_reset(b) == 0 and lib.avr_batch_set_verify_k1(b, 1) == 0
        assert lib.avr_batch_add_slice_range(b, oracle_lib.ptr(recs), recs.size) == 0
        assert lib.avr_batch_expect(b, 0, oracle_lib.ptr(codes), 4) == -1          # a K2 batch takes no expectations
        assert lib.avr_batch_run(b) == -1 and b"decompress direction" in lib.avr_last_error()
        assert lib.avr_batch_set_verify_k1(b, 0) == 0 and lib.avr_batch_run(b) == 0 and get(lib, b, 0)[1:] == (OK, [NONE, NONE, NONE])
    finally:
        lib.avr_batch_destroy(b)


def test_the_k1_verifier_and_the_restore_check_answer_as_the_oracle_and_the_plain_rule_do(lib, oracle):
    """Sound slices of codes with expectations that are right, wrong at one byte, too short, too long and absent: the K1 verifier finds
    nothing (the coder's bytes decode to their codes by oracle/spec_cabac.c's decoder), the restore check answers as
    tests/restore_ref.py's first_diff over the oracle's bytes."""
    from test_damaged_recode import codes_of, encode_codes
    rng = np.random.default_rng(4102)
    mlps = oracle.tables()[1]
    slices = []
    for n in (1, 9, 400, 3000, 3001, 2999, 50):
        recs, states = oracle_lib.random_cabac_stream(rng, n, 60)
        slices.append(codes_of(recs, states, mlps))
    coded = [encode_codes(oracle, c)[0] for c in slices]
    for c, codes in zip(coded, slices):                      # the decoder from codes itself: sound bytes decode, a flipped byte does not
        assert cvf.first_bad_codes(oracle, c, codes) == NONE
    assert cvf.first_bad_codes(oracle, bytes([coded[3][0] ^ 0x80]) + coded[3][1:], slices[3]) != NONE
    right = [restore_ref.restored(oracle, c, b"\x55\xaa" if len(c) % 2 else b"\x55\xaa\x33") for c in coded]   # any parity, a last byte
    assert all(restore_ref.restored(oracle, c, r) == r and len(r) > 11 for c, r in zip(coded[2:], right[2:]))   # ... which each restores
    expect = [right[0], right[1], right[2][:10] + bytes([right[2][10] ^ 1]) + right[2][11:], right[3][:-1], right[4] + b"\x00", None, right[6]]
    b = lib.avr_batch_create(0, 16, 20000)
    try:
        assert lib.avr_batch_set_verify_k1(b, 1) == 0
        for i, codes in enumerate(slices):
            assert lib.avr_batch_add_slice_codes(b, oracle_lib.ptr(codes), codes.size) == i
            if expect[i] is not None:
                e = np.frombuffer(expect[i], np.uint8)
                assert lib.avr_batch_expect(b, i, oracle_lib.ptr(e), e.size) == 0
        assert lib.avr_batch_expect(b, 0, oracle_lib.ptr(slices[0]), 1) == -1 and lib.avr_batch_expect(b, 9, oracle_lib.ptr(slices[0]), 1) == -1
        assert lib.avr_batch_run(b) == 0, lib.avr_last_error()
        for i in range(len(slices)):
            data, status, (bad, bad_est, diff) = get(lib, b, i)
            want = NONE if expect[i] is None else restore_ref.first_diff(oracle, coded[i], expect[i])
            assert data == coded[i] and (bad, bad_est) == (NONE, NONE) and diff == want, i
            assert status == (OK if want == NONE else VERIFY_FAILED)
        assert get(lib, b, 2)[2][2] == 10 and get(lib, b, 4)[1] == VERIFY_FAILED     # (the rule's answers, whatever they are, include these)
    finally:
        lib.avr_batch_destroy(b)
