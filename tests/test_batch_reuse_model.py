"""tests/batch_reuse.py's runs and sequences through tests/cpu_batch.cpp, the CPU stand-in for the batch calls, for the kinds it has:
range records, key records and codes.  Two things are held here, on a machine without a GPU: the expectation model itself (the
stand-in codes with the oracle and checks with the oracle's decoders, so a disagreement is a mistake in the model or in the stand-in),
and the reuse of the stand-in, which the command-line comparisons rest on (`recode test <dir>` takes a directory through two of its
batch objects).  The stand-in is loaded as a plain shared library: no sanitizer, nothing preloaded.  Its fault points are set between
runs through its avr_test_hook_set, the test build's call."""
import ctypes
import os
import shutil
import subprocess
from ctypes import POINTER, byref, c_char_p, c_float, c_int, c_size_t, c_uint32, c_void_p

import numpy as np
import pytest

import batch_reuse as br
import oracle_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("codes", "range", "keys")
TYPES = [(k, p) for k in KINDS for p in br.PATHS]


def load_stand_in(source, directory):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++")
    so = os.path.join(str(directory), "cpu_batch.so")
    subprocess.run([cxx, "-O1", "-g", "-shared", "-fPIC", "-std=c++17", "-w", "-I" + os.path.join(ROOT, "tests"), "-o", so, source, "-x", "c",
                    os.path.join(ROOT, "oracle", "avr_oracle.c"), os.path.join(ROOT, "oracle", "spec_cabac.c"), "-pthread"], check=True)
    L = ctypes.CDLL(so)
    L.avr_batch_create.restype = c_void_p
    L.avr_last_error.restype = c_char_p
    P, Z = c_void_p, c_size_t
    for name, args in {"avr_batch_create": [c_int, Z, Z], "avr_batch_destroy": [P], "avr_batch_reset": [P], "avr_batch_run": [P],
                       "avr_batch_add_slice_range": [P, P, Z], "avr_batch_add_slice_codes": [P, P, Z], "avr_batch_begin_group": [P, P],
                       "avr_batch_add_slice_range_keys": [P, P, Z], "avr_batch_set_verify": [P, c_int], "avr_batch_set_verify_k1": [P, c_int],
                       "avr_batch_expect": [P, Z, P, Z], "avr_batch_get": [P, Z, POINTER(P), POINTER(Z), POINTER(c_int)],
                       "avr_batch_get_verify": [P, Z, POINTER(c_uint32)], "avr_batch_get_verify_est": [P, Z, POINTER(c_uint32)],
                       "avr_batch_get_restore": [P, Z, POINTER(c_uint32)], "avr_batch_get_estimators": [P, Z, POINTER(P), POINTER(Z)],
                       "avr_batch_verify_ms": [P, POINTER(c_float)], "avr_batch_verify_est_ms": [P, POINTER(c_float)],
                       "avr_batch_restore_ms": [P, POINTER(c_float)], "avr_test_hook_set": [c_char_p, c_uint32]}.items():
        getattr(L, name).argtypes = args
    return L


class CpuBatch:
    """avr.Batch's methods on the stand-in.  It has avr_batch_run only: submit() runs, wait() has nothing left to do.  One difference
    from the product is relied on: the product refuses avr_batch_run on a batch that has run ("batch already ran") and codes the same
    slices anew through avr_batch_submit / avr_batch_wait, which the stand-in lacks; the stand-in's avr_batch_run takes a batch that
    has run and codes it anew.  So "submitted again as it is" is a second avr_batch_run here."""

    def __init__(self, L, max_slices, max_bins):
        self.L, self.h = L, L.avr_batch_create(0, max_slices, max_bins)

    def _check(self, rc):
        if rc < 0:
            raise RuntimeError(self.L.avr_last_error().decode())
        return rc

    def close(self):
        if self.h:
            self.L.avr_batch_destroy(self.h)
            self.h = None

    def reset(self):
        self._check(self.L.avr_batch_reset(self.h))

    def add_slice_range(self, recs):
        r = np.ascontiguousarray(recs, np.uint16)
        return self._check(self.L.avr_batch_add_slice_range(self.h, oracle_lib.ptr(r), r.size))

    def add_slice_range_keys(self, recs):
        r = np.ascontiguousarray(recs, np.uint16)
        return self._check(self.L.avr_batch_add_slice_range_keys(self.h, oracle_lib.ptr(r), r.size))

    def add_codes(self, codes):
        c = np.ascontiguousarray(codes, np.uint8)
        return self._check(self.L.avr_batch_add_slice_codes(self.h, oracle_lib.ptr(c), c.size))

    def begin_group(self, est=None):
        e = None if est is None else np.ascontiguousarray(est, np.uint8)
        return self._check(self.L.avr_batch_begin_group(self.h, oracle_lib.ptr(e)))

    def set_verify(self, on=True):
        self._check(self.L.avr_batch_set_verify(self.h, int(on)))

    def set_verify_k1(self, on=True):
        self._check(self.L.avr_batch_set_verify_k1(self.h, int(on)))

    def expect(self, i, payload):
        p = np.frombuffer(bytes(payload), np.uint8)
        self._check(self.L.avr_batch_expect(self.h, i, oracle_lib.ptr(p) if p.size else None, p.size))

    def run(self):
        self._check(self.L.avr_batch_run(self.h))

    submit = run

    def wait(self):
        pass

    def get(self, i):
        p, n, st = c_void_p(), c_size_t(), c_int()
        self._check(self.L.avr_batch_get(self.h, i, byref(p), byref(n), byref(st)))
        return (ctypes.string_at(p.value, n.value) if n.value else b""), st.value

    def _answer(self, f, i):
        v = c_uint32()
        self._check(f(self.h, i, byref(v)))
        return v.value

    def get_verify(self, i):
        return self._answer(self.L.avr_batch_get_verify, i)

    def get_verify_est(self, i):
        return self._answer(self.L.avr_batch_get_verify_est, i)

    def get_restore(self, i):
        return self._answer(self.L.avr_batch_get_restore, i)

    def get_estimators(self, g):
        p, n = c_void_p(), c_size_t()
        self._check(self.L.avr_batch_get_estimators(self.h, g, byref(p), byref(n)))
        return np.frombuffer(ctypes.string_at(p.value, n.value * 2), np.uint8).reshape(n.value, 2).copy()

    def _ms(self, f):
        v = c_float()
        self._check(f(self.h, byref(v)))
        return v.value

    def verify_ms(self):
        return self._ms(self.L.avr_batch_verify_ms)

    def verify_est_ms(self):
        return self._ms(self.L.avr_batch_verify_est_ms)

    def restore_ms(self):
        return self._ms(self.L.avr_batch_restore_ms)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return load_stand_in(os.path.join(ROOT, "tests", "cpu_batch.cpp"), tmp_path_factory.mktemp("cpu_batch_reuse"))


@pytest.fixture
def new_batch(lib):
    made = []

    def make(max_slices, max_bins):
        made.append(CpuBatch(lib, max_slices, max_bins))
        return made[-1]
    yield make
    for b in made:
        b.close()
    lib.avr_test_hook_set(b"reset", 0)


@pytest.fixture
def setter(lib):
    def set_hook(name, value):
        assert lib.avr_test_hook_set(name.encode(), int(value)) == 0, lib.avr_last_error()
    return set_hook


_fresh = {}


def fresh_of(new_batch, run):
    if run.name not in _fresh:
        _fresh[run.name] = br.fresh(new_batch, run)
    return _fresh[run.name]


def test_the_run_types_are_what_they_are_meant_to_be():
    """Every dirty run is larger than every small run of the other path too, has a finding of its kind's hook, a malformed record (but
    for codes, which have no bad value) and the shapes the lane kernels change their step at; the chunked shapes hold a slice of no bins."""
    for kind, path in br.RUN_TYPES:
        A, B = br.run_type(kind, path, "A"), br.run_type(kind, path, "B")
        assert (len(A.slices), len(B.slices)) == ((130, len(B.slices)) if path == "lanes" else (5, len(B.slices)))
        assert 60 <= len(B.slices) <= 65 if path == "lanes" else 3 <= len(B.slices) <= 4
        assert set(br.EDGE_LENGTHS) <= set(A.lengths) and set(br.EDGE_LENGTHS) <= set(B.lengths) if path == "lanes" else 0 in A.lengths and 0 in B.lengths
        assert A.n_states > B.n_states or kind not in ("cabac", "cabac8")
        for other in br.PATHS:
            small = br.run_type(kind, other, "B")
            assert A.total > small.total and (len(A.slices) > len(small.slices) or path == "chunked")
        want = br.expected(A, hooked=True)
        statuses = [st for _, st in want.out]
        assert (br.BAD_RECORD in statuses) == (kind != "codes") and br.VERIFY_FAILED in statuses and statuses.count(br.OK) > len(statuses) // 2
        plain = br.expected(A)
        assert all(v == br.NONE for v in plain.verify) and all(v in (None, br.NONE) for v in plain.verify_est)
        assert (br.VERIFY_FAILED in [st for _, st in plain.out]) == (kind in br.K1)          # the product: only the restore check finds something
        assert all(st == br.OK for _, st in br.expected(B).out)
    assert sorted({len(br.run_type(k, "lanes", "B").slices) for k in br.KINDS} & {63, 64, 65}) == [63, 64, 65]


@pytest.mark.parametrize("b_type", TYPES, ids=lambda t: "B-%s-%s" % t)
@pytest.mark.parametrize("a_type", TYPES, ids=lambda t: "A-%s-%s" % t)
def test_every_ordered_pair(new_batch, setter, a_type, b_type):
    A, B = br.run_type(*a_type, "A"), br.run_type(*b_type, "B")
    br.seq_pair(new_batch, setter, A, B, fresh_of(new_batch, B))


@pytest.mark.parametrize("family", ("k1", "k2"))
def test_the_checks_across_runs(new_batch, setter, family):
    br.seq_checks(new_batch, setter, br.check_runs(family, ("codes",)))


@pytest.mark.parametrize("a_type", TYPES, ids=lambda t: "A-%s-%s" % t)
def test_an_empty_run_reports_nothing_of_the_run_before(new_batch, setter, a_type):
    A = br.run_type(*a_type, "A")
    B = br.run_type(*TYPES[(TYPES.index(a_type) + 3) % len(TYPES)], "B")
    br.seq_empty(new_batch, setter, A, B, fresh_of(new_batch, B))


@pytest.mark.parametrize("kind", KINDS)
def test_a_refused_submit_leaves_a_sound_object(new_batch, kind):
    B = br.run_type(kind, "lanes", "B")
    br.seq_refused(new_batch, B, fresh_of(new_batch, B))


@pytest.mark.parametrize("kind", KINDS)
def test_a_refused_add_leaves_no_trace(new_batch, kind):
    br.seq_capacity(new_batch, br.run_type(kind, "lanes", "B"))
