"""The streams of tests/range_domain.py held to their preconditions on the CPU, before tests/test_gpu_range_domain.py takes them to
the device: every slice holds every (pos, neg) of [1, 127]^2, the renormalisations by 16 bits the double-precision walk has a branch
of its own for do occur, the oracle codes every slice, the CPU emulation of K2p (tests/k2p_emul.cpp: the kernels' own functions with
x86's arithmetic) gives the oracle's bytes, and its double-precision walk hands a slice over exactly where a collapse was planted."""
import ctypes

import numpy as np
import pytest

import range_domain as rd
from test_k2p_emul import emul, emul_encode                      # noqa: F401 (the fixture that builds tests/_k2p_emul.so)

SEED_DOMAIN, SEED_COLLAPSE = 2054, 2055


@pytest.fixture(scope="module")
def domain():
    return rd.domain_batch(SEED_DOMAIN)


@pytest.fixture(scope="module")
def collapse():
    return rd.collapse_batch(SEED_COLLAPSE)


def pairs_of(recs):
    return set(zip(((recs >> 1) & 0x7f).tolist(), ((recs >> 8) & 0x7f).tolist()))


def fp_walk(emul, recs):                                          # noqa: F811
    emul.k2p_emul_fp_walk.restype = ctypes.c_size_t
    recs = np.ascontiguousarray(recs, np.uint16)
    return emul.k2p_emul_fp_walk(recs.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(recs.size))


def test_the_batches_have_the_shapes_the_device_tests_count_on(domain, collapse):
    every = {(p, n) for p in range(1, 128) for n in range(1, 128)}
    labels = rd.domain_labels()
    assert len(domain) == 32 and len(labels) == 32
    lengths = sorted(len(s) for s in domain)
    assert lengths[:2] == [0, 8] and sorted(set(lengths[2:])) == [rd.N_PAIRS + e for e in rd.EXTRAS]
    assert (rd.N_PAIRS + 255) % 1024 == 0
    for label, s in zip(labels, domain):
        assert s.dtype == np.uint16 and not (s & 0x8000).any()
        if len(s) > 8:
            assert pairs_of(s) == every and pairs_of(s[:rd.N_PAIRS]) == every, label
    slices, planted = collapse
    assert len(slices) == len(planted) == len(rd.COLLAPSE_AT) * (len(rd.COLLAPSE_P) + 2)
    seen = set()
    for s, at in zip(slices, planted):
        assert len(s) == rd.N_PAIRS
        odd = [i for i in range(len(s)) if not ((s[i] >> 1) & 0x7f) or not ((s[i] >> 8) & 0x7f)]
        assert len(odd) == 1 and len(pairs_of(np.delete(s, odd[0]))) == rd.N_PAIRS - 1
        r = int(s[odd[0]])
        if at is None:
            assert odd[0] in rd.COLLAPSE_AT and ((r & 1 and not (r >> 8) & 0x7f) or (not r & 1 and not (r >> 1) & 0x7f))
        else:
            assert odd[0] == at and not r & 1 and not (r >> 8) & 0x7f
            seen.add((at, (r >> 1) & 0x7f))
    assert seen == {(at, p) for at in rd.COLLAPSE_AT for p in rd.COLLAPSE_P}


@pytest.mark.parametrize("mode", rd.MODES)
def test_integer_walk_meets_high_totals_and_shifts_by_16(domain, mode):
    """One slice a mode (the longest), in plain Python integers: 2 080 of the 16 129 pairs have a total above 190; the new range
    never falls below 2^39 (the double-precision form covers the whole slice); renormalisations by 16 bits are common where the
    bins do not follow the estimators and occur where they do."""
    s = domain[rd.domain_labels().index(f"{mode}+2999")]
    high, by16, smallest = rd.integer_walk(s)
    print(f"{mode}: {high} totals above 190, {by16} shifts by 16, smallest new range 2^{np.log2(smallest):.1f}")
    assert high >= 2080
    assert rd.integer_walk(s[:rd.N_PAIRS])[0] == 2080
    assert smallest >= 1 << 39
    assert by16 > 50 if mode != "match" else by16 >= 1


@pytest.mark.parametrize("chunk", [1024, 1])
def test_emulator_equals_the_oracle_on_the_domain_batch(emul, oracle, domain, chunk):    # noqa: F811
    for label, s in zip(rd.domain_labels(), domain):
        want, status = oracle.range_encode(s)
        got, info = emul_encode(emul, s, chunk)
        assert status == 0 and got == want, f"{label} chunk={chunk} info={info}"
        assert info[3] == len(s) and fp_walk(emul, s) == len(s), label


def test_collapse_batch_hands_over_at_the_planted_bin(emul, oracle, collapse):           # noqa: F811
    """The double-precision walk leaves at the planted bin and nowhere else; the certain records that keep the range it keeps.  Both
    outcomes of a collapse occur in the batch: the slice is coded (the emulator's bytes are the oracle's), or range mod p was 0 and
    the oracle reports the bin of probability zero."""
    slices, planted = collapse
    statuses = []
    for i, (s, at) in enumerate(zip(slices, planted)):
        want, status = oracle.range_encode(s)
        statuses.append(status)
        assert fp_walk(emul, s) == (len(s) if at is None else len(s) + 1 + at), f"slice {i}"
        for chunk in (1024, 1):
            got, info = emul_encode(emul, s, chunk)
            if at is None:
                assert status == 0 and got == want and info[3] == len(s), f"slice {i} chunk={chunk}"
            else:
                assert status in (0, rd.ZERO_PROB) and got == (want if status == 0 else None), f"slice {i} chunk={chunk}"
    hit = [st for st, at in zip(statuses, planted) if at is not None]
    assert 0 in hit and rd.ZERO_PROB in hit
