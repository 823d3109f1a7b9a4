"""CPU: the rule for malformed records (tests/bad_records.py) against the oracle.  On clean streams it is the oracle; on the records the
oracle does not see (K1 bits 12..15, K2 bit 15) it says BAD_RECORD; and BAD_RECORD wins over an earlier error, where the oracle
reports the first one."""
import numpy as np
import pytest

import bad_records as br
import oracle_lib


@pytest.fixture(scope="module")
def oracle():
    return br.oracle()


def test_clean_streams_are_the_oracle(oracle):
    rng = np.random.default_rng(5)
    for i, n in enumerate([0, 1, 7, 8, 9, 1023, 1025, 5000]):
        r, s = oracle_lib.random_cabac_stream(rng, n, 100, terminate=bool(i % 2))
        data, states, st = oracle.cabac_encode(r, s)
        assert st == 0 and br.expected(br.KIND_CABAC, r, s) == (st, data, states)
        assert br.expected(br.KIND_CABAC8, oracle_lib_to8(r), s) == (st, data, states)
        k2 = oracle_lib.random_range_stream(rng, n, adaptive=bool(i % 2))
        data, st = oracle.range_encode(k2)
        assert st == 0 and br.expected(br.KIND_RANGE, k2) == (0, data, None)


def oracle_lib_to8(recs):
    sel = (np.asarray(recs) >> 1).astype(np.int64)
    sel8 = np.where(sel == 1024, 126, np.where(sel == 1025, 127, sel))
    return ((sel8 << 1) | (np.asarray(recs) & 1)).astype(np.uint8)


def test_every_k1_record_value(oracle):
    """Each of the 65 536 two-byte values in the middle of a clean slice: BAD_RECORD exactly where the oracle says so, or where a bit
    of 12..15 is set (which the oracle masks away)."""
    rng = np.random.default_rng(6)
    r, s = oracle_lib.random_cabac_stream(rng, 40, 100)
    for v in range(1 << 16):
        spoiled = br.spoil(r, 20, v)
        st = br.expected(br.KIND_CABAC, spoiled, s)[0]
        want_bad = oracle.cabac_encode(spoiled, s)[2] == br.SLICE_BAD_RECORD or v >> 12 != 0
        assert (st == br.SLICE_BAD_RECORD) == want_bad, hex(v)
    assert br.expected(br.KIND_CABAC, br.spoil(r, 20, br.SEL_NOP << 1), s)[0] == br.SLICE_BAD_RECORD


def test_every_k2_record_value(oracle):
    """Each of the 65 536 values in the middle of a clean K2 slice: BAD_RECORD where the oracle says so (total 0) or bit 15 is set."""
    rng = np.random.default_rng(7)
    r = oracle_lib.random_range_stream(rng, 40)
    for v in range(1 << 16):
        spoiled = br.spoil(r, 20, v)
        st = br.expected(br.KIND_RANGE, spoiled)[0]
        ost = oracle.range_encode(spoiled)[1]
        assert (st == br.SLICE_BAD_RECORD) == (ost == br.SLICE_BAD_RECORD or bool(v & 0x8000)), hex(v)
        if st != br.SLICE_BAD_RECORD:
            assert st == ost
    for v in (0x0000, 0x0001, 0x8000, 0x8001, 0x8000 | (3 << 1) | (4 << 8)):
        assert oracle.range_encode(br.spoil(r, 20, v))[1] in (0, br.SLICE_BAD_RECORD)
        assert br.expected(br.KIND_RANGE, br.spoil(r, 20, v)) == (br.SLICE_BAD_RECORD, b"", None)


def test_k1_terminate_and_one_byte_rules():
    rng = np.random.default_rng(8)
    r, s = oracle_lib.random_cabac_stream(rng, 300, 60)                 # ends in put_terminate(1)
    assert br.expected(br.KIND_CABAC, r, s)[0] == 0
    assert br.expected(br.KIND_CABAC, br.spoil(r, 299, br.TERM1), s)[0] == br.SLICE_BAD_RECORD   # one before the last, which is one too
    assert br.expected(br.KIND_CABAC, br.spoil(r, 300, 1024 << 1), s)[0] == 0                   # terminate(1) gone: no rule broken
    r8 = oracle_lib_to8(r)
    assert br.expected(br.KIND_CABAC8, r8, s)[0] == 0
    assert br.expected(br.KIND_CABAC8, r8, s, rec_off=8)[0] == br.SLICE_BAD_RECORD
    assert br.expected(br.KIND_CABAC8, br.spoil(r8, 5, 60 << 1), s)[0] == br.SLICE_BAD_RECORD      # selector n_states
    assert br.expected(br.KIND_CABAC8, br.spoil(r8, 5, 125 << 1), s)[0] == br.SLICE_BAD_RECORD
    assert br.expected(br.KIND_CABAC8, br.spoil(r8, 5, 126 << 1), s)[0] == 0                       # bypass
    assert br.expected(br.KIND_CABAC8, br.spoil(r8, 5, br.TERM1_8), s)[0] == br.SLICE_BAD_RECORD
    assert br.expected(br.KIND_CABAC, br.spoil(r, 150, 1023 << 1), np.zeros(1024, np.uint8))[0] == 0   # 1024 contexts: 1023 is one


def test_bad_record_wins_over_an_earlier_error(oracle):
    """The oracle stops at a slice's first error; the library's status is BAD_RECORD wherever the bad record sits."""
    rng = np.random.default_rng(9)
    r = oracle_lib.random_range_stream(rng, 3000)
    zero = br.spoil(r, 100, 1 | (0 << 1) | (9 << 8))                    # bin 1 with pos 0: probability zero
    assert oracle.range_encode(zero)[1] == br.SLICE_ZERO_PROB
    st, data, _ = br.expected(br.KIND_RANGE, zero)
    assert st == br.SLICE_ZERO_PROB and data is None
    for v in (0x0000, 0x0001, 0x8000 | (7 << 1) | (2 << 8)):
        both = br.spoil(zero, 2500, v)
        assert oracle.range_encode(both)[1] == br.SLICE_ZERO_PROB        # the oracle reports the first error
        assert br.expected(br.KIND_RANGE, both) == (br.SLICE_BAD_RECORD, b"", None)
    c, s = oracle_lib.random_cabac_stream(rng, 3000, 50)
    late = br.spoil(c, 2900, 0x8000 | (4 << 1))                           # invisible to the oracle, behind nothing
    assert oracle.cabac_encode(late, s)[2] == 0 and br.expected(br.KIND_CABAC, late, s)[0] == br.SLICE_BAD_RECORD


def test_spoilers_cover_the_kernels_boundaries():
    assert br.positions(20000, 3) == [0, 7, 8, 63, 64, 1023, 1024, 3071, 3072, 4095, 4096, 19998, 19999]
    assert br.positions(10, 1) == [0, 7, 8, 9]
    rng = np.random.default_rng(10)
    for kind, make, ns in ((br.KIND_CABAC, lambda n: oracle_lib.random_cabac_stream(rng, n - 1, 100)[0], 100),
                           (br.KIND_CABAC8, lambda n: oracle_lib_to8(oracle_lib.random_cabac_stream(rng, n - 1, 100)[0]), 100),
                           (br.KIND_RANGE, lambda n: oracle_lib.random_range_stream(rng, n), 0)):
        made = br.spoiled_set(np.random.default_rng(11), kind, make, ns)
        assert len(made) >= 20
        values = {v for _, v in br.bad_values(kind, ns)}
        seen = set()
        for recs, what in made:
            seen |= values & set(np.asarray(recs).tolist())
        assert seen == values
        # every spoiled slice but those with terminate(1) put last is bad
        bad = [br.breaks_rule(kind, r, ns) for r, _ in made]
        assert sum(bad) >= len(made) - 2
