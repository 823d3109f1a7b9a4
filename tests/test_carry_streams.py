"""The long-carry stream makers of tests/carry_streams.py do what the GPU and emulator tests rely on: the oracle's output of
a chain holds a run of at least the chain's length, 0x00 where the chain ends by pushing low above its point and 0xff,
at the same place, where the same records end below it."""
import numpy as np
import pytest

import carry_streams as cs


def test_range_probability_is_the_oracles():
    rng = np.random.default_rng(3)
    ranges = [cs.RANGE_ONE, cs.RANGE_MIN_RANGE, cs.RANGE_RENORM, cs.RANGE_MIN_RANGE - 1] + \
        [int(x) for x in rng.integers(cs.RANGE_MIN_RANGE, cs.RANGE_ONE, 300, dtype=np.uint64)]
    for r in ranges:
        for pos, neg in ((1, 1), (1, 127), (127, 1), (0x5f, 0x5f), (int(rng.integers(1, 128)), int(rng.integers(1, 128)))):
            assert cs.range_probability(r, pos, neg) == cs.oracle_range_probability(r, pos, neg)


def _runs_agree(carry, none, start, length):
    """carry has 0x00 and none 0xff on [start, start + length), and the carry out of the run in the byte before it."""
    assert start > 0 and carry[:start - 1] == none[:start - 1] and carry[start - 1] == none[start - 1] + 1
    assert carry[start:start + length] == b"\0" * length
    assert none[start:start + length] == b"\xff" * length


@pytest.mark.parametrize("n_lead,n_chain,p_bypass", [(0, 30, 0.2), (100, 2200, 0.2), (7, 9000, 0.5), (50, 3000, 1.0)])
def test_cabac_chain_is_a_carry_chain(oracle, n_lead, n_chain, p_bypass):
    out = {}
    for end in cs.ENDS:
        recs, st = cs.carry_chain_cabac(np.random.default_rng(n_chain), n_lead, n_chain, end, p_bypass=p_bypass)
        data, final, status = oracle.cabac_encode(recs, st)
        assert status == 0
        out[end] = (recs, data)
    (rc, carry), (rn, none) = out["carry"], out["none"]
    k = min(rc.size, rn.size) - 2
    assert np.array_equal(rc[:k], rn[:k])                     # the same lead and chain; only the ends differ
    start, length = cs.longest_run(none, 0xff)
    assert cs.longest_run(carry, 0)[0] == start
    length = min(length, cs.longest_run(carry, 0)[1])
    assert 2 * n_lead <= start <= 2 * n_lead + 6 and length >= 2 * (n_chain - 3)
    _runs_agree(carry, none, start, length)
    cut = out["cut"][1]                                       # finish() decides: either way the run is there, whole
    assert cut[:start - 1] == none[:start - 1] and cs.longest_run(cut, cut[start])[1] >= length


@pytest.mark.parametrize("n_lead,n_chain", [(0, 20), (100, 64), (33, 5000)])
def test_range_chain_is_a_carry_chain(oracle, n_lead, n_chain):
    out = {}
    for end in cs.ENDS:
        recs = cs.carry_chain_range(np.random.default_rng(n_chain), n_lead, n_chain, end)
        data, status = oracle.range_encode(recs)
        assert status == 0
        out[end] = (recs, data)
    (rc, carry), (rn, none) = out["carry"], out["none"]
    k = min(rc.size, rn.size) - 1
    assert np.array_equal(rc[:k], rn[:k])
    start, length = cs.longest_run(none, 0xff)
    assert cs.longest_run(carry, 0)[0] == start
    length = min(length, cs.longest_run(carry, 0)[1])
    assert n_lead <= start <= n_lead + 9 and length >= n_chain - 9
    _runs_agree(carry, none, start, length)
    cut = out["cut"][1]
    assert cut[:start - 1] == none[:start - 1] and cs.longest_run(cut, cut[start])[1] >= length


def test_cabac_chain_without_lps():
    """p_bypass=1 with contexts at pStateIdx 62: no coded LPS at all (the K1p scheme must decline such a slice)."""
    recs, st = cs.carry_chain_cabac(np.random.default_rng(9), 10, 2000, "carry", n_ctx=4, p_bypass=1.0,
                                    init_states=[124, 125, 124, 125])
    lps, mlps = cs.cabac_tables()
    s = [int(x) for x in st]
    coded_lps = 0
    for r in recs[:-1]:
        sel, b = int(r) >> 1, int(r) & 1
        if sel < cs.BYPASS:
            coded_lps += b != (s[sel] & 1)
            s[sel] = mlps[127 - s[sel]] if b != (s[sel] & 1) else mlps[128 + s[sel]]
    assert coded_lps <= 1 and recs.size > 17 * 1024       # (the push that ends a "carry" chain may be one)
