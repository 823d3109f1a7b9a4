"""CABAC record streams for the digit path of K1p's phase C (csrc/avr_k1p.h, c_stretch_in): the bulk loop takes the digits of
four bins without a loop (none, one or a pair), the kernel stages them per lane in LDS and empties the stage where a wave's lanes
are together.  tests/test_k1p_digits_emul.py runs these through the CPU emulator, tests/test_gpu_k1p_digits.py through the
kernels; both against the oracle.  Every slice has N_STATES context states so that all of them fit one batch."""
import numpy as np

import carry_streams
import oracle_lib

N_STATES = 1024                      # the most a slice can have: the top-rate stream uses them all
CHUNK = 1024
SEL_BYPASS = 1024


def _recs(bins, sels):
    return (np.asarray(bins, np.uint16) | (np.asarray(sels, np.uint16) << 1)).astype(np.uint16)


def _padded(states):
    st = np.zeros(N_STATES, np.uint8)
    st[:len(states)] = states
    return st


def all_mps(n, lps_every=0):
    """Context bins that are all MPS from a saturated state (pStateIdx 62, valMPS 1): almost no digits.  As it stands the
    slice has no coded LPS and K1p declines it (a stretch longer than 16 chunks); lps_every > 0 puts an LPS at every
    lps_every-th bin, which keeps the slice in phase C."""
    bins = np.ones(n, np.uint16)
    if lps_every:
        bins[lps_every - 1::lps_every] = 0
    return _recs(bins, np.zeros(n)), _padded([125])


def all_bypass(rng, n, lps_every=0):
    """Bypass bins only: exactly one digit per 16 bins.  lps_every as in all_mps (the LPS of a context parked at pStateIdx 62)."""
    bins = rng.integers(0, 2, n).astype(np.uint16)
    sels = np.full(n, SEL_BYPASS)
    if lps_every:
        sels[lps_every - 1::lps_every] = 3
        bins[lps_every - 1::lps_every] = 0
    return _recs(bins, sels), _padded([125, 125, 125, 125])


def top_rate(n, n_ctx=N_STATES):
    """The maximum rate: n_ctx contexts at pStateIdx 62 (valMPS alternating), each hit once with its LPS, repeated.  The first
    round is six and five shifts a bin in turn (tests/test_k1p_digits_emul.py works it out): 22 bits a look of the bulk loop, one
    digit or a pair at every look; the rounds after it find the contexts at lower states and slow down."""
    st = (124 + (np.arange(n_ctx) & 1)).astype(np.uint8)
    sels = np.arange(n) % n_ctx
    bins = 1 - (sels & 1)                                   # the LPS of the initial state, every round
    return _recs(bins, sels), _padded(st)


def rate_extremes():
    """24 chunks a slice, the three rates next to each other so that every wave of phase C (64 consecutive chunks) has lanes of
    each kind: the kinds as they are named above (the first two are declined and come back through the serial kernel), and the first
    two with an LPS every 3 000 bins or so, which phase C codes itself."""
    rng = np.random.default_rng(8101)
    n = 24 * CHUNK
    out = []
    for k in range(3):
        out += [all_mps(n - 5 * k, lps_every=2900 + 111 * k), top_rate(n - k, N_STATES if k != 1 else 1000),
                all_bypass(rng, n - 16 * k, lps_every=3100 + 7 * k)]
    out += [all_mps(n), all_bypass(rng, n), top_rate(n)]
    return out


def random_long():
    """Random streams of 40 and more chunks, slices of different lengths: stretches start at every phase of the digit grid and
    their digits at every alignment of the slice's sums."""
    rng = np.random.default_rng(8102)
    out = []
    for i, n in enumerate((40 * CHUNK, 41 * CHUNK + 7, 45 * CHUNK + 1001, 52001, 60013, 48 * CHUNK - 1)):
        r, s = oracle_lib.random_cabac_stream(rng, n, 64, p_bypass=(0.0, 0.2, 0.6)[i % 3], terminate=bool(i % 3))
        out.append((r, _padded(s)))
    return out


BOUNDARY_LENGTHS = (0, 1, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, 2047, 2049)


def boundary_lengths():
    """Lengths around the boundaries of c_stretch_in's paths: head and tail only, no bulk, a stretch that closes in its first group."""
    rng = np.random.default_rng(8103)
    out = []
    for i, n in enumerate(BOUNDARY_LENGTHS):
        r, s = oracle_lib.random_cabac_stream(rng, n, 30, p_bypass=0.3 if i % 2 else 0.05, terminate=bool(i % 3))
        out.append((r, _padded(s)))
    return out


CHAINS = (30, 70, 9000)


def carry_chains():
    """Carry chains of 30, 70 and 9 000 digits (tests/carry_streams.py), ending in each way: the carry runs through digits that
    were taken as a pair."""
    out = []
    for k, (n_chain, end) in enumerate(zip(CHAINS, ("carry", "none", "cut"))):
        r, s = carry_streams.carry_chain_cabac(np.random.default_rng(8200 + k), 3 + 11 * k, n_chain, end)
        out.append((r, _padded(s)))
    r, s = carry_streams.carry_chain_cabac(np.random.default_rng(8210), 0, 9000, "carry")
    out.append((r, _padded(s)))
    return out


GROUPS = {"rate-extremes": rate_extremes, "random-long": random_long, "boundary-lengths": boundary_lengths, "carry-chains": carry_chains}
