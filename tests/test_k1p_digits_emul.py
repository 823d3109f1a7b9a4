"""K1p phase C takes the digits of four bins at once -- none, one or a pair, without a loop (csrc/avr_k1p.h, c_stretch_in) -- and
an adder that offers only store / add / flush gets the same calls as before.  The CPU emulator (tests/k1p_emul.cpp, HostAdder)
on the streams of tests/digit_streams.py against the oracle: bytes, final states, and the emulator's own count of plain stores and
atomic adds against what the slice's stretches imply.  tests/test_gpu_k1p_digits.py runs the same streams through the kernels."""
import numpy as np
import pytest

import digit_streams
from test_k1p_emul import emul, k1p  # noqa: F401  (the emulator's build fixture and its driver)


@pytest.mark.parametrize("group", sorted(digit_streams.GROUPS))
def test_digit_streams_on_the_emulator(emul, oracle, group):
    declined = 0
    for i, (recs, st) in enumerate(digit_streams.GROUPS[group]()):
        want = oracle.cabac_encode(recs, st)
        data, final, info = k1p(emul, recs, st)
        if info[3]:                                          # no coded LPS for more than 16 chunks: left to the serial kernel
            declined += 1
            continue
        assert (data, final) == want[:2], f"{group} slice {i} n={len(recs)} info={info}"
        # every digit below the final window is written exactly once: the first two of each stretch and its two window digits
        # (one when the window holds a single digit) as adds, the rest as plain stores
        n_active, n_digits, stores, adds = int(info[0]), int(info[6]), int(info[4]), int(info[5])
        assert n_active <= adds <= 4 * n_active and stores <= n_digits
        assert stores + adds >= n_digits
    assert declined == (2 if group == "rate-extremes" else 0)


def test_the_top_rate_stream_is_the_top_rate(emul, oracle):
    """The first round of digit_streams.top_rate codes nothing but the LPS of pStateIdx 62, whose table row is 6, 7, 8, 9: from the
    initial range 510 (quarter 3) the LPS range 9 takes five shifts to 288, quarter 0 gives 6 and six shifts to 384, quarter 2
    gives 8 and five shifts to 256, quarter 0 again -- 5, then 6 and 5 in turn: 5 632 shifts for 1 024 bins, 352 digits, a pair of
    digits at three looks of eight and one at the others.  (If the stream were slower the staging's worst case would go untested.)"""
    recs, st = digit_streams.top_rate(1024)
    data = oracle.cabac_encode(recs, st)[0]
    assert 2 * 351 <= len(data) <= 2 * 352 + 5
    _, _, info = k1p(emul, recs, st)
    assert info[1] == 5 + 512 * 6 + 511 * 5                   # t_total: shifts over the slice


def test_pair_pop_equals_the_loop():
    """The arithmetic of the look on its own, against the loop it replaces (the head and tail of a stretch still run the loop):
    200 000 random (L2, sp) with sp in [-7, 42] and L2 below 2^(sp + 18), and the corners."""
    rng = np.random.default_rng(8300)
    sps = np.concatenate([rng.integers(-7, 43, 200000), np.repeat(np.arange(-7, 43), 4)])
    for k, sp in enumerate(sps.tolist()):
        top = min(sp + 18, 61)
        corner = k - 200000
        L2 = int(rng.integers(0, 1 << top)) if corner < 0 else ((1 << top) - 1, 0, 1 << (top - 1), (1 << max(sp + 1, 0)) - 1)[corner % 4]
        a, s, loop = L2, sp, []
        while s >= 15:
            loop.append(a >> (s + 1))
            a &= (2 << s) - 1
            s -= 16
        s1 = sp + 1
        nd = max(s1, 0) >> 4
        ks = 16 + (s1 & 15)
        t = L2 >> ks
        pair = [] if nd == 0 else [t] if nd == 1 else [t >> 16, t & 0xffff]
        b = (L2 & 0xffffffff) & (((1 << ks) - 1) if nd else 0xffffffff)
        assert (pair, b, sp - 16 * nd) == (loop, a, s), (L2, sp)
