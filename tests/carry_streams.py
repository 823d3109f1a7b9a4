"""Seeded record streams whose coded output holds one long run of carry-sensitive bytes (tests only).

Every coder in the product writes a digit out as soon as it exists and adds a later carry (low crossing fixed_one,
arithmetic_code.h:154-159) back into the bytes already written.  Random records almost never make that carry travel: a
carry passes a digit only if the digit is all ones.  The makers below choose bins so that the coding interval
[low, low + range) keeps straddling one point.  Only the distance d = point - low and the range are tracked (both shift
with every renormalisation), so a step costs O(1) whatever the run's length.  Once the point sits on a digit boundary
(after two 16-bit digits of CABAC, eight bytes of the recoded coder) every digit written is all ones: the output grows a
run of 0xff that a final push of low above the point turns into 0x00 at once.

The bins follow from d: the coded symbol is 1 (LPS / bypass 1 / bin 1) exactly when d >= r0 = range - r1, so the LPS
rate is the model's own (an LPS every ~10 bins for random context states).  When d == r0 neither symbol keeps low below
the point, and another record is chosen instead.
"""
import ctypes

import numpy as np

import oracle_lib

BYPASS, TERMINATE = 1024, 1025
CABAC_ONE, CABAC_MIN_RANGE, CABAC_RENORM = 1 << 31, 0x200, 1 << 15        # cabac_arithmetic_code: uint32, 16-bit digits
RANGE_ONE, RANGE_MIN_RANGE, RANGE_RENORM = 1 << 63, 1 << 51, 1 << 55     # recoded_code: uint64, 8-bit digits
ENDS = ("carry", "none", "cut")

_tables = None


def cabac_tables():
    """(lps_range[512], mlps_state[256]) as the oracle builds them (cabac_code.h:11-12)."""
    global _tables
    if _tables is None:
        a, b = oracle_lib.load_oracle().tables()
        _tables = (list(a), list(b))
    return _tables


def carry_chain_cabac(rng, n_lead, n_chain, end="carry", n_ctx=40, p_bypass=0.2, init_states=None):
    """(recs uint16[], init_states uint8[n_ctx]): about n_lead random 16-bit digits, then a chain of n_chain digits whose
    bytes are all 0xff while it lasts (from the chain's second or third digit on), then the end:
      "carry"  a bin pushes low above the point and put_terminate(1) follows: the whole run becomes 0x00;
      "none"   a bin drops the interval below the point and put_terminate(1) follows: the 0xff run stays;
      "cut"    put_terminate(1) while the interval still straddles the point: finish() decides.
    The same rng state gives the same lead and chain for every end.  p_bypass: share of bypass records (the rest are
    contexts drawn at random); with p_bypass=1 the chain codes no LPS at all (a context bin is drawn only when a bypass
    bin would land on the point, and it comes out MPS)."""
    assert end in ENDS
    lps, mlps = cabac_tables()
    states = (rng.integers(0, 126, n_ctx).astype(np.uint8) if init_states is None
              else np.array(init_states, dtype=np.uint8, copy=True))
    init = states.copy()
    st = [int(x) for x in states]
    out = []
    rng_draws = iter(())
    rng_u = iter(())
    ties = 0                                             # records in a row that would have landed on the point
    cut_wait = False                                     # "cut": contexts only while waiting (bypass bins alone can cycle
                                                         # without ever bringing the point near the top of the interval)

    def draw():                                          # (selector, uniform) drawn in blocks: a bin costs no numpy call
        nonlocal rng_draws, rng_u
        if ties or cut_wait:                             # after a tie: a context (bypass bins share one r0)
            if ties > 64:
                raise RuntimeError("carry_chain_cabac: no record keeps the interval off the point")
            return int(rng.integers(0, n_ctx)), 0.0
        try:
            return next(rng_draws), next(rng_u)
        except StopIteration:
            k = rng.random(4096)
            sel = np.where(k < p_bypass, BYPASS, rng.integers(0, n_ctx, 4096))
            rng_draws, rng_u = iter(sel.tolist()), iter(rng.random(4096).tolist())
            return next(rng_draws), next(rng_u)

    def r1_of(sel, rng_):
        """probability_of_1 of cabac_code.h: rLPS (:37-41), range / 2 for bypass (:52-54), 2 << normalize (:58-61)."""
        if sel == BYPASS:
            return rng_ // 2
        norm = (rng_ >> 8).bit_length() - 1
        if sel == TERMINATE:
            return 2 << norm
        return lps[((rng_ >> (norm - 1)) & 0x180) + st[sel]] << norm

    def code(sel, sym, rng_):
        """Append the record coding symbol `sym` on `sel`, update its state; returns the new range before renormalising."""
        r1 = r1_of(sel, rng_)
        if sel < BYPASS:
            s = st[sel]
            out.append((((s & 1) ^ sym) | (sel << 1)))
            st[sel] = mlps[127 - s] if sym else mlps[128 + s]       # cabac_code.h:43-47
        else:
            out.append(sym | (sel << 1))
        return r1 if sym else rng_ - r1

    def renorm(rng_, d):
        digits = 0
        if rng_ < CABAC_MIN_RANGE:
            while rng_ < CABAC_RENORM:
                rng_, d, digits = rng_ << 16, d << 16, digits + 1
        return rng_, d, digits

    rng_ = (CABAC_ONE // 0x200) * 0x1FE                   # cabac_code.h:30
    done = 0
    while done < n_lead:                                  # the lead: bins at the model's own odds
        sel, u = draw()
        r1 = r1_of(sel, rng_)
        rng_ = code(sel, int(u * rng_ < r1), rng_)
        rng_, _, k = renorm(rng_, 0)
        done += k
    d = rng_ // 2 + rng_ // 7                              # the point: not a dyadic midpoint, which a bypass bin would hit
    done = extra = 0
    while True:
        sel, _ = draw()
        r1 = r1_of(sel, rng_)
        r0 = rng_ - r1
        if d == r0:
            ties += 1
            continue
        ties = 0
        if done >= n_chain:
            extra += 1
            if extra > 1 << 20:
                raise RuntimeError("carry_chain_cabac: the chain does not end")
            if end == "carry" and d < r0:                 # symbol 1 with d < r0: low ends above the point
                code(sel, 1, rng_)
                break
            if end == "none" and d > r0:                  # symbol 0 with d > r0: the interval ends below the point
                code(sel, 0, rng_)
                break
            if end == "cut":
                t0 = rng_ - r1_of(TERMINATE, rng_)
                if d > t0:                                # put_terminate(1) keeps the point inside: finish() decides
                    code(TERMINATE, 1, rng_)
                    return np.array(out, dtype=np.uint16), init
                cut_wait = True
        sym = int(d > r0)
        rng_ = code(sel, sym, rng_)
        if sym:
            d -= r0
        rng_, d, k = renorm(rng_, d)
        done += k
    out.append(1 | (TERMINATE << 1))
    return np.array(out, dtype=np.uint16), init


def range_probability(rng_, pos, neg):
    """probability_of_1 of the recoded coder (recode.cpp:823-827), as avr_oracle_probability computes it."""
    return (rng_ // (pos + neg)) * pos


def oracle_range_probability(rng_, pos, neg):
    """avr_oracle_probability itself, for checking range_probability against it."""
    L = oracle_lib.load_oracle().L

    class Est(ctypes.Structure):
        _fields_ = [("pos", ctypes.c_int), ("neg", ctypes.c_int)]
    return int(L.avr_oracle_probability(ctypes.c_uint64(rng_), ctypes.byref(Est(pos, neg))))


def carry_chain_range(rng, n_lead, n_chain, end="carry", max_count=0x5f):
    """uint16 K2 records (bin | pos << 1 | neg << 8, pos and neg drawn from 1..max_count): about n_lead random bytes, then a
    chain of n_chain bytes that are all 0xff while it lasts (from its ninth byte or so on), then the end as for
    carry_chain_cabac -- "cut" simply ends the stream with the point inside the interval, so that finish() decides."""
    assert end in ENDS
    out = []
    block = iter(())

    def draw():
        nonlocal block
        try:
            return next(block)
        except StopIteration:
            pn = rng.integers(1, max_count + 1, (4096, 2))
            block = iter(zip(pn[:, 0].tolist(), pn[:, 1].tolist(), rng.random(4096).tolist()))
            return next(block)

    def renorm(rng_, d):
        digits = 0
        if rng_ < RANGE_MIN_RANGE:
            while rng_ < RANGE_RENORM:
                rng_, d, digits = rng_ << 8, d << 8, digits + 1
        return rng_, d, digits

    rng_ = RANGE_ONE
    done = 0
    while done < n_lead:
        pos, neg, u = draw()
        r1 = range_probability(rng_, pos, neg)
        sym = int(u * rng_ < r1)
        out.append(sym | (pos << 1) | (neg << 8))
        rng_ = r1 if sym else rng_ - r1
        rng_, _, k = renorm(rng_, 0)
        done += k
    d = rng_ // 2 + rng_ // 7
    done = 0
    while True:
        pos, neg, _ = draw()
        r1 = range_probability(rng_, pos, neg)
        r0 = rng_ - r1
        if d == r0:
            continue
        if done >= n_chain:
            if end == "cut":
                break
            if (end == "carry" and d < r0) or (end == "none" and d > r0):
                out.append(int(end == "carry") | (pos << 1) | (neg << 8))
                break
        sym = int(d > r0)
        out.append(sym | (pos << 1) | (neg << 8))
        if sym:
            rng_, d = r1, d - r0
        else:
            rng_ = r0
        rng_, d, k = renorm(rng_, d)
        done += k
    return np.array(out, dtype=np.uint16)


def longest_run(data, value):
    """(start, length) of the longest run of byte `value` in data."""
    a = np.frombuffer(data, dtype=np.uint8) == value
    if not a.any():
        return 0, 0
    edges = np.flatnonzero(np.diff(np.concatenate([[0], a.astype(np.int8), [0]])))
    starts, ends = edges[::2], edges[1::2]
    k = int(np.argmax(ends - starts))
    return int(starts[k]), int(ends[k] - starts[k])
