"""The library's one rule for malformed records, stated once for every test (include/avrecode_ms_amd.h, "Malformed records").

A slice breaks the rule when one of its records -- [0, n), never the padding behind it -- is one no recorder writes:
  K1, two-byte records   a bit of 12..15 set; a selector that is neither < n_states nor bypass (1024) / terminate (1025), the no-op
                         selector 1026 among them; a put_terminate(1) that is not the slice's last record
  K1, one-byte records   a selector in [n_states, 126); a put_terminate(1) that is not last; a rec_off that is not a multiple of 16
  K2                     bit 15 set, or pos + neg = 0
Such a slice comes back AVR_SLICE_BAD_RECORD with length 0, on every path, whatever else is wrong with it: BAD_RECORD wins over
ZERO_PROB, OVERFLOW and any hand-over inside a path.  For every other slice the oracle (oracle/avr_oracle.c) is the answer -- but
the oracle masks K1 selectors to 11 bits, ignores K2 bit 15 and reports the FIRST error of a slice, so it cannot state the rule
alone: expected() adds what it does not see."""
import numpy as np

from avrecode_ms_amd import CHUNK_BINS, SORT_BLOCK_BINS          # AVR_CHUNK_BINS, AVR_SORT_BLOCK_BINS (tests/test_cabi.py holds them to the header)

KIND_CABAC, KIND_RANGE, KIND_CABAC8 = 0, 1, 3
SLICE_OK, SLICE_ZERO_PROB, SLICE_OVERFLOW, SLICE_BAD_RECORD = 0, 1, 2, 3
SEL_BYPASS, SEL_TERMINATE, SEL_NOP = 1024, 1025, 1026
SEL8_BYPASS, SEL8_TERMINATE, MAX_STATES8 = 126, 127, 126
TERM1, TERM1_8 = (SEL_TERMINATE << 1) | 1, (SEL8_TERMINATE << 1) | 1
RING_BINS = 64                                                   # K2p's kRingBins

_oracle = None


def oracle():
    global _oracle
    if _oracle is None:
        import oracle_lib
        _oracle = oracle_lib.load_oracle()
    return _oracle


def breaks_rule(kind, recs, n_states=0, rec_off=0):
    """True when a record of the slice is one the rule calls bad."""
    r = np.asarray(recs).astype(np.int64)
    if kind == KIND_RANGE:
        return bool(((r & 0x8000) != 0).any() or ((r & 0x7ffe) == 0).any())
    if kind == KIND_CABAC:
        if ((r >> 12) != 0).any():
            return True
        sel = r >> 1
        fine = (sel < min(n_states, 1024)) | (sel == SEL_BYPASS) | (sel == SEL_TERMINATE)
        term1 = r == TERM1
    elif kind == KIND_CABAC8:
        if rec_off % 16:
            return True
        sel = (r & 0xff) >> 1
        fine = (sel < n_states) | (sel >= MAX_STATES8)
        term1 = (r & 0xff) == TERM1_8
    else:
        raise ValueError(f"kind {kind}")
    return bool((~fine).any() or term1[:-1].any())


def widen8(recs8):
    """One-byte K1 records as the two-byte records they stand for."""
    r = np.asarray(recs8, dtype=np.uint8).astype(np.uint16)
    sel = r >> 1
    sel = np.where(sel == SEL8_BYPASS, SEL_BYPASS, np.where(sel == SEL8_TERMINATE, SEL_TERMINATE, sel))
    return ((sel << 1) | (r & 1)).astype(np.uint16)


def expected(kind, recs, init_states=None, n_states=None, rec_off=0):
    """(status, bytes, final states) the library promises for one slice.  None stands for "not specified": the final states of a
    BAD_RECORD slice and of every K2 slice, and the bytes of a ZERO_PROB slice (the library stops where the oracle does, but only the
    status is part of the contract)."""
    if n_states is None:
        n_states = len(init_states) if init_states is not None else 0
    if breaks_rule(kind, recs, n_states, rec_off):
        return SLICE_BAD_RECORD, b"", None
    if kind == KIND_RANGE:
        data, st = oracle().range_encode(np.asarray(recs, dtype=np.uint16))
        return st, (None if st == SLICE_ZERO_PROB else data), None
    two = widen8(recs) if kind == KIND_CABAC8 else np.asarray(recs, dtype=np.uint16)
    data, states, st = oracle().cabac_encode(two, init_states)
    return st, data, states


def spoil(recs, at, value):
    """A copy of the slice with record `at` replaced by `value`."""
    r = np.array(recs, copy=True)
    r[at] = value
    return r


def positions(n, seg_len=3):
    """Where the kernels cut a slice, clipped to [0, n): the first record, the ends of the first 8-record group, the K2p lane form's
    ring batch, a chunk (AVR_CHUNK_BINS), a sort block and census block (AVR_SORT_BLOCK_BINS), a K2p segment of seg_len chunks, and
    the slice's last two records."""
    at = [0, 7, 8, RING_BINS - 1, RING_BINS, CHUNK_BINS - 1, CHUNK_BINS, SORT_BLOCK_BINS - 1, SORT_BLOCK_BINS,
          seg_len * CHUNK_BINS - 1, seg_len * CHUNK_BINS, n - 2, n - 1]
    return sorted({a for a in at if 0 <= a < n})


def bad_values(kind, n_states):
    """(what, record) for each way a record breaks the rule."""
    if kind == KIND_RANGE:
        return [("total 0", 0x0000), ("total 0, bin 1", 0x0001), ("bit 15", 0x8000 | (5 << 1) | (9 << 8)),
                ("bit 15, total 0", 0x8001)]
    if kind == KIND_CABAC8:
        out = [("terminate(1) not last", TERM1_8), ("selector 125", (125 << 1) | 1)]
        if n_states < 125:
            out.append(("selector n_states", n_states << 1))
        return out
    out = [("no-op", SEL_NOP << 1), ("no-op, bin 1", (SEL_NOP << 1) | 1), ("selector 1027", 1027 << 1), ("selector 2047", 0xfff),
           ("bit 15", 0x8000 | (5 << 1)), ("bit 12", 0x1000 | (3 << 1) | 1), ("terminate(1) not last", TERM1)]
    if n_states < 1024:
        out.append(("selector n_states", (n_states << 1) | 1))
    return out


def spoiled_set(rng, kind, make, n_states, seg_len=3, long_n=(4200, 13000), short_n=(9, 130)):
    """Seeded spoiled slices: every position of positions() in a long slice and the short slice's positions, each with a bad value
    taken in turn (every value at least once, the first -- the no-op / total 0 -- at several places).  make(n) -> a clean slice's
    records.  Returns [(recs, what)]."""
    values = bad_values(kind, n_states)
    out, k = [], 0
    for n_lo, n_hi in (long_n, short_n):
        n = int(rng.integers(n_lo, n_hi))
        for at in positions(n, seg_len):
            what, v = values[k % len(values)] if k % 3 else values[0]
            k += 1
            recs = make(n)
            out.append((spoil(recs, at, v), f"{what} at {at} of {n}"))
    for what, v in values:                                      # every value somewhere in the middle
        n = int(rng.integers(*long_n))
        out.append((spoil(make(n), int(rng.integers(1, n - 1)), v), f"{what} mid-slice of {n}"))
    return out
