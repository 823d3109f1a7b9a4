"""K2 streams over the whole domain the ABI accepts: every (pos, neg) in [1, 127]^2 in every slice, so that totals reach 254 and
the upper quarter of every reciprocal table of the device's coders is read (tests/test_range_domain.py holds the streams to their
preconditions on the CPU; tests/test_gpu_range_domain.py takes them through every library path that reads a K2 record).
numpy only: nothing here touches a device."""
import numpy as np

MODES = ("match", "anti", "half", "lo", "hi")
EXTRAS = (0, 1, 7, 255, 1023, 2999)                              # 16 129 + 255 = 16 x 1024: one length ends 1 short of a chunk
N_PAIRS = 127 * 127
COLLAPSE_P = (2, 3, 5, 77, 96, 127)
# the slice's first bins, around the first chunk's end, the first bin of a later segment under k2p_seg_len 1 and 3, somewhere, the last
COLLAPSE_AT = (0, 7, 8, 1023, 1024, 1025, 3 * 1024, 5000, N_PAIRS - 1)
ZERO_PROB = 1                                                    # AVR_SLICE_ZERO_PROB, and the oracle's status for it


def rec(b, pos, neg):
    return b | (pos << 1) | (neg << 8)


def _pairs(rng):
    k = rng.permutation(N_PAIRS)
    return 1 + k // 127, 1 + k % 127


def all_pairs_slice(rng, mode, extra):
    """A permutation of all 16 129 pairs (pos, neg) of [1, 127]^2, then the first `extra` records of a second permutation; the bins
    are 1 with probability pos / total (match: what the estimators claim), neg / total (anti), 0.5 (half), 0.02 (lo) or 0.98 (hi)."""
    pos, neg = _pairs(rng)
    pos2, neg2 = _pairs(rng)
    pos, neg = np.concatenate([pos, pos2[:extra]]), np.concatenate([neg, neg2[:extra]])
    p1 = {"match": pos / (pos + neg), "anti": neg / (pos + neg), "half": 0.5, "lo": 0.02, "hi": 0.98}[mode]
    bins = (rng.random(pos.size) < p1).astype(np.int64)
    return rec(bins, pos, neg).astype(np.uint16)


def domain_batch(seed):
    """32 slices: the five modes times the six lengths, an empty slice and one of 8 bins (the most lopsided pairs of the domain)."""
    rng = np.random.default_rng(seed)
    slices = [all_pairs_slice(rng, mode, extra) for mode in MODES for extra in EXTRAS]
    slices.insert(11, np.zeros(0, np.uint16))
    slices.insert(23, np.array([rec(0, 127, 1), rec(1, 1, 127), rec(1, 127, 127), rec(0, 1, 126), rec(0, 126, 127), rec(1, 96, 127),
                                rec(1, 127, 1), rec(0, 1, 127)], np.uint16))
    return slices


def domain_labels():
    labels = [f"{mode}+{extra}" for mode in MODES for extra in EXTRAS]
    labels.insert(11, "empty")
    labels.insert(23, "eight")
    return labels


def collapse_batch(seed):
    """(slices, planted): `match` slices of all pairs with one record replaced.  planted[i] = the replaced bin where it is
    `bin 0, pos p, neg 0` -- the new range is range mod p, below 2^7: the double-precision walk must hand the slice to the integer
    one, and a remainder of 0 is a bin of probability zero -- or None where it is a certain record that keeps the range
    (`bin 1, neg 0`; `bin 0, pos 0`), which the double-precision walk must keep."""
    rng = np.random.default_rng(seed)
    slices, planted = [], []
    for at in COLLAPSE_AT:
        for p in COLLAPSE_P:
            s = all_pairs_slice(rng, "match", 0)
            s[at] = rec(0, p, 0)
            slices.append(s)
            planted.append(at)
        for benign in (rec(1, 77 + at % 50, 0), rec(0, 0, 3 + at % 120)):
            s = all_pairs_slice(rng, "match", 0)
            s[at] = benign
            slices.append(s)
            planted.append(None)
    return slices, planted


def integer_walk(recs):
    """The range recurrence in plain Python integers (arithmetic_code.h:106-122 with recode.cpp:823-827): (bins with a total above
    190, renormalisations by 16 bits or more, the smallest new range before its shift)."""
    rng_, high, by16, smallest = 1 << 63, 0, 0, 1 << 63
    for r in recs.tolist():
        b, pos, neg = r & 1, (r >> 1) & 0x7f, (r >> 8) & 0x7f
        total = pos + neg
        high += total > 190
        r1 = rng_ // total * pos
        rng_ = r1 if b else rng_ - r1
        smallest = min(smallest, rng_)
        if rng_ < 1 << 51:
            assert rng_ > 0
            by16 += rng_ < 1 << 47
            while rng_ < 1 << 55:
                rng_ <<= 8
    return high, by16, smallest
