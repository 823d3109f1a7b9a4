"""What the tests of the K2 verifier (csrc/avr_verify.h, avr_verify.hip) share: the seeded slices, and the expected answer -- the first
bin at which the ORACLE's decoder (oracle/avr_oracle.c: avr_oracle_range_decode), given the same bytes and records, decodes another
value than the record's."""
import numpy as np

import oracle_lib

VERIFY_NONE = 0xFFFFFFFF
BIN_COUNTS = (0, 1, 2, 7, 8, 9, 63, 64, 65, 200, 1023, 1024, 1025, 3000)
MASKS = (0x01, 0x80, 0xFF)


def first_bad(decoder, data, recs):
    """Index of the first bin `decoder` (the oracle, or oracle/_ref) decodes differently from the records, or VERIFY_NONE."""
    recs = np.asarray(recs, np.uint16)
    if recs.size == 0:
        return VERIFY_NONE
    diff = np.nonzero(decoder.range_decode(bytes(data), recs) != (recs & 1).astype(np.uint8))[0]
    return int(diff[0]) if diff.size else VERIFY_NONE


def seeded_slices(seed=2024, counts=BIN_COUNTS):
    """[(recs, coded bytes)]: for every bin count an adaptive and a fixed random_range_stream, coded by the oracle."""
    rng = np.random.default_rng(seed)
    oracle = oracle_lib.load_oracle()
    out = []
    for n in counts:
        for adaptive in (True, False):
            recs = oracle_lib.random_range_stream(rng, n, adaptive=adaptive)
            data, status = oracle.range_encode(recs)
            assert status == 0
            out.append((recs, data))
    return out


def flipped(data, p, mask):
    b = bytearray(data)
    b[p] ^= mask
    return bytes(b)
