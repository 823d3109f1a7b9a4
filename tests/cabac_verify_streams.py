"""What the tests of the K1 verifier (csrc/avr_cabac_verify.h, avr_cabac_verify.hip) share: the seeded slices, the five record forms
of one slice, and the expected answer -- the first bin at which the ORACLE's decoder (oracle/spec_cabac.c: avr_spec_cabac_decode, written
from the standard), given the same bytes, records and states, decodes another value than the record's."""
import numpy as np

import oracle_lib

VERIFY_NONE = 0xFFFFFFFF
BIN_COUNTS = (0, 1, 2, 7, 8, 9, 15, 16, 17, 63, 64, 65, 200, 1023, 1024, 1025, 3000)
LONG_COUNTS = (30000, 70000, 41237, 55001)
MASKS = (0x01, 0x80, 0xFF)
TILES2, SLICES2, TILES8, SLICES8, CODES = range(5)           # cabac_verify::Form
FORMS = (TILES2, SLICES2, TILES8, SLICES8, CODES)
NOP_CABAC = 1026 << 1


class Slice:
    """One slice: two-byte records, initial states, and what the oracle's encoder makes of them."""

    def __init__(self, recs, states, oracle):
        self.recs = np.ascontiguousarray(recs, np.uint16)
        self.states = np.ascontiguousarray(states, np.uint8)
        self.data, final, status = oracle.cabac_encode(self.recs, self.states)
        assert status == 0
        self.final = np.frombuffer(final, np.uint8).copy()
        self.n_bins, self.n_states = int(self.recs.size), int(self.states.size)


def first_bad(oracle, data, recs, states):
    """Index of the first bin the oracle's spec decoder decodes differently from the records, or VERIFY_NONE."""
    recs = np.asarray(recs, np.uint16)
    if recs.size == 0:
        return VERIFY_NONE
    bins, _ = oracle.spec_cabac_decode(bytes(data), recs, states)
    diff = np.nonzero(bins != (recs & 1).astype(np.uint8))[0]
    return int(diff[0]) if diff.size else VERIFY_NONE


def seeded_slices(n_ctx, seed=2025, counts=BIN_COUNTS, wide_states=False):
    """For every bin count a terminated and an unterminated random_cabac_stream over n_ctx contexts, coded by the oracle.
    wide_states: the initial states drawn from [0, 128) -- pStateIdx 63 among them -- instead of the stream maker's [0, 126)."""
    rng = np.random.default_rng(seed)
    oracle = oracle_lib.load_oracle()
    out = []
    for n in counts:
        for t in (True, False):
            recs, states = oracle_lib.random_cabac_stream(rng, n, n_ctx, terminate=t)
            if wide_states:
                states = rng.integers(0, 128, n_ctx).astype(np.uint8)
            out.append(Slice(recs, states, oracle))
    return out


def flipped(data, p, mask):
    b = bytearray(data)
    b[p] ^= mask
    return bytes(b)


def codes_of(recs, states, mlps):
    """The resolved codes of a slice (AVR_CODE_CONTEXT / _BYPASS / _TERMINATE, include/avrecode_ms_amd.h): what a hook adapter records
    per bin.  mlps: the libavcodec-layout transition table (oracle.tables()[1])."""
    state = [int(x) for x in states]
    out = np.zeros(len(recs), np.uint8)
    for j, r in enumerate(recs):
        b, sel = int(r) & 1, int(r) >> 1
        if sel < 1024:
            s = state[sel]
            out[j] = 255 - ((b ^ s) & 1) if s >= 126 else (s << 1) | b
            state[sel] = mlps[127 - s] if b != (s & 1) else mlps[128 + s]
        else:
            out[j] = (252 | b) if sel == 1024 else 255 - b
    return out


def narrowed(recs):
    """Two-byte records as one-byte records (AVR_KIND_CABAC8): contexts below 126 as they are, bypass 126, terminate 127."""
    recs = np.asarray(recs, np.uint16)
    sel = recs >> 1
    assert np.all((sel < 126) | (sel == 1024) | (sel == 1025))
    sel8 = np.where(sel == 1024, 126, np.where(sel == 1025, 127, sel))
    return ((sel8 << 1) | (recs & 1)).astype(np.uint8)


def slice_major(form, s, mlps=None, pad8=0xA5):
    """The slice's records as the slice-major forms and the codes hold them: whole 16-byte chunks, the two-byte padding no-ops, the
    one-byte and code padding `pad8` (anything: it is never decoded)."""
    if form in (TILES2, SLICES2):
        a = np.full((s.n_bins + 7) // 8 * 8, NOP_CABAC, np.uint16)
        a[:s.n_bins] = s.recs
        return a.view(np.uint8)
    body = narrowed(s.recs) if form in (TILES8, SLICES8) else codes_of(s.recs, s.states, mlps)
    a = np.full((s.n_bins + 15) // 16 * 16, pad8, np.uint8)
    a[:s.n_bins] = body
    return a


def one_slice_tile(form, s, lane, fill=0x5A):
    """A tile whose column `lane` holds the slice (chunk c at byte (64 c + lane) * 16); every other column holds `fill`."""
    rows = slice_major(form, s).reshape(-1, 16)
    tile = np.full((rows.shape[0], 64, 16), fill, np.uint8)
    tile[:, lane, :] = rows
    return tile.reshape(-1)


def region_capacity(n_bins):
    """What the batch API gives a K1 slice: enough for any stream of n_bins bins, a multiple of 8."""
    return (n_bins + 64 + 7) // 8 * 8
