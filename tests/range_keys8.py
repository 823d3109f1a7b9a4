"""Shared by the tests of one-byte key records (AVR_KIND_RANGE_KEYS8): tests/range_keys.py's generators narrowed, the one-byte
slice-major layout, and what ties the two widths together.

A one-byte key record is bin | id << 1 with id 0..127 -- numerically the two-byte key record of key `id`, and every id below 128 is a
valid two-byte key.  So the serial rule of tests/range_keys.py (resolve, resolve_group, plain_resolve) applies to the WIDENED records as it
stands, entries 0..127 of its 1026-entry tables being the one-byte form's table.  Nothing here computes an estimator."""
import numpy as np

import range_keys as rk

N_KEYS8 = 128
SEL8_BYPASS, SEL8_TERMINATE = 126, 127


def narrow(recs16):
    """two-byte key records with their keys folded into 0..127: the skew and the hot key stay (a fold merges keys, it splits none)"""
    r = np.asarray(recs16, np.uint16)
    return ((r & 1) | (((r >> 1) % N_KEYS8) << 1)).astype(np.uint8)


def widen(recs8):
    return np.asarray(recs8, np.uint8).astype(np.uint16)


def random_keys8(rng, n, mode):
    return narrow(rk.random_keys(rng, n, mode))


def narrow_case(case):
    """(slices, group_first) of a range_keys case, narrowed"""
    slices, gf = case
    return [narrow(s) for s in slices], gf


def random_table8(rng):
    return rk.random_table(rng)[:N_KEYS8].copy()


def widen_table(t8):
    """the 1026-entry table whose entries 0..127 are t8 (None: fresh), the rest fresh -- no widened record names them"""
    t = rk.fresh_table()
    if t8 is not None:
        t[:N_KEYS8] = t8
    return t


def widen_tables(tables8):
    return None if tables8 is None else [widen_table(t) for t in tables8]


def garbage(rng, n):
    """n bytes none of which is zero: padding that reads as a key record with a bin whichever way it is looked at"""
    return rng.integers(1, 256, n).astype(np.uint8)


def layout8(slices8, rng, gap=0):
    """One-byte slice-major layout: rec_off (bytes, multiples of 16, `gap` groups of sixteen left unused between slices), n_bins and
    the byte array, readable 16 bytes past rec_off[-1] -- every padding byte and every gap non-zero garbage."""
    n_bins = np.array([len(s) for s in slices8], np.uint32)
    rec_off = np.zeros(len(slices8) + 1, np.uint64)
    for i, s in enumerate(slices8):
        rec_off[i + 1] = rec_off[i] + ((len(s) + 15) // 16 + gap) * 16
    recs = garbage(rng, int(rec_off[-1]) + 16)
    for i, s in enumerate(slices8):
        recs[int(rec_off[i]):int(rec_off[i]) + len(s)] = s
    return recs, rec_off, n_bins


def widened_layout(recs8, rec_off, n_bins):
    """The two-byte slice-major buffer that holds the same slices at the same rec_off counted in records (multiples of 16 are
    multiples of 8), 0xeeee elsewhere: what the two-byte route and range_keys.plain_resolve take."""
    out = np.full(int(rec_off[-1]) + 16, 0xEEEE, np.uint16)
    for i in range(len(n_bins)):
        o, n = int(rec_off[i]), int(n_bins[i])
        out[o:o + n] = recs8[o:o + n]
    return out


def expected_records(want, rec_off, n_bins, size, fill):
    """range_keys.expected_layout for a recs_out of `size` records: the records, AVR_NOP_RANGE to each slice's next multiple of EIGHT,
    `fill` everywhere else (from there to the next multiple of 16 included)."""
    out = np.full(size, fill, np.uint16)
    mask = np.ones(size, bool)
    for i, w in enumerate(want):
        o, n = int(rec_off[i]), int(n_bins[i])
        if w is None:
            mask[o:o + (n + 7) // 8 * 8] = False
            continue
        out[o:o + n] = w
        out[o + n:o + (n + 7) // 8 * 8] = 0
    return out, mask


def resolver_quote(n_slices, n_groups, total_chunks):
    """the issue's formula, restated"""
    a = lambda x: (x + 255) // 256 * 256
    return a(4 * n_slices) + a(4 * n_groups) + 2 * ((total_chunks + 15) // 16) * 768


def checker_quote(n_slices, total_chunks):
    a = lambda x: (x + 255) // 256 * 256
    return a(4 * n_slices) + 2 * ((total_chunks + 15) // 16) * 512
