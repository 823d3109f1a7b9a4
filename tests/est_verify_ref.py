"""The reference answer of the estimator checker (avr_range_keys_verify_device): a plain statement of its five conditions over the
slice-major layout of tests/range_keys.py.  step(e, b): pos += b, neg += 1 - b, both halved rounding up if pos + neg > 0x60.
Over a group's bins in stream order, the slices that take part only (those before the group's first AVR_SLICE_BAD_RECORD):
  1  bit 0 of the resolved record is bit 0 of its key record, and the key record is well-formed (key < 1026);
  2  a key's first bin in the group carries est_in[group][key], {1, 1} without est_in;
  3  every other bin carries step of the RECORDED pair of the key's previous bin and that bin;
  4  the records from n_bins to the slice's next multiple of 8 are 0;
  5  est_out[group][key] is step of the key's last recorded pair and bin, or the start entry of a key the group never met (not
     checked for a group with a slice that takes no part, nor for a group without slices).
first_bad of a slice: its smallest bin that violates 1-3; n_bins for 4, and for 5 on the group's last slice; VERIFY_NONE otherwise."""
import numpy as np

import range_keys as rk

VERIFY_NONE = 0xFFFFFFFF
OK, BAD_RECORD, VERIFY_FAILED = 0, rk.BAD_RECORD, 4


def pair_of(rec):
    """{pos, neg} a resolved record carries, as pos | neg << 8 (bit 15 of the record counts as part of neg)"""
    rec = np.asarray(rec).astype(np.int64)
    return ((rec >> 1) & 0x7F) | (rec & 0xFF00)


def step(e, b):
    e, b = np.asarray(e).astype(np.int64), np.asarray(b).astype(np.int64)
    pos, neg = (e & 0xFF) + b, (e >> 8) + 1 - b
    halve = pos + neg > 0x60
    pos, neg = np.where(halve, (pos + 1) >> 1, pos), np.where(halve, (neg + 1) >> 1, neg)
    return pos | (neg << 8)


def step_plain(pos, neg, b):
    """the rule as tests/range_keys.py writes it, on one pair"""
    e = [pos, neg]
    e[1 - b] += 1
    if e[0] + e[1] > 0x60:
        e[0], e[1] = (e[0] + 1) >> 1, (e[1] + 1) >> 1
    return e[0], e[1]


def expect(keys, recs, rec_off, n_bins, group_first, est_in=None, est_out=None, status=None):
    """Per slice (would fail, first_bad).  keys / recs: the flat uint16 arrays; est_in / est_out: (groups, 1026, 2) uint8 or None;
    status: the statuses on entry (None: all AVR_SLICE_OK)."""
    keys, recs = np.asarray(keys, np.uint16).astype(np.int64), np.asarray(recs, np.uint16).astype(np.int64)
    rec_off, n_bins = np.asarray(rec_off).astype(np.int64), np.asarray(n_bins).astype(np.int64)
    n = n_bins.size
    status = np.zeros(n, np.int64) if status is None else np.asarray(status).astype(np.int64)
    first = np.full(n, VERIFY_NONE, np.int64)
    for g in range(len(group_first) - 1):
        s0, s1 = int(group_first[g]), int(group_first[g + 1])
        if s0 == s1:
            continue
        bad = [i for i in range(s0, s1) if status[i] == BAD_RECORD]
        part = list(range(s0, bad[0] if bad else s1))
        start = np.full(rk.N_KEYS, 0x101, np.int64) if est_in is None else \
            np.asarray(est_in[g], np.uint8).astype(np.int64)[:, 0] | (np.asarray(est_in[g], np.uint8).astype(np.int64)[:, 1] << 8)
        K = np.concatenate([keys[rec_off[i]:rec_off[i] + n_bins[i]] for i in part] + [np.zeros(0, np.int64)])
        R = np.concatenate([recs[rec_off[i]:rec_off[i] + n_bins[i]] for i in part] + [np.zeros(0, np.int64)])
        sl = np.concatenate([np.full(n_bins[i], i, np.int64) for i in part] + [np.zeros(0, np.int64)])
        at = np.concatenate([np.arange(n_bins[i], dtype=np.int64) for i in part] + [np.zeros(0, np.int64)])
        key, valid = K >> 1, (K >> 1) < rk.N_KEYS
        viol = ~valid | (((K ^ R) & 1) == 1)
        nxt = step(pair_of(R), K & 1)
        table = start.copy()
        idx = np.flatnonzero(valid)
        if idx.size:
            order = idx[np.argsort(key[idx], kind="stable")]             # by key, stream order inside a key
            same = np.concatenate([[False], key[order][1:] == key[order][:-1]])
            expected = np.where(same, np.concatenate([[0], nxt[order][:-1]]), start[key[order]])
            viol[order] |= pair_of(R[order]) != expected
            is_last = np.concatenate([~same[1:], [True]])
            table[key[order][is_last]] = nxt[order][is_last]
        for i, j in zip(sl[viol].tolist(), at[viol].tolist()):
            first[i] = min(first[i], j)
        for i in part:                                                     # condition 4
            o, nb = int(rec_off[i]), int(n_bins[i])
            if recs[o + nb:o + (nb + 7) // 8 * 8].any():
                first[i] = min(first[i], nb)
        if est_out is not None and not bad:                                # condition 5
            t = np.asarray(est_out[g], np.uint8).astype(np.int64)
            if ((t[:, 0] | (t[:, 1] << 8)) != table).any():
                first[s1 - 1] = min(first[s1 - 1], int(n_bins[s1 - 1]))
    return [(bool(f != VERIFY_NONE), int(f)) for f in first]


def expect_status(answers, status=None):
    """the statuses after the call: AVR_SLICE_OK with a finding becomes AVR_SLICE_VERIFY_FAILED, everything else stays"""
    status = [0] * len(answers) if status is None else [int(s) for s in status]
    return [VERIFY_FAILED if fail and st == OK else st for (fail, _), st in zip(answers, status)]
