"""Shared by the key-record tests: a plain restatement of the compress direction's estimator rule (recode.cpp:823-827,
1037-1052 for the 1026 keys of h264_model's flat_[]: estimators start {1, 1}; a bin is coded with its key's pair as it
stands; then pos or neg goes up by one and, when pos + neg exceeds 0x60, both are halved rounding up), random key streams,
and the slice-major layout of the device calls."""
import numpy as np

N_KEYS = 1026
BAD_RECORD = 3


def fresh_table():
    return np.ones((N_KEYS, 2), np.uint8)


def random_table(rng):
    """A valid start table: pos >= 1, neg >= 1, totals 2 .. 96."""
    total = rng.integers(2, 97, N_KEYS)
    pos = 1 + (rng.random(N_KEYS) * (total - 1)).astype(np.int64)
    pos = np.minimum(pos, total - 1)
    return np.stack([pos, total - pos], 1).astype(np.uint8)


def resolve_group(slices, table=None):
    """K2 records of a group's slices (key records in stream order) and the group's table afterwards; a slice with a malformed
    record and every later one give None."""
    est = (fresh_table() if table is None else np.asarray(table, np.uint8)).astype(np.int64).tolist()
    out, ok = [], True
    for recs in slices:
        recs = np.asarray(recs, np.uint16).tolist()
        if ok and any((r >> 1) >= N_KEYS for r in recs):
            ok = False
        if not ok:
            out.append(None)
            continue
        res = np.zeros(len(recs), np.uint16)
        for i, r in enumerate(recs):
            e = est[r >> 1]
            res[i] = (r & 1) | (e[0] << 1) | (e[1] << 8)
            e[1 - (r & 1)] += 1
            if e[0] + e[1] > 0x60:
                e[0], e[1] = (e[0] + 1) >> 1, (e[1] + 1) >> 1
        out.append(res)
    return out, (np.array(est, np.uint8) if ok else None)


def resolve(slices, group_first, tables=None):
    """resolve_group over groups: group g = slices[group_first[g]:group_first[g + 1]]."""
    out, tabs = [], []
    for g in range(len(group_first) - 1):
        o, t = resolve_group(slices[group_first[g]:group_first[g + 1]], None if tables is None else tables[g])
        out += o
        tabs.append(t)
    return out, tabs


def random_keys(rng, n, mode):
    """n key records.  mode: 'one' = a single key holds every bin; 'skew' = a few hot keys (the hottest about a tenth, as in real
    streams), a tail of rare ones and keys that occur once; 'flat' = uniform over all 1026."""
    if mode == "one":
        key = np.full(n, int(rng.integers(0, N_KEYS)))
    elif mode == "flat":
        key = rng.integers(0, N_KEYS, n)
    else:
        hot = rng.choice(N_KEYS, 40, replace=False)
        w = 1.0 / np.arange(1, 41) ** 1.2
        key = hot[rng.choice(40, n, p=w / w.sum())]
        rare = rng.random(n) < 0.02
        key[rare] = rng.integers(0, N_KEYS, int(rare.sum()))
        if n:                                                         # keys that occur once (if the rest leaves them alone)
            once = rng.choice(n, min(n, 5), replace=False)
            key[once] = rng.choice(N_KEYS, once.size, replace=False)
    p1 = rng.random(N_KEYS)                                           # each key with a bias of its own
    bins = rng.random(n) < p1[key]
    return (bins.astype(np.uint16) | (key.astype(np.uint16) << 1)).astype(np.uint16)


def layout(slices, gap=0):
    """Slice-major layout: rec_off (multiples of 8 records, `gap` groups of eight left unused between slices), n_bins and the record
    array -- the padding up to each slice's next multiple of 8 and the gaps filled with 0xeeee (a malformed record: must not be read
    as one)."""
    n_bins = np.array([len(s) for s in slices], np.uint32)
    rec_off = np.zeros(len(slices) + 1, np.uint64)
    for i, s in enumerate(slices):
        rec_off[i + 1] = rec_off[i] + ((len(s) + 7) // 8 + gap) * 8
    recs = np.full(int(rec_off[-1]) + 8, 0xEEEE, np.uint16)
    for i, s in enumerate(slices):
        recs[int(rec_off[i]):int(rec_off[i]) + len(s)] = s
    return recs, rec_off, n_bins


def expected_layout(want, rec_off, n_bins, fill=0xABCD):
    """What recs_out must hold after a call on a buffer preset to `fill`: the records, AVR_NOP_RANGE up to each slice's next
    multiple of 8, `fill` everywhere else.  A slice whose records are None (malformed) is left out: see `mask`."""
    out = np.full(int(rec_off[-1]) + 8, fill, np.uint16)
    mask = np.ones(out.size, bool)
    for i, w in enumerate(want):
        o, n = int(rec_off[i]), int(n_bins[i])
        if w is None:
            mask[o:o + (n + 7) // 8 * 8] = False                      # undefined records: the status says so
            continue
        out[o:o + n] = w
        out[o + n:o + (n + 7) // 8 * 8] = 0
    return out, mask
