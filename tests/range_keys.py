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


# ------------------------------------------------------------------ rows and blocks: what an input makes the resolver do
CHUNK, WINDOW, ROW_BLOCK = 1024, 16, 64                            # the device's sizes (csrc/avr_est.h), restated


def row_plan(slices, group_first):
    """`slices`: the slices or their bin counts.  From the definitions alone (a slice occupies max(1, ceil(bins / CHUNK)) chunks; a group over global chunks [a, b) that crosses a
    window boundary has (b - 1) // WINDOW - a // WINDOW + 1 rows, scanned and chained in blocks of ROW_BLOCK rows, a block beginning in
    window a // WINDOW + ROW_BLOCK * kb): chunks, rows of every spanning group in order, their sum, blocks beyond a group's first
    (kb > 0), and the windows in which two blocks begin (one of a group that ends there or goes on, one of the group that starts there)."""
    chunks = np.array([max(1, -(-(s if isinstance(s, (int, np.integer)) else len(s)) // CHUNK)) for s in slices], np.int64)
    base = np.concatenate([[0], np.cumsum(chunks)])
    rows, heads, later = [], {}, 0
    for g in range(len(group_first) - 1):
        a, b = int(base[group_first[g]]), int(base[group_first[g + 1]])
        if b <= a or a // WINDOW == (b - 1) // WINDOW:
            continue
        n = (b - 1) // WINDOW - a // WINDOW + 1
        rows.append(n)
        blocks = -(-n // ROW_BLOCK)
        later += blocks - 1
        for kb in range(blocks):
            w = a // WINDOW + ROW_BLOCK * kb
            heads[w] = heads.get(w, 0) + 1
    return {"chunks": int(base[-1]), "rows": rows, "total_rows": sum(rows), "later_blocks": later,
            "two_head_windows": sum(1 for v in heads.values() if v == 2)}


def tiny_slices(rng, n, mode="skew", lo=0, hi=130):
    """n slices of lo .. hi - 1 bins: a chunk each, so rows and blocks for almost no bins"""
    return [random_keys(rng, int(rng.integers(lo, hi)), mode) for _ in range(n)]


def grouped(sizes):
    """group_first of consecutive groups of these sizes"""
    return [0] + np.cumsum(sizes).tolist()


def rows_case(rng, n_rows, mid_window):
    """A group of exactly n_rows rows.  On a window boundary: after 16 slices in groups of four, at chunk 16.  Mid-window: after a
    spanning group of 23 slices, at chunk 23 -- its first row 2 * 1 + 1 lies beside that group's row 2 * 1.  Then a group of three."""
    if mid_window:
        sizes = [23, WINDOW * n_rows + 9 - 23, 3]
    else:
        sizes = [4, 4, 4, 4, WINDOW * (n_rows - 1) + 5, 3]
    return tiny_slices(rng, sum(sizes)), grouped(sizes)


def two_heads_case(rng):
    """Five one-slice groups; a group over chunks [5, 1030): 65 rows, its second block begins (and ends) in window 64; a group over
    [1030, 2130): 70 rows from window 64 on, so window 64 holds two block heads; three one-slice groups."""
    sizes = [1] * 5 + [1025, 1100] + [1] * 3
    return tiny_slices(rng, sum(sizes)), grouped(sizes)


def long_groups_case(rng):
    """Five one-slice groups, groups of 2100 and of 1040 slices (132 and 66 rows: 3 and 2 blocks), three one-slice groups: the long
    groups share their first and last windows with groups that do not span."""
    sizes = [1] * 5 + [2100, 1040] + [1] * 3
    return tiny_slices(rng, sum(sizes)), grouped(sizes)


def hot_key_case(rng, mode):
    """Three short slices, then a group of 1100 slices of 1000 .. 1024 bins (69 rows, 2 blocks).  mode 'one': every bin of the batch on
    one key -- about 340 halvings a row, so every row function is in the renormalised form and a block's aggregate composes 64 of them;
    'skew': the mix of real streams."""
    slices = tiny_slices(rng, 3, mode) + tiny_slices(rng, 1100, mode, 1000, 1025)
    if mode == "one":
        key = int(slices[3][0]) >> 1
        slices = [((s & 1) | (key << 1)).astype(np.uint16) for s in slices]
    return slices, [0, 3, 1103]


def empties_case(rng):
    """Two slices; a group of 1100 slices of which about a third are empty (each still a chunk); a group of 40 empty slices (it spans
    windows and codes nothing: its table afterwards is its start table); a group of 1100 more; two slices."""
    sizes = [2, 1100, 40, 1100, 2]
    slices = tiny_slices(rng, sum(sizes))
    for i in range(2, 1102):
        if rng.random() < 0.33:
            slices[i] = slices[i][:0]
    for i in range(1102, 1142):
        slices[i] = slices[i][:0]
    return slices, grouped(sizes)


ROW_BLOCK_CASES = {f"rows{n}{'mid' if mid else ''}": (lambda rng, n=n, mid=mid: rows_case(rng, n, mid)) for n in (64, 65, 128, 129) for mid in (False, True)}
ROW_BLOCK_CASES.update(two_heads=two_heads_case, long_groups=long_groups_case, hot_one=lambda rng: hot_key_case(rng, "one"),
                       hot_skew=lambda rng: hot_key_case(rng, "skew"), empties=empties_case)
# what each must make the resolver do: (rows of its spanning groups, blocks with kb > 0, windows with two block heads)
ROW_BLOCK_PLANS = {"rows64": ([64], 0, 0), "rows64mid": ([2, 64], 0, 0), "rows65": ([65], 1, 0), "rows65mid": ([2, 65], 1, 0),
                   "rows128": ([128], 1, 0), "rows128mid": ([2, 128], 1, 0), "rows129": ([129], 2, 0), "rows129mid": ([2, 129], 2, 0),
                   "two_heads": ([65, 70], 2, 1), "long_groups": ([132, 66], 3, 0), "hot_one": ([69], 1, 0), "hot_skew": ([69], 1, 0),
                   "empties": ([69, 4, 70], 2, 0)}


def row_block_case(name):
    """(slices, group_first) of a ROW_BLOCK_CASES input, the same on every machine"""
    return ROW_BLOCK_CASES[name](np.random.default_rng(8600 + sorted(ROW_BLOCK_CASES).index(name)))


# ------------------------------------------------------------------ the rule compiled (tests/est_plain.cpp), for inputs of 10^8 bins
def plain_lib():
    import ctypes
    import os
    import subprocess
    here = os.path.dirname(os.path.abspath(__file__))
    src, so = os.path.join(here, "est_plain.cpp"), os.path.join(here, "_est_plain.so")
    if not os.path.exists(so) or os.path.getmtime(src) > os.path.getmtime(so):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so + ".tmp", src], check=True)
        os.replace(so + ".tmp", so)
    lib = ctypes.CDLL(so)
    lib.est_plain_resolve.restype = ctypes.c_uint64
    lib.est_plain_resolve.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_uint32] + [ctypes.c_void_p] * 4
    return lib


def plain_resolve(keys, rec_off, n_bins, group_first, est_in=None, fill=0xABCD):
    """est_plain_resolve on slice-major key records (uint16 array, rec_off, n_bins as the device calls take them): (recs_out preset to
    `fill`, status preset to -1, est_out preset to 0xCC) as the rule leaves them."""
    keys = np.ascontiguousarray(keys, np.uint16)
    rec_off = np.ascontiguousarray(rec_off, np.uint64)
    n_bins = np.ascontiguousarray(n_bins, np.uint32)
    gf = np.ascontiguousarray(group_first, np.uint32)
    assert rec_off.size == n_bins.size + 1 and int(gf[-1]) == n_bins.size and int(rec_off[-1]) <= keys.size
    est_in = None if est_in is None else np.ascontiguousarray(est_in, np.uint8)
    assert est_in is None or est_in.size == (gf.size - 1) * N_KEYS * 2
    out = np.full(keys.size, fill, np.uint16)
    status = np.full(n_bins.size, -1, np.int32)
    est_out = np.full((gf.size - 1, N_KEYS, 2), 0xCC, np.uint8)
    P = lambda a: None if a is None else a.ctypes.data
    plain_lib().est_plain_resolve(P(keys), P(rec_off), P(n_bins), P(gf), gf.size - 1, P(est_in), P(est_out), P(out), P(status))
    return out, status, est_out
