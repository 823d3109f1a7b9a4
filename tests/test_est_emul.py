"""The estimator resolver (csrc/avr_est.h: key records -> K2 range records, per group of slices) emulated on the CPU by
tests/est_emul.cpp with the very functions the kernels run, against a plain restatement of the update rule
(tests/range_keys.py).  Chunk and window sizes down to one force every boundary case: a halving on, before and after a
chunk, a row and a slice boundary; groups inside one window and groups over many."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import range_keys as rk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "avrecode-ms_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "est_emul.cpp")
SO = os.path.join(ROOT, "tests", "_est_emul.so")
CHUNKS = [1, 2, 7, 47, 48, 49, 95, 96, 1024]


@pytest.fixture(scope="module")
def emul():
    deps = [SRC, os.path.join(CSRC, "avr_est.h"), os.path.join(CSRC, "avr_layout.h"), os.path.join(CSRC, "avr_k1p.h"), os.path.join(CSRC, "avr_chunk.h")]
    if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I" + CSRC, "-o", SO, SRC], check=True)
    lib = ctypes.CDLL(SO)
    lib.est_emul_workspace_bytes.restype = ctypes.c_uint64
    lib.est_emul_workspace_bytes.argtypes = [ctypes.c_uint64] * 3
    return lib


def emul_resolve(emul, slices, group_first, chunk, window, tables=None, gap=0, want_out=True):
    recs, rec_off, n_bins = rk.layout(slices, gap)
    gf = np.asarray(group_first, np.uint32)
    n_groups = gf.size - 1
    est_in = None if tables is None else np.ascontiguousarray(np.stack(tables), np.uint8)
    est_out = np.full((n_groups, rk.N_KEYS, 2), 0xCC, np.uint8) if want_out else None
    out = np.full(recs.size, 0xABCD, np.uint16)
    status = np.zeros(len(slices), np.int32)
    info = (ctypes.c_uint32 * 4)()
    P = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    rc = emul.est_emul_resolve(P(recs), P(rec_off), P(n_bins), ctypes.c_uint32(len(slices)), P(gf), ctypes.c_uint32(n_groups), P(est_in),
                               P(est_out), ctypes.c_uint32(chunk), ctypes.c_uint32(window), P(out), P(status), info)
    assert rc == 0
    return out, status, est_out, (rec_off, n_bins), list(info)


def check(emul, slices, group_first, chunk, window, tables=None, gap=0):
    want, want_tabs = rk.resolve(slices, group_first, tables)
    out, status, est_out, (rec_off, n_bins), info = emul_resolve(emul, slices, group_first, chunk, window, tables, gap)
    exp, mask = rk.expected_layout(want, rec_off, n_bins)
    diff = np.flatnonzero((out != exp) & mask)
    assert diff.size == 0, f"chunk={chunk} window={window}: first difference at record {diff[0]}: {out[diff[0]]:#x} != {exp[diff[0]]:#x} info={info}"
    assert status.tolist() == [rk.BAD_RECORD if w is None else 0 for w in want]
    for g, t in enumerate(want_tabs):
        if t is not None:
            assert np.array_equal(est_out[g], t), f"table of group {g} chunk={chunk} window={window}"
    return info, est_out


def groupings(n):
    """groups of 1, of 3 and of all slices"""
    return [list(range(n + 1)), list(range(0, n, 3)) + [n], [0, n]]


@pytest.mark.parametrize("chunk", CHUNKS)
def test_resolver_equals_the_rule_on_skewed_streams(emul, chunk):
    rng = np.random.default_rng(900 + chunk)
    spanned = 0
    for k in range(6):
        n_slices = int(rng.integers(4, 12))
        scale = 60 * min(chunk, 64)
        lens = [0 if rng.random() < 0.2 else int(rng.integers(1, scale)) for _ in range(n_slices)]      # empty slices inside a group
        slices = [rk.random_keys(rng, n, "skew") for n in lens]
        for gf in groupings(n_slices):
            for window in (1, 3, 16):
                info, _ = check(emul, slices, gf, chunk, window, gap=k % 2)
                spanned += info[2]
    assert spanned > 0                                       # groups over several windows did occur


@pytest.mark.parametrize("chunk", CHUNKS)
def test_one_key_holds_every_bin_and_every_halving_rank_meets_every_boundary(emul, chunk):
    """One key: halvings after its 95th bin and every 48th from there, so with these chunk sizes a halving falls on the last bin of
    a chunk, on the first of the next and in between, and (slices of chunk-multiple and other lengths) of a slice."""
    rng = np.random.default_rng(7 + chunk)
    lens = [95, 1, 47, 48, 49, 96, 143, 144, 3 * chunk, 3 * chunk + 1, 0, 500]
    slices = [rk.random_keys(rng, n, "one") for n in lens]
    key = int(slices[0][0]) >> 1
    slices = [((s & 1) | (key << 1)).astype(np.uint16) for s in slices]
    for gf in groupings(len(slices)):
        for window in (1, 2, 16):
            check(emul, slices, gf, chunk, window)


@pytest.mark.parametrize("chunk", [1, 7, 48, 96, 1024])
def test_start_tables_and_chaining_of_halves(emul, chunk):
    """Random valid start tables (totals 2 .. 96); the table after one half of a group fed as the start of the other half gives the
    records and the table of the unsplit group."""
    rng = np.random.default_rng(50 + chunk)
    for k in range(4):
        n_slices = 8
        slices = [rk.random_keys(rng, int(rng.integers(0, 50 * min(chunk, 48) + 200)), "skew" if k % 2 else "flat") for _ in range(n_slices)]
        tables = [rk.random_table(rng), rk.random_table(rng)]
        gf = [0, 5, n_slices]
        for window in (1, 4, 16):
            _, whole = check(emul, slices, gf, chunk, window, tables)
        # group 0 split after its second slice, the second part begun from the first one's table
        _, first = check(emul, slices[:2], [0, 2], chunk, 2, tables[:1])
        _, second = check(emul, slices[2:5], [0, 3], chunk, 2, [first[0]])
        assert np.array_equal(second[0], whole[0])
        want, _ = rk.resolve(slices[:5], [0, 5], tables[:1])
        out, status, _, (rec_off, n_bins), _ = emul_resolve(emul, slices[2:5], [0, 3], chunk, 2, [first[0]])
        for i in range(3):
            assert np.array_equal(out[int(rec_off[i]):int(rec_off[i]) + int(n_bins[i])], want[2 + i])


def test_long_group_renormalises_the_row_functions(emul):
    """Rows with more than 16 halvings of one key: the function of a row is renormalised (fn_normalise) and stays exact."""
    rng = np.random.default_rng(3)
    slices = [rk.random_keys(rng, 40000, "one") for _ in range(3)] + [rk.random_keys(rng, 30000, "skew")]
    for chunk, window in ((1024, 16), (1024, 2), (96, 16)):
        info, _ = check(emul, slices, [0, 4], chunk, window, [rk.random_table(rng)])
        assert info[2] == 1


def test_malformed_record_ends_its_group_from_that_slice_on(emul):
    rng = np.random.default_rng(11)
    slices = [rk.random_keys(rng, int(rng.integers(10, 3000)), "skew") for _ in range(9)]
    for bad in (0x1000, 0x8000, 1026 << 1, (2047 << 1) | 1):
        s = [x.copy() for x in slices]
        s[4][int(rng.integers(0, s[4].size))] = bad
        for gf in ([0, 3, 7, 9], [0, 9], list(range(10))):
            for chunk, window in ((1024, 16), (7, 3), (64, 1)):
                want, _ = rk.resolve(s, gf)
                g = max(i for i in range(len(gf) - 1) if gf[i] <= 4)
                assert [w is None for w in want] == [4 <= i < gf[g + 1] for i in range(9)]
                check(emul, s, gf, chunk, window)


def test_groups_without_slices_and_empty_batches(emul):
    rng = np.random.default_rng(5)
    slices = [rk.random_keys(rng, 100, "flat") for _ in range(3)]
    tables = [rk.random_table(rng) for _ in range(4)]
    info, est_out = check(emul, slices, [0, 0, 2, 2, 3], 1024, 16, tables)
    assert np.array_equal(est_out[0], tables[0]) and np.array_equal(est_out[2], tables[2])


@pytest.mark.parametrize("name", sorted(rk.ROW_BLOCK_CASES))
def test_row_block_inputs_reach_the_blocks_they_are_meant_to(emul, name):
    """The inputs of tests/test_gpu_range_keys_scale.py at the device's sizes: each makes the rows, the blocks beyond a group's first and
    the windows with two block heads it is there for (by the definitions, range_keys.row_plan, and as the emulation counts them), and
    the emulation resolves it exactly."""
    slices, gf = rk.row_block_case(name)
    rows, later, two = rk.ROW_BLOCK_PLANS[name]
    plan = rk.row_plan(slices, gf)
    assert (plan["rows"], plan["later_blocks"], plan["two_head_windows"]) == (rows, later, two)
    assert name.startswith("rows64") or later > 0                  # (64 rows: the largest group of one block)
    rng = np.random.default_rng(77)
    info, _ = check(emul, slices, gf, rk.CHUNK, rk.WINDOW, [rk.random_table(rng) for _ in range(len(gf) - 1)], gap=1)
    assert info == [plan["chunks"], plan["total_rows"], len(rows), later]


def test_plain_compiled_rule_equals_the_python_rule():
    """tests/est_plain.cpp (the reference of the full-size GPU comparisons) against range_keys.resolve: random streams in every mix,
    fresh and given tables, empty slices and groups, gaps, malformed records of every kind at any place."""
    rng = np.random.default_rng(4242)
    for k in range(40):
        n_slices = int(rng.integers(1, 14))
        mode = ("skew", "flat", "one")[k % 3]
        slices = [rk.random_keys(rng, 0 if rng.random() < 0.2 else int(rng.integers(1, 4000)), mode) for _ in range(n_slices)]
        cuts = sorted(rng.integers(0, n_slices + 1, int(rng.integers(0, 5))).tolist())
        gf = [0] + cuts + [n_slices]                                 # (a repeated cut: a group without slices)
        tables = None if k % 2 else [rk.random_table(rng) for _ in range(len(gf) - 1)]
        if k % 4 >= 2:
            for _ in range(int(rng.integers(1, 3))):
                i = int(rng.integers(0, n_slices))
                if slices[i].size:
                    slices[i][int(rng.integers(0, slices[i].size))] = (0x1000, 0x8001, 1026 << 1, (2047 << 1) | 1)[int(rng.integers(0, 4))]
        want, want_tabs = rk.resolve(slices, gf, tables)
        recs, rec_off, n_bins = rk.layout(slices, gap=k % 3)
        out, status, est_out = rk.plain_resolve(recs, rec_off, n_bins, gf, None if tables is None else np.stack(tables))
        exp, mask = rk.expected_layout(want, rec_off, n_bins)
        assert np.array_equal(out[mask], exp[mask]) and (out[~mask] == 0xABCD).all(), f"round {k}"
        assert status.tolist() == [rk.BAD_RECORD if w is None else 0 for w in want]
        for g, t in enumerate(want_tabs):
            assert np.array_equal(est_out[g], t if t is not None else np.full((rk.N_KEYS, 2), 0xCC, np.uint8)), f"round {k} group {g}"


def test_workspace_is_small_for_many_one_slice_groups(emul):
    """A batch of 1 Mi one-slice groups pays far less than one estimator table (1026 x 2 bytes) per group."""
    n = 1 << 20
    assert emul.est_emul_workspace_bytes(n, n, n) <= n * 1026 * 2 // 2


@pytest.mark.parametrize("name", ["realshort.mp4", "cockatoo.mp4"])
def test_real_streams_key_records_resolve_to_the_host_recorders_range_records(emul, avr, oracle, name):
    """With the residual hooks off the decompress direction's K1 records ARE the compress direction's key records, bin for bin:
    taken as one group per clip, every slice must resolve to exactly the K2 records the host recorder makes (its own estimator
    look-up and update, compress_recorder::record)."""
    from test_h264 import CLIPS, _stream_records, clip
    from test_host import host as host_fixture
    host = host_fixture.__wrapped__(avr)
    data = open(clip(name), "rb").read()
    k2, payloads, offered = _stream_records(host, data, 0, 0)
    assert len(k2) == CLIPS[name][0]
    recoded = []
    for r in k2:
        coded, st = oracle.range_encode(r)
        assert st == 0
        recoded.append(coded)
    k1, _ = _stream_records(host, data, 0, 1, recoded, offered)
    assert len(k1) == len(k2)
    out, status, est_out, (rec_off, n_bins), info = emul_resolve(emul, k1, [0, len(k1)], 1024, 16)
    assert not status.any()
    assert info[2] == 1                                          # the clip is one group over many windows
    total = 0
    for i, want in enumerate(k2):
        got = out[int(rec_off[i]):int(rec_off[i]) + int(n_bins[i])]
        assert got.size == want.size and np.array_equal(got, want), f"{name} slice {i}"
        total += want.size
    print(name, "records:", total, "keys in use:", int((est_out[0] != 1).any(1).sum()))
