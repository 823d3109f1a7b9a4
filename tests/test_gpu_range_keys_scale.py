"""GPU: the estimator resolver (AVR_KIND_RANGE_KEYS, csrc/avr_est.hip) at the sizes and through the routes it ships at -- what
tests/test_gpu_range_keys.py stops short of.  Every comparison is exact and complete: records with their padding, bytes, lengths,
statuses, estimator tables, of every slice and every group.

  A  groups of more than one block of 64 rows (the kb > 0 branches of the scan and chain kernels), against the Python rule; the inputs
     are range_keys.ROW_BLOCK_CASES, whose rows and blocks tests/test_est_emul.py asserts on any machine
  B  the shapes of tools/range_keys_bench.py at full size: one group per slice against the synthetic generator's own range records
     (a serial estimator per slice, csrc/avr_synth.h), on the device; config 2 as one group and as 64 against the compiled plain rule
     (tests/est_plain.cpp), on the host
  C  the device-resident route: resolve_range() and then encode() / encode_chunked()
  D  one avr_batch reused for key records of changing shapes and for plain range records in between

Run time on an MI355X (one machine, one visit): this file 44 s of 275 s for the whole `-m gpu` run, 273 tests (233 s and 243 tests
before this file joined it).  Part B is 39 s of the 44: config 2 with a group per slice 19.0 s and config 4 at 16 384 slices (3.98 G bins)
9.3 s (most of it the generator making the two record kinds of long slices), config 5 at 1 Mi slices (1.62 G bins, 3.2 GB a record
array) 0.3 s, config 2's key records generated and copied to the host 7.7 s, then per grouping the plain rule 0.5 s and copy + compare
0.1 s.  Part A's Python reference is under 1 s a case."""
import time

import numpy as np
import pytest

import range_keys as rk
from test_gpu_range_keys import FILL, check_device, device_resolve, run_keys, run_range

pytestmark = pytest.mark.gpu

BAD_RECORDS = (0x1000, 0x8001, 1026 << 1, (2047 << 1) | 1)


@pytest.fixture(scope="module", autouse=True)
def report_time(request):
    t0 = time.time()
    yield
    with request.config.pluginmanager.getplugin("capturemanager").global_and_fixture_disabled():
        print(f"\ntests/test_gpu_range_keys_scale.py: {time.time() - t0:.1f} s")


def say(request, text):
    with request.config.pluginmanager.getplugin("capturemanager").global_and_fixture_disabled():
        print(f"\n  {text}", end="")


# ------------------------------------------------------------------ A: row blocks

@pytest.mark.parametrize("name", sorted(rk.ROW_BLOCK_CASES))
def test_row_blocks_equal_the_rule(avr, name):
    slices, gf = rk.row_block_case(name)
    rows, later, two = rk.ROW_BLOCK_PLANS[name]
    plan = rk.row_plan(slices, gf)
    assert (plan["rows"], plan["later_blocks"], plan["two_head_windows"]) == (rows, later, two)
    rng = np.random.default_rng(8700)
    check_device(avr, slices, gf)
    tables = [rk.random_table(rng) for _ in range(len(gf) - 1)]
    est_out = check_device(avr, slices, gf, tables, gap=2)
    for g in range(len(gf) - 1):
        if all(len(s) == 0 for s in slices[gf[g]:gf[g + 1]]):     # a group that codes nothing: its start table
            assert np.array_equal(est_out[g], tables[g]), f"group {g}"


def test_malformed_record_in_the_third_block_of_a_long_group(avr):
    """long_groups: groups of 132 and 66 rows between one-slice groups.  A malformed record in a row of the first one's third block:
    the slices before it keep their exact records and status 0, that slice and the rest of its group are BAD_RECORD, every other group
    is bit-identical to the clean run."""
    slices, gf = rk.row_block_case("long_groups")
    rng = np.random.default_rng(8701)
    tables = [rk.random_table(rng) for _ in range(len(gf) - 1)]
    clean, clean_status, clean_est, rec_off, n_bins = device_resolve(avr, slices, gf, tables, gap=1)
    assert not clean_status.any()
    k = 5 + 2070                                                   # chunk 2075: row 129 of the group that starts in window 0
    while len(slices[k]) == 0:
        k += 1
    assert gf[5] == 5 and k < gf[6] and (k // rk.WINDOW) // rk.ROW_BLOCK == 2
    for bad in BAD_RECORDS:
        s = [x.copy() for x in slices]
        s[k][int(rng.integers(0, s[k].size))] = bad
        check_device(avr, s, gf)
        check_device(avr, s, gf, tables, gap=1)
        out, status, est_out, _, _ = device_resolve(avr, s, gf, tables, gap=1)
        assert status.tolist() == [rk.BAD_RECORD if k <= i < gf[6] else 0 for i in range(len(s))]
        first_bad, group_end = int(rec_off[k]), int(rec_off[gf[6]])
        assert np.array_equal(out[:first_bad], clean[:first_bad]) and np.array_equal(out[group_end:], clean[group_end:])
        for g in range(len(gf) - 1):
            if g != 5:
                assert np.array_equal(est_out[g], clean_est[g]), f"table of group {g}"


def test_multi_block_group_split_across_two_calls(avr):
    """A group of 144 rows cut after 69: the second call (75 rows) begun from the first one's est_out gives the unsplit records and table."""
    rng = np.random.default_rng(8702)
    slices = rk.tiny_slices(rng, 2300)
    cut = 1100
    assert rk.row_plan(slices, [0, 2300])["rows"] == [144] and rk.row_plan(slices[:cut], [0, cut])["rows"] == [69]
    assert rk.row_plan(slices[cut:], [0, 2300 - cut])["rows"] == [75]
    start = rk.random_table(rng)
    whole = check_device(avr, slices, [0, 2300], [start])
    first = check_device(avr, slices[:cut], [0, cut], [start])
    second = check_device(avr, slices[cut:], [0, 2300 - cut], [first[0]])
    assert np.array_equal(second[0], whole[0])
    out_w, _, _, off_w, _ = device_resolve(avr, slices, [0, 2300], [start])
    out_2, _, _, off_2, _ = device_resolve(avr, slices[cut:], [0, 2300 - cut], [first[0]])
    assert np.array_equal(out_2[:int(off_2[-1])], out_w[int(off_w[cut]):int(off_w[-1])])


# ------------------------------------------------------------------ B: the published shapes at full size

def synth_slice_major(avr, workload, n, kind):
    """(records, rec_off, n_bins) of BASELINE config `workload`, slice-major on the device (not densified: the K1 records keep the
    contexts' own numbers, which are the model keys)."""
    w = avr.DeviceWorkload.synth(workload, n, kind, 0, 1000)
    recs, rec_off = w._slice_major()
    return recs, rec_off, w.n_bins


def first_difference(torch, got, want, rec_off, n_bins, nop, block=1 << 26):
    """On the device: the first record of [0, rec_off[-1]) where `got` is neither `want` (below its slice's n_bins) nor `nop` (from
    there to the slice's next multiple of eight, which is the next slice's rec_off): (slice, record in the slice, got, expected), or None."""
    total = int(rec_off[-1])
    nop = torch.tensor(nop, dtype=got.dtype, device=got.device)
    for r0 in range(0, total, block):
        r1 = min(total, r0 + block)
        idx = torch.arange(r0, r1, device=got.device)
        s = torch.searchsorted(rec_off, idx, right=True) - 1
        exp = torch.where(idx - rec_off[s] < n_bins[s], want[r0:r1], nop)
        diff = got[r0:r1] != exp
        if bool(diff.any()):
            i = int(diff.nonzero()[0])
            return int(s[i]), int(idx[i] - rec_off[s[i]]), int(got[r0 + i]) & 0xffff, int(exp[i]) & 0xffff
    return None


@pytest.mark.parametrize("workload,n", [(5, 1 << 20), (2, 512), (4, 16384)])
def test_one_group_per_slice_equals_the_generators_own_estimators(avr, request, workload, n):
    """The generator's AVR_KIND_CABAC records of a slice are key records of the bins whose AVR_KIND_RANGE records it makes with a serial
    fresh-start estimator per slice: with every slice a group of its own the resolver must reproduce those, at every record."""
    import torch
    t0 = time.time()
    keys, rec_off, n_bins = synth_slice_major(avr, workload, n, avr.KIND_CABAC)
    want, want_off, want_bins = synth_slice_major(avr, workload, n, avr.KIND_RANGE)
    assert torch.equal(n_bins, want_bins) and torch.equal(rec_off, want_off)
    w = avr.DeviceWorkload.from_device_keys(keys, rec_off, n_bins, np.arange(n + 1))
    w.rec_flat.fill_(np.array(FILL, np.uint16).view(np.int16).item())
    w.resolve_keys()
    torch.cuda.synchronize()
    plan = w._chunk_plan()["plan"]
    bins = w.total_bins
    d = first_difference(torch, w.rec_flat, want, rec_off, n_bins, avr.NOP_RANGE)
    assert d is None, f"slice {d[0]} record {d[1]}: {d[2]:#x} != {d[3]:#x}"
    last = int((n_bins > 0).nonzero()[-1])                         # the comparison itself: one bit of the last record is found, and where
    at = int(rec_off[last]) + int(n_bins[last]) - 1
    w.rec_flat[at] ^= 2
    d = first_difference(torch, w.rec_flat, want, rec_off, n_bins, avr.NOP_RANGE)
    assert d is not None and d[:2] == (last, int(n_bins[last]) - 1) and d[2] == d[3] ^ 2
    assert (w.rec_flat[int(rec_off[-1]):].cpu().numpy().view(np.uint16) == FILL).all()
    assert not bool(w.status.any())
    say(request, f"config {workload}, {n} slices, {bins} bins, {plan.total_chunks} chunks: {time.time() - t0:.1f} s")
    del w, keys, want
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def config2(avr):
    """Config 2 at the size its times are published at (512 slices, about 310 M bins): the key records on the device and on the host."""
    import torch
    keys, rec_off, n_bins = synth_slice_major(avr, 2, 512, avr.KIND_CABAC)
    yield keys, rec_off, n_bins, keys.cpu().numpy().view(np.uint16), rec_off.cpu().numpy(), n_bins.cpu().numpy()
    del keys
    torch.cuda.empty_cache()


@pytest.mark.parametrize("name,per_group", [("w2_one", 512), ("w2_groups8", 8), ("w2_each", 1)])
def test_config2_at_full_size_equals_the_plain_rule(avr, request, config2, name, per_group):
    """tools/range_keys_bench.py's w2_one (one group of all 512 slices: about 18 900 rows, 296 blocks) and w2_groups8 (64 groups), and
    one group per slice: the records copied back and compared whole, every group's est_out with the plain rule's table."""
    import torch
    t0 = time.time()
    keys, rec_off, n_bins, h_keys, h_off, h_bins = config2
    gf = list(range(0, 512, per_group)) + [512]
    plan = rk.row_plan([int(b) for b in h_bins], gf)
    if name == "w2_one":
        assert len(plan["rows"]) == 1 and plan["later_blocks"] >= 290
    if name == "w2_groups8":
        assert len(plan["rows"]) == 64 and plan["later_blocks"] >= 64 * 3
    w = avr.DeviceWorkload.from_device_keys(keys, rec_off, n_bins, gf)
    w.rec_flat.fill_(np.array(FILL, np.uint16).view(np.int16).item())
    w.est_out.fill_(0xCC)
    w.resolve_keys()
    torch.cuda.synchronize()
    t1 = time.time()
    exp, exp_status, exp_est = rk.plain_resolve(h_keys, h_off, h_bins, gf, fill=FILL)
    t2 = time.time()
    assert not exp_status.any()
    got = w.rec_flat.cpu().numpy().view(np.uint16)
    if not np.array_equal(got, exp):
        at = int(np.flatnonzero(got != exp)[0])
        s = int(np.searchsorted(h_off, at, side="right")) - 1
        raise AssertionError(f"{name}: slice {s} record {at - int(h_off[s])}: {got[at]:#x} != {exp[at]:#x}")
    assert not w.status.cpu().numpy().any()
    est = w.est_out.cpu().numpy().reshape(-1, rk.N_KEYS, 2)
    for g in range(len(gf) - 1):
        assert np.array_equal(est[g], exp_est[g]), f"{name}: table of group {g}"
    say(request, f"{name}: {int(h_bins.sum())} bins, rows {plan['total_rows']}, later blocks {plan['later_blocks']}: device {t1 - t0:.1f} s, "
                 f"plain rule {t2 - t1:.1f} s, copy and compare {time.time() - t2:.1f} s")


# ------------------------------------------------------------------ C: the device-resident route

ROUTE_SHAPES = {"short": (300, 0, 4000), "long": (6, 20000, 60000)}          # (slices, shortest, longest), as SHAPES of test_gpu_range_keys.py


def route_slices(rng, shape):
    n, lo, hi = ROUTE_SHAPES[shape]
    slices = [rk.random_keys(rng, int(rng.integers(lo, hi)), "skew") for _ in range(n)]
    if shape == "short":
        slices[5] = slices[5][:0]
    return slices


def route_groupings(n):
    return [list(range(n + 1)), [0, n], [0, n // 3, n // 2, n]]


def coded(w, chunked):
    """The resolved workload through the coder: (bytes, status) per slice, out_len as the coder left it (preset to 777)."""
    w.out_len.fill_(777)
    w.out.zero_()
    (w.encode_chunked if chunked else w.encode)()
    data, status = w.results()
    return list(zip(data, status)), w.out_len.cpu().numpy().tolist()


@pytest.mark.parametrize("shape,chunked", [("short", False), ("long", False), ("long", True)])
def test_resolve_range_then_encode_equals_the_oracle(avr, oracle, shape, chunked):
    rng = np.random.default_rng(8800 + len(shape))
    slices = route_slices(rng, shape)
    n = len(slices)
    for gf in route_groupings(n):
        for tables in (None, [rk.random_table(rng) for _ in range(len(gf) - 1)]):
            want, want_tabs = rk.resolve(slices, gf, tables)
            kw = avr.DeviceWorkload.from_host_keys(slices, gf, tables, 0, gap=1 if tables else 0)
            got, lens = coded(kw.resolve_range(), chunked)
            for i in range(n):
                assert got[i] == oracle.range_encode(want[i]), f"slice {i} of {n}, groups {gf[:4]}..."
                assert lens[i] == len(got[i][0])
            est = kw.est_out.cpu().numpy().reshape(-1, rk.N_KEYS, 2)
            for g in range(len(gf) - 1):
                assert np.array_equal(est[g], want_tabs[g])


@pytest.mark.parametrize("shape,chunked", [("short", False), ("long", False), ("long", True)])
def test_resolve_range_carries_a_malformed_record_into_the_coder(avr, oracle, shape, chunked):
    rng = np.random.default_rng(8900 + len(shape))
    slices = route_slices(rng, shape)
    n = len(slices)
    gf = [0, n // 3, n // 3 * 2, n] if shape == "short" else [0, 2, 5, 6]
    clean, _ = coded(avr.DeviceWorkload.from_host_keys(slices, gf).resolve_range(), chunked)
    want, _ = rk.resolve(slices, gf)
    assert clean == [oracle.range_encode(r) for r in want]
    k = gf[1] + 1                                                  # the second slice of the second group
    for bad in BAD_RECORDS:
        s = [x.copy() for x in slices]
        assert s[k].size
        s[k][int(rng.integers(0, s[k].size))] = bad
        got, lens = coded(avr.DeviceWorkload.from_host_keys(s, gf).resolve_range(), chunked)
        for i in range(n):
            if k <= i < gf[2]:
                assert got[i] == (b"", rk.BAD_RECORD) and lens[i] == 0, f"slice {i}"
            else:
                assert got[i] == clean[i], f"slice {i}"


@pytest.mark.parametrize("shape", ["short", "long"])
def test_resolve_range_twice_does_not_depend_on_the_workspace(avr, oracle, shape):
    """The second resolve_range() of a workload runs in the workspace the first one left (cached with the plan): the same records,
    tables, statuses and bytes, and also with every byte of that workspace overwritten in between."""
    import torch
    rng = np.random.default_rng(9000 + len(shape))
    slices = route_slices(rng, shape)
    n = len(slices)
    gf = [0, n // 3, n // 2, n]
    tables = [rk.random_table(rng) for _ in range(3)]
    want, want_tabs = rk.resolve(slices, gf, tables)
    want_bytes = [oracle.range_encode(r) for r in want]
    kw = avr.DeviceWorkload.from_host_keys(slices, gf, tables)
    ws = None
    for poison in (None, 0xFF, 0x00, 0x5A):
        if poison is not None:
            assert kw._chunk_plan()["ws_est"] is ws
            ws.fill_(poison)
            kw.rec_flat.fill_(np.array(FILL, np.uint16).view(np.int16).item())
            kw.est_out.fill_(0xCC)
        rw = kw.resolve_range()
        torch.cuda.synchronize()
        ws = kw._chunk_plan()["ws_est"]
        recs, rec_off, n_bins = rw.rec_flat.cpu().numpy().view(np.uint16), kw.rec_off.cpu().numpy(), kw.n_bins.cpu().numpy()
        for i in range(n):
            o, nb = int(rec_off[i]), int(n_bins[i])
            assert np.array_equal(recs[o:o + nb], want[i]) and not recs[o + nb:(o + nb + 7) // 8 * 8].any(), f"slice {i} after poison {poison}"
        est = kw.est_out.cpu().numpy().reshape(-1, rk.N_KEYS, 2)
        assert all(np.array_equal(est[g], want_tabs[g]) for g in range(3))
        got, _ = coded(rw, shape == "long")
        assert got == want_bytes, f"after poison {poison}"


# ------------------------------------------------------------------ D: one avr_batch reused

def fill_keys(b, slices, group_first, tables=None):
    g = 0
    for i, s in enumerate(slices):
        while g < len(group_first) - 1 and group_first[g] == i:
            assert b.begin_group(None if tables is None else tables[g]) == g
            g += 1
        assert b.add_slice_range_keys(s) == i


def test_one_batch_reused_for_changing_shapes_and_kinds(avr, oracle):
    """One Batch through five runs with reset between them; each run equals the same run on a fresh Batch and the oracle's coding of the
    rule's records, and get_estimators gives the tables of the run at hand."""
    rng = np.random.default_rng(9100)
    MAX = 64
    mk = lambda n, lo, hi: [rk.random_keys(rng, int(rng.integers(lo, hi)), "skew") for _ in range(n)]
    runs = [("keys", mk(12, 0, 3000), [0, 4, 9, 12], True),          # start tables: d_est_in in use
            ("keys", mk(MAX, 100, 6000), list(range(MAX + 1)), False),   # more groups (as many as max_slices) and more bins, all fresh
            ("range", None, None, False),
            ("keys", mk(5, 20000, 40000), [0, 5], False),            # fewer groups, few long slices (K2p)
            ("keys", mk(20, 0, 2000), [0, 7, 7, 20], True)]          # tables again, a group without slices among them
    with avr.Batch(0, MAX, 1 << 21) as b:
        for r, (kind, slices, gf, with_tables) in enumerate(runs):
            if r:
                b.reset()
            if kind == "range":
                recs = [w for w in rk.resolve(mk(30, 0, 3000), [0, 30])[0]]
                for x in recs:
                    b.add_slice_range(x)
                b.run()
                got = [b.get(i) for i in range(len(recs))]
                assert got == [oracle.range_encode(x) for x in recs] and got == run_range(avr, recs), f"run {r}"
                with pytest.raises(avr.AvrError, match="not a batch of key records"):
                    b.get_estimators(0)
                continue
            tables = [rk.random_table(rng) for _ in range(len(gf) - 1)] if with_tables else None
            want, want_tabs = rk.resolve(slices, gf, tables)
            fill_keys(b, slices, gf, tables)
            b.run()
            got = [b.get(i) for i in range(len(slices))]
            tabs = [b.get_estimators(g) for g in range(len(gf) - 1)]
            again = [b.get_estimators(g) for g in range(len(gf) - 1)]
            fresh, _, fresh_tabs, _ = run_keys(avr, slices, gf, tables)
            assert got == fresh and got == [oracle.range_encode(x) for x in want], f"run {r}"
            for g in range(len(gf) - 1):
                assert np.array_equal(tabs[g], want_tabs[g]) and np.array_equal(again[g], tabs[g]) and np.array_equal(fresh_tabs[g], tabs[g]), f"run {r} group {g}"
        # get_estimators before and after a further run: each run's own tables (the first fetch is not kept across a run)
        before = b.get_estimators(0)
        assert np.array_equal(before, want_tabs[0])
        b.reset()
        slices, gf = mk(9, 0, 2500), [0, 2, 9]
        want, want_tabs = rk.resolve(slices, gf)
        fill_keys(b, slices, gf)
        b.run()
        after = [b.get_estimators(g) for g in range(2)]
        assert np.array_equal(after[0], want_tabs[0]) and np.array_equal(after[1], want_tabs[1]) and not np.array_equal(after[0], before)
        assert np.array_equal(b.get_estimators(0), after[0])
        assert [b.get(i) for i in range(9)] == [oracle.range_encode(x) for x in want]
