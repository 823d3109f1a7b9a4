"""GPU: one-byte key records (AVR_KIND_RANGE_KEYS8) through the device calls, DeviceWorkload and the batch API.

Expected answers never come from the code under test: the serial Python rule of tests/range_keys.py (resolve) on the widened records,
for the long cases the compiled plain rule (range_keys.plain_resolve, tests/est_plain.cpp), for bytes the oracle's range coder.  Every
case also runs the two-byte route on the widened stream: resolved records, est_out[:128], coded bytes, lengths and statuses are
identical.  Every padding byte and gap of the one-byte input holds non-zero garbage (range_keys8.layout8 / garbage)."""
import ctypes

import numpy as np
import pytest

import guarded
import range_keys as rk
import range_keys8 as rk8

pytestmark = pytest.mark.gpu

FILL = 0xABCD
FILL16 = int(np.array(FILL, np.uint16).view(np.int16))
NONE, OK, BAD, VERIFY_FAILED = 0xFFFFFFFF, 0, 3, 4


def workloads(avr, slices8, gf, tables8, rng, gap=0, plan="torch"):
    """the one-byte workload and the two-byte one of the widened stream, recs_out preset to FILL and est_out to 0xCC"""
    w8 = avr.DeviceWorkload.from_host_keys8(slices8, gf, tables8, 0, gap, plan, pad_bytes=rk8.garbage(rng, 4099))
    w16 = avr.DeviceWorkload.from_host_keys([rk8.widen(s) for s in slices8], gf, rk8.widen_tables(tables8), 0, gap)
    for w in (w8, w16):
        w.rec_flat.fill_(FILL16)
        w.est_out.fill_(0xCC)
    return w8, w16


def host(w, n_keys):
    import torch
    torch.cuda.synchronize()
    return (w.rec_flat.cpu().numpy().view(np.uint16), w.status.cpu().numpy(), w.est_out.cpu().numpy().reshape(-1, n_keys, 2),
            w.rec_off.cpu().numpy(), w.n_bins.cpu().numpy())


def compare_routes(avr, oracle, slices8, gf, tables8=None, gap=0, plan="torch", rule="python", seed=1, encode=("tiles", "chunked"),
                   oracle_slices=20):
    rng = np.random.default_rng(seed)
    w8, w16 = workloads(avr, slices8, gf, tables8, rng, gap, plan)
    r8, r16 = w8.resolve_range(), w16.resolve_range()
    out8, st8, est8, off8, nb = host(w8, rk8.N_KEYS8)
    out16, st16, est16, off16, _ = host(w16, rk.N_KEYS)
    n = len(slices8)
    # against the rule
    if rule == "python":
        want, want_tabs = rk.resolve([rk8.widen(s) for s in slices8], gf, rk8.widen_tables(tables8))
        exp, mask = rk8.expected_records(want, off8, nb, out8.size, FILL)
        diff = np.flatnonzero((out8 != exp) & mask)
        assert diff.size == 0, f"first difference at record {diff[0]}: {out8[diff[0]]:#x} != {exp[diff[0]]:#x} ({diff.size} in all)"
        assert st8.tolist() == [OK] * n
        for g, t in enumerate(want_tabs):
            assert np.array_equal(est8[g], t[:rk8.N_KEYS8]), f"table of group {g}"
    else:
        keys16 = rk8.widened_layout(w8.key_flat.cpu().numpy(), off8, nb)
        est_in = None if tables8 is None else np.stack(rk8.widen_tables(tables8))
        exp, exp_st, exp_est = rk.plain_resolve(keys16, off8, nb, gf, est_in, FILL)
        diff = np.flatnonzero(out8 != exp)
        assert diff.size == 0, f"first difference at record {diff[0]}: {out8[diff[0]]:#x} != {exp[diff[0]]:#x} ({diff.size} in all)"
        assert st8.tolist() == exp_st.tolist() == [OK] * n
        assert np.array_equal(est8, exp_est[:, :rk8.N_KEYS8])
        want = [exp[int(off8[i]):int(off8[i]) + int(nb[i])] for i in range(n)]
    # against the two-byte route
    assert st16.tolist() == st8.tolist()
    assert np.array_equal(est16[:, :rk8.N_KEYS8], est8)
    for i in range(n):
        k = (int(nb[i]) + 7) // 8 * 8
        assert np.array_equal(out8[int(off8[i]):int(off8[i]) + k], out16[int(off16[i]):int(off16[i]) + k]), f"slice {i}"
    # the checker is content, and changes nothing
    status, first_bad = w8.verify_keys()
    assert (first_bad.cpu().numpy() == -1).all() and status.cpu().numpy().tolist() == [OK] * n
    # the coded bytes
    for mode in encode:
        for r in (r8, r16):
            r.encode() if mode == "tiles" else r.encode_chunked()
        got8, got16 = r8.results(), r16.results()
        assert got8 == got16, mode
        for i in list(range(n))[:oracle_slices]:
            assert (got8[0][i], got8[1][i]) == oracle.range_encode(want[i]), f"{mode}, slice {i}"
    return est8


# ------------------------------------------------------------------ short groups, one wave each

SHORT = [0, 1, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025]


@pytest.mark.parametrize("groups", ["each", "threes"])
@pytest.mark.parametrize("plan", ["torch", "device"])
def test_short_groups(avr, oracle, groups, plan):
    rng = np.random.default_rng(8801)
    lens = SHORT + [1] if groups == "threes" else SHORT
    slices = [rk8.random_keys8(rng, n, "skew" if i % 2 else "flat") for i, n in enumerate(lens)]
    gf = list(range(len(lens) + 1)) if groups == "each" else list(range(0, len(lens) + 1, 3))
    compare_routes(avr, oracle, slices, gf, seed=1, plan=plan)
    tables = [rk8.random_table8(rng) for _ in range(len(gf) - 1)]
    compare_routes(avr, oracle, slices, gf, tables, gap=0 if plan == "device" else 2, seed=2, plan=plan)


# ------------------------------------------------------------------ window seams (a window is 16 chunks)

@pytest.mark.parametrize("given", [False, True])
def test_one_group_over_two_windows_with_a_hot_key(avr, oracle, given):
    rng = np.random.default_rng(8802)
    slices = [rk8.random_keys8(rng, n, "skew") for n in (13000, 14001, 13003)]       # 13 + 14 + 13 chunks: windows 0, 1 and 2
    hot = slices[1].copy()
    hot[::3] = (hot[::3] & 1) | (5 << 1)                         # key 5 every third bin: 21 to a step, halvings fall inside steps
    slices[1] = hot
    assert rk.row_plan([len(s) for s in slices], [0, 3])["rows"] == [3]
    compare_routes(avr, oracle, slices, [0, 3], [rk8.random_table8(rng)] if given else None, rule="python", plan="device" if given else "torch")


@pytest.mark.parametrize("name", ["two_heads", "empties"])
def test_groups_that_meet_mid_window_and_empty_groups(avr, oracle, name):
    slices, gf = rk8.narrow_case(rk.row_block_case(name))
    assert rk.row_plan(slices, gf)["rows"] == rk.ROW_BLOCK_PLANS[name][0]
    compare_routes(avr, oracle, slices, gf, rule="plain", encode=("tiles",), oracle_slices=8)


# ------------------------------------------------------------------ block seams (a block is 64 rows)

@pytest.mark.parametrize("name", [f"rows{n}{m}" for n in (64, 65, 128, 129) for m in ("", "mid")])
def test_groups_of_64_65_128_and_129_rows(avr, oracle, name):
    slices, gf = rk8.narrow_case(rk.row_block_case(name))
    plan = rk.row_plan(slices, gf)
    assert (plan["rows"], plan["later_blocks"]) == rk.ROW_BLOCK_PLANS[name][:2]
    rng = np.random.default_rng(8803)
    tables = [rk8.random_table8(rng) for _ in range(len(gf) - 1)]
    compare_routes(avr, oracle, slices, gf, tables, rule="plain", encode=("tiles",), oracle_slices=4)


# ------------------------------------------------------------------ exact sizes between canaries, dirty, on a stream of the caller's own; a misaligned rec_off

def guarded_case(avr, misalign):
    import torch
    rng = np.random.default_rng(8804)
    lens = [700, 0, 20000, 1500, 33, 17000, 9]                   # a group inside a window, one of three slices over two windows, one more
    gf = [0, 2, 5, 7]
    slices = [rk8.random_keys8(rng, n, "skew") for n in lens]
    tables = [rk8.random_table8(rng) for _ in range(3)]
    w = avr.DeviceWorkload.from_host_keys8(slices, gf, tables, 0, 1, "torch", pad_bytes=rk8.garbage(rng, 4099))
    if misalign:
        w.rec_off[3] += 8                                        # the middle slice of the three-slice group: 8 mod 16 (its gap has the room)
    dev = w.n_bins.device
    L, p = avr.lib(), w._chunk_plan()
    p["ws_est_bytes"] = L.avr_range_resolve8_workspace_bytes(w.n_slices, w.n_groups, ctypes.byref(p["plan"]))
    p["ws_estv_bytes"] = L.avr_range_keys8_verify_workspace_bytes(w.n_slices, w.n_groups, ctypes.byref(p["plan"]))
    assert p["ws_est_bytes"] == rk8.resolver_quote(w.n_slices, w.n_groups, p["plan"].total_chunks)
    assert p["ws_estv_bytes"] == rk8.checker_quote(w.n_slices, p["plan"].total_chunks)
    n_recs = int(w.rec_off[-1])
    gs = dict(ws_est=guarded.Guarded(p["ws_est_bytes"], dev, "ws_est"), ws_estv=guarded.Guarded(p["ws_estv_bytes"], dev, "ws_estv"),
              recs_out=guarded.Guarded(2 * n_recs, dev, "recs_out"), est_out=guarded.Guarded(w.n_groups * rk8.N_KEYS8 * 2, dev, "est_out"))
    p["ws_est"], p["ws_estv"] = gs["ws_est"].view, gs["ws_estv"].view
    w.rec_flat, w.est_out = gs["recs_out"].as_dtype(torch.int16), gs["est_out"].view
    return w, gs, slices, gf, tables


@pytest.mark.parametrize("misalign", [False, True])
def test_exact_workspaces_between_canaries_dirty_on_an_own_stream(avr, misalign):
    import torch
    w, gs, slices, gf, tables = guarded_case(avr, misalign)
    want, want_tabs = rk.resolve([rk8.widen(s) for s in slices], gf, rk8.widen_tables(tables))
    bad = [3, 4] if misalign else []
    for i in bad:
        want[i] = None
    rec_off, nb = w.rec_off.cpu().numpy(), w.n_bins.cpu().numpy()
    stream = torch.cuda.Stream()                                 # (torch's streams are non-blocking ones)
    for poison in (0x00, 0xFF, 0x5A):
        with torch.cuda.stream(stream):
            for g in gs.values():
                g.view.fill_(poison)
            w.status.zero_()
            w.resolve_keys()
            resolved = w.status.clone()
            status, first_bad = w.verify_keys()
            stream.synchronize()
        for g in gs.values():
            g.check()
        out = w.rec_flat.cpu().numpy().view(np.uint16)
        exp, mask = rk8.expected_records(want, rec_off, nb, out.size, poison | poison << 8)
        diff = np.flatnonzero((out != exp) & mask)
        assert diff.size == 0, f"poison {poison:#x}: first difference at record {diff[0]} ({diff.size} in all)"
        if misalign:                                             # nothing of the misaligned slice is written
            o = int(rec_off[3])
            assert (out[o:o + (int(nb[3]) + 7) // 8 * 8] == (poison | poison << 8)).all()
        expect_status = [BAD if i in bad else OK for i in range(len(slices))]
        assert resolved.cpu().numpy().tolist() == expect_status
        assert status.cpu().numpy().tolist() == expect_status   # the checker: no finding, bad slices take no part
        assert (first_bad.cpu().numpy() == -1).all()
        est = w.est_out.cpu().numpy().reshape(-1, rk8.N_KEYS8, 2)
        for g, t in enumerate(want_tabs):
            if not (misalign and g == 1):
                assert np.array_equal(est[g], t[:rk8.N_KEYS8]), f"table of group {g}"


def test_misaligned_slice_its_group_and_the_others_as_bytes(avr, oracle):
    """the first slice of the misaligned slice's group and the other groups are CODED: the oracle's bytes; the bad ones have length 0"""
    w, gs, slices, gf, tables = guarded_case(avr, True)
    want, _ = rk.resolve([rk8.widen(s) for s in slices], gf, rk8.widen_tables(tables))
    w.rec_flat.fill_(0x5A5A)                                     # what the resolver leaves alone reads as a valid K2 record
    for mode in ("tiles", "chunked"):
        r = w.resolve_range()
        r.encode() if mode == "tiles" else r.encode_chunked()
        data, status = r.results()
        for g in gs.values():
            g.check()
        for i in range(len(slices)):
            if i in (3, 4):
                assert (data[i], status[i]) == (b"", BAD), f"{mode}, slice {i}"
            else:
                assert (data[i], status[i]) == oracle.range_encode(want[i]), f"{mode}, slice {i}"


def test_checker_fails_a_misaligned_slice_that_takes_part_at_bin_0(avr):
    """the checker's own rule for a rec_off off its multiple of 16 (the resolver's verdict wiped: status zeroed, so the slice takes part):
    a finding at bin 0 and AVR_SLICE_VERIFY_FAILED without reading the slice, in k_estv_check, and no entry of its in k_estv_last (the
    group crosses a span); the slice before it in the group and the other groups have no finding"""
    import torch
    w, gs, slices, gf, tables = guarded_case(avr, True)
    w.status.zero_()
    w.resolve_keys()
    w.status.zero_()
    status, first_bad = w.verify_keys()
    torch.cuda.synchronize()
    for g in gs.values():
        g.check()
    status, first_bad = status.cpu().numpy().tolist(), first_bad.cpu().numpy().tolist()
    assert (first_bad[3], status[3]) == (0, VERIFY_FAILED)
    for i in (0, 1, 2, 5, 6):                                    # (slice 4 follows the unread slice in its group: its table is not the resolver's)
        assert (first_bad[i], status[i]) == (-1, OK), f"slice {i}"


# ------------------------------------------------------------------ the batch API

SHAPES = {"lanes": (90, 0, 1500), "k2p": (5, 9000, 14000)}       # (slices, shortest, longest): either side of the batch's rule


def shape_slices(rng, path):
    n, lo, hi = SHAPES[path]
    slices = [rk8.random_keys8(rng, int(rng.integers(lo, hi)), "skew") for _ in range(n)]
    if path == "lanes":
        slices[5] = slices[5][:0]
    return slices


def run_batch(avr, slices, gf, tables=None, one_byte=True, verify=None, reserve=False, batch=None):
    """a batch of key records, one-byte or the widened stream as two-byte ones; `batch`: an object to reuse (reset first)"""
    b = batch if batch is not None else avr.Batch(0, len(slices), sum(len(s) for s in slices) + 8)
    try:
        if batch is not None:
            b.reset()
        if verify is not None:
            b.set_verify(verify)
        g = 0
        for i, s in enumerate(slices):
            while g < len(gf) - 1 and gf[g] == i:
                t = None if tables is None else tables[g]
                assert (b.begin_group8(t) if one_byte else b.begin_group(rk8.widen_table(t) if t is not None else None)) == g
                g += 1
            if reserve:
                idx, view = b.reserve(avr.KIND_RANGE_KEYS8 if one_byte else avr.KIND_RANGE_KEYS, len(s))
                view[:] = s
                assert idx == i and view.dtype == (np.uint8 if one_byte else np.uint16)
            else:
                assert (b.add_slice_range_keys8(s) if one_byte else b.add_slice_range_keys(rk8.widen(s))) == i
        b.submit()
        b.wait()
        n = range(len(slices))
        tabs = [b.get_estimators(k) for k in range(len(gf) - 1)]
        assert all(t.shape == ((rk8.N_KEYS8 if one_byte else rk.N_KEYS), 2) for t in tabs)
        return dict(got=[b.get(i) for i in n], chunked=b.run_info()["chunked"], tabs=[t[:rk8.N_KEYS8] for t in tabs],
                    fb=[b.get_verify(i) for i in n], est=[b.get_verify_est(i) for i in n], h2d=b.timings()["h2d_ms"])
    finally:
        if batch is None:
            b.close()


def same(a, b):
    return all(a[k] == b[k] for k in ("got", "chunked", "fb", "est")) and all(np.array_equal(x, y) for x, y in zip(a["tabs"], b["tabs"]))


@pytest.mark.parametrize("path", ["lanes", "k2p"])
def test_batch_on_both_k2_paths_verify_off_and_on_and_the_reserve_form(avr, oracle, path):
    rng = np.random.default_rng(8810 + len(path))
    slices = shape_slices(rng, path)
    n = len(slices)
    for gf in (list(range(n + 1)), [0, n], [0, n // 3, n // 2, n]):
        tables = [rk8.random_table8(rng) for _ in range(len(gf) - 1)] if len(gf) == 4 else None
        want, want_tabs = rk.resolve([rk8.widen(s) for s in slices], gf, rk8.widen_tables(tables))
        coded = [oracle.range_encode(w) for w in want]
        two = run_batch(avr, slices, gf, tables, one_byte=False, verify=True)
        for verify, reserve in ((None, False), (True, False), (False, True)):
            one = run_batch(avr, slices, gf, tables, verify=verify, reserve=reserve)
            assert one["chunked"] == int(path == "k2p")          # the path this shape is meant to take did run
            assert one["got"] == coded
            assert one["fb"] == one["est"] == [NONE] * n
            assert same(one, two)
            for g in range(len(gf) - 1):
                assert np.array_equal(one["tabs"][g], want_tabs[g][:rk8.N_KEYS8])


@pytest.mark.parametrize("path", ["lanes", "k2p"])
def test_hooks_plant_a_fault_only_the_estimator_checker_sees(avr, oracle, hooks, path):
    rng = np.random.default_rng(8820 + len(path))
    slices = shape_slices(rng, path)
    n = len(slices)
    gf = list(range(n + 1))                                      # a group a slice: a planted fault cannot reach another slice's expectations
    k, m = 3, 41
    if path == "lanes":
        slices[k - 1] = rk8.random_keys8(rng, 300, "skew")
    clean = run_batch(avr, slices, gf, verify=True)
    hooks(est_flip=k, est_flip_bin=m)
    one = run_batch(avr, slices, gf, verify=True)
    two = run_batch(avr, slices, gf, one_byte=False, verify=True)
    assert one["chunked"] == int(path == "k2p")
    assert one["fb"] == [NONE] * n                               # the decoder reads the planted pair too: it is content
    assert one["est"] == [m if i == k - 1 else NONE for i in range(n)]
    assert [st for _, st in one["got"]] == [VERIFY_FAILED if i == k - 1 else OK for i in range(n)]
    assert [one["got"][i] for i in range(n) if i != k - 1] == [clean["got"][i] for i in range(n) if i != k - 1]
    assert same(one, two)
    off = run_batch(avr, slices, gf, verify=False)               # with verify off the hook is not read
    assert off["got"] == clean["got"] and off["est"] == [NONE] * n


@pytest.mark.parametrize("path", ["lanes", "k2p"])
def test_group_split_across_two_batches(avr, oracle, path):
    rng = np.random.default_rng(8830 + len(path))
    slices = shape_slices(rng, path)
    n, cut = len(slices), len(slices) // 2
    start = rk8.random_table8(rng)
    whole = run_batch(avr, slices, [0, n], [start])
    first = run_batch(avr, slices[:cut], [0, cut], [start])
    second = run_batch(avr, slices[cut:], [0, n - cut], [first["tabs"][0]])
    assert first["got"] + second["got"] == whole["got"]
    assert np.array_equal(second["tabs"][0], whole["tabs"][0])
    want, want_tabs = rk.resolve([rk8.widen(s) for s in slices], [0, n], [rk8.widen_table(start)])
    assert np.array_equal(whole["tabs"][0], want_tabs[0][:rk8.N_KEYS8])
    assert whole["got"] == [oracle.range_encode(w) for w in want]


def narrow_cabac(recs16):
    sel = recs16 >> 1
    sel8 = np.where(sel == 1024, 126, np.where(sel == 1025, 127, sel))
    return ((recs16 & 1) | (sel8 << 1)).astype(np.uint8)


def test_one_object_reused_keys8_keys_keys8_cabac8(avr, oracle):
    import oracle_lib
    rng = np.random.default_rng(8840)
    a, b, c = (shape_slices(rng, p) for p in ("lanes", "k2p", "lanes"))
    c = c[:40]
    ta = [rk8.random_table8(rng)]
    cabac = [oracle_lib.random_cabac_stream(rng, int(rng.integers(0, 900)), 60) for _ in range(30)]
    fresh = [run_batch(avr, a, [0, len(a)], ta, verify=True), run_batch(avr, b, [0, 2, len(b)], one_byte=False),
             run_batch(avr, c, list(range(len(c) + 1)))]
    with avr.Batch(0, 100, 200000) as obj:
        again = [run_batch(avr, a, [0, len(a)], ta, verify=True, batch=obj), run_batch(avr, b, [0, 2, len(b)], one_byte=False, batch=obj)]
        obj.set_verify(False)
        again.append(run_batch(avr, c, list(range(len(c) + 1)), batch=obj))
        for f, g in zip(fresh, again):
            assert same(f, g)
        obj.reset()
        for r, s in cabac:
            obj.add_slice_cabac8(narrow_cabac(r), s)
        with pytest.raises(avr.AvrError, match="one kind"):
            obj.begin_group8()
        obj.run()
        for i, (r, s) in enumerate(cabac):
            data, status = obj.get(i)
            assert (data, obj.get_states(i), status) == oracle.cabac_encode(r, s), f"K1 slice {i}"
        with pytest.raises(avr.AvrError, match="not a batch of key records"):
            obj.get_estimators(0)


def test_batch_refusals(avr):
    rng = np.random.default_rng(8850)
    keys = rk8.random_keys8(rng, 100, "flat")
    with avr.Batch(0, 8, 4096) as b:
        for entry in ((0, 1), (1, 0), (0x30, 0x31), (0x60, 1)):
            t = np.ones((rk8.N_KEYS8, 2), np.uint8)
            t[127] = entry
            with pytest.raises(avr.AvrError, match="start table entry 127"):
                b.begin_group8(t)
        with pytest.raises(avr.AvrError, match="128 x 2 entries"):
            b.begin_group8(rk.fresh_table())
        assert b.begin_group() == 0                              # nothing was begun by the refused calls: the batch is still of no kind
        with pytest.raises(avr.AvrError, match="avr_batch_begin_group8 on a batch of two-byte key records"):
            b.begin_group8()
        with pytest.raises(avr.AvrError, match="one kind"):
            b.add_slice_range_keys8(keys)
        b.reset()
        t = np.ones((rk8.N_KEYS8, 2), np.uint8)
        t[3] = (0x5f, 1)                                         # pos + neg = 0x60: the largest valid total
        assert b.begin_group8(t) == 0                            # before the first slice: it fixes the batch's kind
        with pytest.raises(avr.AvrError, match="avr_batch_begin_group on a batch of one-byte key records"):
            b.begin_group()
        for other in (lambda: b.add_slice_range_keys(rk8.widen(keys)), lambda: b.add_slice_range(np.zeros(4, np.uint16)),
                      lambda: b.add_slice_cabac8(keys, np.zeros(4, np.uint8)), lambda: b.reserve(avr.KIND_RANGE_KEYS, 8)):
            with pytest.raises(avr.AvrError, match="one kind"):
                other()
        assert b.add_slice_range_keys8(keys) == 0
        assert b.begin_group8() == 1
        b.submit()
        with pytest.raises(avr.AvrError, match="in flight"):
            b.begin_group8()
        with pytest.raises(avr.AvrError, match="in flight"):
            b.add_slice_range_keys8(keys)
        b.wait()
        want, tabs = rk.resolve([rk8.widen(keys)], [0, 1], [rk8.widen_table(t)])
        import oracle_lib
        assert b.get(0) == oracle_lib.load_oracle().range_encode(want[0])
        assert np.array_equal(b.get_estimators(0), tabs[0][:rk8.N_KEYS8])
        assert np.array_equal(b.get_estimators(1), np.ones((rk8.N_KEYS8, 2), np.uint8))     # a group without slices: its start table
        with pytest.raises(avr.AvrError, match="out of range"):
            b.get_estimators(2)
        b.reset()
        b.add_slice_range_keys(rk8.widen(keys))
        with pytest.raises(avr.AvrError, match="avr_batch_begin_group8 on a batch of two-byte key records"):
            b.begin_group8()
        b.reset()
        b.add_slice_range(np.zeros(0, np.uint16))
        with pytest.raises(avr.AvrError, match="one kind"):
            b.begin_group8()
        with pytest.raises(avr.AvrError, match="unknown kind 7"):
            b.reserve(7, 8)
