"""The device planner (csrc/avr_plan_dev.hip) at the seams of its scan, sort and copy -- the paths tests/test_gpu_plan_device.py never
takes, or takes only with values that cannot tell right from wrong:

  wide sums     64-bit sums whose HIGH halves are carried lane to lane (two 32-bit shuffles), wave to wave (LDS), workgroup to workgroup
                (up[]) and through the second level of sums, in the chunk plan (seven sums a slice), the tile plan and the compaction
  scan seams    n on, one below and one above a multiple of the scan's tile of 1024, and of 1024 * 1024
  sort          more than one 256-key tile a workgroup, with keys whose digits differ from tile to tile
  expansion     more chunks than one trip of k_expand's grid (65 536 workgroups of 256) writes
  promises      one workspace and one totals struct through a chain of calls with nothing but stream order between them, behind a sleep
                kernel; totals in pinned host memory; `dense` and `out` at every byte alignment

Every comparison is exact equality, against the torch twins on CPU tensors (chunk_plan_arrays, plan_tiles), numpy int64 prefix sums and
the out_off / rec_off expressions of expected_plan: nothing expected comes from the code under test.  Every condition that says a case
reaches its seam (a prefix above 2^32 at the index that matters, more than 65 536 * 256 chunks, tiles that differ in their digits) is
asserted on that reference BEFORE the first device call, so a case that misses its seam fails.  Buffers are tests/guarded.py's, of the
exact sizes, both poisons of test_gpu_plan_device, one level a case, a stream of its own each call.

That these tests can fail was shown once each on builds with one line changed (values only, every store still inside the caller's
arrays; none of them committed), next to all of tests/test_gpu_plan_device.py on the same build:
  shfl_up64 returning a zero high half           test_wide_sums_serial_level[4097] fails; the older file fails too, in
                                                  test_tile_plans[bit31] alone (its shuffles at distances 1 and 2)
  ... a zero high half at distances 4 to 32       test_wide_sums_serial_level[4097] fails; the older file passes whole
  k_sort_scatter without its `run[t] +=` line    test_sort_many_tiles_a_workgroup[300001-tile-digits] fails; the older file fails too, in
                                                  test_tile_plans[1Mi+65] alone (with no carry at all even one digit collides)
  ... without the reset of cnt between tiles     test_sort_many_tiles_a_workgroup fails at 300 001 under "uniform" and at 2^20 + 65 under all
                                                  three patterns (two tiles that share no digit hide a count left over: the 300 001
                                                  cases of the other two patterns pass); the older file passes whole
  k_expand leaving its loop after the first trip test_expansion_past_one_grid_trip[bounds] fails; the older file passes whole"""
import ctypes
import functools

import numpy as np
import pytest

import guarded
from test_gpu_plan_device import (ERR_CAPACITY, G32, LENGTHS, LEVEL_ARRAYS, OK, POISONS, WIDTH, compact_case, device_lengths, expected_plan,
                                  prefix, run_chunks, run_compact, run_tiles, seeded, serial_offsets)
from test_gpu_workspace import hold                              # noqa: F401 (the sleep-kernel fixture, as that module has it)

pytestmark = pytest.mark.gpu

SCAN_TILE = 1024                                                 # kScanTile: entries a workgroup of the scan takes
MI = 1 << 20                                                     # 1024 workgroups' sums: the second level's first seam
GRID_TRIP = 65536 * 256                                          # chunks one trip of k_expand's grid writes


def first_above(a, bound=G32):
    """The first index of a non-decreasing array whose entry is above `bound`."""
    assert a[-1] > bound
    return int(np.argmax(a > bound))


def check_chunks(got, totals, want, totals_want, level, poison, total_bins, what):
    """What test_chunk_plans asserts of one run: every array of the level equals the reference, what lies behind the totals and every
    array above the level still holds the poison, the seven totals and the untouched eighth."""
    written = [a for lv in range(level + 1) for a in LEVEL_ARRAYS[lv]]
    for a in WIDTH:
        if a not in written:
            assert (got[a].view(np.uint8) == poison).all(), (what, a)
            continue
        m = len(want[a])
        assert np.array_equal(got[a][:m], want[a]), (what, a)
        assert (got[a][m:].view(np.uint8) == poison).all(), (what, a)
    res_total, dig_total, total_chunks, total_blocks = totals_want
    assert totals.tolist()[:7] == [total_bins, want["out_off"][-1], want["rec_off"][-1], res_total if level >= 3 else 0,
                                   dig_total if level >= 2 else 0, total_chunks if level >= 1 else 0, total_blocks if level >= 3 else 0], what
    assert totals[7:].tobytes() == bytes([poison]) * 8, what


# ------------------------------------------------------------------ wide sums

@pytest.mark.parametrize("n", [4097, MI + 1])
def test_wide_sums_serial_level(avr, n):
    """Lengths over the whole 32 bits: out_off and rec_off reach 2^52, and from the third slice or so on EVERY prefix has a high half
    -- the sums a thread hands the next lane, a wave the next wave, a workgroup the next (up[]) and, at 2^20 + 1, the first 1024
    workgroups the 1025th.  (The first index above 2^32 therefore lies far in front of 1024 here; that it lies behind 1024, so that
    the high half is BORN in the carry between workgroups, is the K1P case's condition below.)"""
    import torch
    lengths = np.random.default_rng(200 + n).integers(0, G32, n).astype(np.int64)
    total_bins = int(lengths.sum())
    want = {r: dict(zip(("out_off", "rec_off"), serial_offsets(lengths, r))) for r in (8, 16)}
    for r in (8, 16):
        for a, w in want[r].items():
            assert w.dtype == np.int64 and w[-1] > G32 and w[-1] < 1 << 62
            at = [8, 256, SCAN_TILE, SCAN_TILE + 8, SCAN_TILE + 256, 4096] + ([MI, MI - SCAN_TILE] if n > MI else [])
            assert (w[at] > G32).all(), (a, "a carry across lanes, waves, workgroups or the second level without a high half")
            local = w[SCAN_TILE:2 * SCAN_TILE] - w[SCAN_TILE]   # the sums inside workgroup 1, before up[] is added
            assert local[8] > G32 and local[256] > G32
    ints = lengths.tolist()
    assert int(want[8]["out_off"][-1]) == sum((x + 16 + 7) // 8 * 8 for x in ints) > 1 << 42 and total_bins == sum(ints)
    assert int(want[16]["rec_off"][-1]) == sum((x + 15) // 16 * 16 for x in ints)
    n_bins = device_lengths(torch, lengths)
    for r in (8, 16):
        runs = [run_chunks(avr, torch, n_bins, total_bins, 0, r, p, caps=(0, 0)) for p in POISONS]
        for (got, totals, _, _), poison in zip(runs, POISONS):
            for a in ("out_off", "rec_off"):
                assert np.array_equal(got[a], want[r][a]), (r, a, poison)
            for a in WIDTH:
                if a not in LEVEL_ARRAYS[0]:
                    assert (got[a].view(np.uint8) == poison).all(), a
            assert totals.tolist()[:7] == [total_bins, want[r]["out_off"][-1], want[r]["rec_off"][-1], 0, 0, 0, 0]
            assert totals[7:].tobytes() == bytes([poison]) * 8


@pytest.mark.parametrize("top", [4_000_000, 6_000_000])
def test_wide_sums_k1p_level(avr, top):
    """4097 slices of up to 4 000 000 bins: no workgroup's own sum reaches 2^32, the prefix passes it in the middle of the array --
    behind index 1024 -- so the high half comes into being in the scan of the workgroups' sums and reaches the entries through up[].
    All seven quantities go through the one sweep; chunk_base and blk_base stay far below 2^32, chunk_slice has about 8 Mi entries.
    With these lengths dig_off (n_bins / 2 + 8 a slice) ends at about 4.10e9, below 2^32 = 4.29e9, whatever the seed: the second case,
    up to 6 000 000 bins, is there for it -- dig_off then passes 2^32 near index 2860 and out_off still behind index 1024."""
    import torch
    n = 4097
    lengths = seeded(n, top, 300 + top // 1_000_000)
    total_bins = int(lengths.sum())
    want, totals_want = expected_plan(torch, lengths, 8)
    wide = ("out_off", "rec_off", "res_off") + (("dig_off",) if top > 4_000_000 else ())
    for a in wide:
        assert want[a].dtype == np.int64 and want[a][-1] > G32 and SCAN_TILE < first_above(want[a]) < n, a
    assert want["dig_off"][-1] > (G32 if top > 4_000_000 else 1 << 31)
    assert 0 < want["chunk_base"][-1] == totals_want[2] < 1 << 25 and 0 < want["blk_base"][-1] == totals_want[3] < 1 << 23
    assert len(want["chunk_slice"]) == totals_want[2] > 7 << 20
    n_bins = device_lengths(torch, lengths)
    runs = [run_chunks(avr, torch, n_bins, total_bins, 3, 8, p) for p in POISONS]
    for (got, totals, _, _), poison in zip(runs, POISONS):
        check_chunks(got, totals, want, totals_want, 3, poison, total_bins, (top, poison))


def test_wide_sums_tile_plan(avr):
    """70 000 lengths over the whole 32 bits: 1094 tiles -- two workgroups of scan<1> -- and the first tile alone is longer than 2^32
    chunks, so every sum that moves between lanes, waves and the two workgroups has a high half."""
    import torch
    from avrecode_ms_amd.device import plan_tiles
    n = 70000
    lengths = np.random.default_rng(41).integers(0, G32, n).astype(np.int64)
    want = {per_chunk: [x.numpy() for x in plan_tiles(torch.from_numpy(lengths), per_chunk)] for per_chunk in (8, 16)}
    for want_order, want_tile_off in want.values():
        sizes = np.diff(want_tile_off)
        assert len(sizes) == 1094 > SCAN_TILE and sizes[0] > G32 and (want_tile_off[1:] > G32).all() and want_tile_off[-1] > 1 << 42
        assert sorted(want_order.tolist()) == list(range(n))
    n_bins = device_lengths(torch, lengths)
    for per_chunk, (want_order, want_tile_off) in want.items():
        runs = [run_tiles(avr, torch, n_bins, per_chunk, p) for p in POISONS]
        for (order, tile_off, totals), poison in zip(runs, POISONS):
            assert np.array_equal(order, want_order) and np.array_equal(tile_off, want_tile_off), per_chunk
            assert totals[7] == want_tile_off[-1] and totals[:7].tobytes() == bytes([poison]) * 56


@pytest.mark.parametrize("n", [4097, MI + 1])
def test_wide_sums_compaction(avr, n):
    """dense_off of regions of up to 2^32 + 8 bytes and lengths over the whole 32 bits, some above their region (clamped), some 0:
    it ends above 2^40.  dense_capacity is 0, so no slice is copied and `out` (16 bytes) is never read."""
    import torch
    rng = np.random.default_rng(500 + n)
    region = rng.integers(0, (G32 + 8) // 8 + 1, n).astype(np.int64) * 8
    region[[5, 1023, 1024, n - 1]] = G32 + 8
    region[[6, 2048]] = 0
    out_len = rng.integers(0, G32, n).astype(np.int64)
    out_len[[5, 1024]] = G32 - 1
    out_len[::11] = 0
    out_off = 8 + prefix(region)
    take = np.minimum(out_len, region)
    want_off = prefix(take)
    assert region.max() == G32 + 8 and (region % 8 == 0).all() and out_len.max() == G32 - 1
    assert (out_len > region).sum() > n // 4 and (take == 0).sum() > n // 12 and (take == region)[out_len > region].all()
    assert want_off[-1] > 1 << 40 and (want_off[[8, 256, SCAN_TILE, n - 1]] > G32).all() and (n <= MI or want_off[MI] > G32)
    out = torch.zeros(16, dtype=torch.uint8, device="cuda")
    for poison in POISONS:
        dense, dense_off = run_compact(avr, torch, out, out_off, out_len, 0, poison)
        assert dense.size == 0 and np.array_equal(dense_off, want_off), poison


# ------------------------------------------------------------------ the scan at its tile seams

def small_regions(n, seed):
    """n regions of 8 to 32 bytes at 8 mod 16 with real bytes in them; lengths of 0, of the whole region, above it, and in between.
    Returns (out, out_off, out_len, dense_off wanted, dense wanted)."""
    rng = np.random.default_rng(seed)
    region = rng.integers(1, 5, n).astype(np.int64) * 8
    out_off = 8 + prefix(region)
    out_len = rng.integers(0, region + 5)
    out_len[::7] = 0
    out_len[1::7] = region[1::7]
    take = np.minimum(out_len, region)
    want_off = prefix(take)
    out = rng.integers(0, 256, int(out_off[-1]), dtype=np.uint8)
    src = np.repeat(out_off[:-1] - want_off[:-1], take) + np.arange(int(want_off[-1]))    # dense byte k comes from out[src[k]]
    return out, out_off, out_len.astype(np.int64), want_off, out[src]


@pytest.mark.parametrize("n", [1023, 1024, 1025, 2047, 2048, 2049, MI - 1, MI, MI + 1])
def test_scan_seams(avr, n):
    """The closing entry in a workgroup's last thread (n a multiple of 1024), in the first thread of one more workgroup (one above),
    a top level of exactly 1024 sums (2^20) and a second level of two (2^20 + 1): all three scans -- seven sums a slice, the
    tiles' (n here chosen for the slices; the tile scan runs over ceil(n / 64)), the lengths'."""
    import torch
    from avrecode_ms_amd.device import plan_tiles
    lengths = seeded(n, 200000 if n < 4096 else 3000, 600 + n % 1000)
    total_bins = int(lengths.sum())
    want, totals_want = expected_plan(torch, lengths, 8)
    assert len(want["out_off"]) == n + 1 and totals_want[2] < 4 << 20
    n_bins = device_lengths(torch, lengths)
    for poison in POISONS:
        got, totals, _, _ = run_chunks(avr, torch, n_bins, total_bins, 3, 8, poison)
        check_chunks(got, totals, want, totals_want, 3, poison, total_bins, (n, poison))
    want_order, want_tile_off = (x.numpy() for x in plan_tiles(torch.from_numpy(lengths), 8))
    for poison in POISONS:
        order, tile_off, totals = run_tiles(avr, torch, n_bins, 8, poison)
        assert np.array_equal(order, want_order) and np.array_equal(tile_off, want_tile_off), (n, poison)
        assert totals[7] == want_tile_off[-1] and totals[:7].tobytes() == bytes([poison]) * 56
    out, out_off, out_len, want_off, want_dense = small_regions(n, 700 + n % 1000)
    d_out = torch.from_numpy(out).cuda()
    for poison in POISONS:
        dense, dense_off = run_compact(avr, torch, d_out, out_off, out_len, int(want_off[-1]), poison)
        assert np.array_equal(dense_off, want_off) and np.array_equal(dense, want_dense), (n, poison)


@pytest.mark.parametrize("n_tiles", [1023, 1024, 1025])
def test_tile_scan_seams(avr, n_tiles):
    """The tile scan's own seam: ceil(n / 64) on and around 1024, with a last tile of one slice."""
    import torch
    from avrecode_ms_amd.device import plan_tiles
    n = 64 * (n_tiles - 1) + 1
    lengths = seeded(n, 200000, 800 + n_tiles)
    want_order, want_tile_off = (x.numpy() for x in plan_tiles(torch.from_numpy(lengths), 16))
    assert len(want_tile_off) == n_tiles + 1
    n_bins = device_lengths(torch, lengths)
    for poison in POISONS:
        order, tile_off, totals = run_tiles(avr, torch, n_bins, 16, poison)
        assert np.array_equal(order, want_order) and np.array_equal(tile_off, want_tile_off), poison
        assert totals[7] == want_tile_off[-1]


# ------------------------------------------------------------------ the sort: more than one tile a workgroup

def sort_keys(n, pattern):
    rng = np.random.default_rng(900 + n % 1000)
    if pattern == "uniform":
        return rng.integers(0, G32, n).astype(np.int64)
    if pattern == "top-byte":                                     # only the last pass orders anything: stability decides the rest
        return (rng.integers(0, 8, n).astype(np.int64) << 24) | 0x00ABCDEF
    tile = np.arange(n) // 256                                    # "tile-digits": tile j holds only digits = j mod 3, in the second pass
    return ((tile % 3 + 3 * rng.integers(0, 85, n)).astype(np.int64)) << 8


@pytest.mark.parametrize("pattern", ["uniform", "top-byte", "tile-digits"])
@pytest.mark.parametrize("n", [300001, MI + 65])
def test_sort_many_tiles_a_workgroup(avr, n, pattern):
    """300 001 keys: 1024 workgroups of two tiles, the last ones empty; 2^20 + 65: five tiles.  A workgroup's place for a digit is carried
    from tile to tile in run[] and the per-wave counts are reset in between: with digits that are absent from one tile and present in
    the next, a wrong carry or a count left over puts keys in the wrong place -- in `order`, and through it in tile_off."""
    import torch
    from avrecode_ms_amd.device import plan_tiles
    tiles = (n + 255) // 256
    per_block = (tiles + 1023) // 1024 * 256
    assert tiles > 1024 and per_block == (512 if n == 300001 else 1280) and 1024 * per_block >= n + per_block    # a workgroup at the end is empty
    lengths = sort_keys(n, pattern)
    assert lengths.min() >= 0 and lengths.max() < G32
    digits = np.stack([(lengths >> s) & 255 for s in (0, 8, 16, 24)])
    if pattern == "uniform":
        assert all(len(np.unique(d)) == 256 for d in digits)
    elif pattern == "top-byte":
        assert [len(np.unique(d)) for d in digits] == [1, 1, 1, 8]
    else:
        assert (digits[1] % 3 == (np.arange(n) // 256) % 3).all() and len(np.unique(digits[1])) == 255
        held = [set(digits[1][k:k + 256].tolist()) for k in range(0, 4 * 256, 256)]
        assert all(a and b and not a & b for a, b in zip(held, held[1:]))          # consecutive tiles share no digit
    want_order, want_tile_off = (x.numpy() for x in plan_tiles(torch.from_numpy(lengths), 8))
    assert (want_order != np.arange(n)).sum() > n // 2            # (the sort has work to do)
    n_bins = device_lengths(torch, lengths)
    for poison in POISONS:
        order, tile_off, totals = run_tiles(avr, torch, n_bins, 8, poison)
        assert np.array_equal(order, want_order), (pattern, poison, int(np.argmax(order != want_order)))
        assert np.array_equal(tile_off, want_tile_off) and totals[7] == want_tile_off[-1], (pattern, poison)


# ------------------------------------------------------------------ the expansion past one trip of its grid

TRIP_LENGTHS = np.array([G32 - 1, 7, G32 - 1, 0, G32 - 1, 1025, G32 - 1, G32 - 1], np.int64)


@functools.lru_cache(maxsize=None)
def trip_reference():
    import torch
    return expected_plan(torch, TRIP_LENGTHS, 8)


@pytest.mark.parametrize("cap", ["bounds", "one-trip-and-three"])
def test_expansion_past_one_grid_trip(avr, cap):
    """20 971 524 chunks: k_expand's grid is 65 536 workgroups, so the entries from 16 777 216 on are written on its second trip.  With
    the caps avr_plan_bounds gives, chunk_slice and blk_slice equal the twin's and what lies behind the totals keeps the poison; with
    cap_chunks three into the second trip, every entry below the cap is right, the guard behind it holds, the totals are the true ones
    and avr_chunk_plan_from refuses the plan."""
    import torch
    L = avr.lib()
    want, totals_want = trip_reference()
    total_bins = int(TRIP_LENGTHS.sum())
    total_chunks, total_blocks = totals_want[2:]
    assert total_chunks == 20_971_524 == len(want["chunk_slice"]) and total_chunks > GRID_TRIP
    assert total_blocks == len(want["blk_slice"]) == 5 * (1 << 20) + 3
    c, b = ctypes.c_uint64(), ctypes.c_uint64()
    L.avr_plan_bounds(len(TRIP_LENGTHS), total_bins, ctypes.byref(c), ctypes.byref(b))
    assert c.value >= total_chunks and b.value >= total_blocks
    caps = (c.value, b.value) if cap == "bounds" else (GRID_TRIP + 3, b.value)
    n_bins = device_lengths(torch, TRIP_LENGTHS)
    for poison in POISONS:
        got, totals, _, arrays = run_chunks(avr, torch, n_bins, total_bins, 3, 8, poison, caps=caps)      # (checks the guards)
        t = avr.PlanTotals(*totals.tolist())
        if cap == "bounds":
            check_chunks(got, totals, want, totals_want, 3, poison, total_bins, poison)
            assert len(got["chunk_slice"]) > total_chunks and len(got["blk_slice"]) > total_blocks       # (so there IS poison behind them)
            plan = avr.ChunkPlan()
            assert L.avr_chunk_plan_from(ctypes.byref(arrays), ctypes.byref(t), ctypes.byref(plan)) == OK
            assert (plan.total_chunks, plan.total_blocks) == (total_chunks, total_blocks)
        else:
            assert len(got["chunk_slice"]) == GRID_TRIP + 3
            assert np.array_equal(got["chunk_slice"], want["chunk_slice"][:GRID_TRIP + 3])
            assert np.array_equal(got["blk_slice"][:total_blocks], want["blk_slice"])
            for a in ("out_off", "rec_off", "res_off", "dig_off", "chunk_base", "blk_base"):
                assert np.array_equal(got[a], want[a]), a
            assert totals.tolist()[5:7] == [total_chunks, total_blocks]
            assert L.avr_chunk_plan_from(ctypes.byref(arrays), ctypes.byref(t), ctypes.byref(avr.ChunkPlan())) == ERR_CAPACITY


# ------------------------------------------------------------------ one workspace, one totals struct, no wait

class PinnedTotals:
    """64 bytes of pinned host memory between two guard bands, as guarded.Guarded lays them out."""

    def __init__(self, torch):
        self.raw = torch.full((2 * guarded.GUARD + 256 + 64,), guarded.CANARY, dtype=torch.uint8).pin_memory()
        self.start = guarded.GUARD + (-(self.raw.data_ptr() + guarded.GUARD)) % 256
        self.view = self.raw[self.start:self.start + 64]
        assert self.raw.is_pinned() and self.view.data_ptr() % 256 == 0

    def check(self):
        assert (self.raw[:self.start] == guarded.CANARY).all() and (self.raw[self.start + 64:] == guarded.CANARY).all(), "pinned totals: guard changed"


@pytest.mark.parametrize("where", ["device", "pinned"])
def test_one_workspace_one_totals_no_wait(avr, hold, where):
    """The header's promises: ONE workspace of the one quote serves each of the three calls and is free again once a call's work has
    run; both plan calls may be handed the same totals, in device or pinned host memory; no call waits.  Chunk plan at level 3, tile
    plan, chunk plan at level 1 into other arrays, compaction, and the workspace overwritten, all enqueued on one stream behind a
    sleep of 150 ms with nothing but stream order between them; each call returns in less than a tenth of the measured sleep (the rule
    of test_gpu_workspace.on_own_stream) and the sleep is still running when the last one has.  The sequence runs once before, without
    the sleep: a first launch loads the kernels and fills the allocator's cache, as the first runs in test_gpu_workspace do."""
    import torch
    from avrecode_ms_amd.device import plan_tiles
    L = avr.lib()
    n = 4097
    lengths = LENGTHS["n4097"]
    total_bins = int(lengths.sum())
    want3, totals3 = expected_plan(torch, lengths, 8)
    want1, totals1 = expected_plan(torch, lengths, 16)
    want_order, want_tile_off = (x.numpy() for x in plan_tiles(torch.from_numpy(lengths), 8))
    out, out_off, out_len, want_off, want_dense = small_regions(n, 77)
    n_bins = device_lengths(torch, lengths)
    d_out, d_off = torch.from_numpy(out).cuda(), torch.from_numpy(out_off).cuda()
    d_len = torch.from_numpy(out_len.astype(np.uint32).view(np.int32)).cuda()
    ws = guarded.Guarded(L.avr_plan_workspace_bytes(n), "cuda", "ws")
    totals = guarded.Guarded(64, "cuda", "totals") if where == "device" else PinnedTotals(torch)
    ws.view.fill_(0xFF)                                           # once: every later call finds what the one before left
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    for rep, poison in enumerate(POISONS):
        behind_sleep = rep == 1
        with torch.cuda.stream(stream):
            totals.view.fill_(poison)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            if behind_sleep:
                hold(150)
            ev[1].record()
            common = dict(ws=ws, stream=stream, defer=True)
            runs = [run_chunks(avr, torch, n_bins, total_bins, 3, 8, poison, totals=totals.view, **common),
                    run_tiles(avr, torch, n_bins, 8, poison, totals=totals.view, **common),
                    run_chunks(avr, torch, n_bins, total_bins, 1, 16, poison, totals=totals.view, **common),
                    run_compact(avr, torch, d_out, d_off, d_len, int(want_off[-1]), poison, **common)]
            ws.view.fill_(0xFF)
            asleep = not ev[1].query()
            stream.synchronize()
        if behind_sleep:
            slept = ev[0].elapsed_time(ev[1])
            assert slept > 150 / 2, slept
            assert asleep, "the sleep had ended before the last call was enqueued: nothing was shown"
            for (_, took), what in zip(runs, ("chunks 3", "tiles", "chunks 1", "compact")):
                assert took * 1e3 < slept / 10, f"{what}: the call took {took * 1e3:.1f} ms behind a sleep of {slept:.0f} ms"
        (got3, _, _, _), (order, tile_off, _), (got1, seen, _, _), (dense, dense_off) = (collect() for collect, _ in runs)
        for a in WIDTH:                                          # the level-3 call's arrays, whole
            m = len(want3[a])
            assert np.array_equal(got3[a][:m], want3[a]) and (got3[a][m:].view(np.uint8) == poison).all(), (where, a)
        written = LEVEL_ARRAYS[0] + LEVEL_ARRAYS[1]
        for a in WIDTH:                                          # the level-1 call's: four arrays, the others untouched
            m = len(want1[a]) if a in written else 0
            assert np.array_equal(got1[a][:m], want1[a][:m]) and (got1[a][m:].view(np.uint8) == poison).all(), (where, a)
        assert np.array_equal(order, want_order) and np.array_equal(tile_off, want_tile_off)
        assert np.array_equal(dense_off, want_off) and np.array_equal(dense, want_dense)
        assert seen.tolist() == [total_bins, want1["out_off"][-1], want1["rec_off"][-1], 0, 0, totals1[2], 0, want_tile_off[-1]], where
        assert totals3[2] == totals1[2] and want3["rec_off"][-1] != want1["rec_off"][-1]       # (the rec_total seen is the later call's)
        ws.check()
        totals.check()
        assert (ws.view == 0xFF).all()
        runs = None                                              # (the buffers go back to the allocator's cache for the next pass)


# ------------------------------------------------------------------ byte pointers of any alignment

@pytest.mark.parametrize("out_at", [0, 3, 5])
def test_unaligned_byte_pointers(avr, out_at):
    """`dense` at 1..7 bytes past an aligned address -- k_compact_wide takes its head from the pointer -- and `out` at 0, 3 and 5 mod
    8: dense equals the concatenation with the capacity exactly met, the bytes in front of it and both guards keep what they held."""
    import torch
    out, out_off, out_len = compact_case()
    take = np.minimum(out_len, np.diff(out_off))
    want_off = prefix(take)
    want = np.concatenate([out[out_off[i]:out_off[i] + take[i]] for i in range(len(take))])
    total = int(want_off[-1])
    raw = torch.zeros(len(out) + 16, dtype=torch.uint8, device="cuda")
    at = (out_at - raw.data_ptr()) % 8
    d_out = raw[at:at + len(out)]
    d_out.copy_(torch.from_numpy(out))
    assert d_out.data_ptr() % 8 == out_at
    for k in range(1, 8):
        for poison in POISONS:
            g = guarded.Guarded(total + k, "cuda", f"dense + {k}")
            g.view.fill_(poison)
            view = g.view[k:]
            assert view.data_ptr() % 8 == k and view.numel() == total
            dense, dense_off = run_compact(avr, torch, d_out, out_off, out_len, total, poison, dense=view)
            assert np.array_equal(dense_off, want_off) and np.array_equal(dense, want), (k, out_at, poison)
            assert (g.view[:k] == poison).all(), (k, out_at)
            g.check()
