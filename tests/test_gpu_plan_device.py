"""The device planner on the GPU (avr_plan_chunks_device, avr_plan_tiles_device, avr_compact_device): what it writes is, element for
element, what the torch twins (chunk_plan_arrays, plan_tiles of avrecode_ms_amd/device.py) give for the same lengths on CPU tensors,
and what the per-slice rules of tests/test_plan.py (PER_SLICE, FIXED) say.  Every comparison is exact equality.  Every array, the
totals and the workspace sit in tests/guarded.py buffers of exactly the quoted or bounded size, each case runs with two different
poisons and on a stream of its own, and the outputs must not depend on the poison, nor a guard byte change.  The compaction is held
to the concatenation numpy makes of the same bytes; DeviceWorkload(plan="device") to DeviceWorkload(plan="torch")."""
import ctypes

import numpy as np
import pytest

import guarded
from test_plan import FIXED, PER_SLICE

pytestmark = pytest.mark.gpu

OK, ERR_CAPACITY = 0, -5
POISONS = (0x00, 0xA7)
G32 = 1 << 32


def seeded(n, hi, seed):
    return np.random.default_rng(seed).integers(0, hi + 1, n).astype(np.int64)


LENGTHS = {
    "fixed": np.array(FIXED, np.int64),
    **{f"n{n}": seeded(n, 200000, 100 + n) for n in (0, 1, 63, 64, 65, 4097)},
    "1Mi+65": seeded((1 << 20) + 65, 3, 7),                       # 1025 workgroup sums: a second level of them
    "2^32-1": np.array([5, G32 - 1, 1025], np.int64),              # a chunk_slice of 4 Mi entries, all but three one slice's
}
TILE_LENGTHS = {
    **LENGTHS,
    "ties": seeded(70000, 7, 8),                                  # eight values over 70 000 slices: the order of equals is most of the answer
    "equal": np.full(1000, 12345, np.int64),
    "zero": np.zeros(777, np.int64),
    "bit31": np.concatenate([seeded(500, 200000, 9), seeded(500, 200000, 10) + (1 << 31), [G32 - 1, 1 << 31, (1 << 31) - 1, 0]]),
}


def device_lengths(torch, lengths):
    """The lengths as the C ABI takes them: uint32 on the device (an int32 tensor's bits)."""
    return torch.from_numpy(lengths.astype(np.uint32).view(np.int32).copy()).cuda()


def prefix(per_slice):
    return np.concatenate([[0], np.cumsum(per_slice, dtype=np.int64)]).astype(np.int64)


def expected_plan(torch, lengths, rec_round):
    """The torch twins on CPU tensors; out_off and rec_off by the expressions DeviceWorkload uses for them."""
    from avrecode_ms_amd.device import chunk_plan_arrays
    t, totals = chunk_plan_arrays(torch.from_numpy(lengths))
    want = {k: v.numpy() for k, v in t.items()}
    want["out_off"], want["rec_off"] = serial_offsets(lengths, rec_round)
    return want, totals


def serial_offsets(lengths, rec_round):
    """out_off and rec_off (AVR_PLAN_SERIAL) by the expressions DeviceWorkload uses for them."""
    return prefix((lengths + 16 + 7) // 8 * 8), prefix((lengths + rec_round - 1) // rec_round * rec_round)


LEVEL_ARRAYS = [("out_off", "rec_off"), ("chunk_base", "chunk_slice"), ("dig_off",), ("res_off", "blk_base", "blk_slice")]
WIDTH = dict(out_off=8, rec_off=8, dig_off=8, res_off=8, chunk_base=4, chunk_slice=4, blk_base=4, blk_slice=4)


def _bytes_of(torch, x):
    """The uint8 tensor of a caller's buffer: a guarded.Guarded's view, or a tensor as it is (pinned host memory, say)."""
    return x if torch.is_tensor(x) else x.view


def _own_stream(torch, stream):
    """The stream a call runs on: the caller's, or one of its own behind whatever the current one holds (the poison)."""
    if stream is None:
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
    return stream


def run_chunks(avr, torch, n_bins, total_bins, level, rec_round, poison, caps=None, with_rec=True, ws=None, totals=None, stream=None,
               defer=False):
    """One avr_plan_chunks_device call into guarded buffers of the exact sizes, on a stream of its own.  Returns ({array: numpy},
    totals as 8 uint64, the buffers, the PlanArrays).
    ws, totals: the caller's own (a guarded.Guarded; totals may be any 64-byte uint8 tensor), neither poisoned nor checked here.
    stream: the caller's; the poison is then filled in on the current stream, which the caller orders.  defer: enqueue only, nothing
    is synchronised: returns (collect, seconds the C call took on the host); collect() gives the tuple above once the caller has
    synchronised the stream."""
    import time
    L = avr.lib()
    n = n_bins.numel()
    if caps is None:
        c, b = ctypes.c_uint64(), ctypes.c_uint64()
        L.avr_plan_bounds(n, total_bins, ctypes.byref(c), ctypes.byref(b))
        caps = (c.value, b.value)
    size = dict(out_off=n + 1, rec_off=n + 1, dig_off=n + 1, res_off=n + 1, chunk_base=n + 1, blk_base=n + 1, chunk_slice=caps[0], blk_slice=caps[1])
    bufs = guarded.Buffers()
    g = {name: bufs.add(name, size[name] * WIDTH[name], "cuda") for name in size}
    if ws is None:
        ws = bufs.add("ws", L.avr_plan_workspace_bytes(n), "cuda")
    if totals is None:
        totals = bufs.add("totals", 64, "cuda")
    for x in bufs.all.values():
        x.view.fill_(poison)
    ptr = lambda name: g[name].view.data_ptr()
    arrays = avr.PlanArrays(ptr("out_off"), ptr("rec_off") if with_rec else None, rec_round, ptr("chunk_base"), ptr("chunk_slice"), caps[0],
                            ptr("dig_off"), ptr("res_off"), ptr("blk_base"), ptr("blk_slice"), caps[1])
    stream = _own_stream(torch, stream)                          # (the poison was filled in on the current one)
    with torch.cuda.stream(stream):
        t0 = time.perf_counter()
        rc = L.avr_plan_chunks_device(0, ctypes.c_void_p(stream.cuda_stream), n_bins.data_ptr(), n, level, ctypes.byref(arrays),
                                      ws.view.data_ptr(), ws.n, _bytes_of(torch, totals).data_ptr())
        took = time.perf_counter() - t0
    assert rc == OK, L.avr_last_error()

    def collect():
        bufs.check()
        got = {name: g[name].view.cpu().numpy().view(np.int64 if WIDTH[name] == 8 else np.int32) for name in size}
        return got, _bytes_of(torch, totals).cpu().numpy().view(np.uint64), bufs, arrays
    if defer:
        return collect, took
    stream.synchronize()
    return collect()


@pytest.mark.parametrize("name", sorted(LENGTHS))
def test_chunk_plans(avr, name):
    import torch
    lengths = LENGTHS[name]
    n, total_bins = len(lengths), int(lengths.sum())
    n_bins = device_lengths(torch, lengths)
    want8, totals_want = expected_plan(torch, lengths, 8)
    want16, _ = expected_plan(torch, lengths, 16)
    for level in range(4):
        for rec_round, want in ((8, want8), (16, want16)):
            runs = [run_chunks(avr, torch, n_bins, total_bins, level, rec_round, p) for p in POISONS]
            for (got, totals, _, _), poison in zip(runs, POISONS):
                written = [a for lv in range(level + 1) for a in LEVEL_ARRAYS[lv]]
                for a in WIDTH:
                    if a not in written:                         # an array above the level is ignored: left as it was
                        assert (got[a].view(np.uint8) == poison).all(), (level, a)
                        continue
                    m = len(want[a])
                    assert np.array_equal(got[a][:m], want[a]), (level, rec_round, a)
                    assert (got[a][m:].view(np.uint8) == poison).all(), (level, a)      # chunk_slice / blk_slice behind the total: untouched
                res_total, dig_total, total_chunks, total_blocks = totals_want
                assert totals.tolist()[:7] == [total_bins, want["out_off"][-1], want["rec_off"][-1], res_total if level >= 3 else 0,
                                               dig_total if level >= 2 else 0, total_chunks if level >= 1 else 0, total_blocks if level >= 3 else 0]
                assert totals[7:].tobytes() == bytes([poison]) * 8                      # tile_chunks is the tile plan's field
            for a in WIDTH:                                      # the same whatever the buffers held, up to what is written
                m = len(want[a]) if a in [x for lv in range(level + 1) for x in LEVEL_ARRAYS[lv]] else 0
                assert np.array_equal(runs[0][0][a][:m], runs[1][0][a][:m]), a
    got, totals, _, _ = run_chunks(avr, torch, n_bins, total_bins, 0, 8, 0x5C, with_rec=False)       # rec_off NULL: not written, no total
    assert (got["rec_off"].view(np.uint8) == 0x5C).all() and totals[2] == 0 and np.array_equal(got["out_off"], want8["out_off"])


def test_fixed_lengths_by_the_recorded_numbers(avr):
    """FIXED against PER_SLICE of tests/test_plan.py, the numbers worked out by hand."""
    import torch
    lengths = LENGTHS["fixed"]
    got, totals, _, arrays = run_chunks(avr, torch, device_lengths(torch, lengths), int(lengths.sum()), 3, 8, 0x11)
    for a, of in (("out_off", "out"), ("res_off", "work"), ("dig_off", "digits"), ("chunk_base", "chunks"), ("blk_base", "blocks")):
        assert got[a].tolist() == prefix(PER_SLICE[of][0]).tolist(), a
    assert got["chunk_slice"][:84].tolist() == [i for i, k in enumerate(PER_SLICE["chunks"][0]) for _ in range(k)]
    assert got["blk_slice"][:26].tolist() == [i for i, k in enumerate(PER_SLICE["blocks"][0]) for _ in range(k)]
    assert totals.tolist()[:7] == [sum(FIXED), 81416, sum((x + 7) // 8 * 8 for x in FIXED), 81440, 40695, 84, 26]
    t = avr.PlanTotals(*totals.tolist())
    plan = avr.ChunkPlan()
    assert avr.lib().avr_chunk_plan_from(ctypes.byref(arrays), ctypes.byref(t), ctypes.byref(plan)) == OK
    assert (plan.res_total, plan.dig_total, plan.total_chunks, plan.total_blocks) == (81440, 40695, 84, 26)


@pytest.mark.parametrize("short", ["chunks", "blocks"])
def test_a_cap_one_too_small_costs_the_plan_not_memory(avr, short):
    """cap_chunks (cap_blocks) one below the total: chunk_slice (blk_slice) is exactly that long, its guard stays intact, every entry
    below the cap is right, the totals are the true ones, and avr_chunk_plan_from refuses the plan."""
    import torch
    lengths = LENGTHS["fixed"]
    caps = (83, 26) if short == "chunks" else (84, 25)
    want, _ = expected_plan(torch, lengths, 8)
    for poison in POISONS:
        got, totals, _, arrays = run_chunks(avr, torch, device_lengths(torch, lengths), int(lengths.sum()), 3, 8, poison, caps=caps)   # (checks the guards)
        assert np.array_equal(got["chunk_slice"], want["chunk_slice"][:caps[0]]) and np.array_equal(got["blk_slice"], want["blk_slice"][:caps[1]])
        assert totals.tolist()[5:7] == [84, 26]
        t = avr.PlanTotals(*totals.tolist())
        assert avr.lib().avr_chunk_plan_from(ctypes.byref(arrays), ctypes.byref(t), ctypes.byref(avr.ChunkPlan())) == ERR_CAPACITY


def run_tiles(avr, torch, n_bins, per_chunk, poison, ws=None, totals=None, stream=None, defer=False):
    """One avr_plan_tiles_device call: (order, tile_off, totals as 8 uint64).  ws, totals, stream, defer: as run_chunks takes them."""
    import time
    L = avr.lib()
    n = n_bins.numel()
    bufs = guarded.Buffers()
    order = bufs.add("order", 4 * n, "cuda")
    tile_off = bufs.add("tile_off", 8 * ((n + 63) // 64 + 1), "cuda")
    if ws is None:
        ws = bufs.add("ws", L.avr_plan_workspace_bytes(n), "cuda")
    if totals is None:
        totals = bufs.add("totals", 64, "cuda")
    for x in bufs.all.values():
        x.view.fill_(poison)
    stream = _own_stream(torch, stream)                          # (the poison was filled in on the current one)
    with torch.cuda.stream(stream):
        t0 = time.perf_counter()
        rc = L.avr_plan_tiles_device(0, ctypes.c_void_p(stream.cuda_stream), n_bins.data_ptr(), n, per_chunk, order.view.data_ptr(),
                                     tile_off.view.data_ptr(), ws.view.data_ptr(), ws.n, _bytes_of(torch, totals).data_ptr())
        took = time.perf_counter() - t0
    assert rc == OK, L.avr_last_error()

    def collect():
        bufs.check()
        return (order.view.cpu().numpy().view(np.int32), tile_off.view.cpu().numpy().view(np.int64),
                _bytes_of(torch, totals).cpu().numpy().view(np.uint64))
    if defer:
        return collect, took
    stream.synchronize()
    return collect()


@pytest.mark.parametrize("name", sorted(TILE_LENGTHS))
def test_tile_plans(avr, name):
    import torch
    from avrecode_ms_amd.device import plan_tiles
    lengths = TILE_LENGTHS[name]
    n_bins = device_lengths(torch, lengths)
    for per_chunk in (8, 16):
        want_order, want_tile_off = (x.numpy() for x in plan_tiles(torch.from_numpy(lengths), per_chunk))
        runs = [run_tiles(avr, torch, n_bins, per_chunk, p) for p in POISONS]
        for (order, tile_off, totals), poison in zip(runs, POISONS):
            assert np.array_equal(order, want_order), per_chunk
            assert np.array_equal(tile_off, want_tile_off), per_chunk
            assert totals[7] == want_tile_off[-1] and totals[:7].tobytes() == bytes([poison]) * 56      # its own field alone


# ------------------------------------------------------------------ compaction

def run_compact(avr, torch, out, out_off, out_len, capacity, poison, ws=None, stream=None, defer=False, dense=None):
    """One avr_compact_device call: (dense, dense_off).  out_off, out_len: numpy, or device tensors as the C ABI takes them (int64,
    and uint32 as an int32 tensor's bits).  dense: the caller's own uint8 view of `capacity` bytes, of any alignment, inside a buffer
    the caller guards.  ws, stream, defer: as run_chunks takes them."""
    import time
    L = avr.lib()
    n = len(out_len)
    bufs = guarded.Buffers()
    if dense is None:
        dense = bufs.add("dense", capacity, "cuda").view
    assert dense.numel() == capacity
    dense_off = bufs.add("dense_off", 8 * (n + 1), "cuda")
    if ws is None:
        ws = bufs.add("ws", L.avr_plan_workspace_bytes(n), "cuda")
    for x in bufs.all.values():
        x.view.fill_(poison)
    d_off = out_off if torch.is_tensor(out_off) else torch.from_numpy(out_off).cuda()
    d_len = out_len if torch.is_tensor(out_len) else torch.from_numpy(out_len.astype(np.uint32).view(np.int32)).cuda()
    stream = _own_stream(torch, stream)
    with torch.cuda.stream(stream):
        t0 = time.perf_counter()
        rc = L.avr_compact_device(0, ctypes.c_void_p(stream.cuda_stream), out.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), n,
                                  dense.data_ptr(), capacity, dense_off.view.data_ptr(), ws.view.data_ptr(), ws.n)
        took = time.perf_counter() - t0
    assert rc == OK, L.avr_last_error()

    def collect():
        bufs.check()
        return dense.cpu().numpy(), dense_off.view.cpu().numpy().view(np.int64)
    if defer:
        return collect, took
    stream.synchronize()
    return collect()


def compact_case():
    """Regions at 8 mod 16, of every small size and a few long ones; lengths of 0, of the whole region, above it (clamped), and odd
    ones in between, so that the dense offsets take every residue mod 8."""
    rng = np.random.default_rng(31)
    cap = np.concatenate([np.arange(16, 16 * 24, 16), [4096, 70000 // 16 * 16, 16, 16, 1024], rng.integers(1, 40, 60) * 16]).astype(np.int64)
    n = len(cap)
    out_off = np.zeros(n + 1, np.int64)
    out_off[0] = 8
    out_off[1:] = 8 + np.cumsum(cap)
    out_len = rng.integers(0, cap + 1)
    out_len[::7] = 0
    out_len[1::7] = cap[1::7]
    out_len[2::7] = cap[2::7] + rng.integers(1, 1000, len(cap[2::7]))
    out_len[23], out_len[24] = 4093, cap[24] - 3                  # the long ones nearly full
    out_len[3] = 0xFFFFFFFF                                       # a length of 2^32 - 1 is clamped like any other
    out = rng.integers(0, 256, int(out_off[-1]), dtype=np.uint8)
    return out, out_off, out_len.astype(np.int64)


def test_compaction(avr):
    import torch
    out, out_off, out_len = compact_case()
    take = np.minimum(out_len, np.diff(out_off))
    want_off = prefix(take)
    want = np.concatenate([out[out_off[i]:out_off[i] + take[i]] for i in range(len(take))])
    assert len(set((want_off[:-1] % 8).tolist())) == 8 and (out_off[:-1] % 16 == 8).all()
    d_out = torch.from_numpy(out).cuda()
    total = int(want_off[-1])
    for poison in POISONS:
        dense, dense_off = run_compact(avr, torch, d_out, out_off, out_len, total, poison)         # a capacity that is exactly met
        assert np.array_equal(dense_off, want_off) and np.array_equal(dense, want)
    k = 24                                                        # the capacity cuts slice k in the middle: it and all later ones stay away
    capacity = int(want_off[k] + take[k] // 2)
    assert take[k] > 1000 and want_off[k] < capacity < want_off[k + 1]
    for poison in POISONS:
        dense, dense_off = run_compact(avr, torch, d_out, out_off, out_len, capacity, poison)
        assert np.array_equal(dense_off, want_off) and dense_off[-1] > capacity                    # complete: the caller sees the overflow
        assert np.array_equal(dense[:want_off[k]], want[:want_off[k]])
        assert (dense[want_off[k]:] == poison).all()
    dense, dense_off = run_compact(avr, torch, d_out, out_off, out_len, 0, 0x33)                   # no room at all
    assert np.array_equal(dense_off, want_off) and dense.size == 0
    dense, dense_off = run_compact(avr, torch, d_out, out_off[:1], out_len[:0], 16, 0x33)          # no slices: the single zero
    assert dense_off.tolist() == [0] and (dense == 0x33).all()


def test_compaction_across_a_gap_of_more_than_4_gib(avr):
    """Slice 1's region is 2^32 + 64 bytes: the slices behind it lie above 4 GiB, in one allocation that starts at 0 (as
    tests/far_offsets.py places things).  Only the slices' own bytes are written; the rest of the buffer is never read."""
    import torch
    rng = np.random.default_rng(5)
    out_off = np.array([0, 64, G32 + 128, G32 + 1152, G32 + 1216], np.int64)
    out_len = np.array([61, 40, 1021, 64], np.int64)
    parts = [rng.integers(0, 256, int(x), dtype=np.uint8) for x in out_len]
    out = torch.empty(int(out_off[-1]), dtype=torch.uint8, device="cuda")
    for off, p in zip(out_off, parts):
        out[int(off):int(off) + len(p)] = torch.from_numpy(p).cuda()
    want_off = prefix(out_len)
    for poison in POISONS:
        dense, dense_off = run_compact(avr, torch, out, out_off, out_len, int(want_off[-1]), poison)
        assert np.array_equal(dense_off, want_off) and np.array_equal(dense, np.concatenate(parts))
    del out
    torch.cuda.empty_cache()


# ------------------------------------------------------------------ end to end: DeviceWorkload(plan="device") against plan="torch"

def coded(torch, w, chunked=False):
    (w.encode_chunked if chunked else w.encode)()
    torch.cuda.synchronize()
    w.settle()
    slices, status = w.results()
    final = None if w.final_states is None else w.final_states.cpu().numpy().tobytes()
    return slices, w.out_len.cpu().tolist(), status, final


def same_plans(torch, a, b):
    for name in ("order", "tile_off", "out_off"):
        x, y = getattr(a, name), getattr(b, name)
        assert x.dtype == y.dtype and torch.equal(x, y), name
    assert a.total_bins == b.total_bins


def test_workload_5_through_the_one_lane_coders(avr):
    import torch
    ws = [avr.DeviceWorkload.synth(5, 300, avr.KIND_CABAC, 0, 100, plan=p) for p in ("torch", "device")]
    same_plans(torch, *ws)
    want, got = (coded(torch, w) for w in ws)
    assert got == want and any(want[0]) and not any(want[2])
    dense, dense_off = ws[1].results_dense()
    assert dense.cpu().numpy().tobytes() == b"".join(want[0])
    assert dense_off.cpu().tolist() == prefix([len(s) for s in want[0]]).tolist()
    for w in ws:
        w.densify()                                              # onto the contexts in use: one-byte records name at most 126
    narrow = [w.to_cabac8(narrow_tiles=True) for w in ws]
    same_plans(torch, *narrow)
    assert torch.equal(narrow[0].rec8_off, narrow[1].rec8_off)   # (the padding of rec8_flat is whatever lay behind the two-byte records)
    want8, got8 = (coded(torch, w) for w in narrow)
    assert got8 == want8 and want8[0] == want[0]
    assert narrow[1].results_dense()[0].cpu().numpy().tobytes() == b"".join(want[0])


def test_workload_2_through_the_chunked_kernels(avr):
    import torch
    ws = [avr.DeviceWorkload.synth(2, 37, avr.KIND_CABAC, 0, 100, plan=p) for p in ("torch", "device")]
    same_plans(torch, *ws)
    want, got = (coded(torch, w, chunked=True) for w in ws)
    assert got == want and any(want[0]) and not any(want[2])
    assert torch.equal(ws[0].rec_off, ws[1].rec_off)
    for name, t in ws[0]._chunk_plan()["tensors"].items():
        u = ws[1]._chunk_plan()["tensors"][name]
        assert t.dtype == u.dtype and torch.equal(t, u), name
    assert ws[1].results_dense()[0].cpu().numpy().tobytes() == b"".join(want[0])
    parts = [w.set_parts(2) for w in ws]
    assert parts[0] == parts[1] == 2 and [(p["first"], p["n"]) for p in ws[0]._parts] == [(p["first"], p["n"]) for p in ws[1]._parts]
    for w in ws:
        w.status.zero_()
    again = [coded(torch, w, chunked=True) for w in ws]
    assert again[0] == want and again[1] == want
    k2 = [avr.DeviceWorkload.synth(2, 37, avr.KIND_RANGE, 0, 100, plan=p) for p in ("torch", "device")]
    want2, got2 = (coded(torch, w, chunked=True) for w in k2)
    assert got2 == want2 and any(want2[0]) and not any(want2[2])
    assert k2[1].results_dense()[0].cpu().numpy().tobytes() == b"".join(want2[0])


def test_key_records_through_the_resolver(avr):
    import torch
    src = avr.DeviceWorkload.synth(2, 37, avr.KIND_CABAC, 0, 100)
    keys, rec_off = src._slice_major()
    group_first = [0, 5, 6, 37]
    answers = []
    for p in ("torch", "device"):
        kw = avr.DeviceWorkload.from_device_keys(keys, rec_off, src.n_bins, group_first, plan=p)
        rw = kw.resolve_range()
        answers.append((coded(torch, rw, chunked=True), rw.rec_flat.cpu().numpy().tobytes(), kw.est_out.cpu().numpy().tobytes(), coded(torch, rw)))
    assert answers[0] == answers[1] and any(answers[0][0][0]) and not any(answers[0][0][2])
