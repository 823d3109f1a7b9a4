"""Device-resident helpers: torch owns the HBM buffers and the stream, the C ABI does the work.

torch is plumbing only (allocation, streams, torch.distributed in bench.py); every
function here ends in a call through ``include/avrecode_ms_amd.h``.
"""
from __future__ import annotations

import ctypes

from . import EST_KEYS, EST_KEYS8, KIND_CABAC, KIND_CABAC8, KIND_RANGE, KIND_RANGE_KEYS, KIND_RANGE_KEYS8, MAX_STATES8, NOP_CABAC, NOP_RANGE, AvrError, SynthConfig, _check, lib


def synth_config(workload: int, scale_permille: int = 1000, first_slice: int = 0) -> SynthConfig:
    cfg = SynthConfig()
    _check(lib().avr_synth_config_init(ctypes.byref(cfg), workload, scale_permille, first_slice))
    return cfg


def _stream_ptr(torch):
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def plan_tiles(n_bins, records_per_chunk=8):
    """Processing order and tile offsets for per-slice bin counts (int32 tensor, any device).

    Slices are processed longest first, 64 per tile (one wave); a tile is as long as its
    longest slice.  Returns (order int32[n], tile_off int64[n_tiles+1] in 16-byte chunks).
    records_per_chunk: 8 for two-byte records, 16 for one-byte tiles (avr_pack_tiles8_narrow_device).
    Same plan as plan_tiles() in csrc/avr_plan.h (tests/test_plan.py holds the two to each other).
    """
    import torch
    n = n_bins.numel()
    order = torch.argsort(n_bins.to(torch.int64), descending=True, stable=True)
    chunks = (n_bins.to(torch.int64)[order] + records_per_chunk - 1) // records_per_chunk
    tile_max = chunks[::64]
    tile_off = torch.zeros(tile_max.numel() + 1, dtype=torch.int64, device=n_bins.device)
    tile_off[1:] = torch.cumsum(tile_max * 64, 0)
    return order.to(torch.int32), tile_off


def chunk_plan_arrays(n_bins):
    """The arrays of an avr_chunk_plan for per-slice bin counts (int tensor, any device; no native library needed): a dict of the
    six tensors, on n_bins' device, and the four totals.  res_off / dig_off (int64), chunk_base / blk_base (int32): exclusive prefix
    sums with the total appended; chunk_slice / blk_slice (int32): the slice of every chunk / census block.
    Same rules as fill_plan() in csrc/avr_plan.h (tests/test_plan.py holds the two to each other)."""
    import torch
    from . import CHUNK_BINS, SORT_BLOCK_BINS
    nb = n_bins.to(torch.int64)
    zero = torch.zeros(1, dtype=torch.int64, device=nb.device)
    ar = torch.arange(nb.numel(), device=nb.device)
    n_chunks = torch.clamp((nb + CHUNK_BINS - 1) // CHUNK_BINS, min=1)
    n_blocks = torch.clamp((nb + SORT_BLOCK_BINS - 1) // SORT_BLOCK_BINS, min=1)
    res_off = torch.cat([zero, torch.cumsum((nb + 15) // 16 * 16 + 16, 0)])
    dig_off = torch.cat([zero, torch.cumsum(nb // 2 + 8, 0)])
    chunk_base = torch.cat([zero, torch.cumsum(n_chunks, 0)]).to(torch.int32)
    blk_base = torch.cat([zero, torch.cumsum(n_blocks, 0)]).to(torch.int32)
    t = dict(res_off=res_off, chunk_base=chunk_base, blk_base=blk_base, dig_off=dig_off,
             chunk_slice=torch.repeat_interleave(ar, n_chunks).to(torch.int32),
             blk_slice=torch.repeat_interleave(ar, n_blocks).to(torch.int32))
    return t, (int(res_off[-1]), int(dig_off[-1]), int(chunk_base[-1]), int(blk_base[-1]))


def _plan_workspace(n_slices, dev):
    """(tensor, its 256-byte aligned address, the quoted bytes): the one workspace of the three device plan calls."""
    import torch
    n = lib().avr_plan_workspace_bytes(n_slices)
    ws = torch.empty(n + 256, dtype=torch.uint8, device=dev)
    return ws, _aligned(ws), n


def _device_index(t):
    return t.device.index if t.device.index is not None else 0


def device_plan(n_bins, level=0, rec_round=None, max_total_bins=None):
    """avr_plan_chunks_device on torch's current stream: the arrays of `level` (PLAN_SERIAL .. PLAN_K1P) for per-slice bin counts
    (int32 tensor on a GPU), as a dict of tensors -- out_off, rec_off (rec_round 8 or 16; None: left out), and by level chunk_base,
    chunk_slice, dig_off, res_off, blk_base, blk_slice -- and the PlanTotals.  max_total_bins: an upper bound on the bins, which sizes
    chunk_slice / blk_slice (avr_plan_bounds); None: a PLAN_SERIAL call asks the device for the sum first.  Synchronises once (twice
    without a bound) and checks the bound (avr_chunk_plan_from)."""
    import torch
    from . import PLAN_CHUNKS, PLAN_CODES, PLAN_K1P, ChunkPlan, PlanArrays, PlanTotals
    L = lib()
    dev, n = n_bins.device, n_bins.numel()
    if n_bins.dtype != torch.int32 or dev.type != "cuda":
        raise AvrError("device_plan: n_bins must be an int32 tensor on a GPU")
    n_bins = n_bins.contiguous()
    if level >= PLAN_CHUNKS and max_total_bins is None:
        max_total_bins = device_plan(n_bins)[1].total_bins
    with torch.cuda.device(dev):
        caps = [ctypes.c_uint64(0), ctypes.c_uint64(0)]
        if level >= PLAN_CHUNKS:
            L.avr_plan_bounds(n, int(max_total_bins), ctypes.byref(caps[0]), ctypes.byref(caps[1]))
        t = dict(out_off=torch.empty(n + 1, dtype=torch.int64, device=dev))
        if rec_round is not None:
            t["rec_off"] = torch.empty(n + 1, dtype=torch.int64, device=dev)
        if level >= PLAN_CHUNKS:
            t["chunk_base"] = torch.empty(n + 1, dtype=torch.int32, device=dev)
            t["chunk_slice"] = torch.empty(caps[0].value, dtype=torch.int32, device=dev)
        if level >= PLAN_CODES:
            t["dig_off"] = torch.empty(n + 1, dtype=torch.int64, device=dev)
        if level >= PLAN_K1P:
            t["res_off"] = torch.empty(n + 1, dtype=torch.int64, device=dev)
            t["blk_base"] = torch.empty(n + 1, dtype=torch.int32, device=dev)
            t["blk_slice"] = torch.empty(caps[1].value, dtype=torch.int32, device=dev)
        ptr = lambda name: t[name].data_ptr() if name in t else None
        arrays = PlanArrays(ptr("out_off"), ptr("rec_off"), rec_round or 8, ptr("chunk_base"), ptr("chunk_slice"), caps[0].value,
                            ptr("dig_off"), ptr("res_off"), ptr("blk_base"), ptr("blk_slice"), caps[1].value)
        ws, ws_ptr, ws_bytes = _plan_workspace(n, dev)
        totals = torch.zeros(8, dtype=torch.int64).pin_memory()
        _check(L.avr_plan_chunks_device(_device_index(n_bins), _stream_ptr(torch), n_bins.data_ptr(), n, level, ctypes.byref(arrays),
                                        ws_ptr, ws_bytes, totals.data_ptr()))
        torch.cuda.current_stream().synchronize()
    tot = PlanTotals(*[int(x) & 0xFFFFFFFFFFFFFFFF for x in totals.tolist()])
    _check(L.avr_chunk_plan_from(ctypes.byref(arrays), ctypes.byref(tot), ctypes.byref(ChunkPlan())))
    if "chunk_slice" in t:
        t["chunk_slice"] = t["chunk_slice"][:tot.total_chunks]
    if "blk_slice" in t:
        t["blk_slice"] = t["blk_slice"][:tot.total_blocks]
    return t, tot


def chunk_plan_arrays_device(n_bins, max_total_bins=None):
    """chunk_plan_arrays() made on the device (avr_plan_chunks_device at PLAN_K1P): the same six tensors, shapes and dtypes, and the
    same four totals, for an int32 tensor on a GPU."""
    t, tot = device_plan(n_bins, 3, None, max_total_bins)
    del t["out_off"]
    return t, (tot.res_total, tot.dig_total, tot.total_chunks, tot.total_blocks)


def plan_tiles_device(n_bins, records_per_chunk=8):
    """plan_tiles() made on the device (avr_plan_tiles_device on torch's current stream): (order int32[n], tile_off
    int64[n_tiles + 1]) for an int32 tensor on a GPU.  Enqueues and returns; tile_off[-1] is the tile buffer's size in chunks."""
    import torch
    dev, n = n_bins.device, n_bins.numel()
    if n_bins.dtype != torch.int32 or dev.type != "cuda":
        raise AvrError("plan_tiles_device: n_bins must be an int32 tensor on a GPU")
    n_bins = n_bins.contiguous()
    with torch.cuda.device(dev):
        order = torch.empty(n, dtype=torch.int32, device=dev)
        tile_off = torch.empty((n + 63) // 64 + 1, dtype=torch.int64, device=dev)
        totals = torch.empty(8, dtype=torch.int64, device=dev)
        ws, ws_ptr, ws_bytes = _plan_workspace(n, dev)
        _check(lib().avr_plan_tiles_device(_device_index(n_bins), _stream_ptr(torch), n_bins.data_ptr(), n, records_per_chunk,
                                           order.data_ptr(), tile_off.data_ptr(), ws_ptr, ws_bytes, totals.data_ptr()))
        ws.record_stream(torch.cuda.current_stream())
        totals.record_stream(torch.cuda.current_stream())
    return order, tile_off


def compact_device(out, out_off, out_len, dense_capacity=None):
    """avr_compact_device on torch's current stream: (dense uint8[dense_capacity], dense_off int64[n + 1]) -- every slice's
    min(out_len, region) bytes one behind the other.  dense_capacity None: out_off[-1], which always suffices.  Enqueues and
    returns; dense_off[-1] > dense_capacity says that the slices from the first that did not fit were not copied."""
    import torch
    dev, n = out_off.device, out_len.numel()
    with torch.cuda.device(dev):
        if dense_capacity is None:
            dense_capacity = int(out_off[-1].item())
        dense = torch.empty(dense_capacity, dtype=torch.uint8, device=dev)
        dense_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
        ws, ws_ptr, ws_bytes = _plan_workspace(n, dev)
        _check(lib().avr_compact_device(_device_index(out_off), _stream_ptr(torch), out.data_ptr(), out_off.data_ptr(), out_len.data_ptr(), n,
                                        dense.data_ptr(), dense_capacity, dense_off.data_ptr(), ws_ptr, ws_bytes))
        ws.record_stream(torch.cuda.current_stream())
    return dense, dense_off


def finish_word(last_byte=0, length_parity=0, patch=False, escape=False, zeros_before=0):
    """AVR_FINISH_WORD: a slice's word for finish_device, from what its container block holds."""
    return (last_byte & 0xFF) | (length_parity & 1) << 8 | bool(patch) << 9 | bool(escape) << 10 | min(int(zeros_before), 2) << 11


def finish_capacity(region_bytes, n_slices):
    """Room that holds whatever avr_finish_device makes of n_slices slices in regions of region_bytes in all: the header's bound of
    L + 1 + (L + 1 + z) / 2 for a slice of L bytes with z <= 2 zeros in front, summed (at most 1.5 L + 2.5 each) and rounded up."""
    return region_bytes + (region_bytes + 1) // 2 + 3 * n_slices


def finish_device(out, out_off, out_len, finish, status=None, dense_capacity=None):
    """avr_finish_device on torch's current stream: (dense uint8[dense_capacity], dense_off int64[n + 1]) -- every slice's bytes as
    its NAL unit holds them (stop byte dropped, tail patched, escaped, by its word of `finish`: an int32 tensor on the device, see
    finish_word), one behind the other.  status: the slices' status on the device (int32, one per slice), or None: all sound.
    dense_capacity: the room in `dense`; None: what the slices can grow to at the most, which is worked out from out_off[-1] and so
    WAITS for the stream once.  With a capacity given the call enqueues and returns.  dense_off[-1] > dense_capacity says that the
    slices from the first that did not fit were not written."""
    import torch
    dev, n = out_off.device, out_len.numel()
    for name, t in (("finish", finish), ("status", status)):
        if t is not None and (t.numel() != n or t.dtype != torch.int32 or t.device != dev):
            raise AvrError(f"finish_device: {name} must be an int32 tensor of one word per slice on the slices' device")
    status = None if status is None else status.contiguous()
    finish = finish.contiguous()
    with torch.cuda.device(dev):
        if dense_capacity is None:
            dense_capacity = finish_capacity(int((out_off[-1] - out_off[0]).item()), n)
        dense = torch.empty(dense_capacity, dtype=torch.uint8, device=dev)
        dense_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
        ws_bytes = lib().avr_finish_workspace_bytes(n)
        ws = torch.empty(ws_bytes + 256, dtype=torch.uint8, device=dev)
        _check(lib().avr_finish_device(_device_index(out_off), _stream_ptr(torch), out.data_ptr(), out_off.data_ptr(), out_len.data_ptr(),
                                       None if status is None else status.data_ptr(), n, finish.data_ptr(), dense.data_ptr(), dense_capacity,
                                       dense_off.data_ptr(), _aligned(ws), ws_bytes))
        ws.record_stream(torch.cuda.current_stream())
        finish.record_stream(torch.cuda.current_stream())
    return dense, dense_off


def _aligned(t):
    """t's address rounded up to 256 bytes, as the C ABI wants a workspace (the workspaces here are allocated 256 bytes larger)."""
    return (t.data_ptr() + 255) // 256 * 256


def encode_tiles(kind, tiles, tile_off, n_bins, order, out, out_off, out_len, status,
                 init_states=None, n_states=0, final_states=None, device_index=0):
    """Enqueue K1 (kind 0) or K2 (kind 1) on torch's current stream."""
    import torch
    L = lib()
    n = n_bins.numel()
    sp = _stream_ptr(torch)
    if kind == KIND_CABAC:
        _check(L.avr_cabac_encode_tiles_device(
            device_index, sp, tiles.data_ptr(), tile_off.data_ptr(), n_bins.data_ptr(), order.data_ptr(), n,
            init_states.data_ptr() if init_states is not None else None, n_states,
            out.data_ptr(), out_off.data_ptr(), out_len.data_ptr(), status.data_ptr(),
            final_states.data_ptr() if final_states is not None else None))
    else:
        _check(L.avr_range_encode_tiles_device(
            device_index, sp, tiles.data_ptr(), tile_off.data_ptr(), n_bins.data_ptr(), order.data_ptr(), n,
            out.data_ptr(), out_off.data_ptr(), out_len.data_ptr(), status.data_ptr()))


class DeviceWorkload:
    """A batch of slices resident in HBM in the wave-interleaved tile layout.

    KIND_CABAC8: K1 from one-byte records (bin | dense selector << 1).  Such a workload keeps the records slice-major, one byte
    each (rec8_flat, rec8_off: byte offsets, multiples of 16), for encode_chunked(), and tiles for encode(): by default the two-byte
    tiles avr_pack_tiles8_device makes of them (encode() then blocks like any two-byte K1 call), with narrow_tiles=True the one-byte
    tiles of avr_pack_tiles8_narrow_device (encode() is avr_cabac8_encode_tiles_device: nothing waits)."""

    def __init__(self, kind, device_index, n_bins, order, tile_off, tiles, init_states, n_states, plan="torch"):
        import torch
        if plan not in ("torch", "device"):
            raise AvrError(f"plan={plan!r}: expected 'torch' or 'device'")
        self.plan_mode = plan
        self.kind, self.device_index = kind, device_index
        self.n_bins, self.order, self.tile_off, self.tiles = n_bins, order, tile_off, tiles
        self.init_states, self.n_states = init_states, n_states
        self.n_slices = n_bins.numel()
        dev = n_bins.device
        if plan == "device":                                      # avr_plan_chunks_device: the regions and the sum of the bins
            t, tot = device_plan(n_bins)
            self.out_off, out_total, self.total_bins = t["out_off"], tot.out_total, tot.total_bins
        else:
            cap = (n_bins.to(torch.int64) + 16 + 7) // 8 * 8      # worst case 8 bits per bin + stop bytes
            self.out_off = torch.zeros(self.n_slices + 1, dtype=torch.int64, device=dev)
            self.out_off[1:] = torch.cumsum(cap, 0)
            out_total = int(self.out_off[-1].item())
        self.out = torch.empty(out_total, dtype=torch.uint8, device=dev)
        self.out_len = torch.zeros(self.n_slices, dtype=torch.int32, device=dev)
        self.status = torch.zeros(self.n_slices, dtype=torch.int32, device=dev)
        self.final_states = (torch.empty(self.n_slices * max(n_states, 1), dtype=torch.uint8, device=dev)
                             if kind in (KIND_CABAC, KIND_CABAC8) else None)
        if plan != "device":
            self.total_bins = int(n_bins.to(torch.int64).sum().item())
        # K1 sized by the context count of the previous run of this object (avr_cabac_encode_*_device_hinted): no host round trip
        # in the call; settle() looks at what the device reported once the caller has synchronised
        self.rows_hint, self._hinted_path = 0, None
        self._counts = torch.zeros(2, dtype=torch.int32).pin_memory() if dev.type == "cuda" and kind == KIND_CABAC else None

    @classmethod
    def synth(cls, workload, n_slices, kind=KIND_CABAC, device_index=0, scale_permille=1000, first_slice=0, plan="torch"):
        """Generate BASELINE.json config `workload` on the device (avr_synth_*_device).  plan="device": the order, the tiles, the
        regions, the record offsets and the chunk plans of this workload come from the device planner (avr_plan_*_device) instead
        of torch ops -- the same values."""
        import torch
        L = lib()
        dev = torch.device("cuda", device_index)
        cfg = synth_config(workload, scale_permille, first_slice)
        with torch.cuda.device(dev):
            sp = _stream_ptr(torch)
            n_bins = torch.zeros(n_slices, dtype=torch.int32, device=dev)
            _check(L.avr_synth_count_device(device_index, sp, ctypes.byref(cfg), kind, n_slices, n_bins.data_ptr()))
            order, tile_off = plan_tiles_device(n_bins) if plan == "device" else plan_tiles(n_bins)
            tiles = torch.empty(int(tile_off[-1].item()) * 16, dtype=torch.uint8, device=dev)
            init_states = (torch.empty(n_slices * cfg.n_states, dtype=torch.uint8, device=dev)
                           if kind == KIND_CABAC else None)
            _check(L.avr_synth_generate_tiles_device(
                device_index, sp, ctypes.byref(cfg), kind, n_slices, order.data_ptr(), tile_off.data_ptr(),
                tiles.data_ptr(), init_states.data_ptr() if init_states is not None else None))
            torch.cuda.synchronize(dev)
        w = cls(kind, device_index, n_bins, order, tile_off, tiles, init_states, cfg.n_states if kind == KIND_CABAC else 0, plan)
        w.cfg = cfg
        return w

    @classmethod
    def from_host(cls, kind, recs_list, init_states_list=None, device_index=0, pad_bytes=None, narrow_tiles=False, plan="torch"):
        """Upload per-slice uint16 record arrays and pack them into tiles on the device.  KIND_CABAC8: uint8 records, slice-major
        at multiples of 16 bytes; the bytes between a slice's last record and the next slice are taken from pad_bytes (a uint8
        array, repeated over the whole buffer; default zeros) -- the kernels must not code them, whatever they hold.
        narrow_tiles (KIND_CABAC8 only): one-byte tiles for encode(), which then never blocks."""
        import numpy as np
        import torch
        if kind == KIND_CABAC8:
            return cls._from_host8(recs_list, init_states_list, device_index, pad_bytes, narrow_tiles, plan)
        if narrow_tiles:
            raise AvrError("narrow_tiles: one-byte tiles hold KIND_CABAC8 records only")
        L = lib()
        dev = torch.device("cuda", device_index)
        n = len(recs_list)
        nb = np.array([len(r) for r in recs_list], dtype=np.int32)
        padded = (nb.astype(np.int64) + 7) // 8 * 8
        rec_off = np.zeros(n + 1, dtype=np.int64)
        rec_off[1:] = np.cumsum(padded)
        flat = np.full(int(rec_off[-1]) + 8, NOP_CABAC if kind == KIND_CABAC else NOP_RANGE, dtype=np.uint16)
        for i, r in enumerate(recs_list):
            flat[rec_off[i]:rec_off[i] + len(r)] = r
        n_states = len(init_states_list[0]) if (kind == KIND_CABAC and init_states_list) else 0
        with torch.cuda.device(dev):
            d_flat = torch.from_numpy(flat.view(np.int16)).to(dev)
            d_off = torch.from_numpy(rec_off).to(dev)
            n_bins = torch.from_numpy(nb).to(dev)
            order, tile_off = plan_tiles_device(n_bins) if plan == "device" else plan_tiles(n_bins)
            tiles = torch.empty(max(int(tile_off[-1].item()), 1) * 16, dtype=torch.uint8, device=dev)
            pack_status = torch.zeros(n, dtype=torch.int32, device=dev)
            _check(L.avr_pack_tiles_device(device_index, _stream_ptr(torch), kind, n_states, d_flat.data_ptr(),
                                           d_off.data_ptr(), n_bins.data_ptr(), order.data_ptr(), n, tile_off.data_ptr(),
                                           tiles.data_ptr(), pack_status.data_ptr()))
            init = None
            if kind == KIND_CABAC:
                init = torch.from_numpy(np.concatenate([np.asarray(s, dtype=np.uint8) for s in init_states_list])
                                        if n_states else np.zeros(1, np.uint8)).to(dev)
            torch.cuda.synchronize(dev)
        w = cls(kind, device_index, n_bins, order, tile_off, tiles, init, n_states, plan)
        w.rec_flat, w.rec_off = d_flat, d_off
        w.status.copy_(pack_status)
        return w

    @classmethod
    def from_host_keys(cls, recs_list, group_first, tables=None, device_index=0, gap=0):
        """KEY records (bin | model key << 1) from the host with their groups: group g = slices group_first[g] .. group_first[g + 1]
        (len(group_first) = groups + 1), each group starting from tables[g] (EST_KEYS x 2 uint8 {pos, neg}) or, tables=None, fresh.
        `gap`: groups of eight records left unused between slices.  The padding and the gaps hold 0xeeee (a malformed record:
        the kernels must not read it as one).  resolve_range() gives the AVR_KIND_RANGE workload."""
        import numpy as np
        import torch
        dev = torch.device("cuda", device_index)
        nb = np.array([len(r) for r in recs_list], dtype=np.int32)
        rec_off = np.zeros(len(recs_list) + 1, dtype=np.int64)
        rec_off[1:] = np.cumsum((nb.astype(np.int64) + 7) // 8 * 8 + 8 * gap)
        flat = np.full(int(rec_off[-1]) + 8, 0xEEEE, dtype=np.uint16)
        for i, r in enumerate(recs_list):
            flat[rec_off[i]:rec_off[i] + len(r)] = r
        with torch.cuda.device(dev):
            est_in = None if tables is None else torch.from_numpy(np.ascontiguousarray(np.stack(tables), np.uint8)).to(dev)
            return cls.from_device_keys(torch.from_numpy(flat.view(np.int16)).to(dev), torch.from_numpy(rec_off).to(dev),
                                        torch.from_numpy(nb).to(dev), group_first, est_in, device_index)

    @classmethod
    def from_device_keys(cls, key_flat, rec_off, n_bins, group_first, est_in=None, device_index=0, plan="torch"):
        """The same from slice-major key records already on the device (a synthetic K1 record is a key record)."""
        return cls._from_device_keys(KIND_RANGE_KEYS, key_flat, rec_off, n_bins, group_first, est_in, device_index, plan)

    @classmethod
    def _from_device_keys(cls, kind, key_flat, rec_off, n_bins, group_first, est_in, device_index, plan):
        """A workload of key records of either width: est_out sized by the kind's table, rec_flat two-byte records at the keys' rec_off."""
        import numpy as np
        import torch
        dev = n_bins.device
        order, tile_off = plan_tiles_device(n_bins) if plan == "device" else plan_tiles(n_bins)
        tiles = torch.empty(max(int(tile_off[-1].item()), 1) * 16, dtype=torch.uint8, device=dev)
        w = cls(kind, device_index, n_bins, order, tile_off, tiles, None, 0, plan)
        w.key_flat, w.rec_off = key_flat, rec_off
        w.group_first = torch.from_numpy(np.asarray(group_first, dtype=np.int32)).to(dev)
        w.n_groups = w.group_first.numel() - 1
        w.est_in = est_in
        w.est_out = torch.empty(max(w.n_groups, 1) * (EST_KEYS8 if kind == KIND_RANGE_KEYS8 else EST_KEYS) * 2, dtype=torch.uint8, device=dev)
        w.rec_flat = torch.empty(key_flat.numel(), dtype=torch.int16, device=dev)
        return w

    @classmethod
    def from_host_keys8(cls, recs8_list, group_first, tables=None, device_index=0, gap=0, plan="torch", pad_bytes=None):
        """ONE-BYTE key records (bin | dense key id << 1, KIND_RANGE_KEYS8) from the host with their groups, as from_host_keys:
        slice i at byte rec_off[i], a multiple of 16; tables[g]: EST_KEYS8 x 2 uint8.  `gap`: groups of sixteen bytes left unused
        between slices (plan="torch" only).  The padding and the gaps hold pad_bytes (a uint8 array repeated over the whole buffer;
        default 0xee): every byte value is a key, so the kernels must tell padding by its index.  plan="device": the offsets from avr_plan_chunks_device with rec_round = 16."""
        import numpy as np
        import torch
        dev = torch.device("cuda", device_index)
        nb = np.array([len(r) for r in recs8_list], dtype=np.int32)
        with torch.cuda.device(dev):
            n_bins = torch.from_numpy(nb).to(dev)
            if plan == "device":
                if gap:
                    raise AvrError("from_host_keys8: the device planner leaves no gaps")
                d_off = device_plan(n_bins, 0, 16)[0]["rec_off"]
                rec_off = d_off.cpu().numpy()
            else:
                rec_off = np.zeros(len(recs8_list) + 1, dtype=np.int64)
                rec_off[1:] = np.cumsum((nb.astype(np.int64) + 15) // 16 * 16 + 16 * gap)
                d_off = torch.from_numpy(rec_off).to(dev)
            size = int(rec_off[-1]) + 16
            flat = np.full(size, 0xEE, np.uint8) if pad_bytes is None else np.resize(np.asarray(pad_bytes, dtype=np.uint8), size)
            for i, r in enumerate(recs8_list):
                flat[rec_off[i]:rec_off[i] + len(r)] = np.asarray(r, dtype=np.uint8)
            est_in = None if tables is None else torch.from_numpy(np.ascontiguousarray(np.stack(tables), np.uint8)).to(dev)
            return cls.from_device_keys8(torch.from_numpy(flat).to(dev), d_off, n_bins, group_first, est_in, device_index, plan)

    @classmethod
    def from_device_keys8(cls, key8_flat, rec_off, n_bins, group_first, est_in=None, device_index=0, plan="torch"):
        """The same from slice-major one-byte key records already on the device (uint8 tensor, readable to rec_off[-1] rounded up to 16).
        The resolved two-byte records go to self.rec_flat at the same rec_off, counted in records."""
        return cls._from_device_keys(KIND_RANGE_KEYS8, key8_flat, rec_off, n_bins, group_first, est_in, device_index, plan)

    def resolve_keys(self):
        """avr_range_resolve_device (one-byte key records: avr_range_resolve8_device) alone: the K2 records (slice-major, self.rec_off)
        of this key workload, the groups' tables in self.est_out; enqueues and returns."""
        import torch
        if self.kind not in (KIND_RANGE_KEYS, KIND_RANGE_KEYS8):
            raise AvrError("not a workload of key records")
        p = self._chunk_plan()
        L = lib()
        quote, call = ((L.avr_range_resolve8_workspace_bytes, L.avr_range_resolve8_device) if self.kind == KIND_RANGE_KEYS8 else
                       (L.avr_range_resolve_workspace_bytes, L.avr_range_resolve_device))
        if "ws_est" not in p:
            n = quote(self.n_slices, self.n_groups, ctypes.byref(p["plan"]))
            p["ws_est"] = torch.empty(n + 256, dtype=torch.uint8, device=self.n_bins.device)
            p["ws_est_bytes"] = n
        _check(call(
            self.device_index, _stream_ptr(torch), self.key_flat.data_ptr(), self.rec_off.data_ptr(), self.n_bins.data_ptr(),
            self.n_slices, self.group_first.data_ptr(), self.n_groups, self.est_in.data_ptr() if self.est_in is not None else None,
            self.est_out.data_ptr(), ctypes.byref(p["plan"]), _aligned(p["ws_est"]), p["ws_est_bytes"],
            self.rec_flat.data_ptr(), self.status.data_ptr()))
        return self.rec_flat

    def verify_keys(self):
        """avr_range_keys_verify_device behind resolve_keys() / resolve_range() on torch's current stream: the resolved records
        (self.rec_flat) and self.est_out held to the key records by the model's update rule, record by record -- a check that shares
        nothing with the resolver.  Returns (self.status, first_bad): first_bad an int32 tensor (VERIFY_NONE reads as -1; n_bins: the
        slice's padding or its group's table), SLICE_VERIFY_FAILED in the status of a slice with a finding.  Enqueues and returns."""
        import torch
        if self.kind not in (KIND_RANGE_KEYS, KIND_RANGE_KEYS8):
            raise AvrError("verify_keys: not a workload of key records")
        p = self._chunk_plan()
        L = lib()
        quote, call = ((L.avr_range_keys8_verify_workspace_bytes, L.avr_range_keys8_verify_device) if self.kind == KIND_RANGE_KEYS8 else
                       (L.avr_range_keys_verify_workspace_bytes, L.avr_range_keys_verify_device))
        if "ws_estv" not in p:
            n = quote(self.n_slices, self.n_groups, ctypes.byref(p["plan"]))
            p["ws_estv"] = torch.empty(n + 256, dtype=torch.uint8, device=self.n_bins.device)
            p["ws_estv_bytes"] = n
        first_bad = torch.empty(self.n_slices, dtype=torch.int32, device=self.n_bins.device)
        _check(call(
            self.device_index, _stream_ptr(torch), self.key_flat.data_ptr(), self.rec_flat.data_ptr(), self.rec_off.data_ptr(),
            self.n_bins.data_ptr(), self.n_slices, self.group_first.data_ptr(), self.n_groups,
            self.est_in.data_ptr() if self.est_in is not None else None, self.est_out.data_ptr(), ctypes.byref(p["plan"]),
            _aligned(p["ws_estv"]), p["ws_estv_bytes"], self.status.data_ptr(), first_bad.data_ptr()))
        return self.status, first_bad

    def resolve_range(self):
        """The resolved AVR_KIND_RANGE workload on the device: the estimators resolved (resolve_keys) and the records packed into
        tiles, its status carrying what the resolver found malformed.  encode() / encode_chunked() of the result code it."""
        import torch
        self.status.zero_()
        recs = self.resolve_keys()
        w = DeviceWorkload(KIND_RANGE, self.device_index, self.n_bins, self.order, self.tile_off, self.tiles, None, 0, self.plan_mode)
        w.rec_flat, w.rec_off = recs, self.rec_off
        w.status.copy_(self.status)
        _check(lib().avr_pack_tiles_device(self.device_index, _stream_ptr(torch), KIND_RANGE, 0, recs.data_ptr(), self.rec_off.data_ptr(),
                                           self.n_bins.data_ptr(), self.order.data_ptr(), self.n_slices, self.tile_off.data_ptr(),
                                           self.tiles.data_ptr(), w.status.data_ptr()))
        return w

    @classmethod
    def _from_host8(cls, recs_list, init_states_list, device_index, pad_bytes, narrow_tiles=False, plan="torch"):
        import numpy as np
        import torch
        dev = torch.device("cuda", device_index)
        n = len(recs_list)
        nb = np.array([len(r) for r in recs_list], dtype=np.int32)
        rec_off = np.zeros(n + 1, dtype=np.int64)
        rec_off[1:] = np.cumsum((nb.astype(np.int64) + 15) // 16 * 16)
        size = int(rec_off[-1]) + 16
        flat = np.zeros(size, np.uint8) if pad_bytes is None else np.resize(np.asarray(pad_bytes, dtype=np.uint8), size)
        for i, r in enumerate(recs_list):
            flat[rec_off[i]:rec_off[i] + len(r)] = np.asarray(r, dtype=np.uint8)
        n_states = len(init_states_list[0]) if init_states_list else 0
        with torch.cuda.device(dev):
            init = torch.from_numpy(np.concatenate([np.asarray(s, dtype=np.uint8) for s in init_states_list])
                                    if n_states else np.zeros(1, np.uint8)).to(dev)
            w = cls._pack8(device_index, torch.from_numpy(flat).to(dev), torch.from_numpy(rec_off).to(dev),
                           torch.from_numpy(nb).to(dev), init, n_states, narrow_tiles, plan)
            torch.cuda.synchronize(dev)
        return w

    @classmethod
    def _pack8(cls, device_index, rec8_flat, rec8_off, n_bins, init_states, n_states, narrow_tiles=False, plan="torch"):
        """A KIND_CABAC8 workload from one-byte slice-major records on the device: two-byte tiles by avr_pack_tiles8_device, or
        one-byte tiles by avr_pack_tiles8_narrow_device (narrow_tiles)."""
        import torch
        if n_states > MAX_STATES8:
            raise AvrError(f"n_states {n_states} > {MAX_STATES8}: one-byte records name at most {MAX_STATES8} contexts")
        dev = n_bins.device
        n = n_bins.numel()
        order, tile_off = (plan_tiles_device if plan == "device" else plan_tiles)(n_bins, 16 if narrow_tiles else 8)
        tiles = torch.empty(max(int(tile_off[-1].item()), 1) * 16, dtype=torch.uint8, device=dev)
        pack_status = torch.zeros(n, dtype=torch.int32, device=dev)
        pack = lib().avr_pack_tiles8_narrow_device if narrow_tiles else lib().avr_pack_tiles8_device
        _check(pack(device_index, _stream_ptr(torch), n_states, rec8_flat.data_ptr(), rec8_off.data_ptr(),
                    n_bins.data_ptr(), order.data_ptr(), n, tile_off.data_ptr(), tiles.data_ptr(), pack_status.data_ptr()))
        w = cls(KIND_CABAC8, device_index, n_bins, order, tile_off, tiles, init_states, n_states, plan)
        w.rec8_flat, w.rec8_off, w.narrow_tiles = rec8_flat, rec8_off, bool(narrow_tiles)
        w.status.copy_(pack_status)
        return w

    def to_cabac8(self, narrow_tiles=False):
        """This K1 workload as one-byte records (a new KIND_CABAC8 workload on the same device): selector s < n_states stays s,
        bypass becomes SEL8_BYPASS, terminate SEL8_TERMINATE.  Needs n_states <= MAX_STATES8 -- after densify() for a stream that
        numbers its contexts sparsely.  The padding bytes are whatever the two-byte layout had there, narrowed (no-op records
        become a context's byte): never coded.  narrow_tiles: one-byte tiles for encode() (see from_host)."""
        import torch
        if self.kind != KIND_CABAC or self.n_states > MAX_STATES8:
            raise AvrError(f"to_cabac8 needs a KIND_CABAC workload with n_states <= {MAX_STATES8} (densify() first)")
        recs, rec_off = self._slice_major()
        dev = self.n_bins.device
        with torch.cuda.device(dev):
            nb = self.n_bins.to(torch.int64)
            pad16 = (nb + 15) // 16 * 16
            if self.plan_mode == "device":                       # the one-byte records' offsets: rec_round 16
                off8 = device_plan(self.n_bins, 0, 16)[0]["rec_off"]
            else:
                off8 = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(pad16, 0)])
            total = int(off8[-1])
            slice_of = torch.repeat_interleave(torch.arange(self.n_slices, device=dev), pad16)
            src = torch.arange(total, device=dev) - off8[:-1][slice_of] + rec_off[:-1][slice_of]   # (< rec_off[-1] + 8: in the copy)
            del slice_of
            r = recs[src].to(torch.int32) & 0xffff
            del src
            sel = r >> 1
            sel8 = torch.where(sel == 1024, 126, torch.where(sel == 1025, 127, sel))
            flat8 = torch.zeros(total + 16, dtype=torch.uint8, device=dev)
            flat8[:total] = (((sel8 << 1) | (r & 1)) & 0xff).to(torch.uint8)
            del r, sel, sel8
            w = DeviceWorkload._pack8(self.device_index, flat8, off8, self.n_bins, self.init_states, self.n_states, narrow_tiles, self.plan_mode)
            torch.cuda.synchronize(dev)
        return w

    def encode(self):
        """One pass of the hot path over the batch (enqueued on torch's current stream).  K1: sized by the context count the previous
        run of this object reported (none yet: the call asks the device and waits); exact whatever the guess.  settle() after a
        synchronisation takes the count over for the next run.  KIND_CABAC8 with narrow_tiles: avr_cabac8_encode_tiles_device, which
        has nothing to count and never blocks."""
        self._verify_layout = "tiles"
        if getattr(self, "narrow_tiles", False):
            import torch
            _check(lib().avr_cabac8_encode_tiles_device(
                self.device_index, _stream_ptr(torch), self.tiles.data_ptr(), self.tile_off.data_ptr(), self.n_bins.data_ptr(),
                self.order.data_ptr(), self.n_slices, self.init_states.data_ptr() if self.init_states is not None else None, self.n_states,
                self.out.data_ptr(), self.out_off.data_ptr(), self.out_len.data_ptr(), self.status.data_ptr(),
                self.final_states.data_ptr() if self.final_states is not None else None))
            return
        if self.kind == KIND_CABAC and self._counts is not None:
            import torch
            self._hinted_path = "tiles"
            _check(lib().avr_cabac_encode_tiles_device_hinted(
                self.device_index, _stream_ptr(torch), self.tiles.data_ptr(), self.tile_off.data_ptr(), self.n_bins.data_ptr(),
                self.order.data_ptr(), self.n_slices, self.init_states.data_ptr() if self.init_states is not None else None, self.n_states,
                self.out.data_ptr(), self.out_off.data_ptr(), self.out_len.data_ptr(), self.status.data_ptr(),
                self.final_states.data_ptr() if self.final_states is not None else None, self.rows_hint, self._counts.data_ptr()))
            return
        kind = KIND_CABAC if self.kind == KIND_CABAC8 else self.kind      # (KIND_CABAC8: two-byte tiles, made by avr_pack_tiles8_device)
        encode_tiles(kind, self.tiles, self.tile_off, self.n_bins, self.order, self.out, self.out_off,
                     self.out_len, self.status, self.init_states, self.n_states, self.final_states, self.device_index)

    def _part_array(self, rows_hint):
        """avr_chunked_part[n_parts]: the batch's arrays from each part's first slice on, the part's own plan, workspace and counts."""
        from . import ChunkedPart
        recs, rec_off = self._slice_major()
        ns = max(self.n_states, 1)
        arr = (ChunkedPart * self.n_parts)()
        for i, p in enumerate(self._parts):
            a = p["first"]
            arr[i] = ChunkedPart(
                rec_off.data_ptr() + 8 * a, self.n_bins.data_ptr() + 4 * a, p["n"], self.init_states.data_ptr() + ns * a,
                ctypes.addressof(p["plan"]), _aligned(p["ws"]), p["ws_bytes"],
                self.out_off.data_ptr() + 8 * a, self.out_len.data_ptr() + 4 * a, self.status.data_ptr() + 4 * a,
                (self.final_states.data_ptr() + ns * a) if self.final_states is not None else None,
                rows_hint, self._part_counts.data_ptr() + 8 * i)
        return arr

    def settle(self, stream=None):
        """After the caller has synchronised the stream of encode() / encode_chunked(): what the device reported about the run that
        was sized by a guess.  Returns {"rows": context rows the batch needs, "hint": what the run was sized by, "redone": ...}.
        The one-lane-per-slice path is exact whatever the guess; the chunked path is run again (asking the device) if the batch needed
        more rows than guessed, and its second pass is run if slices were left for it -- then the device is synchronised again, or,
        given `stream` (torch's current stream, the one the run was enqueued on), that stream alone: whatever the library ran on
        streams of its own has been joined back to it."""
        import torch
        wait = stream.synchronize if stream is not None else (lambda: torch.cuda.synchronize(self.n_bins.device))
        if self._counts is None or self._hinted_path is None:
            return {"rows": 0, "hint": 0, "redone": False}
        if self._hinted_path == "parts":                     # what every part reported
            used, redone = self.rows_hint, False
            rows = max(int(self._part_counts[2 * i]) for i in range(self.n_parts))
            if used and rows > used:                         # a part needed more rows than guessed: all of them once more, asking
                self.status.copy_(self._status_before)
                self.rows_hint = 0
                self.encode_chunked()
                wait()
                rows, redone = max(int(self._part_counts[2 * i]) for i in range(self.n_parts)), True
            recs, rec_off = self._slice_major()
            for i, p in enumerate(self._parts):
                if int(self._part_counts[2 * i + 1]):        # slices the part left for a second pass
                    q = self._part_args[i]
                    _check(lib().avr_cabac_encode_chunked_second_pass_device(
                        self.device_index, _stream_ptr(torch), recs.data_ptr(), q.rec_off, q.n_bins, q.n_slices, q.init_states,
                        self.n_states, q.plan, q.workspace, q.workspace_bytes, self.out.data_ptr(), q.out_off, q.out_len, q.status,
                        q.final_states))
                    redone = True
            if redone:
                wait()
            if rows:
                self.rows_hint = min(self.n_states, rows + 8)
            return {"rows": rows, "hint": used, "redone": redone, "parts": self.n_parts}
        rows, left, used = int(self._counts[0]), int(self._counts[1]), self.rows_hint
        redone = False
        if self._hinted_path == "chunked" and used and rows > used:
            self.status.copy_(self._status_before)
            self.rows_hint = 0
            self.encode_chunked()
            wait()
            rows, left, redone = int(self._counts[0]), int(self._counts[1]), True
        if self._hinted_path == "chunked" and left:
            recs, rec_off = self._slice_major()
            p = self._chunk_plan()
            ws_ptr = _aligned(p["ws"])
            _check(lib().avr_cabac_encode_chunked_second_pass_device(
                self.device_index, _stream_ptr(torch), recs.data_ptr(), rec_off.data_ptr(), self.n_bins.data_ptr(),
                self.n_slices, self.init_states.data_ptr(), self.n_states, ctypes.byref(p["plan"]), ws_ptr, p["ws_bytes"],
                self.out.data_ptr(), self.out_off.data_ptr(), self.out_len.data_ptr(), self.status.data_ptr(),
                self.final_states.data_ptr() if self.final_states is not None else None))
            wait()
            redone = True
        if rows:
            self.rows_hint = min(self.n_states, rows + 8)        # a little room, as avr_batch leaves (csrc/avr_api.cpp)
        return {"rows": rows, "hint": used, "redone": redone}

    def densify(self):
        """Renumber the batch onto the contexts it uses (fewer state bytes in LDS -> more waves per CU).

        Records (tiles and, if present, the slice-major copy) are rewritten in place, init_states
        is gathered to the dense numbering; final states are scattered back by final_states_full().
        Coded bytes do not change: they depend on (bin, state) sequences only."""
        import numpy as np
        import torch
        if self.kind != KIND_CABAC or getattr(self, "dense_index", None) is not None:
            return self
        L = lib()
        dev = self.n_bins.device
        sp = _stream_ptr(torch)
        bitmap = torch.zeros(32, dtype=torch.int32, device=dev)
        n_tile_recs = self.tiles.numel() // 2
        _check(L.avr_context_census_device(self.device_index, sp, self.tiles.data_ptr(), n_tile_recs, bitmap.data_ptr()))
        bits = np.unpackbits(bitmap.cpu().numpy().view(np.uint8), bitorder="little")[:1024]
        used = np.nonzero(bits)[0].astype(np.uint16)
        used = used[used < self.n_states] if self.n_states else used
        table = np.zeros(1024, dtype=np.uint16)
        table[used] = np.arange(used.size, dtype=np.uint16)
        d_table = torch.from_numpy(table.view(np.int16)).to(dev)
        d_index = torch.from_numpy(used.view(np.int16)).to(dev)
        _check(L.avr_context_remap_device(self.device_index, sp, self.tiles.data_ptr(), n_tile_recs, d_table.data_ptr()))
        if getattr(self, "rec_flat", None) is not None:
            _check(L.avr_context_remap_device(self.device_index, sp, self.rec_flat.data_ptr(),
                                              int(self.rec_off[-1]), d_table.data_ptr()))
        n_dense = max(int(used.size), 1)
        dense_init = torch.zeros(self.n_slices * n_dense, dtype=torch.uint8, device=dev)
        _check(L.avr_states_permute_device(self.device_index, sp, self.init_states.data_ptr(), self.n_states,
                                           dense_init.data_ptr(), n_dense, d_index.data_ptr(), int(used.size), self.n_slices, 0))
        torch.cuda.synchronize(dev)
        self.full_n_states, self.full_init_states = self.n_states, self.init_states
        self.dense_index, self.init_states, self.n_states = d_index, dense_init, n_dense
        self.final_states = torch.empty(self.n_slices * n_dense, dtype=torch.uint8, device=dev)
        self._plan = None
        return self

    def final_states_full(self):
        """final states in the original context numbering (contexts never touched keep their initial state)."""
        import torch
        if getattr(self, "dense_index", None) is None:
            return self.final_states
        full = self.full_init_states.clone()
        _check(lib().avr_states_permute_device(self.device_index, _stream_ptr(torch), self.final_states.data_ptr(), self.n_states,
                                               full.data_ptr(), self.full_n_states, self.dense_index.data_ptr(),
                                               self.dense_index.numel(), self.n_slices, 1))
        return full

    def _slice_major(self):
        """Slice-major records on the device (what the intra-slice parallel path reads)."""
        import torch
        if self.kind == KIND_CABAC8:
            return self.rec8_flat, self.rec8_off
        if getattr(self, "rec_flat", None) is None:
            dev = self.n_bins.device
            nb = self.n_bins.to(torch.int64)
            if self.plan_mode == "device":
                self.rec_off = device_plan(self.n_bins, 0, 8)[0]["rec_off"]
            else:
                self.rec_off = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum((nb + 7) // 8 * 8, 0)])
            self.rec_flat = torch.empty(int(self.rec_off[-1]) + 8, dtype=torch.int16, device=dev)
            _check(lib().avr_synth_generate_slices_device(
                self.device_index, _stream_ptr(torch), ctypes.byref(self.cfg), self.kind, self.n_slices,
                self.rec_off.data_ptr(), self.rec_flat.data_ptr(), None))
            if getattr(self, "dense_index", None) is not None:      # keep the copy in the batch's numbering
                import numpy as np
                table = np.zeros(1024, dtype=np.uint16)
                idx = self.dense_index.cpu().numpy().view(np.uint16)
                table[idx] = np.arange(idx.size, dtype=np.uint16)
                d_table = torch.from_numpy(table.view(np.int16)).to(dev)
                _check(lib().avr_context_remap_device(self.device_index, _stream_ptr(torch), self.rec_flat.data_ptr(),
                                                      int(self.rec_off[-1]), d_table.data_ptr()))
                torch.cuda.synchronize(dev)
        return self.rec_flat, self.rec_off

    def _plan_of(self, a, b):
        """Plan arrays and workspace of the intra-slice parallel path for slices [a, b), numbered from 0."""
        import torch
        from . import ChunkPlan
        if self.plan_mode == "device":
            t, totals = chunk_plan_arrays_device(self.n_bins[a:b], self.total_bins)
        else:
            t, totals = chunk_plan_arrays(self.n_bins[a:b])
        plan = ChunkPlan(t["res_off"].data_ptr(), t["chunk_base"].data_ptr(), t["chunk_slice"].data_ptr(),
                         t["blk_base"].data_ptr(), t["blk_slice"].data_ptr(), t["dig_off"].data_ptr(), *totals)
        p = dict(tensors=t, plan=plan, first=a, n=b - a)
        if self.kind in (KIND_CABAC, KIND_CABAC8):      # (K2 sizes its own workspace, see encode_chunked)
            ws_of = lib().avr_cabac8_chunked_workspace_bytes if self.kind == KIND_CABAC8 else lib().avr_cabac_chunked_workspace_bytes
            ws_bytes = ws_of(b - a, self.n_states, ctypes.byref(plan))
            p.update(ws_bytes=ws_bytes, ws=torch.empty(ws_bytes + 256, dtype=torch.uint8, device=self.n_bins.device))
        return p

    def set_parts(self, n_parts, weights=None):
        """The batch through the intra-slice parallel path as n_parts parts of consecutive slices at once, each on a stream of its
        own (avr_cabac_encode_chunked_device_parts): parts of near-equal chunk counts.  0: by the batch's size -- two parts once the
        batch is more than one round of workgroups of the path's longest kernel (what the parts fill are the part-empty last rounds:
        config 2 1.43 -> 1.37 ms in two parts, 1.49 in three; config 4 - 2 %), one part below that (128 slices of config 2: 0.67 ms in
        one, 0.70 in two)."""
        import torch
        from . import MAX_PARTS
        if self.plan_mode == "device":
            chunk_base = device_plan(self.n_bins, 1, None, self.total_bins)[0]["chunk_base"]
        else:
            chunk_base = chunk_plan_arrays(self.n_bins)[0]["chunk_base"]
        total = int(chunk_base[-1])
        if n_parts == 0:
            waves = (total + 63) // 64
            n_parts = 2 if (waves >= 2048 and self.n_slices >= 64) else 1
        n_parts = max(1, min(int(n_parts), MAX_PARTS, self.n_slices))
        self._parts = None
        self.n_parts = n_parts
        if n_parts > 1 and self.kind == KIND_CABAC and self._counts is not None:
            csum = chunk_base[1:].cpu().numpy()
            import numpy as np
            share = np.cumsum(np.asarray(weights if weights else [1.0] * n_parts, dtype=np.float64))
            share = share / share[-1]                            # (weights: the parts' shares of the chunks, for experiments; default equal)
            cuts = [0] + [int(np.searchsorted(csum, total * share[i])) + 1 for i in range(n_parts - 1)] + [self.n_slices]
            cuts = sorted(set(min(max(c, 0), self.n_slices) for c in cuts))
            self._parts = [self._plan_of(a, b) for a, b in zip(cuts[:-1], cuts[1:]) if b > a]
            self.n_parts = len(self._parts)
            self._part_counts = torch.zeros(2 * self.n_parts, dtype=torch.int32).pin_memory()
        return self.n_parts

    def _chunk_plan(self):
        """Plan arrays and workspace of the intra-slice parallel path (built once, reused)."""
        if getattr(self, "_plan", None) is None:
            self._plan = self._plan_of(0, self.n_slices)
        return self._plan

    def encode_chunked(self):
        """K1 / K2 through the intra-slice parallel kernels (same bytes as encode())."""
        import torch
        self._verify_layout = "slices"
        recs, rec_off = self._slice_major()
        p = self._chunk_plan()
        if self.kind == KIND_CABAC8:                         # one-byte records: nothing to guess, nothing waits
            _check(lib().avr_cabac8_encode_chunked_device(
                self.device_index, _stream_ptr(torch), recs.data_ptr(), rec_off.data_ptr(), self.n_bins.data_ptr(),
                self.n_slices, self.init_states.data_ptr(), self.n_states, ctypes.byref(p["plan"]), _aligned(p["ws"]),
                p["ws_bytes"], self.out.data_ptr(), self.out_off.data_ptr(), self.out_len.data_ptr(), self.status.data_ptr(),
                self.final_states.data_ptr()))
            return
        if self.kind != KIND_CABAC:
            L = lib()
            out_total = int(self.out_off[-1].item()) if "out_total" not in p else p["out_total"]
            p["out_total"] = out_total
            if "ws_k2" not in p:
                n = L.avr_range_chunked_workspace_bytes(self.n_slices, ctypes.byref(p["plan"]), out_total)
                p["ws_k2"] = torch.empty(n + 256, dtype=torch.uint8, device=self.n_bins.device)
                p["ws_k2_bytes"] = n
            ws_ptr = _aligned(p["ws_k2"])
            _check(L.avr_range_encode_chunked_device(
                self.device_index, _stream_ptr(torch), recs.data_ptr(), rec_off.data_ptr(), self.n_bins.data_ptr(), self.n_slices,
                ctypes.byref(p["plan"]), ws_ptr, p["ws_k2_bytes"], self.out.data_ptr(), self.out_off.data_ptr(), out_total,
                self.out_len.data_ptr(), self.status.data_ptr()))
            return
        ws_ptr = _aligned(p["ws"])
        if self._counts is not None and getattr(self, "_parts", None):
            self._hinted_path = "parts"
            if getattr(self, "_status_before", None) is None:
                self._status_before = self.status.clone()
            self._part_args = self._part_array(self.rows_hint)
            _check(lib().avr_cabac_encode_chunked_device_parts(
                self.device_index, _stream_ptr(torch), recs.data_ptr(), self.n_states, self.out.data_ptr(),
                ctypes.cast(self._part_args, ctypes.c_void_p), self.n_parts))
            return
        if self._counts is not None:                         # sized by the previous run's context count: see encode(), settle()
            self._hinted_path = "chunked"
            if getattr(self, "_status_before", None) is None:
                self._status_before = self.status.clone()    # (a run whose guess was too small is repeated from these)
            _check(lib().avr_cabac_encode_chunked_device_hinted(
                self.device_index, _stream_ptr(torch), recs.data_ptr(), rec_off.data_ptr(), self.n_bins.data_ptr(),
                self.n_slices, self.init_states.data_ptr(), self.n_states, ctypes.byref(p["plan"]), ws_ptr, p["ws_bytes"],
                self.out.data_ptr(), self.out_off.data_ptr(), self.out_len.data_ptr(), self.status.data_ptr(),
                self.final_states.data_ptr() if self.final_states is not None else None, self.rows_hint, self._counts.data_ptr()))
            return
        _check(lib().avr_cabac_encode_chunked_device(
            self.device_index, _stream_ptr(torch), recs.data_ptr(), rec_off.data_ptr(), self.n_bins.data_ptr(),
            self.n_slices, self.init_states.data_ptr(), self.n_states, ctypes.byref(p["plan"]), ws_ptr, p["ws_bytes"],
            self.out.data_ptr(), self.out_off.data_ptr(), self.out_len.data_ptr(), self.status.data_ptr(),
            self.final_states.data_ptr() if self.final_states is not None else None))

    def resolve(self):
        """Stage 1 of K1p alone: resolved codes (uint8 tensor, slice i at res_off[i]) on the device."""
        import torch
        recs, rec_off = self._slice_major()
        p = self._chunk_plan()
        L = lib()
        if "codes" not in p:
            n = L.avr_cabac_resolve_workspace_bytes(self.n_slices, self.n_states, ctypes.byref(p["plan"]))
            p["ws1"] = torch.empty(n + 256, dtype=torch.uint8, device=self.n_bins.device)
            p["ws1_bytes"] = n
            p["codes"] = torch.empty(p["plan"].res_total + 32 + 256, dtype=torch.uint8, device=self.n_bins.device)
        _check(L.avr_cabac_resolve_device(
            self.device_index, _stream_ptr(torch), recs.data_ptr(), rec_off.data_ptr(), self.n_bins.data_ptr(), self.n_slices,
            self.init_states.data_ptr(), self.n_states, ctypes.byref(p["plan"]), _aligned(p["ws1"]), p["ws1_bytes"], _aligned(p["codes"]),
            self.status.data_ptr(), self.final_states.data_ptr() if self.final_states is not None else None))
        off = _aligned(p["codes"]) - p["codes"].data_ptr()
        return p["codes"][off:off + p["plan"].res_total + 32]

    def encode_resolved(self, codes):
        """Stage 2 of K1p alone: arithmetic coding from resolved codes (same bytes as encode())."""
        import torch
        self._verify_layout, self._verify_codes = "codes", codes
        p = self._chunk_plan()
        L = lib()
        if "ws2" not in p:
            n = L.avr_cabac_resolved_workspace_bytes(self.n_slices, ctypes.byref(p["plan"]))
            p["ws2"] = torch.empty(n + 256, dtype=torch.uint8, device=self.n_bins.device)
            p["ws2_bytes"] = n
        _check(L.avr_cabac_encode_resolved_device(
            self.device_index, _stream_ptr(torch), codes.data_ptr(), self.n_bins.data_ptr(), self.n_slices,
            ctypes.byref(p["plan"]), _aligned(p["ws2"]), p["ws2_bytes"], self.out.data_ptr(),
            self.out_off.data_ptr(), self.out_len.data_ptr(), self.status.data_ptr()))

    def encode_codes_serial(self, codes):
        """K1 from resolved codes with one lane per slice (k_cabac_encode_codes): same bytes as encode()."""
        import torch
        self._verify_layout, self._verify_codes = "codes", codes
        p = self._chunk_plan()
        _check(lib().avr_cabac_encode_codes_device(
            self.device_index, _stream_ptr(torch), codes.data_ptr(), p["tensors"]["res_off"].data_ptr(), self.n_bins.data_ptr(),
            self.order.data_ptr(), self.n_slices, self.out.data_ptr(), self.out_off.data_ptr(), self.out_len.data_ptr(),
            self.status.data_ptr()))

    def encode_slice_major(self):
        """Same result from the slice-major layout (only for workloads built with from_host)."""
        import torch
        self._verify_layout = "slices"
        L = lib()
        sp = _stream_ptr(torch)
        if self.kind == KIND_CABAC:
            _check(L.avr_cabac_encode_slices_device(
                self.device_index, sp, self.rec_flat.data_ptr(), self.rec_off.data_ptr(), self.n_bins.data_ptr(),
                self.order.data_ptr(), self.n_slices, self.init_states.data_ptr(), self.n_states, self.out.data_ptr(),
                self.out_off.data_ptr(), self.out_len.data_ptr(), self.status.data_ptr(), self.final_states.data_ptr()))
        else:
            _check(L.avr_range_encode_slices_device(
                self.device_index, sp, self.rec_flat.data_ptr(), self.rec_off.data_ptr(), self.n_bins.data_ptr(),
                self.order.data_ptr(), self.n_slices, self.out.data_ptr(), self.out_off.data_ptr(),
                self.out_len.data_ptr(), self.status.data_ptr()))

    def verify(self):
        """K2 only, behind encode() / encode_chunked() / encode_slice_major() on torch's current stream: every AVR_SLICE_OK slice
        decoded back on the device against its records (avr_range_verify_tiles_device after encode(), avr_range_verify_slices_device
        after the two slice-major calls).  Returns the first_bad tensor (int32; VERIFY_NONE reads as -1) and leaves the statuses in
        self.status: SLICE_VERIFY_FAILED for a slice whose bytes do not decode to its bins.  Enqueues and returns."""
        import torch
        if self.kind != KIND_RANGE:
            raise AvrError("verify: the verifier exists for K2 (KIND_RANGE) workloads only")
        layout = getattr(self, "_verify_layout", None)
        if layout is None:
            raise AvrError("verify: nothing was encoded yet")
        L = lib()
        first_bad = torch.empty(self.n_slices, dtype=torch.int32, device=self.n_bins.device)
        if layout == "tiles":
            _check(L.avr_range_verify_tiles_device(
                self.device_index, _stream_ptr(torch), self.tiles.data_ptr(), self.tile_off.data_ptr(), self.n_bins.data_ptr(),
                self.order.data_ptr(), self.n_slices, self.out.data_ptr(), self.out_off.data_ptr(), self.out_len.data_ptr(),
                self.status.data_ptr(), first_bad.data_ptr()))
        else:
            recs, rec_off = self._slice_major()
            _check(L.avr_range_verify_slices_device(
                self.device_index, _stream_ptr(torch), recs.data_ptr(), rec_off.data_ptr(), self.n_bins.data_ptr(), None,
                self.n_slices, self.out.data_ptr(), self.out_off.data_ptr(), self.out_len.data_ptr(), self.status.data_ptr(),
                first_bad.data_ptr()))
        return first_bad

    def verify_k1(self):
        """K1 only (KIND_CABAC, KIND_CABAC8), behind encode() / encode_chunked() / encode_slice_major() / encode_resolved() /
        encode_codes_serial() on torch's current stream: every AVR_SLICE_OK slice decoded back on the device by the CABAC decoder of
        the standard against what that call read -- two-byte or one-byte tiles after encode(), the slice-major records after the two
        slice-major calls, the codes after the two code calls -- and, where the call left final states, the decoder's states compared
        with them.  Returns the first_bad tensor (int32; VERIFY_NONE reads as -1, n_bins: only the final states differ) and leaves the
        statuses in self.status: SLICE_VERIFY_FAILED for a slice that does not decode.  Enqueues and returns.  (A slice that a hinted
        run has handed to its second pass is skipped until settle() has coded it.)"""
        import torch
        if self.kind not in (KIND_CABAC, KIND_CABAC8):
            raise AvrError("verify_k1: the K1 verifier exists for K1 (KIND_CABAC, KIND_CABAC8) workloads only")
        layout = getattr(self, "_verify_layout", None)
        if layout is None:
            raise AvrError("verify_k1: nothing was encoded yet")
        L, sp = lib(), _stream_ptr(torch)
        first_bad = torch.empty(self.n_slices, dtype=torch.int32, device=self.n_bins.device)
        init = self.init_states.data_ptr() if self.init_states is not None and self.n_states else None
        final = self.final_states.data_ptr() if self.final_states is not None and self.n_states else None
        tail = (self.out.data_ptr(), self.out_off.data_ptr(), self.out_len.data_ptr())
        if layout == "codes":
            _check(L.avr_cabac_verify_codes_device(
                self.device_index, sp, self._verify_codes.data_ptr(), self._chunk_plan()["tensors"]["res_off"].data_ptr(),
                self.n_bins.data_ptr(), None, self.n_slices, *tail, self.status.data_ptr(), first_bad.data_ptr()))
        elif layout == "tiles":
            call = L.avr_cabac8_verify_tiles_device if getattr(self, "narrow_tiles", False) else L.avr_cabac_verify_tiles_device
            _check(call(self.device_index, sp, self.tiles.data_ptr(), self.tile_off.data_ptr(), self.n_bins.data_ptr(),
                        self.order.data_ptr(), self.n_slices, init, self.n_states, *tail, final, self.status.data_ptr(),
                        first_bad.data_ptr()))
        else:
            recs, rec_off = self._slice_major()
            call = L.avr_cabac8_verify_slices_device if self.kind == KIND_CABAC8 else L.avr_cabac_verify_slices_device
            _check(call(self.device_index, sp, recs.data_ptr(), rec_off.data_ptr(), self.n_bins.data_ptr(), None, self.n_slices,
                        init, self.n_states, *tail, final, self.status.data_ptr(), first_bad.data_ptr()))
        return first_bad

    def restore_check(self, expect_list):
        """K1 only, behind any encode call of the workload on torch's current stream: the restore check (avr_restore_check_device) of
        every slice against expect_list[i] -- the payload (bytes) slice i is to restore through drop_stop_byte and tail_patch with the
        payload's own parity and last byte, or None for a slice without an expectation.  Returns (status, first_diff): self.status,
        where a slice with a finding has become SLICE_VERIFY_FAILED, and the first differing byte of each slice (int32; VERIFY_NONE
        reads as -1).  Enqueues and returns."""
        import numpy as np
        import torch
        if self.kind not in (KIND_CABAC, KIND_CABAC8):
            raise AvrError("restore_check: the restore check exists for K1 (KIND_CABAC, KIND_CABAC8) workloads only")
        if len(expect_list) != self.n_slices:
            raise AvrError(f"restore_check: {len(expect_list)} expectations for {self.n_slices} slices")
        off, lens, at = np.zeros(self.n_slices, np.int64), np.full(self.n_slices, -1, np.int32), 0     # -1: AVR_EXPECT_NONE
        for i, e in enumerate(expect_list):
            if e is not None:
                off[i], lens[i] = at, len(e)
                at += (len(e) + 7) & ~7
        flat = np.zeros(at + 8, np.uint8)
        for i, e in enumerate(expect_list):
            if e:
                flat[off[i]:off[i] + len(e)] = np.frombuffer(bytes(e), np.uint8)
        dev = self.n_bins.device
        expect, expect_off, expect_len = (torch.from_numpy(a).to(dev) for a in (flat, off, lens))
        first_diff = torch.empty(self.n_slices, dtype=torch.int32, device=dev)
        _check(lib().avr_restore_check_device(
            self.device_index, _stream_ptr(torch), self.out.data_ptr(), self.out_off.data_ptr(), self.out_len.data_ptr(), self.n_slices,
            expect.data_ptr(), expect_off.data_ptr(), expect_len.data_ptr(), self.status.data_ptr(), first_diff.data_ptr()))
        self._restore_expect = (expect, expect_off, expect_len)          # the kernel reads them after this call returns
        return self.status, first_diff

    # ---- accounting (DESIGN.md "algorithmic bytes")
    def output_bytes(self) -> int:
        import torch
        return int(self.out_len.to(torch.int64).sum().item())

    def algorithmic_bytes(self) -> int:
        """2*n_bins + n_states*n_slices (K1) + out_bytes + 16*n_slices."""
        states = self.n_states * self.n_slices if self.kind == KIND_CABAC else 0
        return 2 * self.total_bins + states + self.output_bytes() + 16 * self.n_slices

    def results(self):
        """(list of bytes per slice, status list) copied to the host."""
        import torch
        torch.cuda.synchronize(self.out.device)
        out, off = self.out.cpu().numpy(), self.out_off.cpu().numpy()
        lens, st = self.out_len.cpu().numpy(), self.status.cpu().numpy()
        return [out[off[i]:off[i] + min(int(lens[i]), int(off[i + 1] - off[i]))].tobytes()
                for i in range(self.n_slices)], st.tolist()

    def results_dense(self):
        """The coded bytes compacted on the device (avr_compact_device behind the encode on torch's current stream):
        (dense uint8 tensor, dense_off int64[n + 1]) on the device -- slice i's bytes are dense[dense_off[i]:dense_off[i + 1]], the
        concatenation of what results() returns.  Synchronises once, to size the view by dense_off[-1]."""
        import torch
        dense, dense_off = compact_device(self.out, self.out_off, self.out_len)
        return dense[:int(dense_off[-1].item())], dense_off

    def results_finished(self, finish_words):
        """The slices' bytes as their NAL units hold them (avr_finish_device behind the encode on torch's current stream):
        finish_words: one word per slice (finish_word), a sequence or an int32 tensor.  (dense uint8 tensor, dense_off int64[n + 1]) on
        the device, as results_dense() gives the coded bytes; a slice whose status is not SLICE_OK gives none.  Synchronises once, to
        size the view by dense_off[-1]."""
        import numpy as np
        import torch
        if not torch.is_tensor(finish_words):
            finish_words = torch.from_numpy(np.asarray(finish_words, dtype=np.uint32).view(np.int32).copy())
        dense, dense_off = finish_device(self.out, self.out_off, self.out_len, finish_words.to(self.out_off.device), self.status)
        return dense[:int(dense_off[-1].item())], dense_off
