"""A DeviceWorkload re-homed in sparse, very large caller-owned buffers, for tests/test_gpu_far_offsets.py.

Every device-resident call takes the caller's own 64-bit placement arrays (rec_off, out_off, tile_off; res_off and dig_off with
res_total and dig_total in an avr_chunk_plan) and the kernels index them unchecked.  Rehome takes a workload built by
DeviceWorkload.from_host -- packed from 0, as every other test leaves it -- and moves ONE placement array at a time (or all of them)
to offsets that do not fit in 32 bits, so that a kernel which keeps only the low word of one of them reads or writes the wrong
place.  Every large buffer starts at offset 0 and is allocated whole, so the wrong place is lower in the same allocation.

Layouts (the unit of an axis is what its offsets count: records for two-byte rec_off, bytes for one-byte rec_off, out_off and
res_off, 32-bit words for dig_off, 16-byte chunks for tile_off):
  F     far base: the slices packed as before, the first one at 2^32 units (tile_off: 2^28 units, a byte offset of 4 GiB; tile_off
        values at or above 2^32 -- 64 GiB of tiles before the first one -- stay untested: with the library's workspaces beside them
        they do not fit the 64 GiB a case may take)
  S     straddle: the same packing moved so that the middle of slice `k` (a carry chain of several chunks: its digit sums and the
        positions its chunks share matter) lies at 2^32 units -- it begins below and ends above, the other slices on either side
  W0, W8, Wlow (out_off only): the slices where they were, but the region of slice `k` declared 2^32 bytes, 2^32 + 8 bytes, or
        2^32 + align8(len) - 8 bytes long (eight bytes too few for a kernel that looks at the low word of a region's size alone);
        the slices behind it lie above 4 GiB

The slices' data is copied to its new place by torch indexing on the device; every large buffer is torch.empty + fill_(poison); the
host never holds, copies or compares a whole large buffer.  Workspaces, the code buffer and the outputs are tests/guarded.py buffers
of exactly the quoted / documented size (64 KiB of canary either side).  Nothing is allocated before materialize(), which is given
the sum first (`need`: the buffers, the library's quotes, and the 1 GiB block untouched() compares at a time)."""
import ctypes

import numpy as np

import guarded

B32 = 1 << 32
TILE_BASE = 1 << 28                                          # 16-byte chunks: a byte offset of 4 GiB
BLOCK = 1 << 30                                              # untouched() compares this many bytes at a time
RECORD_POISON, TILE_POISON = 0x5A, 0xFF


def _base(layout, off, k, unit, mid=None):
    """What to add to every offset: F 2^32; S so that the middle (`mid` units in, default half its extent) of slice k lies at 2^32."""
    if layout == "F":
        return B32
    assert layout == "S", layout
    half = (int(off[k + 1]) - int(off[k])) // 2 if mid is None else int(mid)
    at = (int(off[k]) + half) // unit * unit
    assert int(off[k]) < at < int(off[k + 1]), "the straddling slice needs more than a unit either side"
    return B32 - at


def count_not(t, value, lo=0, hi=None):
    """How many elements of t[lo:hi] differ from `value`: counted on the device, a block at a time; a 0-d tensor."""
    import torch
    hi = t.numel() if hi is None else hi
    step = BLOCK // t.element_size()
    bad = torch.zeros((), dtype=torch.int64, device=t.device)
    for a in range(lo, hi, step):
        bad += (t[a:min(a + step, hi)] != value).count_nonzero()
    return bad


class Rehome:
    """w: a DeviceWorkload from from_host (or from_host_keys); k: the slice that straddles / gets the wide region; lens: the expected
    output length of every slice (what W's regions and out_off S are placed by).  Call the axis methods, then buffers(), then
    materialize(); `need` is the number of bytes that will allocate."""

    def __init__(self, avr, w, k, lens=None):
        self.avr, self.w, self.k, self.lens = avr, w, k, lens
        self.dev = w.n_bins.device
        self.need = BLOCK
        self.steps = []                                      # allocations put off until materialize()
        self.bufs = guarded.Buffers()
        self.moved = {}                                      # axis -> (layout, base): for messages
        self.out_poisoned = None

    # -------------------------------------------------------------- the axes

    def _sparse(self, name, old, base_bytes, poison):
        """A buffer of base_bytes + old's bytes, poison everywhere but old's bytes at base_bytes; the attribute `name` of w is set
        to it (in old's dtype) at materialize()."""
        import torch
        n = old.numel() * old.element_size()
        self.need += base_bytes + n

        def step():
            buf = torch.empty(base_bytes + n, dtype=torch.uint8, device=self.dev)
            buf.fill_(poison)
            buf[base_bytes:] = old.view(torch.uint8) if old.dtype != torch.uint8 else old
            setattr(self.w, name, buf.view(old.dtype))
        self.steps.append(step)

    def rec_off(self, layout):
        """The slice-major records (two-byte: rec_flat, offsets in records; one-byte: rec8_flat, in bytes; key records: key_flat
        and the resolver's output beside it)."""
        w, avr = self.w, self.avr
        one_byte = w.kind == avr.KIND_CABAC8
        name = "rec8_off" if one_byte else "rec_off"
        off = getattr(w, name)
        base = _base(layout, off.cpu().numpy(), self.k, 16 if one_byte else 8)
        setattr(w, name, off + base)
        elem = 1 if one_byte else 2
        if w.kind == avr.KIND_RANGE_KEYS:
            self._sparse("key_flat", w.key_flat, base * elem, RECORD_POISON)
        self._sparse("rec8_flat" if one_byte else "rec_flat", w.rec8_flat if one_byte else w.rec_flat, base * elem, RECORD_POISON)
        self.moved[name] = (layout, base)

    def tile_off(self, layout="F"):
        assert layout == "F"
        self.w.tile_off = self.w.tile_off + TILE_BASE
        self._sparse("tiles", self.w.tiles, TILE_BASE * 16, TILE_POISON)
        self.moved["tile_off"] = (layout, TILE_BASE)

    def out_off(self, layout):
        """Regions of the capacities DeviceWorkload gives (multiples of 8), re-placed; `out` itself is made by buffers()."""
        import torch
        w, k = self.w, self.k
        off = w.out_off.cpu().numpy().astype(np.int64)
        if layout in ("F", "S"):
            base = _base(layout, off, k, 8, None if self.lens is None else max(8, self.lens[k] // 2))
            off = off + base
        else:
            cap = np.diff(off)
            cap[k] = {"W0": B32, "W8": B32 + 8, "Wlow": B32 + (self.lens[k] + 7) // 8 * 8 - 8}[layout]
            if layout == "Wlow":
                assert self.lens[k] > 8, "the low word of the region's size must be smaller than the slice"
            off = np.concatenate([[0], np.cumsum(cap)])
            base = 0
        w.out_off = torch.from_numpy(off).to(self.dev)
        self.moved["out_off"] = (layout, base)

    def _plans(self):
        """The plans the calls read: the parts' own where the batch is cut in parts (the whole batch's is then not used), else the batch's."""
        w = self.w
        return list(getattr(w, "_parts", None) or []) or [w._chunk_plan()]

    def _plan_axis(self, name, total, layout, unit):
        """res_off / dig_off of every plan the calls read (_plans), each by its own base: a part straddles at slice k if it holds
        it, else at its longest slice."""
        import torch
        for p in self._plans():
            t = p["tensors"]
            off = t[name].cpu().numpy()
            k = self.k - p["first"]
            if not 0 <= k < p["n"]:
                k = int(np.argmax(np.diff(off)))
            base = _base(layout, off, k, unit)
            t[name] = t[name] + base
            setattr(p["plan"], name, t[name].data_ptr())
            setattr(p["plan"], total, int(getattr(p["plan"], total)) + base)
            self.moved[name] = (layout, base)

    def res_off(self, layout):
        self._plan_axis("res_off", "res_total", layout, 16)

    def dig_off(self, layout):
        self._plan_axis("dig_off", "dig_total", layout, 1)

    def axis(self, name):
        """'rec-F', 'out-W8', 'dig-S', ...: one axis in one layout."""
        which, layout = name.split("-")
        getattr(self, which + "_off")(layout)

    # -------------------------------------------------------------- the buffers the calls write

    def _guarded(self, name, n, fill=None):
        """A guarded buffer of exactly n bytes, allocated at materialize(); returns a function that gives its view afterwards."""
        self.need += guarded.align256(n) + 2 * guarded.GUARD + 256

        def step():
            g = self.bufs.add(name, n, self.dev)
            if fill is not None:
                fill(g)
        self.steps.append(step)
        return lambda: self.bufs.all[name].view

    def buffers(self, two_stage=False):
        """out (out_off[n] bytes, not one more), out_len, status (keeps its values), final_states, and every workspace the
        workload's calls take, at the size the library quotes for the plan as it now stands."""
        import torch
        w, avr, L = self.w, self.avr, self.avr.lib()
        out_total = int(w.out_off[-1])
        out = self._guarded("out", out_total)
        out_len = self._guarded("out_len", 4 * w.n_slices)
        status0 = w.status
        status = self._guarded("status", 4 * w.n_slices, lambda g: g.as_dtype(torch.int32).copy_(status0))
        fs = self._guarded("final_states", w.n_slices * max(w.n_states, 1)) if w.final_states is not None else None
        p = w._chunk_plan()
        ws = []
        if w.kind in (avr.KIND_CABAC, avr.KIND_CABAC8):
            ws_of = L.avr_cabac8_chunked_workspace_bytes if w.kind == avr.KIND_CABAC8 else L.avr_cabac_chunked_workspace_bytes
            parts = getattr(w, "_parts", None) or []
            for i, part in enumerate(parts):
                part["ws_bytes"] = ws_of(part["n"], w.n_states, ctypes.byref(part["plan"]))
                ws.append((part, "ws", self._guarded(f"ws_part{i}", part["ws_bytes"])))
            p.pop("ws", None)
            if not two_stage:                                # (with parts: DeviceWorkload still aligns the whole batch's, which stays as it was)
                p["ws_bytes"] = ws_of(w.n_slices, w.n_states, ctypes.byref(p["plan"]))
                ws.append((p, "ws", self._guarded("ws", p["ws_bytes"])))
        elif w.kind == avr.KIND_RANGE:
            p["out_total"] = out_total
            p["ws_k2_bytes"] = L.avr_range_chunked_workspace_bytes(w.n_slices, ctypes.byref(p["plan"]), out_total)
            ws.append((p, "ws_k2", self._guarded("ws_k2", p["ws_k2_bytes"])))
        if two_stage:
            p["ws1_bytes"] = L.avr_cabac_resolve_workspace_bytes(w.n_slices, w.n_states, ctypes.byref(p["plan"]))
            p["ws2_bytes"] = L.avr_cabac_resolved_workspace_bytes(w.n_slices, ctypes.byref(p["plan"]))
            ws.append((p, "ws1", self._guarded("ws1", p["ws1_bytes"])))
            ws.append((p, "codes", self._guarded("codes", int(p["plan"].res_total) + 32)))
            ws.append((p, "ws2", self._guarded("ws2", p["ws2_bytes"])))

        def step():
            w.out, w.out_len, w.status = out(), out_len().view(torch.int32), status().view(torch.int32)
            if fs is not None:
                w.final_states = fs()
            for plan, key, view in ws:
                plan[key] = view()
        self.steps.append(step)

    def materialize(self, refuse):
        """Allocate everything that was planned.  refuse(need, free): called instead when the device reports less free memory than
        need + 2 GiB."""
        import torch
        torch.cuda.empty_cache()
        free = torch.cuda.mem_get_info(self.dev)[0]
        if free < self.need + (2 << 30):
            refuse(self.need, free)
        for step in self.steps:
            step()
        self.steps = []
        self.off = self.w.out_off.cpu().numpy().astype(np.int64)
        self.status0 = self.w.status.clone()
        torch.cuda.synchronize()
        return self

    # -------------------------------------------------------------- before and after a call

    def poison(self, value):
        """Every workspace, the code buffer and the outputs filled with `value`; status back to what the packer left."""
        self.bufs.poison(value, self.w)
        self.w.status.copy_(self.status0)
        self.out_poisoned = value

    def untouched(self, spans):
        """How many bytes of `out` outside `spans` ([(begin, end)], ascending) differ from the poison -- counted on the device, a
        block at a time."""
        import torch
        out, poison = self.w.out, self.out_poisoned
        bad = torch.zeros((), dtype=torch.int64, device=self.dev)
        at = 0
        for a, b in list(spans) + [(out.numel(), out.numel())]:
            assert at <= a <= b, "spans overlap or are out of order"
            if a > at:
                bad += count_not(out, poison, at, a)
            at = b
        return int(bad)

    def compare(self, wants, what, left=(), region=()):
        """Status, length, bytes and final states of every slice against `wants` ([(status, bytes, final states)]); every other byte
        of out still the poison; every guard intact.  left: slices left uncoded on purpose; region: slices whose whole region may
        have been written (the header: a slice a coder gives up on while coding it), their status and length checked all the same."""
        import torch
        torch.cuda.synchronize()
        w, off = self.w, self.off
        what = f"{what} [{self.moved}]"
        lens = w.out_len.cpu().numpy().astype(np.int64)
        status = w.status.cpu().numpy()
        fs = w.final_states.cpu().numpy().reshape(w.n_slices, -1) if w.final_states is not None else None
        spans = []
        for i, (st, data, final) in enumerate(wants):
            if i in left:
                spans.append((off[i], off[i + 1]))
                continue
            assert status[i] == st, f"{what}: status of slice {i}: {status[i]}, want {st}"
            if data is None:                                 # (ZERO_PROB: only the status is specified)
                spans.append((off[i], off[i + 1]))
                continue
            assert lens[i] == len(data), f"{what}: length of slice {i}: {lens[i]}, want {len(data)}"
            got = w.out[int(off[i]):int(off[i]) + len(data)].cpu().numpy().tobytes()
            if got != data:
                at = next(j for j in range(len(data)) if got[j] != data[j])
                raise AssertionError(f"{what}: slice {i} ({len(data)} bytes at {off[i]:#x}) differs from byte {at} on")
            spans.append((int(off[i]), int(off[i + 1]) if i in region else int(off[i]) + len(data)))
            if final is not None and fs is not None:
                assert fs[i][:len(final)].tobytes() == final, f"{what}: final states of slice {i}"
        bad = self.untouched(spans)
        assert bad == 0, f"{what}: {bad} bytes of out written outside the slices' bytes"
        self.bufs.check()
