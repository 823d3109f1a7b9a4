"""Caller-owned buffers of EXACTLY the size the library quotes, between guard bands, for tests/test_gpu_workspace.py.

Guarded(n) is one uint8 tensor of guard + align256(n) + guard bytes (plus up to 255 to reach the alignment), the whole of it
filled with a canary byte; .view is n bytes long and starts at a multiple of 256.  A kernel that writes a little before or behind
the bytes it was given writes into the test's own tensor, and .check() reports it as an assertion with the offsets of the first
and the last byte that changed.  The guard (64 KiB a side) is a DETECTOR, not a fence: it covers any off-by-a-row error of the
library's layouts; a write farther out than that leaves the tensor, and nothing here stops it.

The canary and every poison are tensor.fill_(): no kernel of the tests' own writes a buffer.

install() puts such views where DeviceWorkload (avrecode_ms_amd/device.py) keeps its caller-owned buffers: the workspaces in its
plan dictionaries (it passes align256(data_ptr()), which is data_ptr() itself for these views, and the quoted byte count), the
code buffer between the two stages, and out / out_len / status / final_states."""
import ctypes

import numpy as np

GUARD = 64 * 1024
CANARY = 0xC3


def align256(n):
    return (int(n) + 255) // 256 * 256


class Guarded:
    def __init__(self, n, device="cpu", what="buffer", canary=CANARY, guard=GUARD):
        import torch
        assert guard >= GUARD and n >= 0
        self.n, self.what, self.canary = int(n), what, canary
        self.raw = torch.full((guard + align256(n) + guard + 256,), canary, dtype=torch.uint8, device=device)
        self.start = guard + (-(self.raw.data_ptr() + guard)) % 256
        self.view = self.raw[self.start:self.start + self.n]
        assert self.view.data_ptr() % 256 == 0 and self.view.numel() == self.n
        assert self.start >= guard and self.raw.numel() - (self.start + self.n) >= guard

    def as_dtype(self, dtype):
        """The n bytes as a tensor of `dtype` (n a multiple of its size)."""
        return self.view.view(dtype)

    def changed(self):
        """None while both guards hold the canary, else (first, last, count): offsets RELATIVE TO THE VIEW's first byte of the
        first and the last guard byte that changed (negative: in front of the view; >= n: behind it)."""
        front, back = self.raw[:self.start], self.raw[self.start + self.n:]
        at = [int(x) - self.start for x in (front != self.canary).nonzero().flatten().tolist()]
        at += [int(x) + self.n for x in (back != self.canary).nonzero().flatten().tolist()]
        return (at[0], at[-1], len(at)) if at else None

    def check(self):
        c = self.changed()
        assert c is None, (f"{self.what} ({self.n} bytes): {c[2]} guard bytes changed, the first at offset {c[0]}, the last at offset {c[1]} "
                           f"(of the buffer's first byte; it ends at {self.n})")

    def extent(self, poison, block=1 << 26):
        """One past the last byte of the view that differs from `poison` (0: none does)."""
        for lo in range((self.n - 1) // block * block if self.n else 0, -1, -block):
            at = (self.view[lo:lo + block] != poison).nonzero().flatten()
            if at.numel():
                return lo + int(at[-1]) + 1
        return 0


def regions(w, at8=False):
    """The output regions of a workload rebuilt tight -- region i ends where region i + 1 begins and out is out_off[n] bytes, not a
    byte more -- starting at 0 or, at8, at 8 mod 16 (the first eight bytes of out belong to nobody).  Capacities as DeviceWorkload
    gives them (a multiple of 8, so of 16 after rounding: every start keeps the first one's residue)."""
    import torch
    cap = (w.out_off[1:] - w.out_off[:-1]).cpu().numpy().astype(np.int64)
    cap = (cap + 15) // 16 * 16
    off = np.zeros(cap.size + 1, np.int64)
    off[0] = 8 if at8 else 0
    off[1:] = off[0] + np.cumsum(cap)
    w.out_off = torch.from_numpy(off).to(w.out_off.device)
    return off


class Buffers:
    """Every caller-owned buffer of a DeviceWorkload as a Guarded one of the exact size (see install)."""

    def __init__(self):
        self.all = {}                                        # name -> Guarded

    def add(self, name, n, device):
        g = self.all[name] = Guarded(n, device, name)
        return g

    def workspaces(self):
        return {k: g for k, g in self.all.items() if k.startswith("ws")}

    def poison(self, value, w):
        """Fill every workspace, the code buffer and the outputs with `value`; status is the caller's to set."""
        for k, g in self.all.items():
            if k != "status":
                g.view.fill_(value)

    def check(self):
        for g in self.all.values():
            g.check()


def install(avr, w, at8=False, two_stage=False):
    """Replace w's caller-owned buffers with guarded ones of exactly the quoted / documented size:
      out            out_off[n] bytes (regions rebuilt tight, see regions())
      out_len        n_slices * 4;  status  n_slices * 4 (keeps its values);  final_states  n_slices * n_states
      ws / ws_k2     avr_cabac[8]_chunked_workspace_bytes / avr_range_chunked_workspace_bytes -- and each part's, after set_parts
      two_stage      ws1, ws2: avr_cabac_resolve_ / _resolved_workspace_bytes;  codes: res_total + 32
    Returns the Buffers."""
    import torch
    L = avr.lib()
    dev = w.n_bins.device
    b = Buffers()
    off = regions(w, at8)
    w.out = b.add("out", int(off[-1]), dev).view
    w.out_len = b.add("out_len", 4 * w.n_slices, dev).as_dtype(torch.int32)
    status = b.add("status", 4 * w.n_slices, dev).as_dtype(torch.int32)
    status.copy_(w.status)
    w.status = status
    if w.final_states is not None:
        w.final_states = b.add("final_states", w.n_slices * max(w.n_states, 1), dev).view
    p = w._chunk_plan()
    if w.kind in (avr.KIND_CABAC, avr.KIND_CABAC8):
        p["ws"] = b.add("ws", p["ws_bytes"], dev).view
        for i, part in enumerate(getattr(w, "_parts", None) or []):
            part["ws"] = b.add(f"ws_part{i}", part["ws_bytes"], dev).view
    else:
        p["out_total"] = int(off[-1])
        p["ws_k2_bytes"] = L.avr_range_chunked_workspace_bytes(w.n_slices, ctypes.byref(p["plan"]), p["out_total"])
        p["ws_k2"] = b.add("ws_k2", p["ws_k2_bytes"], dev).view
    if two_stage:
        p["ws1_bytes"] = L.avr_cabac_resolve_workspace_bytes(w.n_slices, w.n_states, ctypes.byref(p["plan"]))
        p["ws1"] = b.add("ws1", p["ws1_bytes"], dev).view
        p["codes"] = b.add("codes", p["plan"].res_total + 32, dev).view
        p["ws2_bytes"] = L.avr_cabac_resolved_workspace_bytes(w.n_slices, ctypes.byref(p["plan"]))
        p["ws2"] = b.add("ws2", p["ws2_bytes"], dev).view
    return b
