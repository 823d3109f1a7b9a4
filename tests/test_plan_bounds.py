"""The host side of the device planner (include/avrecode_ms_amd.h, "the plan, and the way back, on the device"): avr_plan_bounds holds
for every list of lengths the plan tests use, avr_chunk_plan_from refuses a plan whose totals passed its caps or 2^32, and the three
device calls refuse every listed argument error with AVR_ERR_INVALID before they look for a device -- there is none here.  The
expected totals are chunk_plan_arrays()', the torch twin's, on CPU tensors; nothing comes from the code under test.  No device needed:
the pointers handed in are addresses inside a host buffer, never dereferenced, and a call that got past its checks would answer
AVR_ERR_NO_DEVICE (with a GPU visible such a call is not made)."""
import ctypes

import pytest

from test_plan import batches

OK, ERR_INVALID, ERR_NO_DEVICE, ERR_CAPACITY = 0, -1, -2, -5

_ARENA = ctypes.create_string_buffer(32 * 256 + 256)            # the fake pointers' addresses: kept alive, never read or written
_BASE = (ctypes.addressof(_ARENA) + 255) & ~255
P = lambda k: _BASE + 256 * k


def bounds(L, n, total):
    c, b = ctypes.c_uint64(), ctypes.c_uint64()
    L.avr_plan_bounds(n, total, ctypes.byref(c), ctypes.byref(b))
    return c.value, b.value


def lists():
    return batches() + [[0] * n for n in (1, 2, 63, 1000)] + [[1024] * 5, [1025] * 5, [4096] * 5, [4097] * 5, [0xFFFFFFFF, 0, 1]]


@pytest.mark.parametrize("which", range(len(lists())))
def test_bounds_hold(avr, which):
    import torch
    from avrecode_ms_amd.device import chunk_plan_arrays
    lengths = lists()[which]
    _, (_, _, total_chunks, total_blocks) = chunk_plan_arrays(torch.tensor(lengths, dtype=torch.int64))
    cap_chunks, cap_blocks = bounds(avr.lib(), len(lengths), sum(lengths))
    assert (cap_chunks, cap_blocks) == (sum(lengths) // 1024 + len(lengths), sum(lengths) // 4096 + len(lengths))
    assert total_chunks <= cap_chunks and total_blocks <= cap_blocks
    if lengths and not any(lengths):                             # n slices of 0 bins: a chunk and a block each, and exactly that much room
        assert (total_chunks, total_blocks) == (cap_chunks, cap_blocks) == (len(lengths), len(lengths))


def test_bounds_take_null_and_the_quote_grows(avr):
    L = avr.lib()
    L.avr_plan_bounds(3, 5000, None, None)
    quotes = [L.avr_plan_workspace_bytes(n) for n in (0, 1, 64, 65, 4097, (1 << 20) + 65, (1 << 31) - 1)]
    assert quotes == sorted(quotes) and quotes[0] >= 256 and all(q % 256 == 0 for q in quotes)
    assert quotes[-2] < 32 * ((1 << 20) + 65)                    # "about 16 bytes a slice and a megabyte"


def plan_from(avr, caps, totals):
    a = avr.PlanArrays(P(0), None, 8, P(1), P(2), caps[0], P(3), P(4), P(5), P(6), caps[1])
    t = avr.PlanTotals(10, 20, 30, totals[0], totals[1], totals[2], totals[3], 0)
    plan = avr.ChunkPlan()
    rc = avr.lib().avr_chunk_plan_from(ctypes.byref(a), ctypes.byref(t), ctypes.byref(plan))
    return rc, plan


def test_chunk_plan_from(avr):
    rc, plan = plan_from(avr, (84, 26), (81440, 40695, 84, 26))                  # FIXED's totals, caps exactly met
    assert rc == OK
    assert (plan.res_off, plan.chunk_base, plan.chunk_slice, plan.blk_base, plan.blk_slice, plan.dig_off) == (P(4), P(1), P(2), P(5), P(6), P(3))
    assert (plan.res_total, plan.dig_total, plan.total_chunks, plan.total_blocks) == (81440, 40695, 84, 26)
    assert plan_from(avr, (83, 26), (81440, 40695, 84, 26))[0] == ERR_CAPACITY     # one chunk over
    assert plan_from(avr, (84, 25), (81440, 40695, 84, 26))[0] == ERR_CAPACITY     # one block over
    assert b"bound" in avr.lib().avr_last_error()
    G = 1 << 32
    assert plan_from(avr, (G - 1, G - 1), (1, 1, G - 1, G - 1))[0] == OK
    assert plan_from(avr, (G, G), (1, 1, G, 5))[0] == ERR_CAPACITY                # 2^32 chunks: chunk_base has wrapped
    assert plan_from(avr, (2 * G, 2 * G), (1, 1, 5, G + 7))[0] == ERR_CAPACITY
    L = avr.lib()
    assert L.avr_chunk_plan_from(None, None, None) == ERR_INVALID


# ---- the refusals of the three device calls

def chunks_call(avr, n=3, level=3, ws=None, ws_short=0, totals=P(9), n_bins=P(10), arrays=True, **fields):
    L = avr.lib()
    f = dict(out_off=P(0), rec_off=P(1), rec_round=8, chunk_base=P(2), chunk_slice=P(3), cap_chunks=100, dig_off=P(4), res_off=P(5),
             blk_base=P(6), blk_slice=P(7), cap_blocks=100)
    f.update(fields)
    a = avr.PlanArrays(*[f[name] for name, _ in avr.PlanArrays._fields_])
    quote = L.avr_plan_workspace_bytes(min(n, (1 << 31) - 1))
    return L.avr_plan_chunks_device(0, None, n_bins, n, level, ctypes.byref(a) if arrays else None, P(11) if ws is None else ws,
                                    max(0, quote - ws_short), totals)


def tiles_call(avr, n=3, per_chunk=8, ws=None, ws_short=0, totals=P(9), n_bins=P(10), order=P(0), tile_off=P(1)):
    L = avr.lib()
    quote = L.avr_plan_workspace_bytes(min(n, (1 << 31) - 1))
    return L.avr_plan_tiles_device(0, None, n_bins, n, per_chunk, order, tile_off, P(11) if ws is None else ws, max(0, quote - ws_short), totals)


def compact_call(avr, n=3, ws=None, ws_short=0, out=P(0), out_off=P(1), out_len=P(2), dense=P(3), cap=1000, dense_off=P(4)):
    L = avr.lib()
    quote = L.avr_plan_workspace_bytes(min(n, (1 << 31) - 1))
    return L.avr_compact_device(0, None, out, out_off, out_len, n, dense, cap, dense_off, P(11) if ws is None else ws, max(0, quote - ws_short))


REFUSALS = {
    # a null array that the level needs, with n_slices > 0
    "chunks: null out_off": lambda a: chunks_call(a, level=0, out_off=None),
    "chunks: null chunk_base": lambda a: chunks_call(a, level=1, chunk_base=None),
    "chunks: null chunk_slice": lambda a: chunks_call(a, level=1, chunk_slice=None),
    "chunks: null dig_off": lambda a: chunks_call(a, level=2, dig_off=None),
    "chunks: null res_off": lambda a: chunks_call(a, level=3, res_off=None),
    "chunks: null blk_base": lambda a: chunks_call(a, level=3, blk_base=None),
    "chunks: null blk_slice": lambda a: chunks_call(a, level=3, blk_slice=None),
    "chunks: null n_bins": lambda a: chunks_call(a, n_bins=None),
    "chunks: null arrays": lambda a: chunks_call(a, arrays=False),
    "chunks: null totals": lambda a: chunks_call(a, totals=None),
    "tiles: null n_bins": lambda a: tiles_call(a, n_bins=None),
    "tiles: null order": lambda a: tiles_call(a, order=None),
    "tiles: null tile_off": lambda a: tiles_call(a, tile_off=None),
    "tiles: null totals": lambda a: tiles_call(a, totals=None),
    "compact: null out": lambda a: compact_call(a, out=None),
    "compact: null out_off": lambda a: compact_call(a, out_off=None),
    "compact: null out_len": lambda a: compact_call(a, out_len=None),
    "compact: null dense": lambda a: compact_call(a, dense=None),
    "compact: null dense_off": lambda a: compact_call(a, dense_off=None),
    # a level outside 0..3
    "chunks: level -1": lambda a: chunks_call(a, level=-1),
    "chunks: level 4": lambda a: chunks_call(a, level=4),
    # rec_round or records_per_chunk not 8 or 16
    "chunks: rec_round 0": lambda a: chunks_call(a, rec_round=0),
    "chunks: rec_round 12": lambda a: chunks_call(a, rec_round=12),
    "chunks: rec_round 32": lambda a: chunks_call(a, rec_round=32),
    "tiles: records_per_chunk 0": lambda a: tiles_call(a, per_chunk=0),
    "tiles: records_per_chunk 4": lambda a: tiles_call(a, per_chunk=4),
    "tiles: records_per_chunk 24": lambda a: tiles_call(a, per_chunk=24),
    # a misaligned array or workspace
    "chunks: out_off + 4": lambda a: chunks_call(a, out_off=P(0) + 4),
    "chunks: rec_off + 4": lambda a: chunks_call(a, rec_off=P(1) + 4),
    "chunks: chunk_base + 2": lambda a: chunks_call(a, chunk_base=P(2) + 2),
    "chunks: chunk_slice + 1": lambda a: chunks_call(a, chunk_slice=P(3) + 1),
    "chunks: dig_off + 4": lambda a: chunks_call(a, dig_off=P(4) + 4),
    "chunks: res_off + 1": lambda a: chunks_call(a, res_off=P(5) + 1),
    "chunks: blk_base + 2": lambda a: chunks_call(a, blk_base=P(6) + 2),
    "chunks: blk_slice + 2": lambda a: chunks_call(a, blk_slice=P(7) + 2),
    "chunks: n_bins + 2": lambda a: chunks_call(a, n_bins=P(10) + 2),
    "chunks: totals + 4": lambda a: chunks_call(a, totals=P(9) + 4),
    "chunks: workspace + 128": lambda a: chunks_call(a, ws=P(11) + 128),
    "chunks: null workspace": lambda a: chunks_call(a, ws=0),
    "tiles: order + 2": lambda a: tiles_call(a, order=P(0) + 2),
    "tiles: tile_off + 4": lambda a: tiles_call(a, tile_off=P(1) + 4),
    "tiles: n_bins + 1": lambda a: tiles_call(a, n_bins=P(10) + 1),
    "tiles: workspace + 8": lambda a: tiles_call(a, ws=P(11) + 8),
    "compact: out_off + 4": lambda a: compact_call(a, out_off=P(1) + 4),
    "compact: out_len + 2": lambda a: compact_call(a, out_len=P(2) + 2),
    "compact: dense_off + 4": lambda a: compact_call(a, dense_off=P(4) + 4),
    "compact: workspace + 64": lambda a: compact_call(a, ws=P(11) + 64),
    # a workspace below the quote
    "chunks: workspace one byte short": lambda a: chunks_call(a, ws_short=1),
    "tiles: workspace one byte short": lambda a: tiles_call(a, ws_short=1),
    "compact: workspace one byte short": lambda a: compact_call(a, ws_short=1),
    "chunks: workspace short, n_slices 0": lambda a: chunks_call(a, n=0, ws_short=1),
    # n_slices >= 2^31
    "chunks: n_slices 2^31": lambda a: chunks_call(a, n=1 << 31),
    "tiles: n_slices 2^31": lambda a: tiles_call(a, n=1 << 31),
    "compact: n_slices 2^31": lambda a: compact_call(a, n=1 << 31),
}


@pytest.mark.parametrize("label", sorted(REFUSALS))
def test_refused_before_a_device_is_touched(avr, label):
    assert REFUSALS[label](avr) == ERR_INVALID, label
    assert avr.lib().avr_last_error() != b""


def test_sound_arguments_get_as_far_as_the_device(avr):
    """The same calls with nothing wrong pass every check: where no GPU is visible they answer AVR_ERR_NO_DEVICE.  An array a level
    does not write may be null or misaligned."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible: the pointers are not device memory")
    assert chunks_call(avr) == ERR_NO_DEVICE
    assert chunks_call(avr, level=0, rec_off=None, chunk_base=None, chunk_slice=P(3) + 1, dig_off=None, res_off=P(5) + 1, blk_base=None,
                       blk_slice=None) == ERR_NO_DEVICE
    assert chunks_call(avr, level=1, dig_off=None, res_off=None, blk_base=None, blk_slice=None) == ERR_NO_DEVICE
    assert chunks_call(avr, rec_round=16) == ERR_NO_DEVICE
    assert tiles_call(avr) == ERR_NO_DEVICE and tiles_call(avr, per_chunk=16) == ERR_NO_DEVICE
    assert compact_call(avr) == ERR_NO_DEVICE
    assert tiles_call(avr, n=0, n_bins=None, order=None) == ERR_NO_DEVICE          # an empty batch needs only what it writes
    assert compact_call(avr, n=0, out=None, out_off=None, out_len=None, dense=None) == ERR_NO_DEVICE

