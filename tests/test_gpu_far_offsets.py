"""GPU: every device path on slices placed beyond 4 GiB offsets (tests/far_offsets.py re-homes the workloads).

The device-resident calls take the caller's own 64-bit rec_off, out_off, tile_off, and res_off / dig_off with res_total / dig_total
in the chunk plan; the census and the remap take a 64-bit n_records.  Every other test packs from 0 (or 8), so the high word of every
one of those address computations was never anything but zero.  Here each path runs with ONE of its placement arrays moved -- F: the
first slice at 2^32 units; S: a carry-chain slice of several chunks astride 2^32 units; for out_off also W0 / W8 / Wlow: one region
declared 2^32, 2^32 + 8 and 2^32 + align8(len) - 8 bytes long -- and once with all of them at F ("all").  tile_off is moved to 2^28
units, a byte offset of 4 GiB; tile_off values of 2^32 and more (64 GiB of tiles in front) stay untested: beside the other buffers
they do not fit a case's budget.

Batches: test_gpu_workspace's cabac_batch / range_batch at their smallest -- the edge lengths 0, 1, 1023, 1024, 1025, 4095, 4096,
4097, four ragged slices below 9000 bins, two carry chains, the two slices K1p declines, a malformed slice in the middle, for K2 the
`neg 0` slice.  Expected answers: bad_records.expected, cached per batch.  Every case checks, under the poisons 0xFF and 0x5A: status,
length, bytes and final states of every slice; that every byte of `out` outside the slices' own bytes still holds the poison (counted
on the device, a GiB at a time: the host sees the slices' bytes only); and that workspaces, the code buffer and the outputs -- each
exactly the quoted or documented size -- left their 64 KiB guards alone.

Memory.  A case adds up what it will allocate before it allocates (Rehome.need: its sparse buffers, the library's quotes for the
plan as moved, a 1 GiB block for the comparisons) and skips only if the device reports less free than that plus 2 GiB -- the one
skip of this file; everything is freed before the next case.  Largest needs, in GiB (the budget is 64):
  packers              rec 9 (one-byte 5), tile 9
  tiles coders         tile 5, out 5, all 9
  slice-major coders   rec 9, out 5, all 13;  from codes: res 5, out 5, all 9
  K1p                  rec 9 (one-byte 5), out 5, res 5, dig 17, all 33;  in two parts: res 9, dig 33, all 53
  two-stage            rec 9, out 5, res 5, dig 17, all 33
  K2p                  rec 9, out 21 (the digit workspace is four bytes to a byte of out_total), all 29
  estimator resolver   17 (key records and the records it writes);  census / remap  9
dig_off F on K1p fits (2^32 words are 16 GiB of digit sums), so no case falls back to a byte-level variant.

That these tests can fail was shown on two builds with one token changed, each run once over this file (a truncated offset lands
lower in the same allocation, in poison: wrong answers, no fault):
  `p.recs + uint32_t(p.rec_off[s])` in k_k1p_replay (K1p's phase A from two-byte records): 15 cases fail -- rec-F, rec-S and all of
      test_k1p_one_call, test_k1p_hinted, test_k1p_second_pass, test_k1p_parts and test_two_stage -- on a slice's status or bytes;
      the other 148 pass (the one-byte records take the kernel's other branch)
  `o0 = uint32_t(out_off[slice])` in k_range_encode: 12 cases fail -- out-F, out-S, out-W0, out-W8, out-Wlow and all of the range
      cases of test_tile_coders and test_slice_major_coders; the other 151 pass
What family W found on the kernels as they were before: a slice's capacity was uint32_t(out_off[i + 1] - out_off[i]) in six
kernels, so a region of exactly 2^32 bytes counted as one of 0 and one of 2^32 + 8 as one of 8 -- all 48 W cases of this file failed
there, every one on "status of slice 3 (2): 2, want 0", AVR_SLICE_OVERFLOW for a valid call; region_capacity() (csrc/avr_coder.h)
saturates the gap, and the 48 pass."""
import ctypes
import gc

import numpy as np
import pytest

import far_offsets
from far_offsets import B32, Rehome
from test_gpu_workspace import cabac_batch, make, narrow, range_batch, run_settled

pytestmark = pytest.mark.gpu

POISONS = (0xFF, 0x5A)
K_CABAC, K_RANGE = 3, 2                                      # the carry chains' places in the two batches
OUT = ["out-F", "out-S", "out-W0", "out-W8", "out-Wlow"]
REC = ["rec-F", "rec-S"]


def batch_cabac(rare=False):
    b = cabac_batch(4100 + rare, 86, ragged=4, top=9000, rare=rare)
    assert len(b[0][K_CABAC][0]) > 4 * 1024 and b[1][K_CABAC][0] == 0
    return b


def batch_cabac8():
    s, w, named = batch_cabac()
    return narrow(s, w) + (named,)


def batch_range():
    b = range_batch(4200, ragged=4, top=9000)
    assert len(b[0][K_RANGE]) > 4 * 1024 and b[1][K_RANGE][0] == 0
    return b


@pytest.fixture(autouse=True)
def freed():
    """Everything a case allocated is given back before the next one; after a fault of the device nothing more is run on it."""
    import torch
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"the device reported an error, no further case is run on it: {e}", returncode=3)
    gc.collect()
    torch.cuda.empty_cache()


def refuse(need, free):
    pytest.skip(f"the case needs {need} bytes and 2 GiB beside them; the device reports {free} free")


def rehome(avr, kind, batch, axes, k, two_stage=False, parts=0, plain=False, narrow_tiles=False):
    """The batch as a DeviceWorkload with `axes` ("rec-F", "out-W8", ...; see axes_of for "all") moved, in guarded buffers."""
    slices, wants, _ = batch
    if narrow_tiles:
        w = avr.DeviceWorkload.from_host(avr.KIND_CABAC8, [r for r, _ in slices], [s for _, s in slices], 0, narrow_tiles=True)
    else:
        w = make(avr, kind, slices)
    if parts:
        assert w.set_parts(parts, [1, 8]) == parts
    if plain:
        w._counts = None                                     # the calls that ask the device themselves, not the hinted ones
    r = Rehome(avr, w, k, [len(x[1]) if x[1] is not None else 0 for x in wants])
    for a in axes:
        r.axis(a)
    r.buffers(two_stage)
    r.materialize(refuse)
    r.wants = wants
    return r


def under_every_poison(r, call, what, after=None, region=()):
    for poison in POISONS:
        r.poison(poison)
        call()
        r.compare(r.wants, f"{what}, poison {poison:#x}", region=region)
        if after:
            after(poison)


def axes_of(layout, every):
    return every if layout == "all" else [layout]


# ------------------------------------------------------------------ the packers

@pytest.mark.parametrize("layout", REC + ["tile-F"])
@pytest.mark.parametrize("entry", ["cabac", "range", "one-byte", "one-byte-narrow"])
def test_packers(avr, entry, layout):
    """avr_pack_tiles_device (both kinds), avr_pack_tiles8_device, avr_pack_tiles8_narrow_device: from records far away, or into
    tiles far away, the very tiles (and statuses: the malformed slice) that the same call makes of the batch packed from 0 -- both
    into 0xFF, since the narrow packer leaves what it does not own -- and not a byte in front of them."""
    import torch
    L = avr.lib()
    kind = {"cabac": avr.KIND_CABAC, "range": avr.KIND_RANGE}.get(entry, avr.KIND_CABAC8)
    batch = batch_range() if entry == "range" else batch_cabac8() if kind == avr.KIND_CABAC8 else batch_cabac()
    k = K_RANGE if entry == "range" else K_CABAC
    slices = batch[0]
    if entry == "one-byte-narrow":
        w = avr.DeviceWorkload.from_host(avr.KIND_CABAC8, [r for r, _ in slices], [s for _, s in slices], 0, narrow_tiles=True)
    else:
        w = make(avr, kind, slices)

    def pack(tiles):
        st = torch.zeros(w.n_slices, dtype=torch.int32, device=tiles.device)
        sp = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        if kind == avr.KIND_CABAC8:
            f = L.avr_pack_tiles8_narrow_device if entry == "one-byte-narrow" else L.avr_pack_tiles8_device
            rc = f(0, sp, w.n_states, w.rec8_flat.data_ptr(), w.rec8_off.data_ptr(), w.n_bins.data_ptr(), w.order.data_ptr(), w.n_slices,
                   w.tile_off.data_ptr(), tiles.data_ptr(), st.data_ptr())
        else:
            rc = L.avr_pack_tiles_device(0, sp, kind, w.n_states, w.rec_flat.data_ptr(), w.rec_off.data_ptr(), w.n_bins.data_ptr(),
                                         w.order.data_ptr(), w.n_slices, w.tile_off.data_ptr(), tiles.data_ptr(), st.data_ptr())
        assert rc == 0
        torch.cuda.synchronize()
        return st

    near = torch.empty_like(w.tiles).fill_(0xFF)
    st_near = pack(near)
    # (one-byte records: the batch's malformed record is a put_terminate(1) that is not last, which the coders find, not the packers)
    assert (st_near != 0).sum() == (0 if kind == avr.KIND_CABAC8 else 1) and torch.equal(st_near, w.status)
    r = Rehome(avr, w, k)
    r.axis(layout)
    r.need += w.tiles.numel() + (far_offsets.TILE_BASE * 16 if layout == "tile-F" else 0)
    r.materialize(refuse)
    front = far_offsets.TILE_BASE * 16 if layout == "tile-F" else 0
    far = torch.empty(front + near.numel(), dtype=torch.uint8, device=near.device).fill_(0xFF)
    st_far = pack(far)
    assert torch.equal(st_far, st_near), f"{entry}, {r.moved}: statuses {st_far.tolist()}"
    assert torch.equal(far[front:], near), f"{entry}, {r.moved}: the tiles differ"
    assert int(far_offsets.count_not(far, 0xFF, 0, front)) == 0, f"{entry}, {r.moved}: bytes written in front of the tiles"


# ------------------------------------------------------------------ one lane per slice, from tiles

@pytest.mark.parametrize("layout", ["tile-F"] + OUT + ["all"])
@pytest.mark.parametrize("entry", ["cabac", "cabac-hinted", "one-byte", "range"])
def test_tile_coders(avr, entry, layout):
    """avr_cabac_encode_tiles_device, its _hinted form (asked, then sized by the guess), avr_cabac8_encode_tiles_device,
    avr_range_encode_tiles_device with avr_range_verify_tiles_device behind it."""
    import torch
    axes = axes_of(layout, ["tile-F", "out-F"])
    if entry == "range":
        r = rehome(avr, avr.KIND_RANGE, batch_range(), axes, K_RANGE)
    elif entry == "one-byte":
        r = rehome(avr, avr.KIND_CABAC8, batch_cabac8(), axes, K_CABAC, narrow_tiles=True)
    else:
        r = rehome(avr, avr.KIND_CABAC, batch_cabac(), axes, K_CABAC, plain=entry == "cabac")
    w = r.w
    # the one-byte coder meets the batch's malformed record -- a put_terminate(1) that is not last -- only while it codes the slice:
    # status and length 0 as on every path, but bytes of that slice's own region are written (the header's MEMORY paragraph)
    given_up = [batch_cabac()[2]["bad"]] if entry == "one-byte" else []

    def call():
        w.encode()
        if entry == "cabac-hinted":
            torch.cuda.synchronize()
            assert w._hinted_path == "tiles" and w.settle()["rows"] >= 1

    def verified(poison):
        first_bad = w.verify()
        torch.cuda.synchronize()
        assert (first_bad == -1).all(), f"verifier over tiles, {r.moved}: first_bad {first_bad.tolist()}"
        r.compare(r.wants, f"behind the verifier, poison {poison:#x}")

    for run in ("asked", "guessed") if entry == "cabac-hinted" else ("once",):
        under_every_poison(r, call, f"tiles, {entry}, {run}", verified if entry == "range" else None, region=given_up)
    assert entry != "cabac-hinted" or w.rows_hint


# ------------------------------------------------------------------ one lane per slice, slice-major

@pytest.mark.parametrize("layout", REC + OUT + ["all"])
@pytest.mark.parametrize("entry", ["cabac", "range"])
def test_slice_major_coders(avr, entry, layout):
    """avr_cabac_encode_slices_device, avr_range_encode_slices_device with avr_range_verify_slices_device behind it."""
    import torch
    axes = axes_of(layout, ["rec-F", "out-F"])
    if entry == "range":
        r = rehome(avr, avr.KIND_RANGE, batch_range(), axes, K_RANGE)
    else:
        r = rehome(avr, avr.KIND_CABAC, batch_cabac(), axes, K_CABAC)
    w = r.w

    def verified(poison):
        first_bad = w.verify()
        torch.cuda.synchronize()
        assert w._verify_layout == "slices" and (first_bad == -1).all(), f"slice-major verifier, {r.moved}: first_bad {first_bad.tolist()}"
        r.compare(r.wants, f"behind the verifier, poison {poison:#x}")

    under_every_poison(r, w.encode_slice_major, f"slice-major, {entry}", verified if entry == "range" else None)


@pytest.mark.parametrize("layout", ["res-F", "res-S"] + OUT + ["all"])
def test_serial_coder_from_codes(avr, layout):
    """avr_cabac_encode_codes_device from the codes avr_cabac_resolve_device left at res_off."""
    r = rehome(avr, avr.KIND_CABAC, batch_cabac(), axes_of(layout, ["res-F", "out-F"]), K_CABAC, two_stage=True)
    under_every_poison(r, lambda: r.w.encode_codes_serial(r.w.resolve()), "serial from codes")


# ------------------------------------------------------------------ K1p

K1P_AXES = REC + OUT + ["res-F", "res-S", "dig-F", "dig-S", "all"]
ALL_K1P = ["rec-F", "out-F", "res-F", "dig-F"]


@pytest.mark.parametrize("layout", K1P_AXES)
def test_k1p_one_call(avr, layout):
    """avr_cabac_encode_chunked_device."""
    r = rehome(avr, avr.KIND_CABAC, batch_cabac(), axes_of(layout, ALL_K1P), K_CABAC, plain=True)
    under_every_poison(r, r.w.encode_chunked, "K1p, one call")
    assert r.w._hinted_path is None


@pytest.mark.parametrize("layout", K1P_AXES)
def test_k1p_hinted(avr, layout):
    """avr_cabac_encode_chunked_device_hinted: asked, then sized by the guess."""
    r = rehome(avr, avr.KIND_CABAC, batch_cabac(), axes_of(layout, ALL_K1P), K_CABAC)
    w = r.w

    def call():
        info = run_settled(w)
        assert w._hinted_path == "chunked" and not info["redone"] and info["rows"] >= 1

    under_every_poison(r, call, "K1p hinted, asked")
    assert w.rows_hint
    under_every_poison(r, call, "K1p hinted, guessed")


@pytest.mark.parametrize("layout", K1P_AXES)
def test_k1p_second_pass(avr, hooks, layout):
    """avr_cabac_encode_chunked_second_pass_device: a census that sees next to nothing (hook census_stride=4099) leaves the slices
    with a rare context for it."""
    import torch
    hooks(census_stride=4099)
    r = rehome(avr, avr.KIND_CABAC, batch_cabac(rare=True), axes_of(layout, ALL_K1P), K_CABAC)
    w = r.w

    def asked():
        w.rows_hint = 0
        assert run_settled(w)["hint"] == 0 and w._hinted_path == "chunked"

    def guessed():
        hint = w.rows_hint
        assert hint
        w.encode_chunked()
        torch.cuda.synchronize()
        assert int(w._counts[0]) <= hint and int(w._counts[1]) >= 3, "the three slices with a rare context at least are left for the second pass"
        assert w.settle()["redone"]

    under_every_poison(r, asked, "K1p second pass, asked")
    under_every_poison(r, guessed, "K1p second pass, guessed")


@pytest.mark.parametrize("layout", K1P_AXES)
def test_k1p_parts(avr, layout):
    """avr_cabac_encode_chunked_device_parts in two parts, each with a plan and a workspace of its own: asked, then guessed."""
    r = rehome(avr, avr.KIND_CABAC, batch_cabac(), axes_of(layout, ALL_K1P), K_CABAC, parts=2)
    w = r.w
    assert len([n for n in r.bufs.all if n.startswith("ws_part")]) == 2

    def call():
        info = run_settled(w)
        assert w._hinted_path == "parts" and info["parts"] == 2 and not info["redone"]

    under_every_poison(r, call, "K1p in two parts, asked")
    assert w.rows_hint
    under_every_poison(r, call, "K1p in two parts, guessed")


@pytest.mark.parametrize("layout", K1P_AXES)
def test_k1p_one_byte_records(avr, layout):
    """avr_cabac8_encode_chunked_device (rec_off in bytes)."""
    r = rehome(avr, avr.KIND_CABAC8, batch_cabac8(), axes_of(layout, ALL_K1P), K_CABAC)
    under_every_poison(r, r.w.encode_chunked, "K1p, one-byte records")


@pytest.mark.parametrize("layout", K1P_AXES)
def test_two_stage(avr, layout):
    """avr_cabac_resolve_device, then avr_cabac_encode_resolved_device from the code buffer of res_total + 32 bytes."""
    r = rehome(avr, avr.KIND_CABAC, batch_cabac(), axes_of(layout, ALL_K1P), K_CABAC, two_stage=True)
    w = r.w

    def call():
        codes = w.resolve()
        assert codes.data_ptr() == r.bufs.all["codes"].view.data_ptr() and codes.numel() == w._plan["plan"].res_total + 32
        w.encode_resolved(codes)

    under_every_poison(r, call, "two-stage")


# ------------------------------------------------------------------ K2p

@pytest.mark.parametrize("layout", REC + OUT + ["all"])
@pytest.mark.parametrize("form", ["default", "seg_len3", "wave2"])
def test_k2p(avr, hooks, form, layout):
    """avr_range_encode_chunked_device as shipped, in segments of three chunks, and with pass 1 by a lane.  out_off also places the
    digit workspace's sums (S + out_off) and sizes it (out_total): that check comes with the out_off layouts."""
    if form != "default":
        hooks(**({"k2p_seg_len": 3} if form == "seg_len3" else {"k2p_wave": 2}))
    r = rehome(avr, avr.KIND_RANGE, batch_range(), axes_of(layout, ["rec-F", "out-F"]), K_RANGE)
    p = r.w._chunk_plan()
    assert p["out_total"] == int(r.off[-1]) and p["ws_k2_bytes"] >= 4 * p["out_total"]
    under_every_poison(r, r.w.encode_chunked, f"K2p {form}")


# ------------------------------------------------------------------ the estimator resolver

@pytest.mark.parametrize("layout", REC)
def test_estimator_resolver(avr, layout):
    """avr_range_resolve_device through from_device_keys: key records read from, and K2 records written to, far rec_off."""
    import torch
    import range_keys as rk
    rng = np.random.default_rng(4300)
    slices = [rk.random_keys(rng, n, "skew") for n in (0, 1, 1023, 1024, 1025, 4097, 20000, 7, 3000)]
    gf = [0, 3, 3, 7, 9]
    want, want_tabs = rk.resolve(slices, gf)
    kw = avr.DeviceWorkload.from_host_keys(slices, gf, gap=2)
    near = int(kw.rec_off[-1])
    r = Rehome(avr, kw, 6)
    r.axis(layout)
    r.materialize(refuse)
    base = r.moved["rec_off"][1]
    assert kw.key_flat.numel() >= base + near and kw.rec_flat.numel() == kw.key_flat.numel()
    kw.rec_flat.view(torch.uint8).fill_(far_offsets.RECORD_POISON)
    kw.status.zero_()
    kw.resolve_keys()
    torch.cuda.synchronize()
    rec_off, n_bins = kw.rec_off.cpu().numpy(), kw.n_bins.cpu().numpy()
    fill = far_offsets.RECORD_POISON * 0x0101
    assert not kw.status.any()
    for i in range(kw.n_slices):
        o, nb = int(rec_off[i]), int(n_bins[i])
        pad = (o + nb + 7) // 8 * 8
        got = kw.rec_flat[o:int(rec_off[i + 1])].cpu().numpy().view(np.uint16)
        assert np.array_equal(got[:nb], want[i]) and not got[nb:pad - o].any(), f"slice {i}, {r.moved}"
        assert (got[pad - o:] == fill).all(), f"the gap behind slice {i} was written, {r.moved}"
    assert int(far_offsets.count_not(kw.rec_flat, fill, 0, int(rec_off[0]))) == 0, f"records written in front of the first slice, {r.moved}"
    est = kw.est_out.cpu().numpy().reshape(-1, rk.N_KEYS, 2)
    assert all(np.array_equal(est[g], want_tabs[g]) for g in range(kw.n_groups))


# ------------------------------------------------------------------ census and remap

def test_census_and_remap_past_4g_records(avr):
    """avr_context_census_device and avr_context_remap_device over 2^32 + 4096 records: no-ops, but for a handful of contexts that
    occur in the first 4096 records only and a handful in the last 4096 only.  The bitmap holds exactly their union; after a remap by
    a random permutation the first and the last 8192 records are numpy's, and the middle is still all no-ops."""
    import torch
    L = avr.lib()
    n, edge = B32 + 4096, 8192
    need = 2 * n + far_offsets.BLOCK
    torch.cuda.empty_cache()
    free = torch.cuda.mem_get_info()[0]
    if free < need + (2 << 30):
        refuse(need, free)
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(4400)
    recs = torch.empty(n, dtype=torch.int16, device=dev)
    recs.fill_(avr.NOP_CABAC)
    ctx = rng.permutation(1024)
    first, last = ctx[:7], ctx[7:12]
    head = np.full(edge, avr.NOP_CABAC, np.uint16)
    tail = head.copy()
    at = rng.permutation(4096)[:600]
    head[at] = (rng.choice(first, at.size) << 1 | rng.integers(0, 2, at.size)).astype(np.uint16)
    head[at[:7]] = (first << 1).astype(np.uint16)            # every one of them at least once
    tail[4096 + at] = (rng.choice(last, at.size) << 1 | rng.integers(0, 2, at.size)).astype(np.uint16)
    tail[4096 + at[:5]] = (last << 1 | 1).astype(np.uint16)
    recs[:edge] = torch.from_numpy(head.view(np.int16)).to(dev)
    recs[n - edge:] = torch.from_numpy(tail.view(np.int16)).to(dev)
    bitmap = torch.zeros(32, dtype=torch.int32, device=dev)
    sp = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert L.avr_context_census_device(0, sp, recs.data_ptr(), n, bitmap.data_ptr()) == 0
    torch.cuda.synchronize()
    bits = np.unpackbits(bitmap.cpu().numpy().view(np.uint8), bitorder="little")[:1024]
    assert sorted(np.flatnonzero(bits).tolist()) == sorted(first.tolist() + last.tolist())
    table = rng.permutation(1024).astype(np.uint16)
    d_table = torch.from_numpy(table.view(np.int16)).to(dev)
    assert L.avr_context_remap_device(0, sp, recs.data_ptr(), n, d_table.data_ptr()) == 0
    torch.cuda.synchronize()

    def remapped(a):
        sel = a >> 1
        return np.where(sel < 1024, (table[np.minimum(sel, 1023)] << 1) | (a & 1), a).astype(np.uint16)

    assert np.array_equal(recs[:edge].cpu().numpy().view(np.uint16), remapped(head)), "the first 8192 records"
    assert np.array_equal(recs[n - edge:].cpu().numpy().view(np.uint16), remapped(tail)), "the last 8192 records"
    assert int(far_offsets.count_not(recs, avr.NOP_CABAC, edge, n - edge)) == 0, "the middle is no longer all no-ops"
