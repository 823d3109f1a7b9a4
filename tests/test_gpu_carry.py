"""GPU: every coder path on long carry chains (tests/carry_streams.py) and on tight, misaligned output regions.

Each path writes a digit out as soon as it exists and adds a later carry back into bytes already written -- the serial
kernels through their staging words and then byte by byte through HBM, K1p's phase D through 33-digit segments chained
by a lookahead across waves and tiles, K2p's finishing pass through 64-position segments in rounds.  Random records
never make a carry travel more than a digit or two; the chains below make one travel up to ~40 000 bytes.  Chain
slices share the batch (and waves) with random slices that carry nothing, and every slice's bytes, final context states
and status must be the oracle's."""
import time

import numpy as np
import pytest

import carry_streams
import oracle_lib
from test_gpu_parity import to_records8

pytestmark = pytest.mark.gpu

N_CTX = 100                      # <= 126: the same slices go through the one-byte records of AVR_KIND_CABAC8
SENTINEL = 0xA5


@pytest.fixture(scope="module", autouse=True)
def report_time(request):
    t0 = time.time()
    yield
    with request.config.pluginmanager.getplugin("capturemanager").global_and_fixture_disabled():
        print(f"\ntests/test_gpu_carry.py: {time.time() - t0:.1f} s")


def _interleave(chains, randoms):
    out = []
    for i in range(max(len(chains), len(randoms))):
        out += randoms[i:i + 1] + chains[i:i + 1]
    return out


@pytest.fixture(scope="module")
def cabac(oracle):
    """(slices, wants, chain_ix): chains past a segment (70 digits), a tile (9 000), two tiles (20 000), ending in each way,
    one with no LPS (declined by K1p), and random neighbours."""
    rng = np.random.default_rng(4242)
    chains = []
    for k, (lead, n_chain, end) in enumerate([(3, 70, "carry"), (10, 2200, "none"), (0, 9000, "carry"), (20, 8448, "cut"),
                                              (5, 20000, "carry"), (40, 300, "cut"), (1, 4300, "none")]):
        chains.append(carry_streams.carry_chain_cabac(np.random.default_rng(900 + k), lead, n_chain, end, n_ctx=N_CTX))
    chains.append(carry_streams.carry_chain_cabac(np.random.default_rng(999), 5, 3000, "carry", n_ctx=N_CTX, p_bypass=1.0,
                                                  init_states=np.array([124, 125] * (N_CTX // 2), np.uint8)))
    randoms = [oracle_lib.random_cabac_stream(rng, int(n), N_CTX, terminate=bool(i % 3))
               for i, n in enumerate(rng.integers(0, 20000, 12))]
    slices = _interleave(chains, randoms)
    chain_ix = [i for i, s in enumerate(slices) if any(s is c for c in chains)]
    wants = [oracle.cabac_encode(r, s) for r, s in slices]
    for i in chain_ix:
        assert wants[i][2] == 0
    return slices, wants, chain_ix


@pytest.fixture(scope="module")
def ranges(oracle):
    rng = np.random.default_rng(4343)
    chains = [carry_streams.carry_chain_range(np.random.default_rng(950 + k), lead, n_chain, end)
              for k, (lead, n_chain, end) in enumerate([(3, 48, "carry"), (20, 72, "none"), (100, 4104, "carry"),
                                                       (7, 4200, "cut"), (1, 9000, "carry"), (60, 30000, "carry"),
                                                       (9, 600, "none")])]
    randoms = [oracle_lib.random_range_stream(rng, int(n), adaptive=bool(i % 2)) for i, n in enumerate(rng.integers(0, 20000, 8))]
    slices = _interleave(chains, randoms)
    chain_ix = [i for i, s in enumerate(slices) if any(s is c for c in chains)]
    return slices, [oracle.range_encode(r) for r in slices], chain_ix


def cabac_workload(avr, slices):
    return avr.DeviceWorkload.from_host(avr.KIND_CABAC, [r for r, _ in slices], [s for _, s in slices], 0)


def check_cabac(w, wants, what, states=True, skip=()):
    got, status = w.results()
    fs = w.final_states.cpu().numpy().reshape(len(wants), -1) if states else None
    for i, (data, final, st) in enumerate(wants):
        if i in skip:
            continue
        assert status[i] == st and got[i] == data, f"{what}: slice {i}"
        if states:
            assert fs[i][:len(final)].tobytes() == final, f"{what}: final states of slice {i}"


def clear(w):
    w.out.zero_(); w.out_len.zero_(); w.final_states.zero_()


# ------------------------------------------------------------------ serial K1

def test_serial_k1_tiles_and_slice_major(avr, cabac):
    import torch
    slices, wants, _ = cabac
    w = cabac_workload(avr, slices)
    w.encode(); torch.cuda.synchronize()
    w.settle()
    check_cabac(w, wants, "tiles, asked")
    clear(w)
    w.encode(); torch.cuda.synchronize()                     # sized by the hint the first run left
    assert not w.settle()["redone"]
    check_cabac(w, wants, "tiles, hinted")
    clear(w)
    w.encode_slice_major()
    check_cabac(w, wants, "slice major")


# ------------------------------------------------------------------ K1p

@pytest.mark.parametrize("mode", ["one-call", "parts2", "parts3", "census", "retry"])
def test_k1p_paths(avr, cabac, hooks, mode):
    """encode_chunked as one call (asked, then sized by the hint), in two and three parts, with a census that sees next to
    nothing (every slice takes the second pass), and with phase D handing every slice to k_cabac_encode_codes."""
    import torch
    if mode == "census":
        hooks(census_stride=4099)
    elif mode == "retry":
        hooks(k1p_force_retry_every=1)
    slices, wants, _ = cabac
    w = cabac_workload(avr, slices)
    if mode.startswith("parts"):
        assert w.set_parts(int(mode[-1])) >= 2
    for run in ("asked", "hinted"):
        w.encode_chunked(); torch.cuda.synchronize()
        w.settle()
        check_cabac(w, wants, f"{mode}, {run}")
        clear(w)


def test_k1p_resolved_and_codes_serial(avr, cabac):
    slices, wants, _ = cabac
    w = cabac_workload(avr, slices)
    codes = w.resolve()
    w.encode_resolved(codes)
    check_cabac(w, wants, "resolve + encode_resolved")
    w.out.zero_(); w.out_len.zero_()
    w.encode_codes_serial(codes)
    check_cabac(w, wants, "encode_codes_serial")


def test_k1p_phase_d_codes_the_chains_itself(avr, cabac, hooks):
    """Phase D checks its own carry lookahead and hands a slice it got wrong to the serial kernel, whose bytes are right: a broken
    propagate side (carries across all-ones segments, waves, tiles) would cost time, not bytes.  With the hand-over left out (test
    hook k1p_keep_retry, on the resolved-codes entry, which never declines a slice) every slice -- every chain among them -- is
    phase D's own work, and exact."""
    hooks(k1p_keep_retry=1)
    slices, wants, chain_ix = cabac
    w = cabac_workload(avr, slices)
    codes = w.resolve()
    w.encode_resolved(codes)
    got, status = w.results()
    assert [status[i] for i in chain_ix] == [0] * len(chain_ix)
    check_cabac(w, wants, "phase D alone")


# ------------------------------------------------------------------ batch API

@pytest.mark.parametrize("path", ["serial", "chunked"])
def test_batch_api_cabac_and_cabac8(avr, cabac, hooks, path):
    hooks(k1_path={"serial": 1, "chunked": 2}[path])
    slices, wants, _ = cabac
    total = sum(len(r) for r, _ in slices) + 64
    with avr.Batch(0, len(slices), total) as b:
        for r, s in slices:
            b.add_slice_cabac(r, s)
        b.run()
        for i, want in enumerate(wants):
            data, status = b.get(i)
            assert (data, b.get_states(i), status) == want, f"{path}: slice {i}"
    with avr.Batch(0, len(slices), total) as b:
        for r, s in slices:
            b.add_slice_cabac8(to_records8(r), s)
        b.run()
        for i, want in enumerate(wants):
            data, status = b.get(i)
            assert (data, b.get_states(i), status) == want, f"{path}, one-byte records: slice {i}"


def test_batch_api_range(avr, ranges):
    slices, wants, _ = ranges
    with avr.Batch(0, len(slices), sum(len(r) for r in slices) + 64) as b:
        for r in slices:
            b.add_slice_range(r)
        b.run()
        for i, want in enumerate(wants):
            assert b.get(i) == want, f"slice {i}"


# ------------------------------------------------------------------ K2, K2p

def check_range(w, wants, what, skip=()):
    got, status = w.results()
    for i, (data, st) in enumerate(wants):
        if i not in skip:
            assert status[i] == st and got[i] == data, f"{what}: slice {i}"


def test_k2_tiles(avr, ranges):
    slices, wants, _ = ranges
    w = avr.DeviceWorkload.from_host(avr.KIND_RANGE, slices, None, 0)
    w.encode()
    check_range(w, wants, "tiles")


@pytest.mark.parametrize("pass1", ["wave", "lane", "both"])
@pytest.mark.parametrize("seg_len", [0, 1, 3])
def test_k2p(avr, ranges, hooks, seg_len, pass1):
    """The hooks of test_range_chunked_random_and_extremes: pass 1 by a wave / a lane / both per slice, the passes in
    segments of 1 and 3 chunks."""
    lane = {"k2p_wave": 2} if pass1 == "lane" else {"k2p_wave": 3} if pass1 == "both" else {}
    hooks(k2p_seg_len=seg_len, **lane)
    slices, wants, _ = ranges
    w = avr.DeviceWorkload.from_host(avr.KIND_RANGE, slices, None, 0)
    w.encode_chunked()
    check_range(w, wants, f"seg_len {seg_len} pass1 {pass1}")


# ------------------------------------------------------------------ output regions

def regions_at_8_mod_16(w, cut=None):
    """Rebuild w.out_off so that every region starts at 8 mod 16 with some slack behind it, and fill a new w.out with the
    sentinel.  cut: (slice, capacity) -- that slice's region is made that small instead."""
    import torch
    cap = (w.out_off[1:] - w.out_off[:-1]).cpu().numpy().astype(np.int64)
    cap = (cap + 24 + 15) // 16 * 16                          # a multiple of 16: every start stays 8 mod 16
    if cut is not None:
        cap[cut[0]] = cut[1]
    off = np.zeros(cap.size + 1, np.int64)
    off[0] = 8
    off[1:] = 8 + np.cumsum(cap)
    w.out_off = torch.from_numpy(off).to(w.out_off.device)
    w.out = torch.full((int(off[-1]) + 64,), SENTINEL, dtype=torch.uint8, device=w.out_off.device)
    assert w.out.data_ptr() % 16 == 0 and all(int(o) % 16 == 8 for o in off[:-1])
    return off


def assert_untouched(w, off, overflowed=()):
    """Every byte outside the slices' [off_i, off_i + len_i) -- outside the whole region for an overflowed slice -- holds the
    sentinel."""
    out = w.out.cpu().numpy()
    lens = w.out_len.cpu().numpy().astype(np.int64)
    mask = np.ones(out.size, bool)
    for i in range(lens.size):
        end = off[i + 1] if i in overflowed else off[i] + lens[i]
        assert off[i] + lens[i] <= off[i + 1] or i in overflowed, f"slice {i}: length past its region"
        mask[off[i]:end] = False
    bad = np.flatnonzero(mask & (out != SENTINEL))
    assert bad.size == 0, f"{bad.size} bytes written outside the slices' bytes, first at {bad[:8].tolist()} (regions {off[:4].tolist()}...)"


def _cut_region(wants, chain_ix):
    """(slice, capacity) cutting the longest chain's region inside its run."""
    i = max(chain_ix, key=lambda k: len(wants[k][0]))
    start, length = carry_streams.longest_run(wants[i][0], wants[i][0][len(wants[i][0]) // 2])
    assert length > 1000
    return i, (start + length // 2) // 16 * 16


@pytest.mark.parametrize("path", ["k1", "k1p", "k1p-parts"])
@pytest.mark.parametrize("tight", [False, True])
def test_k1_output_regions(avr, cabac, path, tight):
    """Regions that start at 8 mod 16 (the shipped serial kernel stores 16 bytes at a time at base + n - 16): nothing is written
    outside a slice's bytes, and every slice is exact.  tight: one chain slice's region ends inside its run -- it comes back
    AVR_SLICE_OVERFLOW, writes nothing past its region, and its neighbours are exact."""
    import torch
    slices, wants, chain_ix = cabac
    w = cabac_workload(avr, slices)
    cut = _cut_region(wants, chain_ix) if tight else None
    off = regions_at_8_mod_16(w, cut)
    if path == "k1":
        w.encode()
    else:
        if path == "k1p-parts":
            assert w.set_parts(2) == 2
        w.encode_chunked(); torch.cuda.synchronize()
        w.settle()
    torch.cuda.synchronize()
    skip = (cut[0],) if tight else ()
    check_cabac(w, wants, f"{path} at 8 mod 16", skip=skip)
    if tight:
        assert w.results()[1][cut[0]] == avr.SLICE_OVERFLOW
    assert_untouched(w, off, overflowed=skip)


@pytest.mark.parametrize("path", ["k2", "k2p"])
@pytest.mark.parametrize("tight", [False, True])
def test_k2_output_regions(avr, ranges, path, tight):
    import torch
    slices, wants, chain_ix = ranges
    w = avr.DeviceWorkload.from_host(avr.KIND_RANGE, slices, None, 0)
    cut = _cut_region(wants, chain_ix) if tight else None
    off = regions_at_8_mod_16(w, cut)
    (w.encode if path == "k2" else w.encode_chunked)()
    torch.cuda.synchronize()
    skip = (cut[0],) if tight else ()
    check_range(w, wants, f"{path} at 8 mod 16", skip=skip)
    if tight:
        assert w.results()[1][cut[0]] == avr.SLICE_OVERFLOW
    assert_untouched(w, off, overflowed=skip)
