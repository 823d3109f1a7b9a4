"""GPU: malformed records on every coder path, against the one rule of tests/bad_records.py.

Which path codes a batch depends on its shape (the batch API takes the intra-slice kernels, which run no packer, for few long
slices), so a slice's status must not depend on it.  Every batch here mixes slices spoiled at the kernels' boundaries (record 0,
the 8-record group, K2p's ring batch, the chunk, the sort block, a K2p segment, the slice's end) with clean neighbours, and every
slice's status, bytes and length -- and a clean slice's final states -- must be what bad_records.expected() says.  The intra-slice
calls get a zeroed status, so that what is tested is their own validation and not the packer's verdict, and an out_len no path
leaves as it is: a slice comes back with no bytes only if the path wrote a length of 0."""
import time

import numpy as np
import pytest

import bad_records as br
import carry_streams
import oracle_lib
from test_gpu_carry import SENTINEL, assert_untouched
from test_gpu_parity import to_records8

pytestmark = pytest.mark.gpu

N_CTX = 100                      # <= 126: the clean slices can be one-byte records as well
POISON_LEN = 0x7fffffff


@pytest.fixture(scope="module", autouse=True)
def report_time(request):
    t0 = time.time()
    yield
    with request.config.pluginmanager.getplugin("capturemanager").global_and_fixture_disabled():
        print(f"\ntests/test_gpu_bad_records.py: {time.time() - t0:.1f} s")


@pytest.fixture(scope="module")
def k1():
    """Two-byte K1 slices: every bad value at the boundaries, and a slice without an LPS (K1p declines it: the serial kernel codes it)
    with a no-op record inside, beside the same slice clean."""
    rng = np.random.default_rng(7001)
    make = lambda n: oracle_lib.random_cabac_stream(rng, n - 1, N_CTX)[0]          # n records, the last put_terminate(1)
    spoiled = br.spoiled_set(rng, br.KIND_CABAC, make, N_CTX)
    slices = []
    for k, (r, what) in enumerate(spoiled):
        c, s = oracle_lib.random_cabac_stream(rng, int(rng.integers(0, 9000)), N_CTX, terminate=bool(k % 2))
        slices.append((c, s, "clean"))
        slices.append((r, rng.integers(0, 126, N_CTX).astype(np.uint8), what))
    no_lps, s = carry_streams.carry_chain_cabac(np.random.default_rng(999), 5, 3000, "carry", n_ctx=N_CTX, p_bypass=1.0,
                                                init_states=np.array([124, 125] * (N_CTX // 2), np.uint8))
    slices.append((no_lps, s, "clean, no LPS"))
    slices.append((br.spoil(no_lps, len(no_lps) // 2, br.SEL_NOP << 1), s, "no LPS, no-op mid-slice"))
    return slices


@pytest.fixture(scope="module")
def k1_8():
    """One-byte K1 slices (AVR_KIND_CABAC8), spoiled the same way."""
    rng = np.random.default_rng(7002)
    make = lambda n: to_records8(oracle_lib.random_cabac_stream(rng, n - 1, N_CTX)[0])
    slices = []
    for k, (r, what) in enumerate(br.spoiled_set(rng, br.KIND_CABAC8, make, N_CTX)):
        c, s = oracle_lib.random_cabac_stream(rng, int(rng.integers(0, 9000)), N_CTX, terminate=bool(k % 2))
        slices.append((to_records8(c), s, "clean"))
        slices.append((r, rng.integers(0, 126, N_CTX).astype(np.uint8), what))
    return slices


def rec(b, pos, neg):
    return b | (pos << 1) | (neg << 8)


@pytest.fixture(scope="module")
def k2():
    """K2 slices: every bad value at the boundaries (segments of 3 chunks), and the hand-over cases -- a record with neg 0 early
    (bin 0: the new range is range mod pos, which the double-precision walk hands to the integer form) alone and with a bad record in
    a later segment, a bin of probability zero alone and with a bad record behind it."""
    rng = np.random.default_rng(7003)
    make = lambda n: oracle_lib.random_range_stream(rng, n)
    slices = []
    for k, (r, what) in enumerate(br.spoiled_set(rng, br.KIND_RANGE, make, 0)):
        slices.append((oracle_lib.random_range_stream(rng, int(rng.integers(0, 9000)), adaptive=bool(k % 2)), None, "clean"))
        slices.append((r, None, what))
    collapse = br.spoil(oracle_lib.random_range_stream(rng, 9000), 100, rec(0, 77, 0))
    zero = br.spoil(oracle_lib.random_range_stream(rng, 6000), 200, rec(1, 0, 9))
    slices += [(collapse, None, "collapse"), (br.spoil(collapse, 5000, 0x0000), None, "collapse, then total 0"),
               (br.spoil(collapse, 7000, 0x8000 | rec(1, 5, 5)), None, "collapse, then bit 15"),
               (zero, None, "zero probability"), (br.spoil(zero, 4500, 0x0001), None, "zero probability, then total 0")]
    assert br.expected(br.KIND_RANGE, collapse)[0] == br.SLICE_OK and br.expected(br.KIND_RANGE, zero)[0] == br.SLICE_ZERO_PROB
    return slices


def wants_of(kind, slices):
    return [br.expected(kind, r, s) for r, s, _ in slices]


def check(kind, slices, got, status, states=None, what="", skip=()):
    for i, ((st, data, fs), (r, _, why)) in enumerate(zip(wants_of(kind, slices), slices)):
        if i in skip:
            continue
        where = f"{what}: slice {i} ({why}, n={len(r)})"
        assert status[i] == st, f"{where}: status {status[i]}, want {st}"
        if data is not None:
            assert got[i] == data, f"{where}: {len(got[i])} bytes, want {len(data)}"
        if states is not None and fs is not None:
            assert states[i][:len(fs)] == fs, f"{where}: final states"


def workload(avr, kind, slices, **kw):
    return avr.DeviceWorkload.from_host(kind, [r for r, _, _ in slices], None if kind == br.KIND_RANGE else [s for _, s, _ in slices],
                                        0, **kw)


def fresh(w, zero_status=True):
    """Outputs no path leaves as they are; the status zeroed (the intra-slice paths' own validation) or left as the packer set it."""
    w.out.fill_(SENTINEL)
    w.out_len.fill_(POISON_LEN)
    if w.final_states is not None:
        w.final_states.zero_()
    if zero_status:
        w.status.zero_()


def results(w):
    got, status = w.results()
    if w.final_states is None:
        return got, status, None
    ns = w.n_states
    fs = w.final_states.cpu().numpy()
    return got, status, [fs[i * ns:(i + 1) * ns].tobytes() for i in range(w.n_slices)]


# ------------------------------------------------------------------ K1, two-byte records

def test_k1_packer_then_tiles(avr, k1):
    import torch
    w = workload(avr, br.KIND_CABAC, k1)
    fresh(w, zero_status=False)                                  # the packer's verdict is what this path has
    w.encode(); torch.cuda.synchronize()
    w.settle()
    check(br.KIND_CABAC, k1, *results(w), what="pack + tiles")


@pytest.mark.parametrize("mode", ["parts1", "parts2", "small-guess", "census", "retry"])
def test_k1p_chunked(avr, k1, hooks, mode):
    """encode_chunked() in one and in two parts, asked and then sized by the hint; a guess too small, which settle() runs again; a
    census that sees next to nothing (every slice with a context bin takes the second pass: the spoiled ones have a missed context
    and a bad record at once); phase D handing every slice over to the serial kernel, which must not code a bad one."""
    import torch
    if mode == "census":
        hooks(census_stride=4099)
    elif mode == "retry":
        hooks(k1p_force_retry_every=1)
    w = workload(avr, br.KIND_CABAC, k1)
    if mode == "parts2":
        assert w.set_parts(2) == 2
    for run in ("asked", "hinted"):
        fresh(w)
        if mode == "small-guess" and run == "hinted":
            w.rows_hint = 4
        w.encode_chunked(); torch.cuda.synchronize()
        info = w.settle()
        if mode == "small-guess" and run == "hinted":
            assert info["redone"]
        check(br.KIND_CABAC, k1, *results(w), what=f"{mode}, {run}")


def test_k1p_resolve_statuses(avr, k1):
    """Stage 1 alone (avr_cabac_resolve_device) shares k_k1p_local: the same statuses, and a clean slice's final states."""
    w = workload(avr, br.KIND_CABAC, k1)
    fresh(w)
    w.resolve()
    _, status, states = results(w)
    for i, ((st, _, fs), (r, _, why)) in enumerate(zip(wants_of(br.KIND_CABAC, k1), k1)):
        assert status[i] == st, f"resolve: slice {i} ({why}): status {status[i]}, want {st}"
        if fs is not None:
            assert states[i][:len(fs)] == fs, f"resolve: final states of slice {i}"


# ------------------------------------------------------------------ K1, one-byte records (the regression net)

@pytest.mark.parametrize("path", ["pack8+tiles", "chunked8"])
def test_k1_one_byte(avr, k1_8, path):
    import torch
    w = workload(avr, br.KIND_CABAC8, k1_8, pad_bytes=np.random.default_rng(5).integers(0, 256, 4099).astype(np.uint8))
    if path == "pack8+tiles":
        fresh(w, zero_status=False)
        w.encode()
    else:
        fresh(w)
        w.encode_chunked()
    torch.cuda.synchronize()
    check(br.KIND_CABAC8, k1_8, *results(w), what=path)


# ------------------------------------------------------------------ K2

def test_k2_packer_then_tiles(avr, k2):
    w = workload(avr, br.KIND_RANGE, k2)
    fresh(w, zero_status=False)
    w.encode()
    check(br.KIND_RANGE, k2, *results(w), what="pack + tiles")


@pytest.mark.parametrize("wave", [0, 2, 3])
@pytest.mark.parametrize("seg_len", [0, 1, 3])
def test_k2p_chunked(avr, k2, hooks, seg_len, wave):
    """K2p with pass 1 by a wave / a lane / both per slice (k2p_wave 0 = by the batch's shape: a wave), in segments of 1 and 3 chunks."""
    hooks(k2p_seg_len=seg_len, k2p_wave=wave)
    w = workload(avr, br.KIND_RANGE, k2)
    fresh(w)
    w.encode_chunked()
    check(br.KIND_RANGE, k2, *results(w), what=f"seg_len {seg_len} wave {wave}")


# ------------------------------------------------------------------ output regions

def regions(w, cuts=None):
    """Every region at 8 mod 16, a new w.out full of the sentinel; cuts: {slice: capacity}."""
    import torch
    cap = (w.out_off[1:] - w.out_off[:-1]).cpu().numpy().astype(np.int64)
    cap = (cap + 24 + 15) // 16 * 16
    for i, c in (cuts or {}).items():
        cap[i] = c
    off = np.zeros(cap.size + 1, np.int64)
    off[0] = 8
    off[1:] = 8 + np.cumsum(cap)
    w.out_off = torch.from_numpy(off).to(w.out_off.device)
    w.out = torch.full((int(off[-1]) + 64,), SENTINEL, dtype=torch.uint8, device=w.out_off.device)
    assert all(int(o) % 16 == 8 for o in off[:-1])
    return off


@pytest.mark.parametrize("path", ["k1", "k1p"])
def test_k1_regions(avr, k1, path):
    """A bad slice has length 0 and writes nothing outside its region; its neighbours are exact and stay inside theirs."""
    import torch
    w = workload(avr, br.KIND_CABAC, k1)
    fresh(w, zero_status=path == "k1p")
    off = regions(w)
    (w.encode if path == "k1" else w.encode_chunked)(); torch.cuda.synchronize()
    w.settle()
    check(br.KIND_CABAC, k1, *results(w), what=f"{path} at 8 mod 16")
    assert_untouched(w, off, overflowed=[i for i, (st, _, _) in enumerate(wants_of(br.KIND_CABAC, k1)) if st == br.SLICE_BAD_RECORD])


@pytest.mark.parametrize("seg_len", [0, 1, 3])
def test_k2p_regions_cut_short(avr, k2, hooks, seg_len):
    """Regions at 8 mod 16, and three slices cut to 64 bytes: the hand-over slice with a bad record in a later segment ends BAD, not
    OVERFLOW, as does a slice whose bad record lies segments behind the chunk that found the region too small; the hand-over slice
    without one ends OVERFLOW.  Nothing is written outside the slices' bytes."""
    import torch
    hooks(k2p_seg_len=seg_len)
    rng = np.random.default_rng(7004)
    late = br.spoil(oracle_lib.random_range_stream(rng, 12000), 11000, 0x0000)
    by = {s[2]: s for s in k2}
    special = [by["collapse"], by["collapse, then total 0"], by["zero probability, then total 0"], (late, None, "total 0 late")]
    clean = [s for s in k2 if s[2] == "clean"][:8]
    slices = [x for pair in zip(clean[:4], special) for x in pair] + clean[4:]
    cut = {i: 64 for i, s in enumerate(slices) if s[2] != "clean"}
    w = workload(avr, br.KIND_RANGE, slices)
    fresh(w)
    off = regions(w, cut)
    w.encode_chunked(); torch.cuda.synchronize()
    got, status, _ = results(w)
    overflowed = [i for i, s in enumerate(slices) if s[2] == "collapse"]
    check(br.KIND_RANGE, slices, got, status, what=f"seg_len {seg_len}", skip=overflowed)
    assert [status[i] for i in overflowed] == [br.SLICE_OVERFLOW]
    assert_untouched(w, off, overflowed=overflowed)


# ------------------------------------------------------------------ batch API

def _batch(avr, kind, slices):
    total = sum(len(r) for r, _, _ in slices) + 64
    b = avr.Batch(0, len(slices), total)
    add = {br.KIND_CABAC: lambda r, s: b.add_slice_cabac(r, s), br.KIND_CABAC8: lambda r, s: b.add_slice_cabac8(r, s),
           br.KIND_RANGE: lambda r, s: b.add_slice_range(r)}[kind]
    for r, s, _ in slices:
        add(r, s)
    return b


def _batch_results(b, kind, n):
    got, status, states = [], [], []
    for i in range(n):
        data, st = b.get(i)
        got.append(data)
        status.append(st)
        states.append(b.get_states(i) if kind != br.KIND_RANGE else None)
    return got, status, (states if kind != br.KIND_RANGE else None)


@pytest.mark.parametrize("path", [1, 2], ids=["serial", "chunked"])
@pytest.mark.parametrize("kind", [br.KIND_CABAC, br.KIND_CABAC8, br.KIND_RANGE], ids=["cabac", "cabac8", "range"])
def test_batch(avr, hooks, k1, k1_8, k2, kind, path):
    hooks(k1_path=path)
    slices = {br.KIND_CABAC: k1, br.KIND_CABAC8: k1_8, br.KIND_RANGE: k2}[kind]
    with _batch(avr, kind, slices) as b:
        b.run()
        check(kind, slices, *_batch_results(b, kind, len(slices)), what=f"batch path {path}")


@pytest.mark.parametrize("path", [1, 2], ids=["serial", "chunked"])
@pytest.mark.parametrize("kind", [br.KIND_CABAC, br.KIND_CABAC8, br.KIND_RANGE], ids=["cabac", "cabac8", "range"])
def test_batch_reused_after_a_bad_slice(avr, hooks, k1, k1_8, k2, kind, path):
    """Run 1 has slice 3 spoiled; after a reset, run 2 has it clean, and it comes back OK with the oracle's bytes: no stale status."""
    hooks(k1_path=path)
    source = {br.KIND_CABAC: k1, br.KIND_CABAC8: k1_8, br.KIND_RANGE: k2}[kind]
    clean = [s for s in source if s[2] == "clean"][:6]
    bad = next(s for s in source if s[2] != "clean" and br.expected(kind, s[0], s[1])[0] == br.SLICE_BAD_RECORD)
    first = clean[:3] + [bad] + clean[3:]
    with _batch(avr, kind, first) as b:
        b.run()
        check(kind, first, *_batch_results(b, kind, len(first)), what="run 1")
        b.reset()
        add = {br.KIND_CABAC: b.add_slice_cabac, br.KIND_CABAC8: b.add_slice_cabac8,
               br.KIND_RANGE: lambda r, s: b.add_slice_range(r)}[kind]
        for r, s, _ in clean:
            add(r, s)
        b.run()
        check(kind, clean, *_batch_results(b, kind, len(clean)), what="run 2")


def test_multi_batch(avr, k1, k2):
    for kind, slices in ((br.KIND_CABAC, k1), (br.KIND_RANGE, k2)):
        with avr.MultiBatch([0, 0], len(slices), sum(len(r) for r, _, _ in slices) + 64) as m:
            for r, s, _ in slices:
                (m.add_slice_cabac(r, s) if kind == br.KIND_CABAC else m.add_slice_range(r))
            m.run()
            got, status = zip(*[m.get(i) for i in range(len(slices))])
            check(kind, slices, list(got), list(status), what=f"multi-batch kind {kind}")
