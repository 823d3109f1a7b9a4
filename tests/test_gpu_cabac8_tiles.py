"""One-byte K1 records (AVR_KIND_CABAC8) in ONE-BYTE tiles: avr_pack_tiles8_narrow_device (validate + transpose, no widening) and the
one-lane-per-slice coder on them, avr_cabac8_encode_tiles_device -- and the one-byte batch of many short slices, which now takes
that route.  Every slice against bad_records.expected() (the oracle on widened records, and the rule for malformed ones); where
noted also against the two-byte route on the same records (avr_pack_tiles8_device + avr_cabac_encode_tiles_device).  A byte has no
no-op value, so every slice's padding bytes hold garbage that would change the bytes if it were coded."""
import ctypes
import time

import numpy as np
import pytest

import bad_records as br
import carry_streams
import oracle_lib

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
EDGES16 = (0, 15, 16, 31, 32, 47, 48)                        # the 16-record edges of the one-byte tiles (positions() stops at 8)


def to8(recs):
    """Two-byte K1 records (selectors below 126, bypass, terminate) as one-byte records."""
    recs = np.asarray(recs, dtype=np.uint16)
    sel = (recs >> 1).astype(np.int64)
    sel8 = np.where(sel == br.SEL_BYPASS, br.SEL8_BYPASS, np.where(sel == br.SEL_TERMINATE, br.SEL8_TERMINATE, sel))
    assert ((sel8 >= 0) & (sel8 < 128)).all()
    return ((sel8 << 1) | (recs & 1)).astype(np.uint8)


def garbage(seed):
    return np.random.default_rng(seed).integers(0, 256, 4099).astype(np.uint8)


def workload(avr, recs8, states, pad_seed, narrow=True):
    return avr.DeviceWorkload.from_host(avr.KIND_CABAC8, recs8, states, pad_bytes=garbage(pad_seed), narrow_tiles=narrow)


def results(w):
    import torch
    torch.cuda.synchronize()
    data, status = w.results()
    ns = w.n_states
    fs = w.final_states.cpu().numpy()
    return data, [fs[i * ns:(i + 1) * ns].tobytes() for i in range(w.n_slices)], status


def run(avr, recs8, states, pad_seed, narrow=True):
    w = workload(avr, recs8, states, pad_seed, narrow)
    w.encode()
    return results(w)


def check(recs8, states, n_states, got, what, rec_offs=None, skip=()):
    data, fs, status = got
    for i, (r, s) in enumerate(zip(recs8, states)):
        if i in skip:
            continue
        st, want, want_fs = br.expected(br.KIND_CABAC8, r, s, n_states, rec_offs[i] if rec_offs else 0)
        assert (status[i], data[i]) == (st, want), f"{what}: slice {i} n={len(r)}"
        if want_fs is not None:
            assert fs[i] == want_fs, f"{what}: final states of slice {i}"


def same_as_two_byte(recs8, states, n_states, narrow, two, what):
    """The narrow route against the two-byte route: bytes and statuses of every slice, final states where they are specified."""
    for i, (r, s) in enumerate(zip(recs8, states)):
        assert (narrow[0][i], narrow[2][i]) == (two[0][i], two[2][i]), f"{what}: slice {i} against the two-byte route"
        if not br.breaks_rule(br.KIND_CABAC8, r, n_states):
            assert narrow[1][i] == two[1][i], f"{what}: final states of slice {i} against the two-byte route"


def random_slices(rng, n_states):
    slices = []
    for n in (0, 1, 15, 16, 17, 31, 32, 33, 47, 48, 49):
        for term in (False, True):
            slices.append(oracle_lib.random_cabac_stream(rng, n, n_states, terminate=term))
    slices.append((np.array([br.TERM1], np.uint16), rng.integers(0, 126, n_states).astype(np.uint8)))    # terminate only
    for i, n in enumerate(np.minimum(rng.pareto(1.2, 280) * 300, 5000).astype(int)):                       # ragged, in shared tiles
        slices.append(oracle_lib.random_cabac_stream(rng, int(n), n_states, terminate=bool(i % 3)))
    return [to8(r) for r, _ in slices], [s for _, s in slices]


@pytest.mark.parametrize("n_states", [1, 60, 126])
def test_random_slices_match_oracle_and_two_byte_route(avr, n_states):
    recs8, states = random_slices(np.random.default_rng(1000 + n_states), n_states)
    assert len(recs8) >= 300
    got = run(avr, recs8, states, pad_seed=n_states)
    check(recs8, states, n_states, got, f"narrow, n_states {n_states}")
    assert not any(got[2])
    same_as_two_byte(recs8, states, n_states, got, run(avr, recs8, states, n_states + 7, narrow=False), f"n_states {n_states}")
    assert run(avr, recs8, states, pad_seed=n_states + 500) == got                # other padding, same everything


def spoiled(rng, n_states):
    """Spoiled slices at the 16-record edges (and n-2, n-1, mid-slice) with every bad value, each beside a clean slice of the same
    length -- sorted longest first, the two share a wave."""
    values = br.bad_values(br.KIND_CABAC8, n_states)
    recs8, states, what = [], [], []
    k = 0
    for n in (2, 17, 33, 50, 700, 2900):
        for at in sorted({a for a in EDGES16 + (n - 2, n - 1, n // 2) if 0 <= a < n}):
            name, v = values[k % len(values)]
            k += 1
            r, s = oracle_lib.random_cabac_stream(rng, n - 1, n_states, terminate=True)
            clean = to8(r)
            recs8 += [br.spoil(clean, at, v), clean]
            states += [s, s]
            what += [f"{name} at {at} of {n}", "clean"]
    for name, v in values:                                  # every value at every edge of one long slice
        for at in EDGES16:
            r, s = oracle_lib.random_cabac_stream(rng, 399, n_states, terminate=False)
            recs8 += [br.spoil(to8(r), at, v)]
            states += [s]
            what += [f"{name} at {at} of 399"]
    return recs8, states, what


@pytest.mark.parametrize("n_states", [60, 126])
def test_spoiled_slices_flag_their_slice_only(avr, n_states):
    import torch
    recs8, states, what = spoiled(np.random.default_rng(77 + n_states), n_states)
    assert any(br.breaks_rule(br.KIND_CABAC8, r, n_states) for r in recs8)
    w = workload(avr, recs8, states, pad_seed=5)
    # one clean slice more gets an offset that is not a multiple of 16: the packer flags it alone (it reads from the multiple below)
    bumped = what.index("clean", len(what) // 2)
    rec_offs = [0] * len(recs8)
    rec_offs[bumped] = 3
    w.rec8_off[bumped] += 3
    w.status.zero_()
    L = avr.lib()
    sp = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert L.avr_pack_tiles8_narrow_device(0, sp, n_states, w.rec8_flat.data_ptr(), w.rec8_off.data_ptr(), w.n_bins.data_ptr(),
                                           w.order.data_ptr(), w.n_slices, w.tile_off.data_ptr(), w.tiles.data_ptr(),
                                           w.status.data_ptr()) == 0
    w.encode()
    got = results(w)
    check(recs8, states, n_states, got, f"spoiled, n_states {n_states}", rec_offs)
    assert got[2][bumped] == br.SLICE_BAD_RECORD and got[0][bumped] == b""
    bad = [i for i, r in enumerate(recs8) if br.breaks_rule(br.KIND_CABAC8, r, n_states)]
    assert len(bad) >= len(EDGES16) * 2
    for i in bad:
        assert got[2][i] == br.SLICE_BAD_RECORD and got[0][i] == b"", what[i]
    w2 = workload(avr, recs8, states, pad_seed=6, narrow=False)
    w2.encode()
    two = results(w2)
    for i in range(len(recs8)):                             # the bumped slice is clean on the two-byte side (its offset is fine there)
        if i != bumped:
            assert (got[0][i], got[2][i]) == (two[0][i], two[2][i]), f"{what[i]}: slice {i} against the two-byte route"


# ------------------------------------------------------------------ carry chains, output regions

N_CTX = 100


@pytest.fixture(scope="module")
def chains(oracle):
    rng = np.random.default_rng(4242)
    slices, chain_ix = [], []
    for k, (lead, n_chain, end) in enumerate([(3, 70, "carry"), (10, 2200, "none"), (0, 9000, "carry"), (20, 8448, "cut"),
                                              (40, 300, "cut"), (1, 4300, "none")]):
        chain_ix.append(len(slices))
        slices.append(carry_streams.carry_chain_cabac(np.random.default_rng(900 + k), lead, n_chain, end, n_ctx=N_CTX))
        slices.append(oracle_lib.random_cabac_stream(rng, int(rng.integers(0, 20000)), N_CTX, terminate=bool(k % 3)))
    wants = [oracle.cabac_encode(r, s) for r, s in slices]
    return [to8(r) for r, _ in slices], [s for _, s in slices], wants, chain_ix


def regions_at_8_mod_16(w, cut=None):
    """Every output region starts at 8 mod 16 with slack behind it, in a buffer full of the sentinel.  cut: (slice, capacity)."""
    import torch
    cap = (w.out_off[1:] - w.out_off[:-1]).cpu().numpy().astype(np.int64)
    cap = (cap + 24 + 15) // 16 * 16
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
    out = w.out.cpu().numpy()
    lens = w.out_len.cpu().numpy().astype(np.int64)
    mask = np.ones(out.size, bool)
    for i in range(lens.size):
        end = off[i + 1] if i in overflowed else off[i] + lens[i]
        assert off[i] + lens[i] <= off[i + 1] or i in overflowed, f"slice {i}: length past its region"
        mask[off[i]:end] = False
    bad = np.flatnonzero(mask & (out != SENTINEL))
    assert bad.size == 0, f"{bad.size} bytes written outside the slices' bytes, first at {bad[:8].tolist()}"


@pytest.mark.parametrize("tight", [False, True])
def test_carry_chains_in_regions_at_8_mod_16(avr, chains, tight):
    recs8, states, wants, chain_ix = chains
    cut = None
    if tight:                                               # the longest chain's region ends inside its run
        i = max(chain_ix, key=lambda k: len(wants[k][0]))
        start, length = carry_streams.longest_run(wants[i][0], wants[i][0][len(wants[i][0]) // 2])
        assert length > 1000
        cut = (i, (start + length // 2) // 16 * 16)
    w = workload(avr, recs8, states, pad_seed=21)
    off = regions_at_8_mod_16(w, cut)
    w.encode()
    data, fs, status = results(w)
    for i, (want, st_, want_st) in enumerate(wants):
        if cut and i == cut[0]:
            continue
        assert (data[i], fs[i], status[i]) == (want, st_, want_st), f"slice {i}"
    if tight:
        assert status[cut[0]] == br.SLICE_OVERFLOW
    assert_untouched(w, off, overflowed=(cut[0],) if cut else ())


# ------------------------------------------------------------------ real clips

@pytest.fixture(scope="module")
def real_streams(avr, oracle):
    import os
    import test_gpu_cabac8 as t8                             # the clips' records, as that module gets them
    host = t8.host_api(avr)
    out = {}
    for name in t8.CLIPS:
        data = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name), "rb").read()
        k2, payloads, offered = t8._stream_records(host, data, 0, 0)
        recoded = [oracle.range_encode(r)[0] for r in k2]
        k1, first = t8._stream_records(host, data, 0, 1, recoded, offered)
        keep = [i for i, r in enumerate(k1) if t8.contexts_of(r) <= br.MAX_STATES8]
        assert len(keep) >= len(k1) // 2
        out[name] = ([t8.narrow(k1[i], first[i], br.MAX_STATES8) for i in keep], [payloads[i] for i in keep])
    return out


@pytest.mark.parametrize("name", ["realshort.mp4", "cockatoo.mp4"])
def test_real_clips_give_back_their_payloads(avr, real_streams, name):
    narrowed, payloads = real_streams[name]
    data, _, status = run(avr, [r for r, _ in narrowed], [s for _, s in narrowed], pad_seed=11)
    assert not any(status)
    for i, p in enumerate(payloads):
        assert avr.tail_patch(avr.drop_stop_byte(data[i]), len(p) & 1, p[-1]) == p, f"{name}: slice {i}"


# ------------------------------------------------------------------ batch API

@pytest.fixture(scope="module")
def short_slices(oracle):
    """Many short slices that name 40 contexts of the 100 they declare."""
    rng = np.random.default_rng(5150)
    slices = []
    for i, n in enumerate(rng.integers(0, 3000, 400)):
        r, _ = oracle_lib.random_cabac_stream(rng, int(n), 40, terminate=bool(i % 2))
        slices.append((to8(r), rng.integers(0, 126, 100).astype(np.uint8)))
    slices[3] = (br.spoil(slices[3][0], 0, 110 << 1), slices[3][1]) if slices[3][0].size else slices[3]   # selector 110 >= n_states
    return slices, [br.expected(br.KIND_CABAC8, r, s) for r, s in slices]


def test_batch_of_short_slices_reads_one_byte_tiles(avr, short_slices):
    slices, wants = short_slices
    total = sum(len(r) for r, _ in slices) + 64
    with avr.Batch(0, len(slices), total) as b:             # no hook: the shape picks one lane per slice
        for r, s in slices:
            b.add_slice_cabac8(r, s)
        for attempt in range(2):                            # the first run and the same batch submitted again
            b.submit()
            b.wait()
            assert b.run_info() == {"chunked": 0, "rows_guessed": 0, "contexts_seen": 100, "ran_again": 0}, attempt
            for i, (st, data, fs) in enumerate(wants):
                got, status = b.get(i)
                assert (status, got) == (st, data), f"run {attempt}: slice {i}"
                if fs is not None:
                    assert b.get_states(i) == fs, f"run {attempt}: final states of slice {i}"


def test_multibatch_of_short_slices(avr, short_slices):
    slices, wants = short_slices
    with avr.MultiBatch([0, 0], len(slices), sum(len(r) for r, _ in slices) + 64) as m:
        for r, s in slices:
            m.add_slice_cabac8(r, s)
        m.run()
        for i, (st, data, _) in enumerate(wants):
            assert m.get(i) == (data, st), f"slice {i}"


# ------------------------------------------------------------------ the calls do not block

def test_calls_do_not_block(avr, oracle):
    """With the stream held up by a 0.5 s sleep kernel, the packer and the coder enqueue and return at once."""
    import torch
    rng = np.random.default_rng(31)
    slices = [oracle_lib.random_cabac_stream(rng, int(n), 90) for n in rng.integers(0, 4000, 2000)]
    recs8, states = [to8(r) for r, _ in slices], [s for _, s in slices]
    w = workload(avr, recs8, states, pad_seed=2)
    w.encode()                                              # warm-up: the kernels are loaded
    torch.cuda.synchronize()
    L = avr.lib()
    sp = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    torch.cuda._sleep(20_000_000)
    ev[1].record()
    torch.cuda.synchronize()
    cycles = int(20_000_000 * 500.0 / max(ev[0].elapsed_time(ev[1]), 1e-3))             # about 0.5 s
    w.status.zero_()
    w.out_len.zero_()
    w.out.zero_()
    ev[0].record()
    torch.cuda._sleep(cycles)
    ev[1].record()
    t0 = time.perf_counter()
    assert L.avr_pack_tiles8_narrow_device(0, sp, w.n_states, w.rec8_flat.data_ptr(), w.rec8_off.data_ptr(), w.n_bins.data_ptr(),
                                           w.order.data_ptr(), w.n_slices, w.tile_off.data_ptr(), w.tiles.data_ptr(),
                                           w.status.data_ptr()) == 0
    t1 = time.perf_counter()
    assert L.avr_cabac8_encode_tiles_device(0, sp, w.tiles.data_ptr(), w.tile_off.data_ptr(), w.n_bins.data_ptr(), w.order.data_ptr(),
                                            w.n_slices, w.init_states.data_ptr(), w.n_states, w.out.data_ptr(), w.out_off.data_ptr(),
                                            w.out_len.data_ptr(), w.status.data_ptr(), w.final_states.data_ptr()) == 0
    t2 = time.perf_counter()
    torch.cuda.synchronize()
    sleep_ms = ev[0].elapsed_time(ev[1])
    assert sleep_ms > 200, sleep_ms
    assert (t1 - t0) * 1e3 < sleep_ms / 10 and (t2 - t1) * 1e3 < sleep_ms / 10, (t1 - t0, t2 - t1, sleep_ms)
    check(recs8, states, 90, results(w), "behind the sleep")


# ------------------------------------------------------------------ scale

def test_config5_narrow_equals_two_byte(avr):
    """BASELINE.json configs[4] at 65 536 slices, densified and narrowed on the device: the one-byte tiles and the two-byte tiles
    give every slice the same bytes, final states and statuses."""
    import torch
    w = avr.DeviceWorkload.synth(5, 65536, avr.KIND_CABAC, 0, 1000)
    w.densify()
    assert w.n_states <= avr.MAX_STATES8
    narrow = w.to_cabac8(narrow_tiles=True)
    two = w.to_cabac8()
    del w
    assert narrow.tiles.numel() < two.tiles.numel()
    narrow.encode()
    two.encode()
    torch.cuda.synchronize()
    a, b = results(narrow), results(two)
    assert not any(a[2])
    assert a[2] == b[2]
    assert a[0] == b[0]
    assert a[1] == b[1]
