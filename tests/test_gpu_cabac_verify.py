"""GPU: the K1 verifier (k_cabac_verify, csrc/avr_cabac_verify.hip) behind every K1 path -- the one-lane-per-slice coders over
two-byte and one-byte tiles, the slice-major coder, K1p from two-byte and one-byte records, both code paths -- through the device calls,
DeviceWorkload.verify_k1, the batch API, the test hook and the command line.  Every expected answer is the oracle's: its encoder
(avr_oracle_cabac_encode) for the bytes, and for a corrupted slice the first bin at which its spec DECODER (avr_spec_cabac_decode), given
the same bytes, records and states, decodes another value than the record's (tests/cabac_verify_streams.py)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import cabac_verify_streams as cvs
import oracle_lib
from cabac_verify_streams import BIN_COUNTS, CODES, LONG_COUNTS, MASKS, SLICES2, SLICES8, TILES2, TILES8, VERIFY_NONE, first_bad, flipped

pytestmark = pytest.mark.gpu

POISON = 0x5A5A5A5A
BAD_RECORD, VERIFY_FAILED = 3, 4
FORM_NAMES = {TILES2: "tiles2", SLICES2: "slices2", TILES8: "tiles8", SLICES8: "slices8", CODES: "codes"}


def make_slices(counts, n_ctx, seed):
    """[(recs, states)] with the given bin counts (a terminated stream has one bin more), terminated and not in turn."""
    rng = np.random.default_rng(seed)
    return [oracle_lib.random_cabac_stream(rng, n, n_ctx, terminate=bool(i % 2)) for i, n in enumerate(counts)]


@pytest.fixture(scope="module")
def short200():
    return make_slices([BIN_COUNTS[i % len(BIN_COUNTS)] for i in range(200)], 20, 9300)


@pytest.fixture(scope="module")
def long4():
    return make_slices(LONG_COUNTS, 20, 9301)


@pytest.fixture(scope="module")
def answers(oracle):
    """The oracle's (bytes, final states, status) of a list of slices, worked out once per list."""
    cache = {}

    def of(slices):
        if id(slices) not in cache:
            cache[id(slices)] = (slices, [oracle.cabac_encode(r, s) for r, s in slices])
        return cache[id(slices)][1]
    return of


def workload(avr, slices, form):
    """The slices as a DeviceWorkload that holds the form's records: two-byte, or one-byte with one-byte tiles."""
    if form in (TILES8, SLICES8):
        return avr.DeviceWorkload.from_host(avr.KIND_CABAC8, [cvs.narrowed(r) for r, _ in slices], [s for _, s in slices],
                                            pad_bytes=np.array([0xA5, 0xFF, 0x00, 0xFD], np.uint8), narrow_tiles=True)
    return avr.DeviceWorkload.from_host(avr.KIND_CABAC, [r for r, _ in slices], [s for _, s in slices])


def encoded(avr, slices, want, form):
    """The slices coded by the one-lane-per-slice coder on regions preset to 0xA5; the device's bytes are the oracle's."""
    w = workload(avr, slices, form)
    w.out.fill_(0xA5)
    w.encode()
    got, status = w.results()
    assert status == [st for _, _, st in want]
    assert got == [data for data, _, _ in want]
    if form == CODES:                                        # the codes by the rule of the header (cabac_verify_streams.codes_of), not the product's
        import torch
        mlps = oracle_lib.load_oracle().tables()[1]
        res_off = w._chunk_plan()["tensors"]["res_off"].cpu().numpy()
        host = np.full(int(res_off[-1]) + 32, 0xA5, np.uint8)                  # what lies behind a slice's codes is never decoded
        for i, (r, st) in enumerate(slices):
            assert res_off[i] % 16 == 0 and res_off[i + 1] - res_off[i] >= (len(r) + 15) // 16 * 16
            host[res_off[i]:res_off[i] + len(r)] = cvs.codes_of(r, st, mlps)
        w.codes = torch.from_numpy(host).to(w.out.device)
    return w


def device_verify(avr, w, form, final=True, with_first_bad=True):
    """The form's device call on a poisoned first_bad: (first_bad uint32[n], status int32[n])."""
    import torch
    L = avr.lib()
    fb = torch.full((w.n_slices,), POISON, dtype=torch.int32, device=w.n_bins.device)
    sp = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    fbp = fb.data_ptr() if with_first_bad else None
    tail = (w.out.data_ptr(), w.out_off.data_ptr(), w.out_len.data_ptr())
    states = (w.init_states.data_ptr(), w.n_states)
    fin = w.final_states.data_ptr() if final else None
    if form == CODES:
        rc = L.avr_cabac_verify_codes_device(0, sp, w.codes.data_ptr(), w._chunk_plan()["tensors"]["res_off"].data_ptr(), w.n_bins.data_ptr(),
                                             None, w.n_slices, *tail, w.status.data_ptr(), fbp)
    elif form in (TILES2, TILES8):
        call = L.avr_cabac_verify_tiles_device if form == TILES2 else L.avr_cabac8_verify_tiles_device
        rc = call(0, sp, w.tiles.data_ptr(), w.tile_off.data_ptr(), w.n_bins.data_ptr(), w.order.data_ptr(), w.n_slices, *states, *tail, fin,
                  w.status.data_ptr(), fbp)
    else:
        recs, rec_off = w._slice_major()
        call = L.avr_cabac_verify_slices_device if form == SLICES2 else L.avr_cabac8_verify_slices_device
        rc = call(0, sp, recs.data_ptr(), rec_off.data_ptr(), w.n_bins.data_ptr(), None, w.n_slices, *states, *tail, fin,
                  w.status.data_ptr(), fbp)
    assert rc == 0, L.avr_last_error().decode()
    torch.cuda.synchronize()
    return fb.cpu().numpy().view(np.uint32), w.status.cpu().numpy()


def flip_on_device(w, slices_at, positions, masks):
    import torch
    dev = w.out.device
    idx = (w.out_off[:-1][torch.tensor(slices_at, device=dev)] + torch.tensor(positions, device=dev)).to(torch.int64)
    w.out[idx] = w.out[idx] ^ torch.tensor(masks, dtype=torch.uint8, device=dev)


def all_clean(fb, status):
    assert (status == 0).all(), np.flatnonzero(status)[:8]
    assert (fb == VERIFY_NONE).all(), (np.flatnonzero(fb != VERIFY_NONE)[:8], fb[fb != VERIFY_NONE][:8])


# ------------------------------------------------------------------ 1. device calls, clean

@pytest.mark.parametrize("n", [64, 65, 200])
@pytest.mark.parametrize("form", [TILES2, TILES8], ids=FORM_NAMES.get)
def test_tiles_clean_slices_verify_and_nothing_is_written(avr, answers, short200, form, n):
    import torch
    slices = short200[:n]
    w = encoded(avr, slices, answers(short200)[:n], form)
    out0, tiles0, len0, fin0 = w.out.clone(), w.tiles.clone(), w.out_len.clone(), w.final_states.clone()
    all_clean(*device_verify(avr, w, form))
    all_clean(*device_verify(avr, w, form, final=False))
    assert torch.equal(w.out, out0) and torch.equal(w.tiles, tiles0) and torch.equal(w.out_len, len0) and torch.equal(w.final_states, fin0)
    fb, status = device_verify(avr, w, form, with_first_bad=False)       # a null first_bad: the status alone
    assert (status == 0).all() and (fb == POISON).all()
    assert (w.verify_k1().cpu().numpy().view(np.uint32) == VERIFY_NONE).all()      # the Python method takes the tiles after encode()


@pytest.mark.parametrize("form", [SLICES2, SLICES8, CODES], ids=FORM_NAMES.get)
def test_slice_major_forms_and_codes_clean(avr, answers, short200, long4, form):
    import torch
    for slices in (short200, long4):
        w = encoded(avr, slices, answers(slices), form)
        out0, len0 = w.out.clone(), w.out_len.clone()
        recs0 = w.codes.clone() if form == CODES else w._slice_major()[0].clone()
        all_clean(*device_verify(avr, w, form))
        assert torch.equal(w.out, out0) and torch.equal(w.out_len, len0)
        assert torch.equal(recs0, w.codes if form == CODES else w._slice_major()[0])


@pytest.mark.parametrize("n_states", [460, 1024])
def test_many_contexts_take_the_large_lds_launch(avr, oracle, n_states):
    """65 slices (two tiles) over 460 and over 1 024 contexts: 29 and 64.25 KiB of state bytes a wave."""
    rng = np.random.default_rng(9302 + n_states)
    slices = [oracle_lib.random_cabac_stream(rng, (3000, 1025, 200, 17, 0)[i % 5], n_states, terminate=bool(i % 2)) for i in range(65)]
    want = [oracle.cabac_encode(r, s) for r, s in slices]
    w = encoded(avr, slices, want, TILES2)
    for form in (TILES2, SLICES2):
        all_clean(*device_verify(avr, w, form))
    k, data = 5, want[5][0]                                   # 3 000 bins
    expect = first_bad(oracle, flipped(data, len(data) // 2, 0x10), *slices[k])
    assert expect != VERIFY_NONE
    flip_on_device(w, [k], [len(data) // 2], [0x10])
    for form in (TILES2, SLICES2):
        fb, st = device_verify(avr, w, form)
        assert st[k] == VERIFY_FAILED and fb[k] == expect and (np.delete(st, k) == 0).all() and (np.delete(fb, k) == VERIFY_NONE).all()
        w.status.zero_()


# ------------------------------------------------------------------ 2. corruption on the device

@pytest.mark.parametrize("form", [TILES2, SLICES2, TILES8, SLICES8, CODES], ids=FORM_NAMES.get)
def test_corrupted_slices_fail_at_the_oracles_bin(avr, oracle, answers, short200, form):
    import torch
    rng = np.random.default_rng(9303)
    want = answers(short200)
    data = [d for d, _, _ in want]
    w = encoded(avr, short200, want, form)
    able = [i for i in range(200) if len(data[i]) >= 3]
    chosen = sorted(rng.choice(able, 40, replace=False).tolist())
    positions, masks, expect = [], [], {}
    for k, i in enumerate(chosen):
        last = len(data[i]) - 3
        p = (0, last, int(rng.integers(0, last + 1)))[k % 3]
        m = MASKS[(k // 3) % 3]
        positions.append(p)
        masks.append(m)
        expect[i] = first_bad(oracle, flipped(data[i], p, m), *short200[i])
        assert expect[i] != VERIFY_NONE                       # the oracle's decoder detects the flip
    flip_on_device(w, chosen, positions, masks)
    out0 = w.out.clone()
    fb, status = device_verify(avr, w, form)
    for i in range(200):
        if i in expect:
            assert status[i] == VERIFY_FAILED and fb[i] == expect[i], f"slice {i}: status {status[i]}, bin {fb[i]}, the oracle's {expect[i]}"
        else:
            assert status[i] == 0 and fb[i] == VERIFY_NONE, f"slice {i}"
    assert torch.equal(w.out, out0)
    got, _ = w.results()                                      # bytes and lengths of a failed slice stay retrievable
    for k, i in enumerate(chosen):
        assert got[i] == flipped(data[i], positions[k], masks[k])
    fb2, status2 = device_verify(avr, w, form)                # a second run skips the slices that failed
    assert (status2 == status).all() and (fb2 == VERIFY_NONE).all()


@pytest.mark.parametrize("form", [TILES2, SLICES8], ids=FORM_NAMES.get)
def test_slices_with_a_bad_record_are_skipped(avr, oracle, short200, form):
    import torch
    slices = [(r.copy(), s) for r, s in short200[:70]]
    bad = 29
    assert slices[bad][0].size >= 200
    slices[bad][0][17] = np.uint16((100 << 1) | 1)            # selector 100: no context of a slice with 20 states
    w = workload(avr, slices, form)
    assert int(w.status[bad]) == BAD_RECORD
    w.out.fill_(0xA5)
    w.encode()
    torch.cuda.synchronize()
    before = w.status.cpu().numpy().copy()
    assert before[bad] == BAD_RECORD and (np.delete(before, bad) == 0).all()
    fb, status = device_verify(avr, w, form)
    assert (status == before).all() and (fb == VERIFY_NONE).all()


# ------------------------------------------------------------------ 3. final states

@pytest.mark.parametrize("form", [TILES2, SLICES2, TILES8, SLICES8], ids=FORM_NAMES.get)
def test_a_changed_final_state_is_reported_at_n_bins(avr, answers, short200, form):
    import torch
    w = encoded(avr, short200, answers(short200), form)
    assert w.final_states.cpu().numpy().tobytes() == b"".join(f for _, f, _ in answers(short200))
    chosen = [0, 63, 64, 130, 199]
    for k, i in enumerate(chosen):
        w.final_states[i * w.n_states + (0, 19, 7, 3, 11)[k]] ^= (1, 2, 4, 64, 1)[k]
    fb, status = device_verify(avr, w, form)
    n_bins = w.n_bins.cpu().numpy()
    for i in range(200):
        assert (status[i], fb[i]) == ((VERIFY_FAILED, n_bins[i]) if i in chosen else (0, VERIFY_NONE)), f"slice {i}"
    w.status.zero_()                                          # without the encoder's states there is nothing to compare
    all_clean(*device_verify(avr, w, form, final=False))


# ------------------------------------------------------------------ 4. encoded by the product, then verified

def _mixed(short200, long4):
    return long4 + short200[:60]


@pytest.mark.parametrize("path", ["encode", "encode_narrow", "encode_wide8", "chunked", "chunked8", "slice_major", "resolved", "codes_serial"])
def test_every_k1_path_of_the_workload_verifies(avr, oracle, short200, long4, path):
    slices = _mixed(short200, long4)
    want = [oracle.cabac_encode(r, s) for r, s in slices]
    if path in ("encode_narrow", "encode_wide8", "chunked8"):
        w = avr.DeviceWorkload.from_host(avr.KIND_CABAC8, [cvs.narrowed(r) for r, _ in slices], [s for _, s in slices],
                                         narrow_tiles=path == "encode_narrow")
    else:
        w = workload(avr, slices, SLICES2)
    w.out.fill_(0xA5)
    if path.startswith("encode"):
        w.encode()
    elif path.startswith("chunked"):
        w.encode_chunked()
    elif path == "slice_major":
        w.encode_slice_major()
    else:
        codes = w.resolve()
        (w.encode_resolved if path == "resolved" else w.encode_codes_serial)(codes)
    got, status = w.results()
    assert not any(status) and got == [d for d, _, _ in want]
    fb = w.verify_k1().cpu().numpy().view(np.uint32)
    assert (fb == VERIFY_NONE).all() and not w.status.cpu().numpy().any()
    k = 2                                                     # and a flipped byte is found behind each of them
    expect = first_bad(oracle, flipped(want[k][0], 1000, 0x04), *slices[k])
    flip_on_device(w, [k], [1000], [0x04])
    fb = w.verify_k1().cpu().numpy().view(np.uint32)
    assert fb[k] == expect != VERIFY_NONE and (np.delete(fb, k) == VERIFY_NONE).all()
    assert w.status.cpu().numpy().tolist() == [VERIFY_FAILED if i == k else 0 for i in range(len(slices))]


def test_verify_k1_is_for_k1_workloads(avr):
    w = avr.DeviceWorkload.from_host(avr.KIND_RANGE, [oracle_lib.random_range_stream(np.random.default_rng(1), 50, adaptive=False)])
    w.encode()
    with pytest.raises(avr.AvrError, match="K1"):
        w.verify_k1()
    r, s = oracle_lib.random_cabac_stream(np.random.default_rng(2), 50, 20)
    with pytest.raises(avr.AvrError, match="nothing was encoded"):
        avr.DeviceWorkload.from_host(avr.KIND_CABAC, [r], [s]).verify_k1()


# ------------------------------------------------------------------ 5. the batch API

@pytest.fixture(scope="module")
def batch_shapes(oracle):
    """shape -> (slices, the oracle's answers, codes): a one-lane shape and a K1p shape."""
    mlps = oracle.tables()[1]
    rng = np.random.default_rng(9304)
    lanes = [oracle_lib.random_cabac_stream(rng, int(rng.integers(0, 3000)), 20, terminate=bool(i % 2)) for i in range(300)]
    lanes[7] = (lanes[7][0][:0], lanes[7][1])
    k1p = [oracle_lib.random_cabac_stream(rng, int(rng.integers(20000, 60000)), 20, terminate=bool(i % 2)) for i in range(6)]
    out = {}
    for name, slices in (("lanes", lanes), ("k1p", k1p)):
        out[name] = (slices, [oracle.cabac_encode(r, s) for r, s in slices], [cvs.codes_of(r, s, mlps) for r, s in slices])
    return out


def run_batch(avr, kind, shape, verify, runs=1):
    """(results [(bytes, status)], final states or None, chunked, verify_ms, timings, first_bad list) of the last of `runs` runs."""
    slices, _, codes = shape
    with avr.Batch(0, len(slices), sum(len(r) for r, _ in slices) + 16 * len(slices) + 64) as b:
        if verify is not None:
            b.set_verify_k1(verify)
        for (r, s), c in zip(slices, codes):
            if kind == "cabac":
                b.add_slice_cabac(r, s)
            elif kind == "cabac8":
                b.add_slice_cabac8(cvs.narrowed(r), s)
            else:
                b.add_codes(c)
        for _ in range(runs):
            b.submit()
            b.wait()
        n = len(slices)
        return ([b.get(i) for i in range(n)], [b.get_states(i) for i in range(n)] if kind != "codes" else None,
                b.run_info(), b.verify_ms(), b.timings(), [b.get_verify(i) for i in range(n)])


@pytest.mark.parametrize("shape", ["lanes", "k1p"])
@pytest.mark.parametrize("kind", ["cabac", "cabac8", "codes"])
def test_batch_with_verify_k1_on_changes_nothing_but_reports(avr, batch_shapes, kind, shape):
    s = batch_shapes[shape]
    want = [(d, st) for d, _, st in s[1]]
    finals = [f for _, f, _ in s[1]] if kind != "codes" else None
    off, fin0, info0, ms0, t0, fb0 = run_batch(avr, kind, s, None)
    on, fin1, info1, ms1, t1, fb1 = run_batch(avr, kind, s, True)
    assert info0["chunked"] == info1["chunked"] == int(shape == "k1p")        # the K1 path this shape is meant to take did run
    assert off == want and on == want and fin0 == finals and fin1 == finals   # verifier on, verifier off, the oracle
    assert ms0 == 0.0 and ms1 > 0.0
    assert fb0 == fb1 == [VERIFY_NONE] * len(want)
    assert list(t1) == ["h2d_ms", "pack_ms", "encode_ms", "d2h_ms"] == list(t0) and all(v >= 0 for v in t1.values())
    assert run_batch(avr, kind, s, False)[3] == 0.0                          # set off again: the run is the default one
    if shape == "k1p" and kind == "cabac":                                   # submitted twice: the second run is sized by a guess
        again, fin2, info2, ms2, _, fb2 = run_batch(avr, kind, s, True, runs=2)
        assert info2["chunked"] == 1 and info2["rows_guessed"] > 0
        assert again == want and fin2 == finals and ms2 > 0.0 and fb2 == [VERIFY_NONE] * len(want)


def test_a_batch_that_wait_runs_again_is_verified_again(avr, oracle, hooks):
    """A batch object whose first batch used 10 contexts and whose second uses 100: the second run is sized by the first's count,
    avr_batch_wait finds the guess too small and runs the batch again -- verifier included; the answers are the last run's."""
    rng = np.random.default_rng(9305)
    mk = lambda n_used: [(r, np.concatenate([s, rng.integers(0, 126, 100 - n_used).astype(np.uint8)]))
                         for r, s in (oracle_lib.random_cabac_stream(rng, 30000 + 2000 * i, n_used) for i in range(5))]
    first, second = mk(10), mk(100)
    hooks(verify_flip=2)
    with avr.Batch(0, 8, 400000) as b:
        b.set_verify_k1(True)
        for k, slices in enumerate((first, second)):
            if k:
                b.reset()                                    # keeps the setting
            for r, s in slices:
                b.add_slice_cabac(r, s)
            b.submit()
            b.wait()
            info = b.run_info()
            assert info["chunked"] == 1 and (info["ran_again"] & 1) == k, info
            for i, (r, s) in enumerate(slices):
                data, final, _ = oracle.cabac_encode(r, s)
                if i == 1:                                   # the hook's slice, in the last run as in the first
                    bad = flipped(data, 0, 0x80)
                    assert b.get(i) == (bad, VERIFY_FAILED) and b.get_verify(i) == first_bad(oracle, bad, r, s) != VERIFY_NONE
                else:
                    assert b.get(i) == (data, 0) and b.get_states(i) == final and b.get_verify(i) == VERIFY_NONE, f"batch {k} slice {i}"
            assert b.verify_ms() > 0.0


def test_the_second_pass_from_wait_is_verified_too(avr, oracle, hooks):
    """tests/test_gpu_parity.py's second-pass batch: a slice with single bins in contexts the sampled census misses is coded by
    avr_batch_wait's second pass when the run was sized by a guess -- behind the verifier of the run.  The verifier follows the
    second pass too, and a slice that failed in front of it keeps its bytes and fails again at the same bin."""
    rng = np.random.default_rng(31)
    slices = []
    for i in range(5):
        r, s = oracle_lib.random_cabac_stream(rng, 30000 + 3000 * i, 50)
        slices.append((r, np.concatenate([s, rng.integers(0, 126, 150).astype(np.uint8)])))
    slices[3][0][12345] = np.uint16((199 << 1) | 1)
    slices[3][0][20001] = np.uint16((77 << 1) | 0)
    want = [oracle.cabac_encode(r, s) for r, s in slices]
    hooks(verify_flip=1)
    with avr.Batch(0, 8, 400000) as b:
        b.set_verify_k1(True)
        for r, s in slices:
            b.add_slice_cabac(r, s)
        for run in range(2):
            b.submit()
            b.wait()
            info = b.run_info()
            assert info["chunked"] == 1 and bool(info["ran_again"] & 2) == (run == 1)
            bad = flipped(want[0][0], 0, 0x80)
            assert b.get(0) == (bad, VERIFY_FAILED) and b.get_verify(0) == first_bad(oracle, bad, *slices[0]) != VERIFY_NONE
            for i in range(1, 5):
                assert (b.get(i), b.get_states(i), b.get_verify(i)) == ((want[i][0], 0), want[i][1], VERIFY_NONE), f"run {run} slice {i}"
            assert b.verify_ms() > 0.0
            t = b.timings()                                      # the second pass: the verifier in front of it is taken off the encode's slot
            assert all(v >= 0.0 for v in t.values()) and t["encode_ms"] > 0.0, t


def test_batch_verify_k1_refusals(avr):
    rng = np.random.default_rng(9306)
    L = avr.lib()
    with avr.Batch(0, 4, 4096) as b:
        b.set_verify_k1(True)
        b.add_slice_range(oracle_lib.random_range_stream(rng, 300, adaptive=False))
        assert L.avr_batch_submit(b._h) == -1 and "decompress direction" in L.avr_last_error().decode()     # AVR_ERR_INVALID
        b.set_verify_k1(False)
        b.run()
        assert b.get(0)[1] == 0 and b.verify_ms() == 0.0 and b.get_verify(0) == VERIFY_NONE
    recs, states = oracle_lib.random_cabac_stream(rng, 500, 20)
    with avr.Batch(0, 4, 4096) as b:
        b.add_slice_cabac(recs, states)
        b.submit()
        with pytest.raises(avr.AvrError, match="in flight"):
            b.set_verify_k1(True)
        b.wait()
        assert b.get_verify(0) == VERIFY_NONE and b.verify_ms() == 0.0


# ------------------------------------------------------------------ 6. a failure travelling through the batch API

@pytest.mark.parametrize("shape,k", [("lanes", 78), ("k1p", 5)])
@pytest.mark.parametrize("kind", ["cabac", "codes"])
def test_a_flipped_byte_comes_back_through_the_batch_api(avr, oracle, hooks, batch_shapes, kind, shape, k):
    s = batch_shapes[shape]
    slices, want = s[0], [(d, st) for d, _, st in s[1]]
    assert len(want[k - 1][0]) >= 3
    hooks(verify_flip=k)
    got, _, info, ms, _, fb = run_batch(avr, kind, s, True)
    assert info["chunked"] == int(shape == "k1p") and ms > 0.0
    bad = flipped(want[k - 1][0], 0, 0x80)
    expect = first_bad(oracle, bad, *slices[k - 1])
    assert expect != VERIFY_NONE
    for i in range(len(slices)):
        if i == k - 1:
            assert got[i] == (bad, VERIFY_FAILED) and fb[i] == expect        # its bytes as they lay on the device, its first bad bin
        else:
            assert got[i] == want[i] and fb[i] == VERIFY_NONE, f"slice {i}"
    hooks(verify_flip=0)
    got, _, _, _, _, fb = run_batch(avr, kind, s, True)
    assert got == want and fb == [VERIFY_NONE] * len(slices)
    hooks(verify_flip=k)                                                     # with the verifier off the hook is not read: nothing is flipped
    assert run_batch(avr, kind, s, False)[0] == want


# ------------------------------------------------------------------ 7. the command line

def test_cli_decompress_with_verify_k1_writes_the_same_bytes(avr, tmp_path):
    from test_h264 import clip
    recode = avr.build_recode()
    packed = tmp_path / "clip.recode"
    run = subprocess.run([recode, "compress", clip("realshort.mp4"), str(packed)], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr
    files = {}
    for name, env in (("plain", {"AVR_TIMING": "1"}), ("verify", {"AVR_VERIFY_K1": "1", "AVR_TIMING": "1"})):
        out = tmp_path / f"{name}.mp4"
        run = subprocess.run([recode, "decompress", str(packed), str(out)], capture_output=True, text=True, timeout=600,
                             env=dict(os.environ, **env))
        assert run.returncode == 0, run.stderr
        assert ("GPU verify (K1)" in run.stderr) == (name == "verify")       # a phase of its own under AVR_TIMING=1, nothing without
        files[name] = out.read_bytes()
    assert len(files["plain"]) > 0 and files["verify"] == files["plain"]
