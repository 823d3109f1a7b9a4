"""GPU: the K2 verifier (k_range_verify, csrc/avr_verify.hip) behind every K2 path -- the one-lane-per-slice coder over tiles, the
slice-major coder, K2p -- through the device calls, the batch API, the test hook and the command line.  Every expected answer is the
oracle's: its encoder for the bytes, and for a corrupted slice the first bin at which its DECODER (avr_oracle_range_decode), given the
same bytes and records, decodes another value than the record's (tests/verify_streams.py)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import oracle_lib
import range_keys as rk
from verify_streams import BIN_COUNTS, VERIFY_NONE, first_bad, flipped

pytestmark = pytest.mark.gpu

POISON = 0x5A5A5A5A
BAD_RECORD, ZERO_PROB, VERIFY_FAILED = 3, 1, 4


def short_slices(n, seed):
    """n slices with the bin counts of the CPU test repeated, adaptive and fixed in turn."""
    rng = np.random.default_rng(seed)
    return [oracle_lib.random_range_stream(rng, BIN_COUNTS[i % len(BIN_COUNTS)], adaptive=bool(i % 2)) for i in range(n)]


@pytest.fixture(scope="module")
def short200():
    return short_slices(200, 9100)


@pytest.fixture(scope="module")
def long4():
    rng = np.random.default_rng(9105)
    return [oracle_lib.random_range_stream(rng, n, adaptive=a) for n, a in ((30000, True), (70000, False), (41237, False), (55001, False))]


def device_verify(avr, w, layout):
    """The device call on a poisoned first_bad: (first_bad uint32[n], status int32[n])."""
    import torch
    L = avr.lib()
    fb = torch.full((w.n_slices,), POISON, dtype=torch.int32, device=w.n_bins.device)
    sp = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    if layout == "tiles":
        rc = L.avr_range_verify_tiles_device(0, sp, w.tiles.data_ptr(), w.tile_off.data_ptr(), w.n_bins.data_ptr(), w.order.data_ptr(),
                                             w.n_slices, w.out.data_ptr(), w.out_off.data_ptr(), w.out_len.data_ptr(), w.status.data_ptr(),
                                             fb.data_ptr())
    else:
        rc = L.avr_range_verify_slices_device(0, sp, w.rec_flat.data_ptr(), w.rec_off.data_ptr(), w.n_bins.data_ptr(), None, w.n_slices,
                                              w.out.data_ptr(), w.out_off.data_ptr(), w.out_len.data_ptr(), w.status.data_ptr(), fb.data_ptr())
    assert rc == 0, L.avr_last_error().decode()
    torch.cuda.synchronize()
    return fb.cpu().numpy().view(np.uint32), w.status.cpu().numpy()


def encoded(avr, oracle, slices):
    """The slices coded over tiles on a region preset to 0xA5: (workload, the oracle's bytes per slice); the device's are the same."""
    import torch
    w = avr.DeviceWorkload.from_host(avr.KIND_RANGE, slices)
    w.out.fill_(0xA5)
    w.encode()
    got, status = w.results()
    want = [oracle.range_encode(r) for r in slices]
    assert status == [st for _, st in want]
    for i, (data, st) in enumerate(want):
        if st == 0:
            assert got[i] == data, f"slice {i}"
    assert not torch.equal(w.order.cpu(), torch.arange(w.n_slices, dtype=torch.int32)) or w.n_slices < 2    # longest first: no identity
    return w, [data for data, _ in want]


def flip_on_device(w, slices_at, positions, masks):
    import torch
    dev = w.out.device
    idx = (w.out_off[:-1][torch.tensor(slices_at, device=dev)] + torch.tensor(positions, device=dev)).to(torch.int64)
    w.out[idx] = w.out[idx] ^ torch.tensor(masks, dtype=torch.uint8, device=dev)


# ------------------------------------------------------------------ 1. tiles, clean

@pytest.mark.parametrize("n", [64, 65, 200])
def test_tiles_clean_slices_verify_and_nothing_is_written(avr, oracle, short200, n):
    w, _ = encoded(avr, oracle, short200[:n])
    out0, tiles0, len0 = w.out.clone(), w.tiles.clone(), w.out_len.clone()
    fb, status = device_verify(avr, w, "tiles")
    assert (status == 0).all()
    assert (fb == VERIFY_NONE).all(), np.flatnonzero(fb != VERIFY_NONE)[:8]
    import torch
    assert torch.equal(w.out, out0) and torch.equal(w.tiles, tiles0) and torch.equal(w.out_len, len0)
    # the Python method, and a null first_bad (the status alone)
    assert (w.verify().cpu().numpy().view(np.uint32) == VERIFY_NONE).all()
    sp = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert avr.lib().avr_range_verify_tiles_device(0, sp, w.tiles.data_ptr(), w.tile_off.data_ptr(), w.n_bins.data_ptr(), w.order.data_ptr(), n,
                                                   w.out.data_ptr(), w.out_off.data_ptr(), w.out_len.data_ptr(), w.status.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert (w.status.cpu().numpy() == 0).all()


# ------------------------------------------------------------------ 2. corruption on the device

def test_tiles_corrupted_slices_fail_at_the_oracles_bin(avr, oracle, short200):
    rng = np.random.default_rng(9102)
    w, data = encoded(avr, oracle, short200)
    able = [i for i in range(200) if len(data[i]) >= 2]
    chosen = sorted(rng.choice(able, 40, replace=False).tolist())
    positions, masks, want = [], [], {}
    for k, i in enumerate(chosen):
        last = len(data[i]) - 2
        p = (0, last, int(rng.integers(0, last + 1)))[k % 3]
        m = (0x01, 0x80, 0xFF)[(k // 3) % 3]
        positions.append(p)
        masks.append(m)
        want[i] = first_bad(oracle, flipped(data[i], p, m), short200[i])
        assert want[i] != VERIFY_NONE                            # the oracle's decoder detects the flip
    flip_on_device(w, chosen, positions, masks)
    out0 = w.out.clone()
    fb, status = device_verify(avr, w, "tiles")
    for i in range(200):
        if i in want:
            assert status[i] == VERIFY_FAILED and fb[i] == want[i], f"slice {i}: status {status[i]}, bin {fb[i]}, the oracle's {want[i]}"
        else:
            assert status[i] == 0 and fb[i] == VERIFY_NONE, f"slice {i}"
    import torch
    assert torch.equal(w.out, out0)
    got, _ = w.results()                                         # bytes and lengths of a failed slice stay retrievable
    for k, i in enumerate(chosen):
        assert got[i] == flipped(data[i], positions[k], masks[k])
    # a second run skips the slices that failed: their status stays, their first_bad is none
    fb2, status2 = device_verify(avr, w, "tiles")
    assert (status2 == status).all() and (fb2 == VERIFY_NONE).all()


# ------------------------------------------------------------------ 3. what lies behind a slice's length

def test_bytes_beyond_the_length_are_not_read_as_the_slices(avr, oracle, short200):
    import torch
    w, data = encoded(avr, oracle, short200)
    off = w.out_off.cpu().numpy()
    assert any(off[i] % 16 == 8 and len(data[i]) for i in range(200))       # a region that starts at 8 mod 16
    host = w.out.cpu().numpy()
    for i in range(200):
        host[off[i] + len(data[i]):off[i + 1]] = 0xFF
    w.out.copy_(torch.from_numpy(host))
    fb, status = device_verify(avr, w, "tiles")
    assert (status == 0).all() and (fb == VERIFY_NONE).all()
    fb, status = device_verify(avr, w, "slices")
    assert (status == 0).all() and (fb == VERIFY_NONE).all()


# ------------------------------------------------------------------ 4. slices that are skipped

def test_slices_with_another_status_are_skipped(avr, oracle, short200):
    slices = [s.copy() for s in short200[:70]]
    bad, zero = 23, 51
    assert slices[bad].size >= 200
    slices[bad][17] |= 0x8000                                                # the packer marks it AVR_SLICE_BAD_RECORD
    slices[zero] = np.concatenate([short200[zero][:40], np.array([0 | (1 << 1) | (0 << 8)], np.uint16), short200[zero][40:]])   # neg = 0, bin 0
    assert oracle.range_encode(slices[zero])[1] == ZERO_PROB
    import torch
    w = avr.DeviceWorkload.from_host(avr.KIND_RANGE, slices)
    assert int(w.status[bad]) == BAD_RECORD
    w.out.fill_(0xA5)
    w.encode()
    torch.cuda.synchronize()
    before = w.status.cpu().numpy().copy()
    assert before[bad] == BAD_RECORD and before[zero] == ZERO_PROB and (np.delete(before, [bad, zero]) == 0).all()
    fb, status = device_verify(avr, w, "tiles")
    assert (status == before).all() and (fb == VERIFY_NONE).all()


# ------------------------------------------------------------------ 5. the slice-major layout and K2p

def test_slice_major_verifier_behind_k2p_and_the_same_answer_over_tiles(avr, oracle, long4):
    import torch
    want = [oracle.range_encode(r)[0] for r in long4]
    w = avr.DeviceWorkload.from_host(avr.KIND_RANGE, long4)
    w.out.fill_(0xA5)
    w.encode_chunked()                                                       # avr_range_encode_chunked_device
    got, status = w.results()
    assert got == want and status == [0] * 4
    fb, st = device_verify(avr, w, "slices")
    assert (st == 0).all() and (fb == VERIFY_NONE).all()
    assert (w.verify().cpu().numpy().view(np.uint32) == VERIFY_NONE).all()  # the Python method takes the slice-major layout after encode_chunked()
    k, p, m = 2, len(want[2]) // 2, 0x10
    expect = first_bad(oracle, flipped(want[k], p, m), long4[k])
    assert expect != VERIFY_NONE
    flip_on_device(w, [k], [p], [m])
    fb, st = device_verify(avr, w, "slices")
    assert st.tolist() == [0, 0, VERIFY_FAILED, 0] and fb.tolist() == [VERIFY_NONE, VERIFY_NONE, expect, VERIFY_NONE]
    # the same four slices through tiles
    w.status.zero_()
    w.out.fill_(0x5A)
    w.encode()
    assert w.results()[0] == want
    fb, st = device_verify(avr, w, "tiles")
    assert (st == 0).all() and (fb == VERIFY_NONE).all()
    flip_on_device(w, [k], [p], [m])
    fb, st = device_verify(avr, w, "tiles")
    assert st.tolist() == [0, 0, VERIFY_FAILED, 0] and fb.tolist() == [VERIFY_NONE, VERIFY_NONE, expect, VERIFY_NONE]


@pytest.mark.parametrize("n", [1025, 2100])
def test_slice_major_verifier_with_several_slices_to_a_wave(avr, oracle, n):
    """Over the slice-major layout a wave takes ceil(n_slices / 1024) slices (one up to 1 024 slices, as in the test above): two and three here."""
    rng = np.random.default_rng(9200 + n)
    counts = (0, 1, 2, 7, 8, 9, 63, 64, 65, 200)
    slices = [oracle_lib.random_range_stream(rng, counts[(i - n) % len(counts)], adaptive=False) for i in range(n)]     # the last one: 200 bins
    w = avr.DeviceWorkload.from_host(avr.KIND_RANGE, slices)
    w.out.fill_(0xA5)
    w.encode_slice_major()
    got, status = w.results()
    assert not any(status)
    fb, st = device_verify(avr, w, "slices")
    assert (st == 0).all() and (fb == VERIFY_NONE).all()
    able = [i for i in range(n) if len(got[i]) >= 2]         # the first and the last of the batch, and either side of the 1 024th slice
    chosen = sorted({able[0], able[1], max(i for i in able if i < 1024), min(i for i in able if i >= 1024), able[-1]})
    assert len(chosen) >= 4 and chosen[-1] == n - 1
    want = {}
    for i in chosen:
        assert got[i] == oracle.range_encode(slices[i])[0]
        want[i] = first_bad(oracle, flipped(got[i], 0, 0x80), slices[i])
        assert want[i] != VERIFY_NONE
    flip_on_device(w, chosen, [0] * len(chosen), [0x80] * len(chosen))
    fb, st = device_verify(avr, w, "slices")
    for i in range(n):
        assert (st[i], fb[i]) == ((VERIFY_FAILED, want[i]) if i in want else (0, VERIFY_NONE)), f"slice {i}"


# ------------------------------------------------------------------ 6. the batch API

def run_batch(avr, slices, verify, keys=None):
    """slices: K2 records, or with keys = group_first: key records.  (results, chunked, verify_ms, timings, first_bad list)"""
    with avr.Batch(0, len(slices), sum(len(s) for s in slices) + 8) as b:
        if verify is not None:
            b.set_verify(verify)
        for i, s in enumerate(slices):
            if keys is not None:
                if i in keys[:-1]:
                    b.begin_group()
                b.add_slice_range_keys(s)
            else:
                b.add_slice_range(s)
        b.submit()
        b.wait()
        return ([b.get(i) for i in range(len(slices))], b.run_info()["chunked"], b.verify_ms(), b.timings(),
                [b.get_verify(i) for i in range(len(slices))])


def batch_case(form):
    rng = np.random.default_rng(9106 + len(form))
    if form == "range_lanes":
        slices = [oracle_lib.random_range_stream(rng, int(rng.integers(0, 3000)), adaptive=i % 10 == 0) for i in range(300)]
        slices[7] = slices[7][:0]
        return slices, slices, None
    if form == "range_k2p":
        slices = [oracle_lib.random_range_stream(rng, int(rng.integers(20000, 60000)), adaptive=i == 0) for i in range(6)]
        return slices, slices, None
    if form == "keys_lanes":
        keys = [rk.random_keys(rng, int(rng.integers(0, 1500)), "skew") for _ in range(150)]
        gf = [0, 60, 150]
    else:
        keys = [rk.random_keys(rng, int(rng.integers(20000, 40000)), "skew") for _ in range(6)]
        gf = [0, 2, 6]
    recs, _ = rk.resolve(keys, gf)
    return keys, recs, gf


@pytest.mark.parametrize("form", ["range_lanes", "range_k2p", "keys_lanes", "keys_k2p"])
def test_batch_with_verify_on_changes_nothing_but_reports(avr, oracle, form):
    fed, recs, gf = batch_case(form)
    want = [oracle.range_encode(r) for r in recs]
    off, chunked0, ms0, t0, fb0 = run_batch(avr, fed, None, gf)
    on, chunked1, ms1, t1, fb1 = run_batch(avr, fed, True, gf)
    assert chunked0 == chunked1 == int(form.endswith("k2p"))               # the K2 path this shape is meant to take did run
    assert off == want and on == want                                       # bytes, lengths and statuses: verify on, verify off, the oracle
    assert ms0 == 0.0 and ms1 > 0.0
    assert fb0 == fb1 == [VERIFY_NONE] * len(fed)
    assert list(t1) == ["h2d_ms", "pack_ms", "encode_ms", "d2h_ms"] == list(t0) and all(v >= 0 for v in t1.values())
    assert run_batch(avr, fed, False, gf)[2] == 0.0                         # set off again: the run is the default one


def test_batch_verify_is_for_the_compress_direction_only(avr):
    rng = np.random.default_rng(9107)
    recs, states = oracle_lib.random_cabac_stream(rng, 500, 20)
    L = avr.lib()
    with avr.Batch(0, 4, 4096) as b:
        b.set_verify(True)
        b.add_slice_cabac(recs, states)
        assert L.avr_batch_submit(b._h) == -1 and "compress direction" in L.avr_last_error().decode()      # AVR_ERR_INVALID
        b.set_verify(False)
        b.run()
        assert b.get(0)[1] == 0 and b.verify_ms() == 0.0 and b.get_verify(0) == VERIFY_NONE
    with avr.Batch(0, 4, 4096) as b:
        b.add_slice_range(oracle_lib.random_range_stream(rng, 300, adaptive=False))
        b.submit()
        with pytest.raises(avr.AvrError, match="in flight"):
            b.set_verify(True)
        b.wait()
        with pytest.raises(avr.AvrError, match="out of range"):
            b.get_verify(1)


# ------------------------------------------------------------------ 7. a failure travelling through the batch API

@pytest.mark.parametrize("path", ["lanes", "k2p"])
def test_a_flipped_byte_comes_back_through_the_batch_api(avr, oracle, hooks, path):
    rng = np.random.default_rng(9108 + len(path))
    if path == "lanes":
        slices = [oracle_lib.random_range_stream(rng, int(rng.integers(200, 2500)), adaptive=False) for _ in range(130)]
        k = 78
    else:
        slices = [oracle_lib.random_range_stream(rng, int(rng.integers(20000, 50000)), adaptive=False) for _ in range(5)]
        k = 4
    want = [oracle.range_encode(r) for r in slices]
    hooks(verify_flip=k)
    got, chunked, ms, _, fb = run_batch(avr, slices, True)
    assert chunked == int(path == "k2p") and ms > 0.0
    bad = flipped(want[k - 1][0], 0, 0x80)
    expect = first_bad(oracle, bad, slices[k - 1])
    assert expect != VERIFY_NONE
    for i in range(len(slices)):
        if i == k - 1:
            assert got[i] == (bad, VERIFY_FAILED) and fb[i] == expect       # its bytes as they lay on the device, its first bad bin
        else:
            assert got[i] == want[i] and fb[i] == VERIFY_NONE, f"slice {i}"
    hooks(verify_flip=0)
    got, _, _, _, fb = run_batch(avr, slices, True)
    assert got == want and fb == [VERIFY_NONE] * len(slices)
    hooks(verify_flip=k)                                                    # with verify off the hook is not read: nothing is flipped
    assert run_batch(avr, slices, False)[0] == want


# ------------------------------------------------------------------ 8. the command line

def test_cli_compress_with_verify_writes_the_same_bytes(avr, tmp_path):
    from test_h264 import clip
    recode = avr.build_recode()
    files = {}
    for name, env in (("plain", {}), ("verify", {"AVR_VERIFY": "1", "AVR_TIMING": "1"}),
                      ("verify_est", {"AVR_VERIFY": "1", "AVR_DEVICE_ESTIMATORS": "1"})):
        out = tmp_path / f"{name}.recode"
        run = subprocess.run([recode, "compress", clip("realshort.mp4"), str(out)], capture_output=True, text=True, timeout=600,
                             env=dict(os.environ, **env))
        assert run.returncode == 0, run.stderr
        assert ("GPU verify" in run.stderr) == (name == "verify")           # a phase of its own under AVR_TIMING=1, nothing without
        files[name] = out.read_bytes()
    assert len(files["plain"]) > 0 and files["verify"] == files["plain"] and files["verify_est"] == files["plain"]
