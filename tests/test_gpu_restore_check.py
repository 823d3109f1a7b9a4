"""GPU: the restore check (k_restore_check, csrc/avr_restore.hip) -- the device call on the emulator's whole table of cases in guarded
buffers of exactly the stated sizes, the entry statuses, offsets beyond 4 GiB, behind every K1 path of a DeviceWorkload, through the
batch API (with and without the K1 verifier, in avr_batch_wait's second runs) and the command line.  Every expected answer is the
plain-Python reference of tests/restore_ref.py; the coded bytes are the oracle's."""
import ctypes
import gc
import os
import shutil
import subprocess

import numpy as np
import pytest

import cabac_verify_streams as cvs
import far_offsets
import oracle_lib
import restore_ref
from guarded import Guarded
from restore_ref import EXPECT_NONE, VERIFY_NONE

pytestmark = pytest.mark.gpu

OK, ZERO_PROB, OVERFLOW, BAD_RECORD, VERIFY_FAILED = 0, 1, 2, 3, 4
POISON = 0x5A5A5A5A


@pytest.fixture(scope="module")
def table(avr):
    """The emulator's table and the reference's answer for every case, worked out once."""
    cases = restore_ref.table()
    return cases, [restore_ref.first_diff(avr, c.out, c.expect) for c in cases]


class DeviceBatch:
    """Cases laid out as one batch on the device, every buffer a guarded one of exactly the stated size."""

    def __init__(self, cases, status=None, expect_len=None):
        import torch
        dev = torch.device("cuda", 0)
        out, out_off, out_len, expect, expect_off, exp_len = restore_ref.layout(cases)
        if expect_len is not None:
            exp_len = np.asarray(expect_len, np.uint32)
        n = self.n = len(cases)
        self.bufs = {}

        def put(name, a):
            a = np.ascontiguousarray(a)
            if a.nbytes == 0:                                    # (no bytes at all: the call still wants a pointer, and reads nothing of it)
                a = np.full(8, restore_ref.FILL, np.uint8)
            g = self.bufs[name] = Guarded(a.nbytes, dev, name)
            if a.nbytes:
                g.view.copy_(torch.from_numpy(a.view(np.uint8).reshape(-1)).to(dev))
            return g.view
        self.out, self.expect = put("out", out), put("expect", expect)
        self.out_off, self.expect_off = put("out_off", out_off), put("expect_off", expect_off)
        self.out_len, self.expect_len = put("out_len", out_len), put("expect_len", exp_len)
        self.status = put("status", np.zeros(n, np.int32) if status is None else np.asarray(status, np.int32))
        self.first_diff = put("first_diff", np.full(n, POISON, np.uint32))
        self.before = {k: self.bufs[k].view.clone() for k in ("out", "out_len", "expect", "out_off", "expect_off", "expect_len")}

    def run(self, avr):
        """The device call on a stream of the caller's own: (first_diff uint32[n], status int32[n]); nothing else has changed."""
        import torch
        torch.cuda.synchronize()
        stream = torch.cuda.Stream()
        rc = avr.lib().avr_restore_check_device(0, ctypes.c_void_p(stream.cuda_stream), self.out.data_ptr(), self.out_off.data_ptr(),
                                                self.out_len.data_ptr(), self.n, self.expect.data_ptr(), self.expect_off.data_ptr(),
                                                self.expect_len.data_ptr(), self.status.data_ptr(), self.first_diff.data_ptr())
        assert rc == 0, avr.lib().avr_last_error().decode()
        stream.synchronize()
        torch.cuda.synchronize()
        for k, was in self.before.items():
            assert torch.equal(self.bufs[k].view, was), f"{k} was written"
        for g in self.bufs.values():
            g.check()
        return self.first_diff.cpu().numpy().view(np.uint32), self.status.cpu().numpy().view(np.int32)


def held_to_reference(cases, want, fd, status, status_in=None):
    for i, c in enumerate(cases):
        was = OK if status_in is None else status_in[i]
        assert fd[i] == want[i], f"{c.name}: first_diff {fd[i]}, the reference's {want[i]}"
        assert status[i] == (VERIFY_FAILED if want[i] != VERIFY_NONE and was == OK else was), f"{c.name}: status {status[i]}"


# ------------------------------------------------------------------ 1. the device call on synthetic bytes

def test_the_whole_table_as_one_batch(avr, table):
    cases, want = table
    fd, status = DeviceBatch(cases).run(avr)
    held_to_reference(cases, want, fd, status)
    assert (fd == VERIFY_NONE).any() and (fd != VERIFY_NONE).any()


@pytest.mark.parametrize("n", [1, 4, 5, 64, 65, 200])
def test_part_filled_workgroups(avr, table, n):
    cases, want = table
    pick = [(37 * i + n) % len(cases) for i in range(n)]         # a spread of the table, the long cases among them
    sub, sub_want = [cases[i] for i in pick], [want[i] for i in pick]
    fd, status = DeviceBatch(sub).run(avr)
    held_to_reference(sub, sub_want, fd, status)


def test_no_slices_is_no_launch(avr):
    assert avr.lib().avr_restore_check_device(0, None, None, None, None, 0, None, None, None, None, None) == 0


# ------------------------------------------------------------------ 2. entry statuses

def test_entry_statuses_and_slices_without_an_expectation(avr, table):
    cases, want = table
    finding = [i for i, w in enumerate(want) if w != VERIFY_NONE and len(cases[i].out) >= 8][:12]
    clean = [i for i, w in enumerate(want) if w == VERIFY_NONE][:6]
    pick = finding + clean
    sub, sub_want = [cases[i] for i in pick], [want[i] for i in pick]
    status_in = [(BAD_RECORD, OVERFLOW, ZERO_PROB, VERIFY_FAILED, OK, OK)[k % 6] for k in range(len(pick))]
    exp_len = [len(c.expect) for c in sub]
    for k in (5, 11, 16):                                        # AVR_SLICE_OK, but no expectation
        assert status_in[k] == OK
        exp_len[k] = EXPECT_NONE
    fd, status = DeviceBatch(sub, status_in, exp_len).run(avr)
    for k, c in enumerate(sub):
        skipped = status_in[k] in (BAD_RECORD, OVERFLOW, ZERO_PROB) or exp_len[k] == EXPECT_NONE
        if skipped:                                              # status kept, no answer
            assert (fd[k], status[k]) == (VERIFY_NONE, status_in[k]), c.name
        else:                                                    # AVR_SLICE_VERIFY_FAILED takes part and stays what it is
            assert fd[k] == sub_want[k], c.name
            assert status[k] == (VERIFY_FAILED if status_in[k] == VERIFY_FAILED or sub_want[k] != VERIFY_NONE else OK), c.name
    assert any(status_in[k] == VERIFY_FAILED and sub_want[k] == VERIFY_NONE for k in range(len(pick)))
    assert any(status_in[k] == VERIFY_FAILED and sub_want[k] != VERIFY_NONE for k in range(len(pick)))


# ------------------------------------------------------------------ 3. offsets beyond 4 GiB

def test_offsets_beyond_4_gib(avr, table):
    """out_off and expect_off with 2^32 added: the bytes lie above 4 GiB in buffers allocated whole and poisoned below, so a kernel that
    keeps the low word of either offset reads the poison.  The one skip: a device with less free memory than the two buffers and 2 GiB."""
    import torch
    cases, want = table
    pick = [i for i, c in enumerate(cases) if len(c.out) > 60000][:24] + list(range(0, len(cases), 29))
    sub, sub_want = [cases[i] for i in pick], [want[i] for i in pick]
    base = far_offsets.B32
    out, out_off, out_len, expect, expect_off, expect_len = restore_ref.layout(sub, far=base)
    need = 2 * base + out.size + expect.size
    torch.cuda.empty_cache()
    free = torch.cuda.mem_get_info()[0]
    if free < need + (2 << 30):
        pytest.skip(f"the case needs {need} bytes and 2 GiB beside them; the device reports {free} free")
    dev = torch.device("cuda", 0)
    try:
        d_out = torch.empty(base + out.size, dtype=torch.uint8, device=dev)
        d_out.fill_(0x5A)
        d_out[base:] = torch.from_numpy(out).to(dev)
        d_expect = torch.empty(base + expect.size, dtype=torch.uint8, device=dev)
        d_expect.fill_(0xA5)
        d_expect[base:] = torch.from_numpy(expect).to(dev)
        t = [torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a.view(np.int32) if a.dtype == np.uint32 else a).to(dev)
             for a in (out_off, out_len, expect_off, expect_len)]
        status = torch.zeros(len(sub), dtype=torch.int32, device=dev)
        fd = torch.full((len(sub),), POISON, dtype=torch.int32, device=dev)
        sp = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        rc = avr.lib().avr_restore_check_device(0, sp, d_out.data_ptr(), t[0].data_ptr(), t[1].data_ptr(), len(sub), d_expect.data_ptr(),
                                                t[2].data_ptr(), t[3].data_ptr(), status.data_ptr(), fd.data_ptr())
        assert rc == 0, avr.lib().avr_last_error().decode()
        torch.cuda.synchronize()
        held_to_reference(sub, sub_want, fd.cpu().numpy().view(np.uint32), status.cpu().numpy())
        assert torch.equal(d_out[base:].cpu(), torch.from_numpy(out)) and torch.equal(d_expect[base:].cpu(), torch.from_numpy(expect))
        assert int(far_offsets.count_not(d_out, 0x5A, 0, base)) == 0 and int(far_offsets.count_not(d_expect, 0xA5, 0, base)) == 0
    finally:
        d_out = d_expect = None
        gc.collect()
        torch.cuda.empty_cache()


# ------------------------------------------------------------------ 4. behind every K1 path of a DeviceWorkload

def payload_for(oracle, raw, i):
    """A payload the coded bytes `raw` restore: the oracle's drop_stop_byte and tail_patch, slices in turn patched in place (the payload
    is as long as the coded body, its last byte another one) and with the last byte appended (one byte longer)."""
    body = oracle.drop_stop_byte(raw)
    if len(body) < 2:                                            # (a payload below two bytes is never patched)
        return body
    if i % 2:
        return oracle.tail_patch(body, (len(body) + 1) & 1, (i * 37 + 11) & 0xFF)
    return oracle.tail_patch(body, len(body) & 1, (i * 37 + 11) & 0xFF)


def changed(payload, p):
    b = bytearray(payload)
    b[p] ^= 0x5A
    return bytes(b)


@pytest.fixture(scope="module")
def workloads(oracle):
    """name -> (slices, the oracle's coded bytes, payloads they restore): A 200 short slices, B 4 slices long enough for K1p."""
    out = {}
    for name, counts, seed in (("A", [cvs.BIN_COUNTS[i % len(cvs.BIN_COUNTS)] for i in range(200)], 9400), ("B", cvs.LONG_COUNTS, 9401)):
        rng = np.random.default_rng(seed)
        slices = [oracle_lib.random_cabac_stream(rng, n, 20, terminate=bool(i % 2)) for i, n in enumerate(counts)]
        raws = [oracle.cabac_encode(r, s)[0] for r, s in slices]
        out[name] = (slices, raws, [payload_for(oracle, raw, i) for i, raw in enumerate(raws)])
    return out


PATHS = ["tiles", "narrow_tiles", "chunked", "chunked8", "slice_major", "resolved", "codes_serial"]


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("which", ["A", "B"])
def test_every_k1_path_of_a_workload_restores(avr, workloads, which, path):
    slices, raws, payloads = workloads[which]
    if path in ("narrow_tiles", "chunked8"):
        w = avr.DeviceWorkload.from_host(avr.KIND_CABAC8, [cvs.narrowed(r) for r, _ in slices], [s for _, s in slices],
                                         narrow_tiles=path == "narrow_tiles")
    else:
        w = avr.DeviceWorkload.from_host(avr.KIND_CABAC, [r for r, _ in slices], [s for _, s in slices])
    w.out.fill_(0xA5)
    if path in ("tiles", "narrow_tiles"):
        w.encode()
    elif path in ("chunked", "chunked8"):
        w.encode_chunked()
    elif path == "slice_major":
        w.encode_slice_major()
    else:
        codes = w.resolve()
        (w.encode_resolved if path == "resolved" else w.encode_codes_serial)(codes)
    got, status = w.results()
    assert not any(status) and got == raws
    status, fd = w.restore_check(payloads)
    assert (fd.cpu().numpy().view(np.uint32) == VERIFY_NONE).all() and not status.cpu().numpy().any()
    a, b = (3, 150) if which == "A" else (1, 2)                  # one expectation changed at byte 0, one at its last byte but one
    assert len(payloads[a]) >= 2 and len(payloads[b]) >= 2
    expect = list(payloads)
    expect[a], expect[b] = changed(payloads[a], 0), changed(payloads[b], len(payloads[b]) - 2)
    status, fd = w.restore_check(expect)
    fd, status = fd.cpu().numpy().view(np.uint32), status.cpu().numpy()
    for i in range(len(slices)):
        want = {a: 0, b: len(payloads[b]) - 2}.get(i, VERIFY_NONE)
        assert (fd[i], status[i]) == (want, VERIFY_FAILED if want != VERIFY_NONE else OK), f"slice {i}"
    assert w.results()[0] == raws                                # the bytes as the encoder left them


def test_restore_check_is_for_k1_workloads(avr):
    w = avr.DeviceWorkload.from_host(avr.KIND_RANGE, [oracle_lib.random_range_stream(np.random.default_rng(1), 50, adaptive=False)])
    w.encode()
    with pytest.raises(avr.AvrError, match="K1"):
        w.restore_check([b""])


# ------------------------------------------------------------------ 5. the batch API

@pytest.fixture(scope="module")
def batch_shapes(oracle):
    """shape -> (slices, the oracle's answers, codes, payloads, the slice whose expectation the tests change): 200 slices of at most 300
    bins (one lane per slice) and 5 slices of 9 000 to 20 000 bins (K1p by the batch's shape)."""
    mlps = oracle.tables()[1]
    rng = np.random.default_rng(9402)
    lanes = [oracle_lib.random_cabac_stream(rng, int(rng.integers(0, 301)), 20, terminate=bool(i % 2)) for i in range(200)]
    lanes[7] = (lanes[7][0][:0], lanes[7][1])
    lanes[78] = oracle_lib.random_cabac_stream(rng, 300, 20, terminate=True)
    k1p = [oracle_lib.random_cabac_stream(rng, int(rng.integers(9000, 20001)), 20, terminate=bool(i % 2)) for i in range(5)]
    out = {}
    for name, slices, k in (("lanes", lanes, 78), ("k1p", k1p, 3)):
        want = [oracle.cabac_encode(r, s) for r, s in slices]
        out[name] = (slices, want, [cvs.codes_of(r, s, mlps) for r, s in slices], [payload_for(oracle, d, i) for i, (d, _, _) in enumerate(want)], k)
    return out


def fill(b, kind, shape, expect=None):
    slices, _, codes, _, _ = shape
    for i, ((r, s), c) in enumerate(zip(slices, codes)):
        if kind == "cabac":
            b.add_slice_cabac(r, s)
        elif kind == "cabac8":
            b.add_slice_cabac8(cvs.narrowed(r), s)
        else:
            b.add_codes(c)
        if expect is not None and expect[i] is not None:
            b.expect(i, expect[i])


def run_batch(avr, kind, shape, expect=None, verify_k1=False):
    """One run: (results, final states, run_info, restore_ms, verify_ms, get_restore list, get_verify list)."""
    slices = shape[0]
    n = len(slices)
    with avr.Batch(0, n, sum(len(r) for r, _ in slices) + 16 * n + 64) as b:
        if verify_k1:
            b.set_verify_k1(True)
        fill(b, kind, shape, expect)
        b.submit()
        b.wait()
        return ([b.get(i) for i in range(n)], [b.get_states(i) for i in range(n)] if kind != "codes" else None, b.run_info(), b.restore_ms(),
                b.verify_ms(), [b.get_restore(i) for i in range(n)], [b.get_verify(i) for i in range(n)])


@pytest.mark.parametrize("verify_k1", [False, True], ids=["restore", "restore+verify_k1"])
@pytest.mark.parametrize("shape", ["lanes", "k1p"])
@pytest.mark.parametrize("kind", ["cabac", "cabac8", "codes"])
def test_batch_with_expectations(avr, batch_shapes, kind, shape, verify_k1):
    s = batch_shapes[shape]
    want, payloads, k = s[1], s[3], s[4]
    n = len(want)
    res_want = [(d, st) for d, _, st in want]
    finals = [f for _, f, _ in want] if kind != "codes" else None
    plain = run_batch(avr, kind, s, None, verify_k1)
    assert plain[0] == res_want and plain[1] == finals and plain[3] == 0.0 and plain[5] == [VERIFY_NONE] * n
    assert plain[2]["chunked"] == int(shape == "k1p")            # the K1 path this shape is meant to take did run
    on = run_batch(avr, kind, s, payloads, verify_k1)
    assert on[0] == plain[0] and on[1] == plain[1] and on[2]["chunked"] == plain[2]["chunked"]     # bytes, lengths, statuses, final states
    assert on[3] > 0.0 and on[5] == [VERIFY_NONE] * n and on[6] == [VERIFY_NONE] * n
    assert (on[4] > 0.0) == verify_k1                            # the K1 verifier's own answer and time beside the check's
    p = len(payloads[k]) // 2
    assert len(payloads[k]) >= 4
    expect = list(payloads)
    expect[k] = changed(payloads[k], p)
    bad = run_batch(avr, kind, s, expect, verify_k1)
    for i in range(n):
        if i == k:                                               # only it fails, at that byte, with its bytes as the encoder left them
            assert bad[0][i] == (want[i][0], VERIFY_FAILED) and bad[5][i] == p and bad[6][i] == VERIFY_NONE
        else:
            assert bad[0][i] == res_want[i] and bad[5][i] == VERIFY_NONE and bad[6][i] == VERIFY_NONE, f"slice {i}"
    assert bad[1] == finals and bad[3] > 0.0
    some = [payloads[i] if i % 3 == 0 else None for i in range(n)]                                  # slices without an expectation are skipped
    some[k] = expect[k]
    part = run_batch(avr, kind, s, some, verify_k1)
    assert part[5] == [p if i == k else VERIFY_NONE for i in range(n)] and part[0] == bad[0]


def test_reset_drops_the_expectations(avr, batch_shapes):
    s = batch_shapes["lanes"]
    payloads, k = s[3], s[4]
    n = len(payloads)
    expect = list(payloads)
    expect[k] = changed(payloads[k], 1)
    with avr.Batch(0, n, 100000) as b:
        fill(b, "codes", s, expect)
        b.run()
        assert b.restore_ms() > 0.0 and b.get_restore(k) == 1 and b.get(k)[1] == VERIFY_FAILED
        b.reset()
        fill(b, "codes", s)
        b.run()
        assert b.restore_ms() == 0.0 and b.get(k) == (s[1][k][0], OK)
        assert [b.get_restore(i) for i in range(n)] == [VERIFY_NONE] * n
        b.reset()                                                # ... and may be set anew
        fill(b, "codes", s, payloads)
        b.run()
        assert b.restore_ms() > 0.0 and [b.get_restore(i) for i in range(n)] == [VERIFY_NONE] * n and b.get(k)[1] == OK


def test_batch_expect_refusals(avr):
    rng = np.random.default_rng(9403)
    L = avr.lib()
    INVALID = -1
    one = (ctypes.c_uint8 * 8)()
    recs, states = oracle_lib.random_cabac_stream(rng, 500, 20)
    with avr.Batch(0, 4, 4096) as b:                             # a K2 batch
        b.add_slice_range(oracle_lib.random_range_stream(rng, 300, adaptive=False))
        assert L.avr_batch_expect(b._h, 0, one, 8) == INVALID and "K1" in L.avr_last_error().decode()
        b.run()
        assert b.get(0)[1] == OK and b.restore_ms() == 0.0 and b.get_restore(0) == VERIFY_NONE
    with avr.Batch(0, 4, 4096) as b:
        assert L.avr_batch_expect(b._h, 0, one, 8) == INVALID and "not been added" in L.avr_last_error().decode()     # nothing added yet
        b.add_slice_cabac(recs, states)
        assert L.avr_batch_expect(b._h, 1, one, 8) == INVALID and "not been added" in L.avr_last_error().decode()
        assert L.avr_batch_expect(b._h, 0, one, 0xFFFFFFFF) == INVALID and "too long" in L.avr_last_error().decode()
        assert L.avr_batch_expect(b._h, 0, one, 1 << 32) == INVALID
        assert L.avr_batch_expect(b._h, 0, None, 8) == INVALID
        assert L.avr_batch_expect(b._h, 0, one, 8) == 0
        assert L.avr_batch_expect(b._h, 0, one, 8) == INVALID and "already" in L.avr_last_error().decode()           # a second one
        b.submit()
        with pytest.raises(avr.AvrError, match="in flight"):
            b.expect(0, b"12345678")
        b.wait()
        assert b.get(0)[1] == VERIFY_FAILED and b.get_restore(0) != VERIFY_NONE and b.get_verify(0) == VERIFY_NONE


# ------------------------------------------------------------------ 6. the second runs of avr_batch_wait

def test_a_batch_that_wait_runs_again_is_checked_again(avr, oracle, hooks):
    """tests/test_gpu_cabac_verify.py's situation: a batch object whose first batch used 10 contexts and whose second uses 100, so that
    avr_batch_wait finds the guess too small and runs the batch again -- the restore check included; the answers are the last run's."""
    rng = np.random.default_rng(9405)
    mk = lambda n_used: [(r, np.concatenate([s, rng.integers(0, 126, 100 - n_used).astype(np.uint8)]))
                         for r, s in (oracle_lib.random_cabac_stream(rng, 30000 + 2000 * i, n_used) for i in range(5))]
    first, second = mk(10), mk(100)
    hooks(verify_flip=0)                                         # the hooks build, nothing flipped
    for verify_k1 in (False, True):
        with avr.Batch(0, 8, 400000) as b:
            b.set_verify_k1(verify_k1)
            for k, slices in enumerate((first, second)):
                if k:
                    b.reset()                                    # drops the expectations: set anew below
                want = [oracle.cabac_encode(r, s) for r, s in slices]
                payloads = [payload_for(oracle, d, i) for i, (d, _, _) in enumerate(want)]
                for i, (r, s) in enumerate(slices):
                    b.add_slice_cabac(r, s)
                    b.expect(i, changed(payloads[i], 100) if i == 1 else payloads[i])
                b.submit()
                b.wait()
                info = b.run_info()
                assert info["chunked"] == 1 and (info["ran_again"] & 1) == k, info
                for i in range(len(slices)):
                    assert b.get(i) == (want[i][0], VERIFY_FAILED if i == 1 else OK) and b.get_states(i) == want[i][1], f"batch {k} slice {i}"
                    assert b.get_restore(i) == (100 if i == 1 else VERIFY_NONE) and b.get_verify(i) == VERIFY_NONE
                assert b.restore_ms() > 0.0 and (b.verify_ms() > 0.0) == verify_k1
                t = b.timings()
                assert all(v >= 0.0 for v in t.values()) and t["encode_ms"] > 0.0, t


def test_the_second_pass_from_wait_is_checked_too(avr, oracle, hooks):
    """tests/test_gpu_parity.py's second-pass batch: a slice with single bins in contexts the sampled census misses is coded by
    avr_batch_wait's second pass when the run was sized by a guess -- behind the restore check of the run, which skipped it.  The check
    follows the second pass too, and a slice it failed in front of the pass keeps its bytes and fails again at the same byte."""
    rng = np.random.default_rng(31)
    slices = []
    for i in range(5):
        r, s = oracle_lib.random_cabac_stream(rng, 30000 + 3000 * i, 50)
        slices.append((r, np.concatenate([s, rng.integers(0, 126, 150).astype(np.uint8)])))
    slices[3][0][12345] = np.uint16((199 << 1) | 1)
    slices[3][0][20001] = np.uint16((77 << 1) | 0)
    want = [oracle.cabac_encode(r, s) for r, s in slices]
    payloads = [payload_for(oracle, d, i) for i, (d, _, _) in enumerate(want)]
    hooks(verify_flip=0)
    for verify_k1, bad_slice in ((False, 0), (True, 3)):         # a finding in a slice of the first pass; in the second pass's own slice
        with avr.Batch(0, 8, 400000) as b:
            b.set_verify_k1(verify_k1)
            for i, (r, s) in enumerate(slices):
                b.add_slice_cabac(r, s)
                b.expect(i, changed(payloads[i], 7) if i == bad_slice else payloads[i])
            for run in range(2):
                b.submit()
                b.wait()
                info = b.run_info()
                assert info["chunked"] == 1 and bool(info["ran_again"] & 2) == (run == 1)
                for i in range(5):
                    assert (b.get(i), b.get_states(i)) == ((want[i][0], VERIFY_FAILED if i == bad_slice else OK), want[i][1]), f"run {run} slice {i}"
                    assert b.get_restore(i) == (7 if i == bad_slice else VERIFY_NONE) and b.get_verify(i) == VERIFY_NONE
                assert b.restore_ms() > 0.0 and (b.verify_ms() > 0.0) == verify_k1
                t = b.timings()                                  # the second pass: the checks in front of it are taken off the encode's slot
                assert all(v >= 0.0 for v in t.values()) and t["encode_ms"] > 0.0, t


# ------------------------------------------------------------------ 7. the command line

@pytest.fixture(scope="module")
def recode(avr):
    return avr.build_recode()


@pytest.mark.parametrize("others", [{}, {"AVR_DEVICE_ESTIMATORS": "1", "AVR_VERIFY": "1"}], ids=["alone", "device_estimators+verify"])
@pytest.mark.parametrize("name", ["cockatoo.mp4", "realshort.mp4"])
def test_cli_compress_with_the_restore_check_writes_the_same_bytes(recode, tmp_path, name, others):
    from test_h264 import clip
    files = {}
    for tag, env in (("plain", {}), ("restore", {"AVR_VERIFY_RESTORE": "1"})):
        out = tmp_path / f"{tag}.recode"
        run = subprocess.run([recode, "compress", clip(name), str(out)], capture_output=True, text=True, timeout=600,
                             env=dict(os.environ, AVR_TIMING="1", **others, **env))
        assert run.returncode == 0, run.stderr
        assert ("compress: GPU restore check (K1)" in run.stderr) == ("compress: restore check kernel" in run.stderr) == (tag == "restore"), run.stderr
        files[tag] = out.read_bytes()
    assert len(files["plain"]) > 0 and files["restore"] == files["plain"]


def test_cli_with_all_eleven_hooks(recode, tmp_path):
    from test_h264 import clip
    files = {}
    for tag, env in (("plain", {}), ("restore", {"AVR_VERIFY_RESTORE": "1"})):
        out = tmp_path / f"{tag}.recode"
        run = subprocess.run([recode, "roundtrip", clip("realshort.mp4"), str(out)], capture_output=True, text=True, timeout=600,
                             env=dict(os.environ, AVR_MODEL_HOOKS="1", **env))
        assert run.returncode == 0 and "Compress-decompress roundtrip succeeded:" in run.stderr, run.stderr
        files[tag] = out.read_bytes()
    assert len(files["plain"]) > 0 and files["restore"] == files["plain"]


def test_cli_test_directory_over_four_files(recode, tmp_path):
    from test_h264 import CLIPS, clip
    dirs = {}
    for tag, env in (("plain", {}), ("restore", {"AVR_VERIFY_RESTORE": "1", "AVR_TIMING": "1"})):
        d = dirs[tag] = tmp_path / tag
        d.mkdir()
        for k in range(2):
            for name in CLIPS:
                shutil.copy(clip(name), d / f"{k}_{name}")
        run = subprocess.run([recode, "test", str(d)], capture_output=True, text=True, timeout=900, env=dict(os.environ, **env))
        assert run.returncode == 0 and "failed on" not in run.stdout, run.stderr + run.stdout
        if tag == "restore":                                     # one restore batch for the window's four files
            assert run.stderr.count("compress: GPU restore check (K1)") == 1 and run.stderr.count("compress: restore check kernel") == 1
    names = sorted(p.name for p in dirs["plain"].iterdir() if p.is_file())
    assert len(names) == 4
    for name in names:
        got, want = (dirs["restore"] / "output" / name).read_bytes(), (dirs["plain"] / "output" / name).read_bytes()
        assert got == want and len(got) > 0, name
    assert (dirs["restore"] / "output" / "log.txt").read_text().count("Compress-decompress roundtrip succeeded:") == 4
