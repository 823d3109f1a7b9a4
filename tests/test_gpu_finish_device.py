"""avr_finish_device on the GPU: the way back's epilogue -- stop byte, tail patch, emulation prevention -- as a dense copy.

Inputs are crafted bytes; `out`, `dense`, dense_off and the workspace sit in tests/guarded.py buffers of exactly the sizes stated or
quoted, every call runs on a stream of its own and with two poisons, and no guard byte may change.  Every expected answer is
tests/finish_ref.py's: the oracle's drop_stop_byte and tail_patch, then the escape rule in plain Python.  Exact equality throughout."""
import ctypes

import numpy as np
import pytest

import finish_ref
import guarded
from test_gpu_plan_device import POISONS, _own_stream, compact_case, prefix, run_compact

pytestmark = pytest.mark.gpu

OK, ERR_INVALID = 0, -1
SLICE_OK = 0


def lay_out(slices, slack=None, first=0):
    """Regions of roundup8(len) + slack[i] * 8 bytes, one behind the other from `first` (a multiple of 8): (out, out_off, out_len);
    what lies outside the slices' bytes is 0x00 -- bytes that would change an escape count if they were read as the slice's."""
    slack = slack if slack is not None else [0] * len(slices)
    cap = np.array([(len(s) + 7) // 8 * 8 + 8 * k for s, k in zip(slices, slack)], np.int64)
    out_off = first + prefix(cap)
    out = np.zeros(int(out_off[-1]), np.uint8)
    for s, o in zip(slices, out_off):
        out[o:o + len(s)] = np.frombuffer(s, np.uint8)
    return out, out_off, np.array([len(s) for s in slices], np.int64)


def expected(oracle, slices, words, status=None):
    parts = [finish_ref.finished(oracle, s, int(w)) if status is None or status[i] == SLICE_OK else b"" for i, (s, w) in enumerate(zip(slices, words))]
    return parts, prefix([len(p) for p in parts])


def run_finish(avr, torch, out, out_off, out_len, words, capacity, poison, status=None, dense=None, check=None):
    """One avr_finish_device call on a stream of its own: (dense, dense_off) as numpy.  out: numpy bytes, placed in a guarded buffer of
    exactly their size.  dense: the caller's own uint8 view of `capacity` bytes, of any alignment, inside a buffer the caller guards."""
    L = avr.lib()
    n = len(out_len)
    bufs = guarded.Buffers()
    if dense is None:
        dense = bufs.add("dense", capacity, "cuda").view
    assert dense.numel() == capacity
    dense_off = bufs.add("dense_off", 8 * (n + 1), "cuda")
    ws = bufs.add("ws", L.avr_finish_workspace_bytes(n), "cuda")
    for x in bufs.all.values():
        x.view.fill_(poison)
    d_out = bufs.add("out", len(out), "cuda")
    d_out.view.copy_(torch.from_numpy(out))
    d_off = torch.from_numpy(np.asarray(out_off, np.int64)).cuda()
    d_len = torch.from_numpy(np.asarray(out_len).astype(np.uint32).view(np.int32)).cuda()
    d_words = torch.from_numpy(np.asarray(words).astype(np.uint32).view(np.int32)).cuda()
    d_status = None if status is None else torch.from_numpy(np.asarray(status, np.int32)).cuda()
    stream = _own_stream(torch, None)
    with torch.cuda.stream(stream):
        rc = L.avr_finish_device(0, ctypes.c_void_p(stream.cuda_stream), d_out.view.data_ptr(), d_off.data_ptr(), d_len.data_ptr(),
                                 None if d_status is None else d_status.data_ptr(), n, d_words.data_ptr(), dense.data_ptr(), capacity,
                                 dense_off.view.data_ptr(), ws.view.data_ptr(), ws.n)
    assert rc == OK, L.avr_last_error()
    stream.synchronize()
    bufs.check()
    if check is not None:
        check()
    assert np.array_equal(d_out.view.cpu().numpy(), out)             # the input is read, never written
    return dense.cpu().numpy(), dense_off.view.cpu().numpy().view(np.int64)


def hold(avr, torch, oracle, slices, words, status=None, slack=None, out_len=None, first=0):
    """The call with a capacity that is exactly met, under both poisons: every slice's bytes and every offset are the reference's."""
    out, out_off, lens = lay_out(slices, slack, first)
    parts, want_off = expected(oracle, slices, words, status)
    want = np.frombuffer(b"".join(parts), np.uint8)
    for poison in POISONS:
        dense, dense_off = run_finish(avr, torch, out, out_off, lens if out_len is None else out_len, words, int(want_off[-1]), poison, status)
        assert np.array_equal(dense_off, want_off)
        bad = np.flatnonzero(dense != want)
        assert bad.size == 0, f"first differing byte {bad[0]}, in slice {np.searchsorted(want_off, bad[0], 'right') - 1}"
    return parts, want_off


def crafted(rng, n):
    """n bytes in which zeros, small values and 0x80 are common."""
    return bytes(rng.choice(np.array([0, 0, 0, 1, 2, 3, 4, 0x80, 0xFF], np.uint8), n).tolist())


LENGTHS = (0, 1, 2, 3, 7, 8, 9, 511, 512, 513, 1025)


def test_every_length_parity_and_patch(avr, oracle):
    """The lengths around a lane's word and a trip, each with every finish word of the table -- no patch, the patch at either parity
    with last bytes that make, need and leave escapes, plain and escaped at every z -- with and without the stop byte."""
    import torch
    rng = np.random.default_rng(11)
    slices, words = [], []
    for n in LENGTHS:
        for w in finish_ref.words():
            for stop in (False, True):
                body = crafted(rng, n)
                if n and not stop and body[-1] == 0x80:
                    body = body[:-1] + b"\x04"
                slices.append(body + (b"\x80" if stop else b""))
                words.append(w)
    assert len(slices) == len(LENGTHS) * 29 * 2
    hold(avr, torch, oracle, slices, words, slack=[i % 3 for i in range(len(slices))], first=8)


@pytest.fixture(scope="module")
def seam_case(oracle):
    """About 4 400 slices of 1 200 bytes of 0xFF, each with a run of 2, 3, 4 or 5 zeros and an 01 behind it, the run starting at every
    offset 0 .. 1099: every lane and trip seam, whatever run length the kernel chose.  z and the patch go round with the index."""
    slices, words = [], []
    for run in (2, 3, 4, 5):
        for at in range(1100):
            body = bytearray(b"\xff" * 1200)
            body[at:at + run + 1] = b"\x00" * run + b"\x01"
            i = len(slices)
            slices.append(bytes(body))
            words.append(finish_ref.word(0x00, i & 1, i % 5 == 0, True, i % 3))
    return slices, words, expected(oracle, slices, words)


def test_zero_runs_at_every_offset(avr, seam_case):
    import torch
    slices, words, (parts, want_off) = seam_case
    out, out_off, lens = lay_out(slices)
    want = np.frombuffer(b"".join(parts), np.uint8)
    assert len(slices) == 4400 and sum(len(p) for p in parts) > sum(map(len, slices)) + 4400       # every slice grew
    dense, dense_off = run_finish(avr, torch, out, out_off, lens, words, int(want_off[-1]), POISONS[1])
    assert np.array_equal(dense_off, want_off) and np.array_equal(dense, want)


def test_the_most_a_slice_can_grow(avr, oracle):
    """All zeros: an escape for every two bytes, the first after 2 - z.  With the last byte appended that is L + 1 + (L + z) / 2 bytes,
    within the header's bound of L + 1 + (L + 1 + z) / 2."""
    import torch
    slices, words = [], []
    for z in (0, 1, 2):
        slices += [bytes(2000), bytes(2000), bytes(1999)]
        words += [finish_ref.word(escaped=True, zeros_before=z), finish_ref.word(0x00, 1, True, True, z), finish_ref.word(0x00, 0, True, True, z)]
    parts, _ = hold(avr, torch, oracle, slices, words)
    for s, w, p in zip(slices, words, parts):
        z = (w >> 11) & 3
        assert len(p) <= len(s) + 1 + (len(s) + 1 + z) // 2 and set(p) <= {0, 3}
    assert [len(p) for p in parts] == [2000 + 999, 2001 + 1000, 2000 + 999,              # z = 0
                                       2000 + 1000, 2001 + 1000, 2000 + 1000,            # z = 1
                                       2000 + 1000, 2001 + 1001, 2000 + 1000]            # z = 2


def test_lengths_above_the_region_and_unsound_slices(avr, oracle):
    """out_len above its region is clamped as compaction clamps it -- the slice is then its region's bytes -- and a slice whose status
    is not AVR_SLICE_OK gives nothing, between slices that do."""
    import torch
    rng = np.random.default_rng(12)
    slices = [crafted(rng, int(n)) for n in rng.integers(0, 700, 60)]
    slices = [s + bytes((-len(s)) % 8) for s in slices]             # whole regions: what a clamped length takes
    words = [finish_ref.words()[i % 29] for i in range(len(slices))]
    out_len = np.array([len(s) for s in slices], np.int64)
    out_len[::4] += rng.integers(1, 5000, len(out_len[::4]))
    out_len[7] = 0xFFFFFFFF
    status = np.zeros(len(slices), np.int32)
    status[[0, 5, 6, 20, 59]] = [1, 2, 3, 4, 1]
    hold(avr, torch, oracle, slices, words, status=status, out_len=out_len)
    hold(avr, torch, oracle, slices, words, status=None, out_len=out_len)


@pytest.mark.parametrize("n", [0, 1, 1030])
def test_slice_counts(avr, oracle, n):
    """None, one, and more than one tile of the scan."""
    import torch
    rng = np.random.default_rng(13 + n)
    slices = [crafted(rng, int(k)) for k in rng.integers(0, 40, n)]
    words = [finish_ref.words()[(3 * i) % 29] for i in range(n)]
    if n:
        hold(avr, torch, oracle, slices, words)
    else:
        dense, dense_off = run_finish(avr, torch, np.zeros(0, np.uint8), np.zeros(1, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64), 16, 0x33)
        assert dense_off.tolist() == [0] and (dense == 0x33).all()


def test_dense_at_all_eight_alignments(avr, oracle):
    import torch
    rng = np.random.default_rng(14)
    slices = [crafted(rng, int(k)) for k in list(range(0, 20)) + [100, 511, 513, 1025, 64, 3]]
    words = [finish_ref.words()[(5 * i) % 29] for i in range(len(slices))]
    out, out_off, lens = lay_out(slices)
    parts, want_off = expected(oracle, slices, words)
    want, total = np.frombuffer(b"".join(parts), np.uint8), int(want_off[-1])
    for shift in range(8):
        g = guarded.Guarded(total + 8, "cuda", "dense")
        g.view.fill_(0x5A)
        view = g.view[shift:shift + total]
        dense, dense_off = run_finish(avr, torch, out, out_off, lens, words, total, 0x5A, dense=view, check=g.check)
        assert np.array_equal(dense_off, want_off) and np.array_equal(dense, want), shift
        rest = g.view.cpu().numpy()
        assert (rest[:shift] == 0x5A).all() and (rest[shift + total:] == 0x5A).all(), shift


def test_a_capacity_that_cuts_off_the_last_three_slices(avr, oracle):
    """dense_off is complete, the slices are whole or absent, nothing at or past the capacity is written."""
    import torch
    rng = np.random.default_rng(15)
    slices = [crafted(rng, int(k)) + b"\x00\x00\x01" for k in rng.integers(50, 900, 40)]
    words = [finish_ref.word(0x01, i & 1, True, True, i % 3) for i in range(len(slices))]
    out, out_off, lens = lay_out(slices)
    parts, want_off = expected(oracle, slices, words)
    want = np.frombuffer(b"".join(parts), np.uint8)
    k = len(slices) - 3
    capacity = int(want_off[k] + len(parts[k]) - 1)                 # one byte short of slice k: it and the two behind it stay away
    for poison in POISONS:
        dense, dense_off = run_finish(avr, torch, out, out_off, lens, words, capacity, poison)
        assert np.array_equal(dense_off, want_off) and dense_off[-1] > capacity
        assert np.array_equal(dense[:want_off[k]], want[:want_off[k]])
        assert (dense[want_off[k]:] == poison).all()
    dense, dense_off = run_finish(avr, torch, out, out_off, lens, words, 0, 0x33)
    assert np.array_equal(dense_off, want_off) and dense.size == 0


def test_all_zero_words_are_compaction(avr):
    """Where every word of `finish` is 0 and no slice ends on 0x80, the call is avr_compact_device: the same offsets, the same bytes."""
    import torch
    out, out_off, out_len = compact_case()
    take = np.minimum(out_len, np.diff(out_off))
    for i in np.flatnonzero(take > 0):
        last = out_off[i] + take[i] - 1
        if out[last] == 0x80:
            out[last] = 0x81
    total = int(take.sum())
    for poison in POISONS:
        c_dense, c_off = run_compact(avr, torch, torch.from_numpy(out).cuda(), out_off, out_len, total, poison)
        dense, dense_off = run_finish(avr, torch, out, out_off, out_len, np.zeros(len(out_len), np.int64), total, poison)
        assert np.array_equal(dense_off, c_off) and np.array_equal(dense, c_dense)


def test_a_real_encode_finished_on_the_device(avr, oracle):
    """Config 5 at a few hundred slices, coded, then DeviceWorkload.results_finished against the host rule slice by slice."""
    w = avr.DeviceWorkload.synth(5, 300, avr.KIND_CABAC, 0, 1000)
    w.encode()
    coded, status = w.results()
    assert not any(status) and sum(map(len, coded)) > 0
    words = [finish_ref.word(0x01 if i % 7 else 0x00, i & 1, i % 4 != 3, i % 2 == 0, i % 3) for i in range(w.n_slices)]
    dense, dense_off = w.results_finished(words)
    dense, dense_off = dense.cpu().numpy(), dense_off.cpu().numpy()
    assert dense_off[0] == 0 and dense_off[-1] == dense.size
    for i, (c, wd) in enumerate(zip(coded, words)):
        assert dense[dense_off[i]:dense_off[i + 1]].tobytes() == finish_ref.finished(oracle, c, wd), i
    assert any(finish_ref.finished(oracle, c, wd) != c for c, wd in zip(coded, words))


def test_refusals(avr):
    """What avr_compact_device refuses, and the same of `finish` and `status`: AVR_ERR_INVALID, with a message, and nothing written."""
    import torch
    L = avr.lib()
    n = 3
    quote = L.avr_finish_workspace_bytes(n)
    assert quote >= 8 * n and quote % 256 == 0 and L.avr_finish_workspace_bytes(0) > 0
    bufs = guarded.Buffers()
    names = dict(out=64, out_off=8 * (n + 1), out_len=4 * n, status=4 * n, finish=4 * n, dense=64, dense_off=8 * (n + 1), ws=quote)
    for k, size in names.items():
        bufs.add(k, size, "cuda").view.fill_(0x77)
    P = {k: bufs.all[k].view.data_ptr() for k in names}

    def call(n=n, ws_bytes=quote, cap=64, **over):
        p = dict(P, **over)
        return L.avr_finish_device(0, None, p["out"], p["out_off"], p["out_len"], p["status"], n, p["finish"], p["dense"], cap, p["dense_off"],
                                   p["ws"], ws_bytes)
    refused = {
        "null out": call(out=None), "null out_off": call(out_off=None), "null out_len": call(out_len=None), "null finish": call(finish=None),
        "null dense": call(dense=None), "null dense_off": call(dense_off=None), "null workspace": call(ws=None),
        "out_off + 4": call(out_off=P["out_off"] + 4), "out_len + 2": call(out_len=P["out_len"] + 2), "status + 2": call(status=P["status"] + 2),
        "finish + 2": call(finish=P["finish"] + 2), "dense_off + 4": call(dense_off=P["dense_off"] + 4), "workspace + 64": call(ws=P["ws"] + 64),
        "workspace one byte short": call(ws_bytes=quote - 1), "n_slices 2^31": call(n=1 << 31, ws_bytes=1 << 40),
    }
    for label, rc in refused.items():
        assert rc == ERR_INVALID, label
    assert L.avr_last_error() != b""
    torch.cuda.synchronize()
    bufs.check()
    for k in names:
        assert (bufs.all[k].view == 0x77).all(), k
