"""GPU: phase B1 as k_k1p_replay and k_k1p_b1 walk it (B1Walk of csrc/avr_k1p.h) on the streams of tests/b1walk_streams.py, whose
coded LPS bins are placed bin by bin: the opening bin at every place of a group, the closing bin at every place of a tail group, none
of either, candidates that meet at once and never, slices of 3 * 1024, 3 * 1024 - 5, 1024 + 9 and 700 bins and shorter ones.  The
same streams as tests/test_k1p_b1walk_emul.py walks on the CPU, here as records over ten contexts, so that k_k1p_local and the chains
have next to nothing to do and what decides the bytes is the stretch summaries.

Every batch is coded once by the one-lane-per-slice kernel (k_cabac_encode), which the oracle confirms, and then by the intra-slice
parallel kernels from two-byte records (avr_cabac_encode_chunked_device), from one-byte records (avr_cabac8_encode_chunked_device) and
from resolved codes (avr_cabac_encode_resolved_device, which is k_k1p_b1): bytes, lengths, statuses and final states are the same.
A wave's 64 lanes are 64 consecutive chunks of the batch, about 25 slices: in every batch here a wave holds lanes that are looking,
on four candidates and merged at once, and in the batch of 64 mixed slices every eighth slice keeps its lanes looking for 300 bins."""
import numpy as np
import pytest

import b1walk_streams as bs
from test_gpu_parity import to_records8

pytestmark = pytest.mark.gpu

BATCHES = {"constructed": lambda t: bs.constructed(*t), "random": lambda t: bs.random_streams(), "mix": lambda t: bs.wave_mix()}
_made = {}


def prepared(avr, oracle, name):
    """The batch's slices (records, initial states, resolved codes) and what the one-lane-per-slice kernel codes them to: made once,
    shared by the tests, never changed."""
    if name not in _made:
        lps_range, mlps = avr.cabac_tables()
        streams = BATCHES[name]((list(lps_range), list(mlps)))
        slices = [(*s.resolve(list(mlps)), s.states) for s in streams]
        w = avr.DeviceWorkload.from_host(avr.KIND_CABAC, [r for r, _, _ in slices], [st for _, _, st in slices], 0)
        w.encode()
        data, status = w.results()
        assert not any(status)
        for i, (r, _, st) in enumerate(slices):
            want = oracle.cabac_encode(r, st)
            assert data[i] == want[0], f"{name}: the one-lane-per-slice kernel and the oracle differ on slice {i} ({streams[i].name})"
        serial = (data, w.out_len.cpu().numpy().copy(), w.final_states.cpu().numpy().reshape(len(slices), -1).copy())
        _made[name] = (streams, slices, serial)
    return _made[name]


def same_as_serial(name, streams, serial, w, final_states=True):
    data, out_len, final = serial
    got, status = w.results()
    assert not any(status), f"{name}: statuses {status}"
    assert (w.out_len.cpu().numpy() == out_len).all()
    for i, s in enumerate(streams):
        assert got[i] == data[i], f"{name}: slice {i} ({s.name}, {s.syms.size} bins)"
    if final_states:
        assert (w.final_states.cpu().numpy().reshape(len(streams), -1)[:, :bs.N_CTX] == final[:, :bs.N_CTX]).all()


@pytest.mark.parametrize("name", list(BATCHES))
def test_two_byte_records(avr, oracle, name):
    streams, slices, serial = prepared(avr, oracle, name)
    w = avr.DeviceWorkload.from_host(avr.KIND_CABAC, [r for r, _, _ in slices], [st for _, _, st in slices], 0)
    w.encode_chunked()
    same_as_serial(name, streams, serial, w)


@pytest.mark.parametrize("name", list(BATCHES))
def test_one_byte_records(avr, oracle, name):
    streams, slices, serial = prepared(avr, oracle, name)
    w = avr.DeviceWorkload.from_host(avr.KIND_CABAC8, [to_records8(r) for r, _, _ in slices], [st for _, _, st in slices], 0)
    w.encode_chunked()
    same_as_serial(name, streams, serial, w)


@pytest.mark.parametrize("name", list(BATCHES))
def test_resolved_codes(avr, oracle, name):
    """Stage 1 gives the codes the CPU test walks; stage 2 from them is k_k1p_b1."""
    streams, slices, serial = prepared(avr, oracle, name)
    w = avr.DeviceWorkload.from_host(avr.KIND_CABAC, [r for r, _, _ in slices], [st for _, _, st in slices], 0)
    codes = w.resolve()
    host, res_off = codes.cpu().numpy(), w._plan["tensors"]["res_off"].cpu().numpy()
    for i, (_, c, _) in enumerate(slices):
        assert np.array_equal(host[int(res_off[i]):int(res_off[i]) + c.size], c), f"{name}: codes of slice {i}"
    w.out.zero_(); w.out_len.zero_()
    w.encode_resolved(codes)
    same_as_serial(name, streams, serial, w, final_states=False)


@pytest.mark.parametrize("name", ["constructed", "mix"])
def test_no_slice_is_handed_over(avr, oracle, hooks, name):
    """With the serial kernel behind phase D left out (test hook k1p_keep_retry) every slice is still coded: the bytes above are the
    parallel kernels' own, made from their stretch summaries."""
    streams, slices, serial = prepared(avr, oracle, name)
    hooks(k1p_keep_retry=1)
    w = avr.DeviceWorkload.from_host(avr.KIND_CABAC, [r for r, _, _ in slices], [st for _, _, st in slices], 0)
    w.encode_chunked()
    same_as_serial(name, streams, serial, w)
