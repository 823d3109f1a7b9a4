"""GPU: the replay's state chain as k_k1p_replay runs it (replay_step8 of csrc/avr_k1p.h: bin j+1's state byte read before bin j's
write-back, bin j's successor handed on where the two share a slot of the lane's column) on the streams of
tests/replay_chain_streams.py, which tests/test_k1p_replay_step_emul.py walks on the CPU: neighbours in one context at every place
of a group -- so also across every 64-byte line of records, across the chunks and in the tail a lane walks past its chunk --, A B A B,
runs, a context through pStateIdx 0 and parked at 62, the pseudo contexts, every state with its successor handed on, random bins
over 2 and 86 contexts; slices of 3 * 1024, 3 * 1024 - 5, 1024 + 9, 700 and 5 bins, whose last group is masked where the length is
no multiple of eight.

Two batches: the streams over four contexts (where the padding's slot and context 3 lie at the same place of their rows of four),
and the wider ones.  Each is coded once by the one-lane-per-slice kernel (k_cabac_encode), which the oracle confirms, and then by
the intra-slice parallel kernels from two-byte records (avr_cabac_encode_chunked_device), from one-byte records
(avr_cabac8_encode_chunked_device, the bytes behind a slice's last record holding context 3's selector) and in two stages
(avr_cabac_resolve_device, which is the replay writing slice-major codes, then avr_cabac_encode_resolved_device): bytes, lengths,
statuses and final states are the same, and the resolved codes are the CPU's."""
import numpy as np
import pytest

import replay_chain_streams as rs
from test_gpu_parity import to_records8

pytestmark = pytest.mark.gpu

BATCHES = {"four": lambda s: s.states.size == 4, "wide": lambda s: s.states.size != 4}
_made = {}


def prepared(avr, oracle, name):
    """The batch's slices (records, resolved codes, initial states) and what the one-lane-per-slice kernel codes them to: made once,
    shared by the tests, never changed."""
    if name not in _made:
        _, mlps = avr.cabac_tables()
        streams = [s for s in rs.device_streams() if BATCHES[name](s)]
        n_states = max(s.states.size for s in streams)
        slices = [(*s.resolve(list(mlps)), np.concatenate([s.states, np.zeros(n_states - s.states.size, np.uint8)])) for s in streams]
        w = avr.DeviceWorkload.from_host(avr.KIND_CABAC, [r for r, _, _ in slices], [st for _, _, st in slices], 0)
        w.encode()
        data, status = w.results()
        assert not any(status)
        for i, (r, _, st) in enumerate(slices):
            want = oracle.cabac_encode(r, st)
            assert data[i] == want[0], f"{name}: the one-lane-per-slice kernel and the oracle differ on slice {i} ({streams[i].name})"
        serial = (data, w.out_len.cpu().numpy().copy(), w.final_states.cpu().numpy().reshape(len(slices), -1).copy())
        _made[name] = (streams, slices, serial, n_states)
    return _made[name]


def same_as_serial(name, prep, w, final_states=True):
    streams, _, (data, out_len, final), n_states = prep
    got, status = w.results()
    assert not any(status), f"{name}: statuses {status}"
    assert (w.out_len.cpu().numpy() == out_len).all()
    for i, s in enumerate(streams):
        assert got[i] == data[i], f"{name}: slice {i} ({s.name}, {s.syms.size} bins)"
    if final_states:
        assert (w.final_states.cpu().numpy().reshape(len(streams), -1)[:, :n_states] == final[:, :n_states]).all()


@pytest.mark.parametrize("name", list(BATCHES))
def test_two_byte_records(avr, oracle, name):
    prep = prepared(avr, oracle, name)
    w = avr.DeviceWorkload.from_host(avr.KIND_CABAC, [r for r, _, _ in prep[1]], [st for _, _, st in prep[1]], 0)
    w.encode_chunked()
    same_as_serial(name, prep, w)


@pytest.mark.parametrize("name", list(BATCHES))
def test_one_byte_records(avr, oracle, name):
    prep = prepared(avr, oracle, name)
    w = avr.DeviceWorkload.from_host(avr.KIND_CABAC8, [to_records8(r) for r, _, _ in prep[1]], [st for _, _, st in prep[1]], 0,
                                     pad_bytes=np.array([3 << 1 | 1], np.uint8))
    w.encode_chunked()
    same_as_serial(name, prep, w)


@pytest.mark.parametrize("name", list(BATCHES))
def test_resolved_codes(avr, oracle, name):
    """Stage 1 is the replay writing its codes slice-major; they are the codes the CPU test walks.  Stage 2 codes from them."""
    prep = prepared(avr, oracle, name)
    w = avr.DeviceWorkload.from_host(avr.KIND_CABAC, [r for r, _, _ in prep[1]], [st for _, _, st in prep[1]], 0)
    codes = w.resolve()
    host, res_off = codes.cpu().numpy(), w._plan["tensors"]["res_off"].cpu().numpy()
    for i, (_, c, _) in enumerate(prep[1]):
        assert np.array_equal(host[int(res_off[i]):int(res_off[i]) + c.size], c), f"{name}: codes of slice {i} ({prep[0][i].name})"
    w.out.zero_(); w.out_len.zero_()
    w.encode_resolved(codes)
    same_as_serial(name, prep, w, final_states=False)
