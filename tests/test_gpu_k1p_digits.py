"""GPU: the digit path of K1p's phase C.  k_k1p_c takes the digits of four bins without a loop, stages them per lane in LDS and
empties the stage where the wave's lanes are together (csrc/avr_k1p.hip, DeviceAdder).  The streams of tests/digit_streams.py --
the extreme rates side by side in one wave, long random slices, lengths around the path boundaries, carry chains through digits
taken as a pair -- through the chunked call and the two-part call: bytes, lengths, statuses and final states against the oracle and
against the one-lane-per-slice kernel; and the hand-over from phase D to the serial kernels."""
import numpy as np
import pytest

import digit_streams

pytestmark = pytest.mark.gpu

_cache = {}


def _group(avr, oracle, name):
    """(slices, the oracle's answers, the one-lane-per-slice kernel's bytes / final states / statuses): once per group."""
    if name not in _cache:
        import torch
        slices = digit_streams.GROUPS[name]()
        wants = [oracle.cabac_encode(r, s) for r, s in slices]
        w = avr.DeviceWorkload.from_host(avr.KIND_CABAC, [r for r, _ in slices], [s for _, s in slices], 0)
        w.encode(); torch.cuda.synchronize()
        w.settle()
        got, status = w.results()
        _cache[name] = (slices, wants, (got, w.final_states.cpu().numpy().copy(), status))
    return _cache[name]


@pytest.mark.parametrize("parts", [1, 2])
@pytest.mark.parametrize("group", sorted(digit_streams.GROUPS))
def test_digit_streams_on_the_kernels(avr, oracle, group, parts):
    import torch
    slices, wants, (serial, serial_fs, serial_status) = _group(avr, oracle, group)
    w = avr.DeviceWorkload.from_host(avr.KIND_CABAC, [r for r, _ in slices], [s for _, s in slices], 0)
    if parts > 1:
        assert w.set_parts(parts) == parts
    for run in ("asked", "hinted"):                          # the second run is sized by what the first reported, as bench.py's steps are
        w.encode_chunked(); torch.cuda.synchronize()
        w.settle()
        got, status = w.results()
        lens = w.out_len.cpu().numpy()
        fs = w.final_states.cpu().numpy()
        for i, (data, final, st) in enumerate(wants):
            what = f"{group}, {parts} part(s), {run}: slice {i} of {len(slices[i][0])} bins"
            assert status[i] == st == serial_status[i] == 0, what
            assert int(lens[i]) == len(data), what
            assert got[i] == data and got[i] == serial[i], what
            assert fs.reshape(len(slices), -1)[i].tobytes() == final, what
        assert np.array_equal(fs, serial_fs)
        w.out.zero_(); w.out_len.zero_(); w.final_states.zero_()


@pytest.mark.parametrize("every", [1, 3])
def test_hand_over_still_codes_what_phase_d_declines(avr, oracle, hooks, every):
    """Test hook k1p_force_retry_every: phase D hands every n-th slice to the serial kernel -- from records and from resolved
    codes -- whatever phase C added into its sums."""
    hooks(k1p_force_retry_every=every)
    slices = digit_streams.random_long()[:3] + digit_streams.carry_chains()[:2] + digit_streams.rate_extremes()[:3]
    _, w_random, _ = _group(avr, oracle, "random-long")
    _, w_carry, _ = _group(avr, oracle, "carry-chains")
    _, w_rates, _ = _group(avr, oracle, "rate-extremes")
    wants = w_random[:3] + w_carry[:2] + w_rates[:3]
    w = avr.DeviceWorkload.from_host(avr.KIND_CABAC, [r for r, _ in slices], [s for _, s in slices], 0)
    w.encode_chunked()
    got, status = w.results()
    fs = w.final_states.cpu().numpy().reshape(len(slices), -1)
    for i, (data, final, st) in enumerate(wants):
        assert status[i] == st == 0 and got[i] == data and fs[i].tobytes() == final, f"records: slice {i}"
    codes = w.resolve()
    w.out.zero_(); w.out_len.zero_()
    w.encode_resolved(codes)
    got, status = w.results()
    for i, (data, final, st) in enumerate(wants):
        assert status[i] == 0 and got[i] == data, f"resolved codes: slice {i}"
