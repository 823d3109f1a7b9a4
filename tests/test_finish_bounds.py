"""avr_finish_device's host side, no GPU needed: the workspace quote (finish_layout of csrc/avr_plan_dev.h) and the refusals, which come
before the call looks for a device -- there is none here, so a call with nothing wrong answers AVR_ERR_NO_DEVICE (with a GPU visible
such a call is not made: the pointers are made up).  tests/test_gpu_finish_device.py repeats the refusals on real buffers."""
import pytest

OK, ERR_INVALID, ERR_NO_DEVICE = 0, -1, -2


def P(k):
    """A made-up device address, 4 KiB aligned; never dereferenced."""
    return 0x7F0000000000 + k * 0x10000


def call(avr, n=3, ws=None, ws_short=0, out=P(0), out_off=P(1), out_len=P(2), status=P(3), finish=P(4), dense=P(5), cap=1000, dense_off=P(6)):
    L = avr.lib()
    quote = L.avr_finish_workspace_bytes(min(n, (1 << 31) - 1))
    return L.avr_finish_device(0, None, out, out_off, out_len, status, n, finish, dense, cap, dense_off, P(7) if ws is None else ws,
                               max(0, quote - ws_short))


def test_the_quote(avr):
    """The final lengths, 8 bytes a slice, and the sums of the scan over them: one per 1024 slices, and one per 1024 of those."""
    L = avr.lib()
    q = L.avr_finish_workspace_bytes
    assert q(0) == 256 and q(1) == 256 and q(32) == 256 and q(33) == 512
    assert q(1024) == 8192                                      # one workgroup of the scan: no sums
    assert q(1025) == 8448 + 256                                # two sums
    n = (1 << 20) + 1
    assert q(n) == (8 * n + 255) // 256 * 256 + (8 * 1025 + 255) // 256 * 256 + 256
    assert all(q(k) % 256 == 0 and q(k) >= 8 * k for k in (2, 63, 4097, 1 << 24, (1 << 31) - 1))


REFUSALS = {
    "null out": dict(out=None), "null out_off": dict(out_off=None), "null out_len": dict(out_len=None), "null finish": dict(finish=None),
    "null dense": dict(dense=None), "null dense_off": dict(dense_off=None), "null dense_off, no slices": dict(n=0, dense_off=None),
    "out_off + 4": dict(out_off=P(1) + 4), "out_len + 2": dict(out_len=P(2) + 2), "status + 2": dict(status=P(3) + 2),
    "finish + 2": dict(finish=P(4) + 2), "dense_off + 4": dict(dense_off=P(6) + 4), "workspace + 64": dict(ws=P(7) + 64),
    "workspace one byte short": dict(ws_short=1), "n_slices 2^31": dict(n=1 << 31),
}


@pytest.mark.parametrize("label", sorted(REFUSALS))
def test_refused_before_a_device_is_looked_for(avr, label):
    assert call(avr, **REFUSALS[label]) == ERR_INVALID, label
    assert avr.lib().avr_last_error() != b""


def test_sound_calls_pass_every_check(avr):
    if avr.device_count() > 0:
        pytest.skip("a GPU is visible: a call with made-up pointers is not made")
    assert call(avr) == ERR_NO_DEVICE
    assert call(avr, status=None) == ERR_NO_DEVICE              # no status: every slice is sound
    assert call(avr, dense=None, cap=0) == ERR_NO_DEVICE        # no room asked for: dense_off alone is written
    assert call(avr, n=0, out=None, out_off=None, out_len=None, finish=None, dense=None) == ERR_NO_DEVICE
