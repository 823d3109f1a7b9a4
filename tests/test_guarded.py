"""The guard bands of tests/guarded.py, on a CPU tensor: the failure path is exercised by a write from Python into the guard, never
by making a kernel overrun."""
import pytest

import guarded


def test_guard_reports_a_write_outside_the_buffer():
    g = guarded.Guarded(1000, "cpu", "probe")
    assert g.view.numel() == 1000 and g.view.data_ptr() % 256 == 0
    assert g.start >= guarded.GUARD and g.raw.numel() - g.start - 1000 >= guarded.GUARD
    g.view.fill_(0x11)
    g.check()
    assert g.extent(0x11) == 0
    g.view[700] = 5
    assert g.extent(0x11) == 701 and g.extent(0x11, block=256) == 701
    g.check()                                                # (a write inside the buffer is the buffer's business)
    g.raw[g.start + 1000] = 0                                # the first byte behind: inside the rounding to 256
    g.raw[g.start - 3] = 1
    assert g.changed() == (-3, 1000, 2)
    with pytest.raises(AssertionError, match=r"probe \(1000 bytes\): 2 guard bytes changed, the first at offset -3, the last at offset 1000"):
        g.check()


def test_guard_of_an_empty_buffer_and_typed_views():
    import torch
    g = guarded.Guarded(0, "cpu")
    g.check()
    assert g.view.numel() == 0 and g.extent(0) == 0
    g = guarded.Guarded(64, "cpu")
    v = g.as_dtype(torch.int32)
    assert v.numel() == 16 and v.data_ptr() == g.view.data_ptr()
    v.fill_(-1)
    g.check()
    assert g.extent(0xFF) == 0 and g.extent(0) == 64
