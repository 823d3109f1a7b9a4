"""The entry points for one-byte K1 records (AVR_KIND_CABAC8) on the device: exported, declared, and refusing bad arguments
before they need a device -- which is what lets these tests run where there is none (a call that passed its checks would
fail with AVR_ERR_NO_DEVICE here, and on a GPU box it would touch the device: every call below is one that must not)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AVR_ERR_INVALID = -1
NEW = ("avr_pack_tiles8_device", "avr_cabac8_chunked_workspace_bytes", "avr_cabac8_encode_chunked_device",
       "avr_multi_add_slice_cabac8")
FAKE = 0x10000                                              # a 16-byte aligned address no call may dereference


def _header():
    text = open(os.path.join(ROOT, "include", "avrecode_ms_amd.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_one_byte_entry_points_are_exported_and_declared(avr):
    handle = ctypes.CDLL(avr.LIB_PATH)
    hdr = _header()
    for name in NEW:
        assert hasattr(handle, name), name
        assert re.search(r"\b%s\s*\(" % name, hdr), f"{name} not declared in include/avrecode_ms_amd.h"
        assert name in avr.SIGNATURES


def _plan(avr):
    a = FAKE
    return avr.ChunkPlan(a, a, a, a, a, a, 1024, 1024, 1, 1)


def _chunked(avr, n_states=37, recs8=FAKE, rec_off=FAKE, n_bins=FAKE, n_slices=1, init=FAKE, plan=None, ws=FAKE, ws_bytes=1 << 40,
             out=FAKE, out_off=FAKE, out_len=FAKE, status=FAKE):
    L = avr.lib()
    p = ctypes.byref(plan if plan is not None else _plan(avr))
    return L.avr_cabac8_encode_chunked_device(0, None, recs8, rec_off, n_bins, n_slices, init, n_states, p, ws, ws_bytes, out,
                                              out_off, out_len, status, None)


def _pack8(avr, n_states=37, recs8=FAKE, rec_off=FAKE, n_bins=FAKE, n_slices=1, tile_off=FAKE, tiles=FAKE, status=FAKE):
    return avr.lib().avr_pack_tiles8_device(0, None, n_states, recs8, rec_off, n_bins, None, n_slices, tile_off, tiles, status)


def _error():
    import avrecode_ms_amd as avr
    return avr.lib().avr_last_error().decode()


@pytest.mark.parametrize("call", ["chunked", "pack"])
def test_one_byte_calls_refuse_bad_arguments_before_the_device(avr, call):
    f = (lambda **kw: _chunked(avr, **kw)) if call == "chunked" else (lambda **kw: _pack8(avr, **kw))
    assert f(n_states=127) == AVR_ERR_INVALID and "at most 126" in _error()
    assert f(n_states=1024) == AVR_ERR_INVALID
    assert f(recs8=None) == AVR_ERR_INVALID and "null" in _error()
    assert f(rec_off=None) == AVR_ERR_INVALID
    assert f(n_bins=None) == AVR_ERR_INVALID
    assert f(recs8=FAKE + 8) == AVR_ERR_INVALID and "16-byte aligned" in _error()          # slice i at recs8 + rec_off[i], multiples of 16
    assert f(rec_off=FAKE + 4) == AVR_ERR_INVALID and "rec_off" in _error()
    if call == "chunked":
        assert f(status=None) == AVR_ERR_INVALID
        assert f(ws=None) == AVR_ERR_INVALID
        assert f(init=None) == AVR_ERR_INVALID
        assert f(plan=avr.ChunkPlan(FAKE, None, FAKE, FAKE, FAKE, FAKE, 1024, 1024, 1, 1)) == AVR_ERR_INVALID and "plan" in _error()
        assert f(ws_bytes=16) == -5                                                          # AVR_ERR_CAPACITY
    else:
        assert f(tiles=None) == AVR_ERR_INVALID
        assert f(status=None) == AVR_ERR_INVALID
        assert f(tile_off=None) == AVR_ERR_INVALID


def test_one_byte_workspace_size(avr):
    L = avr.lib()
    plan = _plan(avr)
    assert L.avr_cabac8_chunked_workspace_bytes(1, 127, ctypes.byref(plan)) == 0
    assert L.avr_cabac8_chunked_workspace_bytes(1, 126, None) == 0
    # the same phases on the same plan: the same workspace as the two-byte call for the same context count
    assert (L.avr_cabac8_chunked_workspace_bytes(1, 126, ctypes.byref(plan))
            == L.avr_cabac_chunked_workspace_bytes(1, 126, ctypes.byref(plan)) > 0)


def test_multi_add_slice_cabac8_refuses_more_than_126_contexts(avr):
    """The check needs no batch, so it comes first: with no batch at all, n_states = 127 is what is refused (a batch cannot be
    made where there is no device)."""
    import numpy as np
    L = avr.lib()
    recs, st = np.zeros(4, np.uint8), np.zeros(127, np.uint8)
    assert L.avr_multi_add_slice_cabac8(None, recs.ctypes.data, 4, st.ctypes.data, 127) == AVR_ERR_INVALID
    assert "at most 126" in _error()
    assert L.avr_multi_add_slice_cabac8(None, recs.ctypes.data, 4, st.ctypes.data, 126) == AVR_ERR_INVALID
    assert "null batch" in _error()
