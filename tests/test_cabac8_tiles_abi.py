"""The one-byte tile calls (avr_pack_tiles8_narrow_device, avr_cabac8_encode_tiles_device): exported, declared, in SIGNATURES, and
refusing bad arguments before they need a device -- a call that passed its checks would fail with AVR_ERR_NO_DEVICE where there is
none, and on a GPU box it would touch the device: every call below is one that must not.  And the one-byte tile plan."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AVR_ERR_INVALID = -1
NEW = ("avr_pack_tiles8_narrow_device", "avr_cabac8_encode_tiles_device")
FAKE = 0x10000                                              # a 16-byte aligned address no call may dereference


def _header():
    text = open(os.path.join(ROOT, "include", "avrecode_ms_amd.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def _error():
    import avrecode_ms_amd as avr
    return avr.lib().avr_last_error().decode()


def test_one_byte_tile_calls_are_exported_and_declared(avr):
    handle = ctypes.CDLL(avr.LIB_PATH)
    hdr = _header()
    for name in NEW:
        assert hasattr(handle, name), name
        assert re.search(r"\b%s\s*\(" % name, hdr), f"{name} not declared in include/avrecode_ms_amd.h"
        assert name in avr.SIGNATURES
    # the same arguments as the calls they stand beside
    assert avr.SIGNATURES["avr_pack_tiles8_narrow_device"] == avr.SIGNATURES["avr_pack_tiles8_device"]
    assert avr.SIGNATURES["avr_cabac8_encode_tiles_device"] == avr.SIGNATURES["avr_cabac_encode_tiles_device"]


def _pack(avr, n_states=37, recs8=FAKE, rec_off=FAKE, n_bins=FAKE, n_slices=1, tile_off=FAKE, tiles=FAKE, status=FAKE):
    return avr.lib().avr_pack_tiles8_narrow_device(0, None, n_states, recs8, rec_off, n_bins, None, n_slices, tile_off, tiles, status)


def _encode(avr, n_states=37, tiles=FAKE, tile_off=FAKE, n_bins=FAKE, n_slices=1, init=FAKE, out=FAKE, out_off=FAKE, out_len=FAKE,
            status=FAKE):
    return avr.lib().avr_cabac8_encode_tiles_device(0, None, tiles, tile_off, n_bins, None, n_slices, init, n_states, out, out_off,
                                                    out_len, status, None)


def test_narrow_packer_refuses_bad_arguments_before_the_device(avr):
    f = lambda **kw: _pack(avr, **kw)                       # noqa: E731
    assert f(n_states=127) == AVR_ERR_INVALID and "at most 126" in _error()
    assert f(n_states=1024) == AVR_ERR_INVALID and "at most 126" in _error()
    assert f(recs8=None) == AVR_ERR_INVALID and "null" in _error()
    assert f(rec_off=None) == AVR_ERR_INVALID and "null" in _error()
    assert f(n_bins=None) == AVR_ERR_INVALID
    assert f(tile_off=None) == AVR_ERR_INVALID
    assert f(tiles=None) == AVR_ERR_INVALID
    assert f(status=None) == AVR_ERR_INVALID
    assert f(recs8=FAKE + 8) == AVR_ERR_INVALID and "16-byte aligned" in _error()         # slice i at recs8 + rec_off[i], multiples of 16
    assert f(recs8=FAKE + 1) == AVR_ERR_INVALID and "16-byte aligned" in _error()
    assert f(rec_off=FAKE + 4) == AVR_ERR_INVALID and "rec_off" in _error()
    assert f(tiles=FAKE + 8) == AVR_ERR_INVALID and "tiles" in _error()


def test_one_byte_tile_coder_refuses_bad_arguments_before_the_device(avr):
    f = lambda **kw: _encode(avr, **kw)                     # noqa: E731
    assert f(n_states=127) == AVR_ERR_INVALID and "at most 126" in _error()
    assert f(n_states=1024) == AVR_ERR_INVALID and "at most 126" in _error()
    for arg in ("tiles", "tile_off", "n_bins", "init", "out", "out_off", "out_len", "status"):
        assert f(**{arg: None}) == AVR_ERR_INVALID and "null" in _error(), arg
    assert f(tiles=FAKE + 8) == AVR_ERR_INVALID and "16-byte aligned" in _error()


def _plan_numpy(n_bins, records_per_chunk):
    """plan_tiles restated: longest first (stable), 64 slices a tile, a tile as long as its first (longest) slice."""
    nb = np.asarray(n_bins, dtype=np.int64)
    order = np.argsort(-nb, kind="stable")
    chunks = (nb[order] + records_per_chunk - 1) // records_per_chunk
    tile_off = np.zeros((nb.size + 63) // 64 + 1, dtype=np.int64)
    tile_off[1:] = np.cumsum(chunks[::64] * 64)
    return order, tile_off


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1000])
def test_plan_tiles_sixteen_records_a_chunk(avr, n):
    import torch
    rng = np.random.default_rng(n)
    nb = rng.integers(0, 5000, n).astype(np.int32)
    if n > 3:
        nb[:4] = [0, 15, 16, 17]
        nb[n // 2:n // 2 + 3] = 33                          # ties keep their order
    order, tile_off = avr.plan_tiles(torch.from_numpy(nb), 16)
    want_order, want_off = _plan_numpy(nb, 16)
    assert order.tolist() == want_order.tolist()
    assert tile_off.tolist() == want_off.tolist()
    # the default is still eight records a chunk
    order8, tile_off8 = avr.plan_tiles(torch.from_numpy(nb))
    assert order8.tolist() == want_order.tolist()
    assert tile_off8.tolist() == _plan_numpy(nb, 8)[1].tolist()
