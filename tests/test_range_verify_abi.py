"""The entry points of the K2 verifier: exported by both builds, declared in the header, bound in Python, and refusing null pointers
before they need a device -- which is what lets these tests run where there is none (every call below is one that must not touch it)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AVR_ERR_INVALID = -1
NEW = ("avr_range_verify_tiles_device", "avr_range_verify_slices_device", "avr_batch_set_verify", "avr_batch_get_verify",
       "avr_batch_verify_ms")
FAKE = 0x10000                                              # an aligned address no call may dereference


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "avrecode_ms_amd.h")).read(), flags=re.S)


def _error(avr):
    return avr.lib().avr_last_error().decode()


def test_verifier_entry_points_are_exported_declared_and_bound(avr):
    handle, hooks = ctypes.CDLL(avr.LIB_PATH), ctypes.CDLL(avr.HOOKS_LIB_PATH)
    hdr = _header()
    for name in NEW:
        assert hasattr(handle, name) and hasattr(hooks, name), name
        assert re.search(r"\b%s\s*\(" % name, hdr), f"{name} not declared in include/avrecode_ms_amd.h"
        assert name in avr.SIGNATURES
    for method in ("set_verify", "get_verify", "verify_ms"):
        assert hasattr(avr.Batch, method)
    assert hasattr(avr.DeviceWorkload, "verify")
    assert "avr_verify.hip" in avr._SOURCES and "avr_verify.h" in avr._DEPS
    assert not hasattr(handle, "avr_test_hook_set") and hasattr(hooks, "avr_test_hook_set")   # the product library has no hooks


def test_constants_match_the_header(avr):
    hdr = _header()
    assert re.search(r"#define\s+AVR_SLICE_VERIFY_FAILED\s+4\b", hdr) and avr.SLICE_VERIFY_FAILED == 4
    m = re.search(r"#define\s+AVR_VERIFY_NONE\s+(0x[0-9A-Fa-f]+)u\b", hdr)
    assert m and int(m.group(1), 16) == avr.VERIFY_NONE == 0xFFFFFFFF
    src = open(os.path.join(ROOT, "avrecode-ms_amd", "csrc", "avr_verify.h")).read()
    assert re.search(r"#define\s+AVR_VERIFY_NONE\s+0xFFFFFFFFu", src)


def _tiles(avr, **kw):
    a = dict(tiles=FAKE, tile_off=FAKE, n_bins=FAKE, order=FAKE, n_slices=1, out=FAKE, out_off=FAKE, out_len=FAKE, status=FAKE, first_bad=FAKE)
    a.update(kw)
    return avr.lib().avr_range_verify_tiles_device(0, None, a["tiles"], a["tile_off"], a["n_bins"], a["order"], a["n_slices"], a["out"],
                                                   a["out_off"], a["out_len"], a["status"], a["first_bad"])


def _slices(avr, **kw):
    a = dict(recs=FAKE, rec_off=FAKE, n_bins=FAKE, order=None, n_slices=1, out=FAKE, out_off=FAKE, out_len=FAKE, status=FAKE, first_bad=FAKE)
    a.update(kw)
    return avr.lib().avr_range_verify_slices_device(0, None, a["recs"], a["rec_off"], a["n_bins"], a["order"], a["n_slices"], a["out"],
                                                    a["out_off"], a["out_len"], a["status"], a["first_bad"])


def test_device_calls_refuse_null_pointers_before_the_device(avr):
    for name in ("tiles", "tile_off", "n_bins", "out", "out_off", "out_len", "status"):
        assert _tiles(avr, **{name: None}) == AVR_ERR_INVALID and "null" in _error(avr), name
    for name in ("recs", "rec_off", "n_bins", "out", "out_off", "out_len", "status", "first_bad"):
        assert _slices(avr, **{name: None}) == AVR_ERR_INVALID and "null" in _error(avr), name
    assert _tiles(avr, n_slices=1 << 31) == AVR_ERR_INVALID and _slices(avr, n_slices=1 << 31) == AVR_ERR_INVALID
    import torch
    if not torch.cuda.is_available():                        # what passes every check needs a device
        assert _tiles(avr, first_bad=None) == -2             # AVR_ERR_NO_DEVICE: first_bad may be null in the tiles call
        assert _slices(avr) == -2
        null = dict(n_bins=None, out=None, out_off=None, out_len=None, status=None, first_bad=None, n_slices=0)
        assert _tiles(avr, tiles=None, tile_off=None, order=None, **null) == -2
        assert _slices(avr, recs=None, rec_off=None, **null) == -2


def test_batch_calls_refuse_a_null_batch(avr):
    L = avr.lib()
    v, ms = ctypes.c_uint32(), ctypes.c_float()
    assert L.avr_batch_set_verify(None, 1) == AVR_ERR_INVALID and "null batch" in _error(avr)
    assert L.avr_batch_get_verify(None, 0, ctypes.byref(v)) == AVR_ERR_INVALID
    assert L.avr_batch_verify_ms(None, ctypes.byref(ms)) == AVR_ERR_INVALID
