"""The entry points of the K1 verifier: exported by both builds, declared in the header, bound in Python, and refusing what they must
before they need a device -- which is what lets these tests run where there is none (every call below is one that must not touch it)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AVR_ERR_INVALID, AVR_ERR_NO_DEVICE = -1, -2
STATE_CALLS = {"avr_cabac_verify_tiles_device": 1024, "avr_cabac_verify_slices_device": 1024,     # name -> the form's limit of n_states
               "avr_cabac8_verify_tiles_device": 126, "avr_cabac8_verify_slices_device": 126}
NEW = tuple(STATE_CALLS) + ("avr_cabac_verify_codes_device", "avr_batch_set_verify_k1")
FAKE = 0x10000                                              # an aligned address no call may dereference


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "avrecode_ms_amd.h")).read(), flags=re.S)


def _error(avr):
    return avr.lib().avr_last_error().decode()


def test_the_six_entry_points_are_exported_declared_and_bound(avr):
    handle, hooks = ctypes.CDLL(avr.LIB_PATH), ctypes.CDLL(avr.HOOKS_LIB_PATH)
    hdr = _header()
    assert len(NEW) == 6
    for name in NEW:
        assert hasattr(handle, name) and hasattr(hooks, name), name
        assert re.search(r"\b%s\s*\(" % name, hdr), f"{name} not declared in include/avrecode_ms_amd.h"
        assert name in avr.SIGNATURES
    assert hasattr(avr.Batch, "set_verify_k1") and hasattr(avr.DeviceWorkload, "verify_k1")
    assert hasattr(avr.Batch, "set_verify") and hasattr(avr.DeviceWorkload, "verify")          # the K2 verifier's stay
    assert "avr_cabac_verify.hip" in avr._SOURCES and "avr_cabac_verify.h" in avr._DEPS
    for f in ("avr_cabac_verify.hip", "avr_cabac_verify.h"):
        assert os.path.exists(os.path.join(ROOT, "avrecode-ms_amd", "csrc", f))


def _states_call(avr, name, **kw):
    """One of the four calls that take states; the records are `tiles` / `tile_off` or `recs` / `rec_off` by position."""
    a = dict(recs=FAKE, off=FAKE, n_bins=FAKE, order=FAKE, n_slices=1, init_states=FAKE, n_states=20, out=FAKE, out_off=FAKE,
             out_len=FAKE, final_states=FAKE, status=FAKE, first_bad=FAKE)
    a.update(kw)
    return getattr(avr.lib(), name)(0, None, a["recs"], a["off"], a["n_bins"], a["order"], a["n_slices"], a["init_states"], a["n_states"],
                                    a["out"], a["out_off"], a["out_len"], a["final_states"], a["status"], a["first_bad"])


def _codes_call(avr, **kw):
    a = dict(recs=FAKE, off=FAKE, n_bins=FAKE, order=None, n_slices=1, out=FAKE, out_off=FAKE, out_len=FAKE, status=FAKE, first_bad=FAKE)
    a.update(kw)
    return avr.lib().avr_cabac_verify_codes_device(0, None, a["recs"], a["off"], a["n_bins"], a["order"], a["n_slices"], a["out"],
                                                   a["out_off"], a["out_len"], a["status"], a["first_bad"])


def test_device_calls_refuse_before_the_device(avr):
    for name, limit in STATE_CALLS.items():
        needed = ["recs", "off", "n_bins", "init_states", "out", "out_off", "out_len", "status"]
        if "slices" in name:
            needed.append("first_bad")                       # may be null in the tiles calls only
        for arg in needed:
            assert _states_call(avr, name, **{arg: None}) == AVR_ERR_INVALID and "null" in _error(avr), (name, arg)
        assert _states_call(avr, name, n_slices=1 << 31) == AVR_ERR_INVALID, name
        assert _states_call(avr, name, n_states=limit + 1) == AVR_ERR_INVALID and "n_states" in _error(avr), name
    for arg in ("recs", "off", "n_bins", "out", "out_off", "out_len", "status", "first_bad"):
        assert _codes_call(avr, **{arg: None}) == AVR_ERR_INVALID and "null" in _error(avr), arg
    assert _codes_call(avr, n_slices=1 << 31) == AVR_ERR_INVALID


def test_what_passes_every_check_needs_a_device(avr):
    import torch
    if torch.cuda.is_available():
        return                                               # (tests/test_gpu_cabac_verify.py runs the calls where there is one)
    null = dict(recs=None, off=None, n_bins=None, order=None, out=None, out_off=None, out_len=None, status=None, first_bad=None, n_slices=0)
    for name, limit in STATE_CALLS.items():
        assert _states_call(avr, name, n_states=limit, final_states=None, order=None if "slices" in name else FAKE) == AVR_ERR_NO_DEVICE, name
        assert _states_call(avr, name, n_states=0, init_states=None) == AVR_ERR_NO_DEVICE, name       # no states: no init_states needed
        if "tiles" in name:
            assert _states_call(avr, name, first_bad=None) == AVR_ERR_NO_DEVICE, name
        assert _states_call(avr, name, init_states=None, final_states=None, **null) == AVR_ERR_NO_DEVICE, name
    assert _codes_call(avr) == AVR_ERR_NO_DEVICE and _codes_call(avr, order=FAKE) == AVR_ERR_NO_DEVICE
    assert _codes_call(avr, **null) == AVR_ERR_NO_DEVICE


def test_batch_call_refuses_a_null_batch(avr):
    L = avr.lib()
    assert L.avr_batch_set_verify_k1(None, 1) == AVR_ERR_INVALID and "null batch" in _error(avr)
    assert L.avr_batch_set_verify_k1(None, 0) == AVR_ERR_INVALID
