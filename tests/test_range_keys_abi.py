"""The entry points for key records (AVR_KIND_RANGE_KEYS: the compress direction's estimators resolved on the device): exported,
declared, bound, and refusing bad arguments before they need a device -- which is what lets these tests run where there is none
(a call that passed its checks would fail with AVR_ERR_NO_DEVICE here, and on a GPU box it would touch the device: every call
below is one that must not)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AVR_ERR_INVALID = -1
NEW = ("avr_range_resolve_workspace_bytes", "avr_range_resolve_device", "avr_batch_begin_group", "avr_batch_add_slice_range_keys",
       "avr_batch_get_estimators")
FAKE = 0x10000                                              # a 256-byte aligned address no call may dereference


def _header(strip=True):
    text = open(os.path.join(ROOT, "include", "avrecode_ms_amd.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S) if strip else text


def test_key_record_entry_points_are_exported_declared_and_bound(avr):
    handle = ctypes.CDLL(avr.LIB_PATH)
    hooks = ctypes.CDLL(avr.HOOKS_LIB_PATH)
    hdr = _header()
    for name in NEW:
        assert hasattr(handle, name) and hasattr(hooks, name), name
        assert re.search(r"\b%s\s*\(" % name, hdr), f"{name} not declared in include/avrecode_ms_amd.h"
        assert name in avr.SIGNATURES
    assert re.search(r"#define\s+AVR_KIND_RANGE_KEYS\s+4\b", hdr) and avr.KIND_RANGE_KEYS == 4
    assert re.search(r"#define\s+AVR_EST_KEYS\s+1026\b", hdr) and avr.EST_KEYS == 1026
    for method in ("begin_group", "add_slice_range_keys", "get_estimators"):
        assert hasattr(avr.Batch, method)
    for method in ("from_host_keys", "resolve_range"):
        assert hasattr(avr.DeviceWorkload, method)


def _plan(avr, chunks=1):
    a = FAKE
    return avr.ChunkPlan(a, a, a, a, a, a, 1024, 1024, chunks, 1)


def _resolve(avr, keys=FAKE, rec_off=FAKE, n_bins=FAKE, n_slices=1, group_first=FAKE, n_groups=1, est_in=None, est_out=None, plan="default",
             ws=FAKE, ws_bytes=1 << 40, recs_out=FAKE + 0x1000, status=FAKE):
    p = ctypes.byref(_plan(avr)) if plan == "default" else (None if plan is None else ctypes.byref(plan))
    return avr.lib().avr_range_resolve_device(0, None, keys, rec_off, n_bins, n_slices, group_first, n_groups, est_in, est_out, p, ws,
                                              ws_bytes, recs_out, status)


def _error(avr):
    return avr.lib().avr_last_error().decode()


def test_resolver_refuses_bad_arguments_before_the_device(avr):
    f = lambda **kw: _resolve(avr, **kw)
    for name in ("keys", "rec_off", "n_bins", "group_first", "recs_out", "status", "ws"):
        assert f(**{name: None}) == AVR_ERR_INVALID and "null" in _error(avr), name
    assert f(n_groups=0) == AVR_ERR_INVALID and "groups" in _error(avr)
    assert f(n_groups=2) == AVR_ERR_INVALID and "groups" in _error(avr)                   # more groups than slices
    assert f(n_slices=3, n_groups=4) == AVR_ERR_INVALID
    assert f(plan=None) == AVR_ERR_INVALID and "plan" in _error(avr)
    assert f(plan=avr.ChunkPlan(FAKE, None, FAKE, FAKE, FAKE, FAKE, 1024, 1024, 1, 1)) == AVR_ERR_INVALID and "plan" in _error(avr)
    need = avr.lib().avr_range_resolve_workspace_bytes(1, 1, ctypes.byref(_plan(avr)))
    assert need > 0
    assert f(ws_bytes=need - 1) == AVR_ERR_INVALID and "workspace" in _error(avr)
    assert f(recs_out=FAKE) == AVR_ERR_INVALID and "alias" in _error(avr)                 # recs_out == keys
    assert f(keys=FAKE + 8) == AVR_ERR_INVALID and "16-byte aligned" in _error(avr)
    assert f(recs_out=FAKE + 0x1002) == AVR_ERR_INVALID and "16-byte aligned" in _error(avr)
    assert f(est_in=FAKE + 1) == AVR_ERR_INVALID and "2-byte aligned" in _error(avr)
    assert f(est_out=FAKE + 1) == AVR_ERR_INVALID
    assert f(ws=FAKE + 16) == AVR_ERR_INVALID and "256-byte aligned" in _error(avr)
    # what passes every check needs a device
    import torch
    if not torch.cuda.is_available():
        assert f(ws_bytes=need) == -2                                                      # AVR_ERR_NO_DEVICE
        assert f(n_slices=0, n_groups=0, keys=None, rec_off=None, n_bins=None, group_first=None, recs_out=None, status=None, ws=None) == -2


def test_resolver_workspace_formula(avr):
    """align256(4 n_slices) + align256(4 n_groups) + 2 ceil(total_chunks / 16) * 6168, as the header says: no term per key and group,
    so 1 Mi one-slice groups pay a fraction of one estimator table (1026 x 2 bytes) each."""
    L = avr.lib()
    a256 = lambda x: (x + 255) // 256 * 256
    for n_slices, n_groups, chunks in ((1, 1, 1), (7, 3, 100), (4096, 4096, 4096), (296, 1, 37000), (1 << 20, 1 << 20, 1 << 20)):
        got = L.avr_range_resolve_workspace_bytes(n_slices, n_groups, ctypes.byref(_plan(avr, chunks)))
        assert got == a256(4 * n_slices) + a256(4 * n_groups) + 2 * ((chunks + 15) // 16) * 6168
    assert L.avr_range_resolve_workspace_bytes(1 << 20, 1 << 20, ctypes.byref(_plan(avr, 1 << 20))) < (1 << 20) * 1026 * 2 // 2
    assert L.avr_range_resolve_workspace_bytes(1, 1, None) == 0
    assert re.search(r"2 ceil\(total_chunks / 16\) \* 6168", _header(strip=False))


def test_batch_calls_refuse_a_null_batch(avr):
    import numpy as np
    L = avr.lib()
    recs = np.zeros(4, np.uint16)
    assert L.avr_batch_begin_group(None, None) == AVR_ERR_INVALID and "null batch" in _error(avr)
    assert L.avr_batch_add_slice_range_keys(None, recs.ctypes.data, 4) == AVR_ERR_INVALID and "null batch" in _error(avr)
    assert L.avr_batch_add_slice_range_keys(None, None, 4) == AVR_ERR_INVALID and "null records" in _error(avr)
    assert L.avr_batch_get_estimators(None, 0, None, None) == AVR_ERR_INVALID
