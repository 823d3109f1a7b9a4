"""One-byte key records (AVR_KIND_RANGE_KEYS8) without a device: the two workspace quotes against their formulas, and what the four
device calls and the new batch calls refuse before anything touches a device -- each with its return code and avr_last_error() text.
The pointers handed to the device calls are addresses inside a host buffer kept here: non-null, distinct, 256-byte aligned, never
dereferenced.  A sound call is made only where no GPU is visible, and returns AVR_ERR_NO_DEVICE there."""
import ctypes

import numpy as np
import pytest

import range_keys8 as rk8

INVALID, NO_DEVICE = -1, -2
_ARENA = ctypes.create_string_buffer(32 * 256 + 256)
_BASE = (ctypes.addressof(_ARENA) + 255) & ~255
P = lambda i: _BASE + 256 * i                                     # the i-th fake pointer


def _gpu_visible():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def plan_of(avr, total_chunks, pointers=True):
    p = avr.ChunkPlan()
    p.total_chunks = total_chunks
    if pointers:
        p.chunk_base, p.chunk_slice = P(20), P(21)
    return p


def test_constants_and_symbols(avr):
    assert (avr.KIND_RANGE_KEYS8, avr.EST_KEYS8) == (5, 128)
    L = avr.lib()
    for name in ("avr_range_resolve8_workspace_bytes", "avr_range_resolve8_device", "avr_range_keys8_verify_workspace_bytes",
                 "avr_range_keys8_verify_device", "avr_batch_begin_group8", "avr_batch_add_slice_range_keys8"):
        assert hasattr(L, name), name
    for name in ("from_host_keys8", "from_device_keys8"):
        assert hasattr(avr.DeviceWorkload, name)


@pytest.mark.parametrize("n_slices", [1, 5, 1024])
@pytest.mark.parametrize("total_chunks", [0, 1, 16, 17, 303000])
def test_quotes_follow_the_formulas_and_lie_below_the_two_byte_ones(avr, n_slices, total_chunks):
    L = avr.lib()
    plan = plan_of(avr, total_chunks)
    for n_groups in sorted({1, n_slices}):
        res = L.avr_range_resolve8_workspace_bytes(n_slices, n_groups, ctypes.byref(plan))
        chk = L.avr_range_keys8_verify_workspace_bytes(n_slices, n_groups, ctypes.byref(plan))
        assert res == rk8.resolver_quote(n_slices, n_groups, total_chunks)
        assert chk == rk8.checker_quote(n_slices, total_chunks)
        assert chk <= res
        res2 = L.avr_range_resolve_workspace_bytes(n_slices, n_groups, ctypes.byref(plan))
        chk2 = L.avr_range_keys_verify_workspace_bytes(n_slices, n_groups, ctypes.byref(plan))
        if total_chunks:
            assert res < res2 and chk < chk2
        else:
            assert res == res2 and chk == chk2                    # no rows, no slots: nothing to shrink
    assert L.avr_range_resolve8_workspace_bytes(n_slices, 1, None) == 0
    assert L.avr_range_keys8_verify_workspace_bytes(n_slices, 1, None) == 0


def resolve8(avr, **over):
    """avr_range_resolve8_device with sound fake arguments, `over` replacing some: (return code, message)"""
    L = avr.lib()
    a = dict(device=0, stream=None, keys8=P(0), rec_off=P(1), n_bins=P(2), n_slices=4, group_first=P(3), n_groups=2, est_in=P(4),
             est_out=P(5), plan=plan_of(avr, 40), workspace=P(6), short=0, recs_out=P(7), status=P(8))
    a.update(over)
    plan = a["plan"]
    quote = L.avr_range_resolve8_workspace_bytes(a["n_slices"], a["n_groups"], ctypes.byref(plan)) if plan is not None else 0
    rc = L.avr_range_resolve8_device(a["device"], a["stream"], a["keys8"], a["rec_off"], a["n_bins"], a["n_slices"], a["group_first"],
                                     a["n_groups"], a["est_in"], a["est_out"], ctypes.byref(plan) if plan is not None else None,
                                     a["workspace"], quote - a["short"], a["recs_out"], a["status"])
    return rc, L.avr_last_error().decode()


def verify8(avr, **over):
    L = avr.lib()
    a = dict(device=0, stream=None, keys8=P(0), recs=P(7), rec_off=P(1), n_bins=P(2), n_slices=4, group_first=P(3), n_groups=2,
             est_in=P(4), est_out=P(5), plan=plan_of(avr, 40), workspace=P(6), short=0, status=P(8), first_bad=P(9))
    a.update(over)
    plan = a["plan"]
    quote = L.avr_range_keys8_verify_workspace_bytes(a["n_slices"], a["n_groups"], ctypes.byref(plan)) if plan is not None else 0
    rc = L.avr_range_keys8_verify_device(a["device"], a["stream"], a["keys8"], a["recs"], a["rec_off"], a["n_bins"], a["n_slices"],
                                         a["group_first"], a["n_groups"], a["est_in"], a["est_out"],
                                         ctypes.byref(plan) if plan is not None else None, a["workspace"], quote - a["short"],
                                         a["status"], a["first_bad"])
    return rc, L.avr_last_error().decode()


REFUSALS = [
    (dict(n_groups=0), "n_groups 0: a batch of 4 slices has between 1 and 4 groups"),
    (dict(n_groups=5), "n_groups 5: a batch of 4 slices has between 1 and 4 groups"),
    (dict(n_slices=1 << 31), "n_slices out of range"),
    (dict(keys8=None), "null device pointer"),
    (dict(rec_off=None), "null device pointer"),
    (dict(n_bins=None), "null device pointer"),
    (dict(group_first=None), "null device pointer"),
    (dict(plan=None), "null plan pointer"),
    (dict(workspace=None), "null workspace"),
    (dict(keys8=P(0) + 8), "keys8 / %s not 16-byte aligned"),
    (dict(est_in=P(4) + 1), "est_in / est_out not 2-byte aligned"),
    (dict(est_out=P(5) + 1), "est_in / est_out not 2-byte aligned"),
    (dict(workspace=P(6) + 128), "workspace not 256-byte aligned"),
]


@pytest.mark.parametrize("call,other,quote", [(resolve8, "recs_out", "avr_range_resolve8_workspace_bytes"),
                                              (verify8, "recs", "avr_range_keys8_verify_workspace_bytes")])
def test_device_calls_refuse_before_a_device_is_touched(avr, call, other, quote):
    for over, text in REFUSALS:
        assert call(avr, **over) == (INVALID, text % other if "%s" in text else text), over
    assert call(avr, **{other: None}) == (INVALID, "null device pointer")
    assert call(avr, **{other: P(0)}) == (INVALID, f"{other} must not alias keys8")
    assert call(avr, **{other: P(7) + 2}) == (INVALID, f"keys8 / {other} not 16-byte aligned")
    rc, text = call(avr, short=1)
    assert rc == INVALID and text.endswith(f"bytes is smaller than {quote}()")
    plan = plan_of(avr, 40, pointers=False)
    assert call(avr, plan=plan) == (INVALID, "null plan pointer")
    if call is resolve8:
        assert call(avr, status=None) == (INVALID, "null device pointer")
    else:
        assert call(avr, status=None) == (INVALID, "null device pointer")
        assert call(avr, first_bad=None) == (INVALID, "null device pointer")
    if not _gpu_visible():                                        # a sound call, and one without the optional tables
        assert call(avr)[0] == NO_DEVICE
        assert call(avr, est_in=None, est_out=None)[0] == NO_DEVICE


# ------------------------------------------------------------------ the batch calls (tests/cpu_batch.cpp knows none of them: the library itself)

# (an avr_batch needs a device to exist: the refusals of a live batch are in tests/test_gpu_range_keys8.py)

def test_batch_calls_without_a_batch(avr):
    L = avr.lib()
    keys = np.zeros(16, np.uint8)
    assert L.avr_batch_begin_group8(None, None) == INVALID and L.avr_last_error() == b"null batch"
    assert L.avr_batch_add_slice_range_keys8(None, keys.ctypes.data, keys.size) == INVALID and L.avr_last_error() == b"null batch"
    if not _gpu_visible():
        assert L.avr_batch_create(0, 4, 1024) is None
        assert b"no HIP device" in L.avr_last_error()
