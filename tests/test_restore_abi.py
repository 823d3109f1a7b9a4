"""The restore check's entry points: exported by both builds, declared in the header, bound in Python, their constants, and refusing what
they must before they need a device -- which is what lets these tests run where there is none (every call below is one that must not
touch it)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AVR_ERR_INVALID, AVR_ERR_NO_DEVICE = -1, -2
NEW = ("avr_restore_check_device", "avr_batch_expect", "avr_batch_get_restore", "avr_batch_restore_ms")
FAKE = 0x10000                                              # an aligned address no call may dereference
ARGS = ("out", "out_off", "out_len", "expect", "expect_off", "expect_len", "status", "first_diff")


def _raw_header():
    return open(os.path.join(ROOT, "include", "avrecode_ms_amd.h")).read()


def _error(avr):
    return avr.lib().avr_last_error().decode()


def _call(avr, **kw):
    a = dict({k: FAKE for k in ARGS}, n_slices=1)
    a.update(kw)
    return avr.lib().avr_restore_check_device(0, None, a["out"], a["out_off"], a["out_len"], a["n_slices"], a["expect"], a["expect_off"],
                                              a["expect_len"], a["status"], a["first_diff"])


def test_the_entry_points_are_exported_declared_and_bound(avr):
    handle, hooks = ctypes.CDLL(avr.LIB_PATH), ctypes.CDLL(avr.HOOKS_LIB_PATH)
    hdr = re.sub(r"/\*.*?\*/", "", _raw_header(), flags=re.S)
    for name in NEW:
        assert hasattr(handle, name) and hasattr(hooks, name), name
        assert re.search(r"\b%s\s*\(" % name, hdr), f"{name} not declared in include/avrecode_ms_amd.h"
        assert name in avr.SIGNATURES
    for m in ("expect", "get_restore", "restore_ms"):
        assert hasattr(avr.Batch, m), m
    assert hasattr(avr.DeviceWorkload, "restore_check")
    assert "avr_restore.hip" in avr._SOURCES and "avr_restore.h" in avr._DEPS
    for f in ("avr_restore.hip", "avr_restore.h"):
        assert os.path.exists(os.path.join(ROOT, "avrecode-ms_amd", "csrc", f))


def test_the_constants(avr):
    hdr = _raw_header()
    assert int(re.search(r"#define\s+AVR_EXPECT_NONE\s+(0x[0-9A-Fa-f]+)u", hdr).group(1), 16) == avr.EXPECT_NONE == 0xFFFFFFFF
    assert int(re.search(r"#define\s+AVR_VERIFY_NONE\s+(0x[0-9A-Fa-f]+)u", hdr).group(1), 16) == avr.VERIFY_NONE == 0xFFFFFFFF
    assert int(re.search(r"#define\s+AVR_SLICE_VERIFY_FAILED\s+(\d+)", hdr).group(1)) == avr.SLICE_VERIFY_FAILED == 4


def test_the_headers_words_for_expect_none():
    """The header says what AVR_EXPECT_NONE is where it defines it and where the call takes it."""
    hdr = _raw_header()
    assert re.search(r"#define\s+AVR_EXPECT_NONE\s+0xFFFFFFFFu\s*/\*\s*expect_len: this slice has no expectation\s*\*/", hdr)
    doc = hdr[hdr.index("/* Restore check:"):hdr.index("int avr_restore_check_device")]
    assert "expect_len[i] == AVR_EXPECT_NONE: no expectation" in doc
    assert "AVR_SLICE_OK or AVR_SLICE_VERIFY_FAILED" in doc and "never blocks, allocates or uses a workspace" in doc
    assert "avr_drop_stop_byte" in doc and "avr_tail_patch" in doc and "shares NOTHING with the encoders" in doc


def test_the_device_call_refuses_before_the_device(avr):
    for arg in ARGS:
        assert _call(avr, **{arg: None}) == AVR_ERR_INVALID and "null" in _error(avr), arg
    assert _call(avr, n_slices=1 << 31) == AVR_ERR_INVALID and "n_slices" in _error(avr)
    for odd in (FAKE + 1, FAKE + 4, FAKE + 7):
        assert _call(avr, expect=odd) == AVR_ERR_INVALID and "aligned" in _error(avr), odd


def test_what_passes_every_check_needs_a_device(avr):
    import torch
    if torch.cuda.is_available():
        return                                               # (tests/test_gpu_restore_check.py runs the call where there is one)
    assert _call(avr) == AVR_ERR_NO_DEVICE
    assert _call(avr, n_slices=(1 << 31) - 1) == AVR_ERR_NO_DEVICE
    assert _call(avr, n_slices=0, **{k: None for k in ARGS}) == AVR_ERR_NO_DEVICE


def test_the_batch_calls_refuse_a_null_batch(avr):
    L = avr.lib()
    one = (ctypes.c_uint8 * 8)()
    v, ms = ctypes.c_uint32(), ctypes.c_float()
    assert L.avr_batch_expect(None, 0, one, 8) == AVR_ERR_INVALID and "null batch" in _error(avr)
    assert L.avr_batch_get_restore(None, 0, ctypes.byref(v)) == AVR_ERR_INVALID
    assert L.avr_batch_restore_ms(None, ctypes.byref(ms)) == AVR_ERR_INVALID
