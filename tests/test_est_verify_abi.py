"""The entry points of the estimator checker: exported by both builds, declared in the header, bound in Python, quoting the
documented workspace, and refusing everything the header lists before they need a device -- which is what lets these tests run
where there is none (every call below is one that must not touch it)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AVR_ERR_INVALID = -1
NEW = ("avr_range_keys_verify_workspace_bytes", "avr_range_keys_verify_device", "avr_batch_get_verify_est", "avr_batch_verify_est_ms")
A, B = 0x10000, 0x20000                                     # aligned addresses no call may dereference


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "avrecode_ms_amd.h")).read(), flags=re.S)


def _error(avr):
    return avr.lib().avr_last_error().decode()


def _plan(avr, total_chunks=1, chunk_base=A, chunk_slice=A):
    p = avr.ChunkPlan()
    p.chunk_base, p.chunk_slice, p.total_chunks = chunk_base, chunk_slice, total_chunks
    return p


def _quote(avr, n_slices, n_groups, total_chunks):
    return avr.lib().avr_range_keys_verify_workspace_bytes(n_slices, n_groups, ctypes.byref(_plan(avr, total_chunks)))


def _call(avr, **kw):
    a = dict(keys=A, recs=B, rec_off=A, n_bins=A, n_slices=2, group_first=A, n_groups=1, est_in=None, est_out=None, plan="own",
             workspace=A, workspace_bytes=None, status=A, first_bad=A, total_chunks=2)
    a.update(kw)
    plan = _plan(avr, a["total_chunks"]) if a["plan"] == "own" else a["plan"]
    if a["workspace_bytes"] is None:
        a["workspace_bytes"] = _quote(avr, a["n_slices"], a["n_groups"], a["total_chunks"])
    return avr.lib().avr_range_keys_verify_device(0, None, a["keys"], a["recs"], a["rec_off"], a["n_bins"], a["n_slices"], a["group_first"],
                                                  a["n_groups"], a["est_in"], a["est_out"], None if plan is None else ctypes.byref(plan),
                                                  a["workspace"], a["workspace_bytes"], a["status"], a["first_bad"])


def test_checker_entry_points_are_exported_declared_and_bound(avr):
    handle, hooks = ctypes.CDLL(avr.LIB_PATH), ctypes.CDLL(avr.HOOKS_LIB_PATH)
    hdr = _header()
    for name in NEW:
        assert hasattr(handle, name) and hasattr(hooks, name), name
        assert re.search(r"\b%s\s*\(" % name, hdr), f"{name} not declared in include/avrecode_ms_amd.h"
        assert name in avr.SIGNATURES
    for method in ("get_verify_est", "verify_est_ms"):
        assert hasattr(avr.Batch, method)
    assert hasattr(avr.DeviceWorkload, "verify_keys")
    assert "avr_est_verify.hip" in avr._SOURCES and "avr_est_verify.h" in avr._DEPS
    with avr.test_hooks(est_flip=1, est_flip_bin=5):         # the hooks exist in the test build ...
        pass
    assert not hasattr(handle, "avr_test_hook_set")          # ... and the product library has none


def test_the_checker_shares_no_code_with_the_resolver():
    csrc = os.path.join(ROOT, "avrecode-ms_amd", "csrc")
    for f in ("avr_est_verify.h", "avr_est_verify.hip"):
        includes = re.findall(r'#include\s+[<"]([^>"]+)[>"]', open(os.path.join(csrc, f)).read())
        assert "avr_est.h" not in includes, f
    # and what it does include leads there neither
    for f in ("avr_layout.h", "avr_internal.h", "avr_k1p.h", "avr_chunk.h"):
        assert "avr_est.h" not in re.findall(r'#include\s+[<"]([^>"]+)[>"]', open(os.path.join(csrc, f)).read()), f


def test_workspace_is_the_documented_formula_and_fits_in_the_resolvers(avr):
    """align256(4 n_slices) + 2 ceil(total_chunks / 16) * 4112, as the header says; never above avr_range_resolve_workspace_bytes"""
    L = avr.lib()
    assert "2 ceil(total_chunks / 16) * 4112" in open(os.path.join(ROOT, "include", "avrecode_ms_amd.h")).read()
    for n, g, tc in ((1, 1, 1), (2, 1, 16), (7, 3, 17), (1000, 10, 33), (64, 64, 64), (1 << 20, 1 << 20, 1 << 20), (3, 1, 300000), (0, 0, 0)):
        want = (4 * n + 255) // 256 * 256 + 2 * ((tc + 15) // 16) * 4112
        assert _quote(avr, n, g, tc) == want, (n, g, tc)
        assert want <= L.avr_range_resolve_workspace_bytes(n, g, ctypes.byref(_plan(avr, tc)))
    assert L.avr_range_keys_verify_workspace_bytes(1, 1, None) == 0


def test_device_call_refuses_what_the_header_lists_before_the_device(avr):
    for name in ("keys", "recs", "rec_off", "n_bins", "group_first", "workspace", "status", "first_bad"):
        assert _call(avr, **{name: None}) == AVR_ERR_INVALID and "null" in _error(avr), name
    assert _call(avr, n_groups=0) == AVR_ERR_INVALID and "n_groups" in _error(avr)
    assert _call(avr, n_groups=3) == AVR_ERR_INVALID and "n_groups" in _error(avr)
    assert _call(avr, plan=None) == AVR_ERR_INVALID and "plan" in _error(avr)
    assert _call(avr, plan=_plan(avr, 2, None, A)) == AVR_ERR_INVALID and "plan" in _error(avr)
    assert _call(avr, plan=_plan(avr, 2, A, None)) == AVR_ERR_INVALID and "plan" in _error(avr)
    assert _call(avr, recs=A) == AVR_ERR_INVALID and "alias" in _error(avr)
    assert _call(avr, keys=A + 8) == AVR_ERR_INVALID and "aligned" in _error(avr)
    assert _call(avr, recs=B + 2) == AVR_ERR_INVALID and "aligned" in _error(avr)
    assert _call(avr, est_in=A + 1) == AVR_ERR_INVALID and "aligned" in _error(avr)
    assert _call(avr, est_out=A + 1) == AVR_ERR_INVALID and "aligned" in _error(avr)
    assert _call(avr, workspace=A + 128) == AVR_ERR_INVALID and "aligned" in _error(avr)
    assert _call(avr, workspace_bytes=_quote(avr, 2, 1, 2) - 1) == AVR_ERR_INVALID and "smaller" in _error(avr)
    assert _call(avr, n_slices=1 << 31, n_groups=1, workspace_bytes=1 << 40) == AVR_ERR_INVALID and "n_slices" in _error(avr)
    import torch
    if not torch.cuda.is_available():                        # what passes every check needs a device
        assert _call(avr) == -2                              # AVR_ERR_NO_DEVICE
        assert _call(avr, est_in=A, est_out=B) == -2
        assert _call(avr, workspace_bytes=_quote(avr, 2, 1, 2) + 4096) == -2       # a larger one, as the resolver's is


def test_batch_calls_refuse_a_null_batch(avr):
    L = avr.lib()
    v, ms = ctypes.c_uint32(), ctypes.c_float()
    assert L.avr_batch_get_verify_est(None, 0, ctypes.byref(v)) == AVR_ERR_INVALID and "batch" in _error(avr)
    assert L.avr_batch_verify_est_ms(None, ctypes.byref(ms)) == AVR_ERR_INVALID
