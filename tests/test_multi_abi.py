"""avr_multi's new entry points: declared in the header, exported by both builds, bound in Python with MultiBatch methods of the same
names, and refusing a null handle with AVR_ERR_INVALID before they need a device -- which is what lets these tests run where there
is none."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AVR_ERR_INVALID = -1
NEW = {  # name -> the MultiBatch method
    "avr_multi_reset": "reset", "avr_multi_created": "created", "avr_multi_submit": "submit", "avr_multi_wait": "wait",
    "avr_multi_begin_group": "begin_group", "avr_multi_add_slice_range_keys": "add_slice_range_keys", "avr_multi_get_estimators": "get_estimators",
    "avr_multi_set_verify": "set_verify", "avr_multi_set_verify_k1": "set_verify_k1", "avr_multi_get_verify": "get_verify",
    "avr_multi_get_verify_est": "get_verify_est", "avr_multi_expect": "expect", "avr_multi_get_restore": "get_restore",
    "avr_multi_get_states": "get_states", "avr_multi_entry_info": "entry_info", "avr_multi_entry_ms": "entry_ms",
}
KEPT = ("avr_multi_create", "avr_multi_destroy", "avr_multi_add_slice_cabac", "avr_multi_add_slice_range", "avr_multi_add_slice_codes",
        "avr_multi_add_slice_cabac8", "avr_multi_run", "avr_multi_get", "avr_multi_placement", "avr_multi_load")


def _header():
    return open(os.path.join(ROOT, "include", "avrecode_ms_amd.h")).read()


def test_the_entry_points_are_declared_exported_and_bound(avr):
    handle, hooks = ctypes.CDLL(avr.LIB_PATH), ctypes.CDLL(avr.HOOKS_LIB_PATH)
    hdr = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for name in list(NEW) + list(KEPT):
        assert hasattr(handle, name) and hasattr(hooks, name), name
        assert re.search(r"\b%s\s*\(" % name, hdr), f"{name} not declared in include/avrecode_ms_amd.h"
        assert name in avr.SIGNATURES, name
    for name, method in NEW.items():
        assert callable(getattr(avr.MultiBatch, method, None)), (name, method)
    assert "avr_multi.cpp" in avr._SOURCES and "avr_multi.h" in avr._DEPS
    for f in ("avr_multi.cpp", "avr_multi.h"):
        assert os.path.exists(os.path.join(ROOT, "avrecode-ms_amd", "csrc", f))
    assert hasattr(__import__("avrecode_ms_amd.sharding", fromlist=["x"]), "lpt_assign_groups")


def test_the_layer_is_written_on_the_public_header_alone():
    """csrc/avr_multi.cpp includes the public header and its own, nothing of the device side -- so it links against the CPU stand-in."""
    src = open(os.path.join(ROOT, "avrecode-ms_amd", "csrc", "avr_multi.cpp")).read()
    mine = re.findall(r'#include\s+"([^"]+)"', src)
    assert sorted(mine) == ["../../include/avrecode_ms_amd.h", "avr_multi.h"], mine
    assert "hip" not in " ".join(re.findall(r"#include\s+<([^>]+)>", src))
    api = open(os.path.join(ROOT, "avrecode-ms_amd", "csrc", "avr_api.cpp")).read()
    assert "struct avr_multi" not in api and "multi_set_error" in api and "multi_check_device" in api


def test_the_header_states_the_group_rule_and_the_equivalence_rule():
    hdr = _header()
    assert "avr_multi has no key records" not in hdr
    doc = hdr[hdr.index("one batch over several GPUs"):hdr.index("typedef struct avr_multi avr_multi;")]
    flat = " ".join(doc.replace(" * ", " ").split())
    assert "what ONE avr_batch on devices[0] given the same calls gives" in flat
    assert "a unit is a whole GROUP" in flat and "A group without slices is no unit" in flat


def test_a_null_handle_is_refused_by_every_new_call(avr):
    L = avr.lib()
    one = (ctypes.c_uint8 * (2 * avr.EST_KEYS))(*([1] * (2 * avr.EST_KEYS)))
    recs = (ctypes.c_uint16 * 8)()
    p, n, v = ctypes.c_void_p(), ctypes.c_size_t(), ctypes.c_uint32()
    info, ms = (ctypes.c_uint32 * 4)(), (ctypes.c_float * 7)()
    calls = {
        "avr_multi_reset": (), "avr_multi_created": (), "avr_multi_submit": (), "avr_multi_wait": (),
        "avr_multi_begin_group": (None,), "avr_multi_add_slice_range_keys": (recs, 8),
        "avr_multi_get_estimators": (0, ctypes.byref(p), ctypes.byref(n)),
        "avr_multi_set_verify": (1,), "avr_multi_set_verify_k1": (1,),
        "avr_multi_get_verify": (0, ctypes.byref(v)), "avr_multi_get_verify_est": (0, ctypes.byref(v)),
        "avr_multi_expect": (0, one, 8), "avr_multi_get_restore": (0, ctypes.byref(v)),
        "avr_multi_get_states": (0, ctypes.byref(p), ctypes.byref(n)),
        "avr_multi_entry_info": (0, info), "avr_multi_entry_ms": (0, ms),
    }
    assert set(calls) == set(NEW)
    for name, args in calls.items():
        assert getattr(L, name)(None, *args) == AVR_ERR_INVALID, name
        assert L.avr_last_error(), name
    assert L.avr_multi_begin_group(None, one) == AVR_ERR_INVALID
    assert L.avr_multi_run(None) == AVR_ERR_INVALID and L.avr_multi_get(None, 0, ctypes.byref(p), ctypes.byref(n), None) == AVR_ERR_INVALID
    L.avr_multi_destroy(None)                                    # (a no-op, as before)
