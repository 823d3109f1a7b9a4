"""What every stateless *_device entry point of the C ABI answers to arguments it must refuse before it needs a device -- and to
sound ones, which on a machine without a GPU get AVR_ERR_NO_DEVICE from the first thing behind the checks.

The entry points and their parameters are read from include/avrecode_ms_amd.h, so a new one is covered when it is declared.  Every
pointer is an address inside a host buffer this module keeps: non-null, distinct, 256-byte aligned, and never dereferenced -- the
checks only look at the values.  Plans, parts and synth configs are real host structs with small fields.  cases(fn) yields
(label, call) pairs; table(handle) runs them all and gives {function: {label: [return code, avr_last_error() text]}}.

tests/golden/device_api_refusals.json is that table as recorded from the library of the commit before the launchers took structs
(tests/golden/make_device_api_refusals.py); tests/test_device_api_refusals.py holds every later library to it."""
import ctypes
import os
import re

import avrecode_ms_amd as avr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "device_api_refusals.json")
NO_DEVICE = -2

_ARENA = ctypes.create_string_buffer(64 * 256 + 256)            # the fake pointers' addresses: kept alive, never read or written
_BASE = (ctypes.addressof(_ARENA) + 255) & ~255
_PLAN_PTRS = ("res_off", "chunk_base", "chunk_slice", "blk_base", "blk_slice", "dig_off")
_PART_PTRS = ("rec_off", "n_bins", "init_states", "plan", "workspace", "out_off", "out_len", "status", "final_states", "counts")
_SCALARS = dict(device=0, stream=None, n_slices=1, n_states=4, n_groups=1, kind=avr.KIND_CABAC, out_total=64, rows_hint=4, n_records=8,
                n_src=4, n_dst=4, n_index=4, scatter=0)
# limit -> the values one past it (n_states: both record widths' limits, whichever the entry point has)
_PAST = dict(n_states=(avr.MAX_STATES8 + 1, 1025), n_slices=(1 << 31,), n_groups=(0, 2, 1 << 31), n_src=(1025,), n_dst=(1025,), n_index=(1025,),
             n_records=(9,))
# entry point -> what quotes its workspace, and that function's arguments
_QUOTES = {
    "avr_cabac_encode_chunked_device": ("avr_cabac_chunked_workspace_bytes", ("n_slices", "n_states", "plan")),
    "avr_cabac_encode_chunked_device_hinted": ("avr_cabac_chunked_workspace_bytes", ("n_slices", "n_states", "plan")),
    "avr_cabac_encode_chunked_second_pass_device": ("avr_cabac_chunked_workspace_bytes", ("n_slices", "n_states", "plan")),
    "avr_cabac8_encode_chunked_device": ("avr_cabac8_chunked_workspace_bytes", ("n_slices", "n_states", "plan")),
    "avr_range_encode_chunked_device": ("avr_range_chunked_workspace_bytes", ("n_slices", "plan", "out_total")),
    "avr_range_resolve_device": ("avr_range_resolve_workspace_bytes", ("n_slices", "n_groups", "plan")),
    "avr_range_keys_verify_device": ("avr_range_keys_verify_workspace_bytes", ("n_slices", "n_groups", "plan")),
    "avr_cabac_resolve_device": ("avr_cabac_resolve_workspace_bytes", ("n_slices", "n_states", "plan")),
    "avr_cabac_encode_resolved_device": ("avr_cabac_resolved_workspace_bytes", ("n_slices", "plan")),
}
PARTS = "avr_cabac_encode_chunked_device_parts"


def entry_points():
    """{name: [(parameter, is a pointer)]} of every int avr_*_device*() the header declares, in its order"""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "avrecode_ms_amd.h")).read(), flags=re.S)
    found = {}
    for name, params in re.findall(r"\bint\s+(avr_\w*_device\w*)\s*\(([^)]*)\)\s*;", text):
        found[name] = [(re.findall(r"\w+", p)[-1], "*" in p) for p in params.split(",")]
    return found


def _plan(slot, null=()):
    p = avr.ChunkPlan()
    for k, f in enumerate(_PLAN_PTRS):
        setattr(p, f, None if f in null or "all" in null else _BASE + 256 * (slot + k))
    p.res_total, p.dig_total, p.total_chunks, p.total_blocks = 64, 64, 2, 1
    return p


def _pointers(params):
    return [n for n, ptr in params if ptr and n not in ("stream", "plan", "cfg", "parts")]


def _call(handle, fn, params, over=(), null=(), plan_null=(), shift=None, short=0):
    """one call: the sound arguments, then `over` (name -> value), `null` (pointers left null; "all": every one), `plan_null` (fields of
    the plan struct left null; "all": every one), `shift` (pointer name -> bytes its address is moved by), `short` (bytes the workspace
    is short of what its quote function asks for)"""
    a, keep = dict(_SCALARS), []
    a.update(over)
    for k, n in enumerate(_pointers(params)):
        a.setdefault(n, None if n in null or "all" in null else _BASE + 256 * k + ((shift or {}).get(n, 0)))
    names = [n for n, _ in params]
    if "plan" in names and "plan" not in a:
        plan = None if "plan" in null or "all" in null else _plan(40, plan_null)
        keep.append(plan)
        a["plan"] = None if plan is None else ctypes.addressof(plan)
    if "cfg" in names:
        cfg = avr.SynthConfig()
        assert handle.avr_synth_config_init(ctypes.byref(cfg), 2, 1000, 0) == 0
        keep.append(cfg)
        a["cfg"] = None if "cfg" in null or "all" in null else ctypes.byref(cfg)
    if "workspace_bytes" in names and "workspace_bytes" not in a:
        quote, args = _QUOTES[fn]
        a["workspace_bytes"] = max(0, getattr(handle, quote)(*[a[x] for x in args]) - short)
    rc = getattr(handle, fn)(*[a[n] for n in names])
    return [rc, handle.avr_last_error().decode() if rc < 0 else ""]


def _parts_call(handle, n_parts=2, over=(), part_over=(), part_null=(), plan_null=(), shift=None, short=0, no_parts=False):
    """the same for avr_cabac_encode_chunked_device_parts: part_over, part_null, plan_null, shift and short change the LAST part"""
    a = dict(device=0, stream=None, recs=_BASE, n_states=4, out=_BASE + 256)
    a.update(over)
    parts, keep = (avr.ChunkedPart * max(n_parts, 1))(), []
    for i in range(min(n_parts, len(parts))):
        last = i == n_parts - 1
        q, f = parts[i], dict(n_slices=1, rows_hint=4)
        f.update(part_over if last else ())
        plan = _plan(40, plan_null if last else ())
        keep.append(plan)
        for k, n in enumerate(_PART_PTRS):
            v = ctypes.addressof(plan) if n == "plan" else _BASE + 256 * (2 + k) + ((shift or {}).get(n, 0) if last else 0)
            f.setdefault(n, None if last and (n in part_null or "all" in part_null) else v)
        quote = handle.avr_cabac_chunked_workspace_bytes(f["n_slices"], a["n_states"], f["plan"])
        f.setdefault("workspace_bytes", max(0, quote - (short if last else 0)))
        for n, v in f.items():
            setattr(q, n, v)
    rc = getattr(handle, PARTS)(a["device"], a["stream"], a["recs"], a["n_states"], a["out"], None if no_parts else parts, n_parts)
    return [rc, handle.avr_last_error().decode() if rc < 0 else ""]


def _parts_cases(handle):
    c = lambda **kw: (lambda: _parts_call(handle, **kw))
    yield "sound", c()
    yield "one part", c(n_parts=1)
    for n in ("recs", "out"):
        yield f"null {n}", c(over={n: None})
        yield f"{n} + 1 byte", c(over={n: _BASE + 1})
    yield "null parts", c(no_parts=True)
    for n in (0, avr.MAX_PARTS + 1):
        yield f"n_parts = {n}", c(n_parts=n)
    for n in _PART_PTRS:
        yield f"part: null {n}", c(part_null=(n,))
        if n != "plan":
            yield f"part: {n} + 1 byte", c(shift={n: 1})
    for f in _PLAN_PTRS:
        yield f"part: null plan.{f}", c(plan_null=(f,))
    yield "part: every pointer null but the plan, n_slices = 0", c(part_over=dict(n_slices=0, plan=None), part_null=("all",), plan_null=("all",))
    for v in _PAST["n_states"]:
        yield f"n_states = {v}", c(over=dict(n_states=v))
    yield "part: n_slices = 2^31", c(part_over=dict(n_slices=1 << 31))
    yield "part: workspace one byte short", c(short=1)


def cases(handle, fn, params):
    """(label, call) for one entry point; call() -> [return code, message]"""
    if fn == PARTS:
        yield from _parts_cases(handle)
        return
    c = lambda **kw: (lambda: _call(handle, fn, params, **kw))
    names, ptrs = [n for n, _ in params], _pointers(params)
    yield "sound", c()
    for n in ptrs + [x for x in ("plan", "cfg") if x in names]:
        yield f"null {n}", c(null=(n,))
    if "plan" in names:
        for f in _PLAN_PTRS:
            yield f"null plan.{f}", c(plan_null=(f,))
        yield "every pointer null but the plan, n_slices = 0", c(over=dict(n_slices=0), null=ptrs, plan_null=("all",))
    yield "every pointer null, n_slices = 0", c(over=dict(n_slices=0), null=("all",))
    for n, values in _PAST.items():
        for v in values if n in names else ():
            yield f"{n} = {v}", c(over={n: v})
    for n in ptrs:
        yield f"{n} + 1 byte", c(shift={n: 1})
    if "workspace_bytes" in names:
        yield "workspace one byte short", c(short=1)
    for other in ("recs_out", "recs"):
        if "keys" in names and other in names:
            yield f"{other} aliases keys", c(over={other: _BASE + 256 * ptrs.index("keys")})


def table(handle, skip=lambda fn, label: False):
    """every case of every entry point run on `handle`, except those skip(fn, label) names"""
    out = {}
    for fn, params in entry_points().items():
        out[fn] = {label: call() for label, call in cases(handle, fn, params) if not skip(fn, label)}
    return out
