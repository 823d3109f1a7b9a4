"""What a batch's slice lengths decide -- the arrays of an avr_chunk_plan, the output regions, the choice of path -- is written once
in C++ (csrc/avr_plan.h) and once in Python (chunk_plan_arrays and plan_tiles in avrecode_ms_amd/device.py).  tests/plan_check.cpp compiles the
header with g++ alone and prints every array for lists of lengths; here the two are held to each other element for element, to the
numbers below (worked out by hand from the rules as they stood, spread over csrc/avr_api.cpp, before the header existed) and to
plan_totals() of tests/test_layouts.py, a third statement of the rules.  The kernels index these arrays unchecked.  No device needed."""
import os
import subprocess

import numpy as np
import pytest

from test_layouts import LENGTHS, N_SLICES, plan_totals

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "plan_check.cpp")
EXE = os.path.join(ROOT, "tests", "_plan_check")
CSRC = os.path.join(ROOT, "avrecode-ms_amd", "csrc")

FIXED = [0, 1, 1023, 1024, 1025, 4096, 4097, 70000]
PER_SLICE = {                                                     # name: (per slice of FIXED, total)
    "chunks": ([1, 1, 1, 1, 2, 4, 5, 69], 84),
    "blocks": ([1, 1, 1, 1, 1, 1, 2, 18], 26),
    "work": ([16, 32, 1040, 1040, 1056, 4112, 4128, 70016], 81440),
    "digits": ([8, 8, 519, 520, 520, 2056, 2056, 35008], 40695),
    "out": ([16, 24, 1040, 1040, 1048, 4112, 4120, 70016], 81416),
}
PREFIX = {"out_off": "out", "res_off": "work", "dig_off": "digits", "chunk_base": "chunks", "blk_base": "blocks"}
PATHS = [((1, 8191), False), ((1, 8192), True), ((3, 24575), False), ((3, 24576), True), ((32768, 32768 * 8192), True),
         ((32769, 32769 * 8192), False)]


def batches():
    """The lists of lengths the C++ and the Python plans are compared on."""
    seeded = np.random.default_rng(20).integers(0, 200001, 300).tolist()
    return [FIXED, [], [0], seeded]


@pytest.fixture(scope="module")
def plan_check():
    """run(text) -> the stand-alone program's output lines."""
    deps = [SRC] + [os.path.join(CSRC, h) for h in ("avr_plan.h", "avr_layout.h", "avr_k1p.h", "avr_chunk.h")]
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in deps):
        subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I" + CSRC, "-o", EXE, SRC], check=True)
    return lambda text: subprocess.run([EXE], input=text, capture_output=True, text=True, check=True).stdout.split("\n")


def cpp_plan(run, lengths):
    """{name: [values]} of one list of lengths: the per-slice values, the arrays of the K1p plan, "totals", "lesser"."""
    out = run("plan %d %s\n" % (len(lengths), " ".join(map(str, lengths))))
    names = ["chunks", "blocks", "work", "digits", "out", "out_off", "res_off", "dig_off", "chunk_base", "chunk_slice", "blk_base",
             "blk_slice", "totals", "lesser"]
    assert [line.split()[0] for line in out[:-1]] == names and out[-1] == ""
    return {line.split()[0]: list(map(int, line.split()[1:])) for line in out[:-1]}


def cpp_big_plan(run, lengths):
    """cpp_plan for slices of millions of chunks: "slices" (the two sizes, and whether every entry is in place) stands for
    chunk_slice and blk_slice."""
    out = run("big %d %s\n" % (len(lengths), " ".join(map(str, lengths))))
    names = ["chunks", "blocks", "work", "digits", "out", "out_off", "res_off", "dig_off", "chunk_base", "blk_base", "slices", "totals", "lesser"]
    assert [line.split()[0] for line in out[:-1]] == names and out[-1] == ""
    return {line.split()[0]: list(map(int, line.split()[1:])) for line in out[:-1]}


def test_fixed_numbers(plan_check):
    p = cpp_plan(plan_check, FIXED)
    for name, (per_slice, total) in PER_SLICE.items():
        assert p[name] == per_slice and sum(per_slice) == total, name
    for name, of in PREFIX.items():                               # exclusive prefix sums, the total appended
        assert p[name] == [sum(PER_SLICE[of][0][:i]) for i in range(len(FIXED) + 1)], name
        assert p[name][-1] == PER_SLICE[of][1]
    assert p["chunk_slice"] == [i for i, k in enumerate(PER_SLICE["chunks"][0]) for _ in range(k)]
    assert p["blk_slice"] == [i for i, k in enumerate(PER_SLICE["blocks"][0]) for _ in range(k)]
    assert p["totals"] == [81440, 40695, 84, 26]
    assert p["lesser"] == [1]                                    # the lesser paths: the same arrays, the others left empty


def test_want_chunked(plan_check):
    out = plan_check("".join("path %d %d\n" % shape for shape, _ in PATHS))
    assert out == ["path %d" % want for _, want in PATHS] + [""]
    assert plan_check("path 0 0\n")[0] == "path 0"                # an empty batch divides by nothing


@pytest.mark.parametrize("which", range(4))
def test_cpp_against_python(plan_check, which):
    import torch
    from avrecode_ms_amd.device import chunk_plan_arrays
    lengths = batches()[which]
    p = cpp_plan(plan_check, lengths)
    t, totals = chunk_plan_arrays(torch.tensor(lengths, dtype=torch.int32))
    assert sorted(t) == ["blk_base", "blk_slice", "chunk_base", "chunk_slice", "dig_off", "res_off"]
    for name, tensor in t.items():
        assert tensor.dtype == (torch.int64 if name in ("res_off", "dig_off") else torch.int32), name
        assert tensor.tolist() == p[name], name
    assert list(totals) == p["totals"] and p["lesser"] == [1]
    assert p["out_off"][-1] == sum((x + 16 + 7) // 8 * 8 for x in lengths)


def test_tile_plan_cpp_against_python(plan_check):
    """plan_tiles of csrc/avr_plan.h and of avrecode_ms_amd/device.py, element for element: lengths full of ties and zeros, so that the
    stable order is what is compared, and slice counts either side of a tile's 64, so that the tiles' boundaries are."""
    import torch
    from avrecode_ms_amd.device import plan_tiles
    rng = np.random.default_rng(64)
    for n in (0, 1, 63, 64, 65, 129):
        lengths = rng.choice([0, 1, 7, 8, 9, 16, 17, 1000], n).tolist()
        for per_chunk in (8, 16):
            out = plan_check("tiles %d %d %s\n" % (per_chunk, n, " ".join(map(str, lengths))))
            assert [line.split()[0] for line in out[:-1]] == ["order", "tile_off"] and out[-1] == ""
            order, tile_off = (list(map(int, line.split()[1:])) for line in out[:-1])
            want_order, want_tile_off = plan_tiles(torch.tensor(lengths, dtype=torch.int32), per_chunk)
            assert want_order.dtype == torch.int32 and want_tile_off.dtype == torch.int64
            assert (order, tile_off) == (want_order.tolist(), want_tile_off.tolist()), (n, per_chunk)
            assert sorted(order) == list(range(n)) and len(tile_off) == (n + 63) // 64 + 1


def test_totals_against_the_layout_tests(plan_check):
    import torch
    from avrecode_ms_amd.device import chunk_plan_arrays
    for n_slices in N_SLICES:
        for first in range(len(LENGTHS)):
            lengths = [LENGTHS[(first + i) % len(LENGTHS)] for i in range(n_slices)]
            p = cpp_plan(plan_check, lengths)
            assert tuple(p["totals"] + [p["out_off"][-1]]) == plan_totals(n_slices, first), (n_slices, first)
            assert chunk_plan_arrays(torch.tensor(lengths, dtype=torch.int32))[1] == plan_totals(n_slices, first)[:4]


def test_offsets_and_totals_above_4g(plan_check):
    """Three slices of 0xfffffff0 bins and an empty one: out_off, res_off and dig_off pass 2^32 (the counts of chunks and blocks do
    not), in C++ and in Python alike and as the per-slice rules, worked out here in Python integers, say."""
    import torch
    from avrecode_ms_amd.device import chunk_plan_arrays
    big = 0xfffffff0
    lengths = [big, big, 0, big]
    G = 1 << 32
    p = cpp_big_plan(plan_check, lengths)
    assert p["out"] == [G, G, 16, G] and p["work"] == [G, G, 16, G] and p["digits"] == [G // 2, G // 2, 8, G // 2]
    assert p["chunks"] == [1 << 22, 1 << 22, 1, 1 << 22] and p["blocks"] == [1 << 20, 1 << 20, 1, 1 << 20]
    assert p["out_off"] == [0, G, 2 * G, 2 * G + 16, 3 * G + 16] and p["res_off"] == p["out_off"]
    assert p["dig_off"] == [0, G // 2, G, G + 8, 3 * G // 2 + 8]
    assert p["chunk_base"] == [0, 1 << 22, 1 << 23, (1 << 23) + 1, 3 * (1 << 22) + 1]
    assert p["blk_base"] == [0, 1 << 20, 1 << 21, (1 << 21) + 1, 3 * (1 << 20) + 1]
    assert p["totals"] == [12884901904, 6442450952, 12582913, 3145729] and p["totals"][0] > G and p["totals"][1] > G
    assert p["slices"] == [12582913, 3145729, 1] and p["lesser"] == [1]
    rules = {"out_off": lambda x: (x + 16 + 7) // 8 * 8, "res_off": lambda x: (x + 15) // 16 * 16 + 16, "dig_off": lambda x: x // 2 + 8,
             "chunk_base": lambda x: max(1, (x + 1023) // 1024), "blk_base": lambda x: max(1, (x + 4095) // 4096)}
    for name, rule in rules.items():
        assert p[name] == [sum(rule(x) for x in lengths[:i]) for i in range(len(lengths) + 1)], name
    t, totals = chunk_plan_arrays(torch.tensor(lengths, dtype=torch.int64))
    for name in ("res_off", "dig_off", "chunk_base", "blk_base"):
        assert t[name].tolist() == p[name], name
    assert list(totals) == p["totals"]
    for name, base in (("chunk_slice", "chunk_base"), ("blk_slice", "blk_base")):
        assert t[name].dtype == torch.int32
        assert np.array_equal(t[name].numpy(), np.repeat(np.arange(len(lengths), dtype=np.int32), np.diff(p[base]))), name
