"""The device workspaces are laid out once, in csrc/avr_layout.h: the quote functions return a layout's total and the launchers
carve by the same struct.  tests/layout_check.cpp compiles that header with g++ alone and prints every layout over a grid of
shapes; here the regions are held to be in order, apart, 256-byte aligned (but for the two documented exceptions) and to end at
the total, the total to be what the library's public function quotes -- and the quotes to be the numbers recorded below from the
library BEFORE the layouts moved into the header, so that a layout change shows in review as an edited number.  No device needed:
the quote functions read a plan's totals only."""
import ctypes
import itertools
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "layout_check.cpp")
EXE = os.path.join(ROOT, "tests", "_layout_check")
CSRC = os.path.join(ROOT, "avrecode-ms_amd", "csrc")

LENGTHS = (0, 1, 1023, 1024, 1025, 1049076)                   # bins of a slice: empty, one, around a chunk, 1 024 chunks and a bit
N_SLICES = (0, 1, 3, 64, 513)
N_STATES = (0, 1, 4, 86, 126, 460, 1024)
N_GROUPS = (1, 5)
QUOTES = ("avr_cabac_chunked_workspace_bytes", "avr_cabac8_chunked_workspace_bytes", "avr_range_chunked_workspace_bytes",
          "avr_range_resolve_workspace_bytes", "avr_cabac_resolve_workspace_bytes", "avr_cabac_resolved_workspace_bytes")
MAX_STATES8 = 126


def plan_totals(n_slices, first):
    """(res_total, dig_total, total_chunks, total_blocks, out_total) of n_slices slices whose lengths go round LENGTHS from
    LENGTHS[first] on, as avrecode_ms_amd/device.py plans them."""
    n = [LENGTHS[(first + i) % len(LENGTHS)] for i in range(n_slices)]
    return (sum((x + 15) // 16 * 16 + 16 for x in n), sum(x // 2 + 8 for x in n), sum(max(1, (x + 1023) // 1024) for x in n),
            sum(max(1, (x + 4095) // 4096) for x in n), sum((x + 16 + 7) // 8 * 8 for x in n))


def grid():
    """(n_slices, n_states, n_groups, first) of every shape."""
    return list(itertools.product(N_SLICES, N_STATES, N_GROUPS, range(len(LENGTHS))))


def quotes(L, shape):
    """The six public quotes for a shape, in QUOTES' order."""
    n_slices, n_states, n_groups, first = shape
    res_total, dig_total, total_chunks, total_blocks, out_total = plan_totals(n_slices, first)

    class Plan(ctypes.Structure):
        _fields_ = [(name, ctypes.c_void_p) for name in ("res_off", "chunk_base", "chunk_slice", "blk_base", "blk_slice", "dig_off")]
        _fields_ += [("res_total", ctypes.c_uint64), ("dig_total", ctypes.c_uint64), ("total_chunks", ctypes.c_uint32),
                     ("total_blocks", ctypes.c_uint32)]
    plan = ctypes.byref(Plan(None, None, None, None, None, None, res_total, dig_total, total_chunks, total_blocks))
    z = ctypes.c_size_t
    for name in QUOTES:
        getattr(L, name).restype = z
    return (L.avr_cabac_chunked_workspace_bytes(z(n_slices), z(n_states), plan),
            L.avr_cabac8_chunked_workspace_bytes(z(n_slices), z(n_states), plan),
            L.avr_range_chunked_workspace_bytes(z(n_slices), plan, ctypes.c_uint64(out_total)),
            L.avr_range_resolve_workspace_bytes(z(n_slices), z(n_groups), plan),
            L.avr_cabac_resolve_workspace_bytes(z(n_slices), z(n_states), plan),
            L.avr_cabac_resolved_workspace_bytes(z(n_slices), plan))


# (n_slices, n_states, n_groups, first): the six quotes.  Recorded from the library of the commit before csrc/avr_layout.h existed
# (e93c715), built in a checkout of its own:   python tests/test_layouts.py <that checkout>/avrecode-ms_amd/libavrecode_hip.so
RECORDED = {
    (0, 0, 1, 0): (79104, 79104, 4352, 256, 78592, 256),
    (1, 1, 1, 0): (211968, 211968, 5376, 12848, 79872, 66560),
    (1, 4, 1, 1): (214016, 214016, 5376, 12848, 81920, 66560),
    (1, 86, 1, 5): (4941056, 4941056, 4214016, 802352, 568576, 3258368),
    (1, 1024, 5, 5): (8423680, 0, 4214016, 802352, 4051200, 3258368),
    (3, 86, 1, 2): (361728, 361728, 17920, 12848, 223488, 72704),
    (3, 126, 5, 3): (5224192, 5224192, 4222208, 802352, 847616, 3262464),
    (3, 460, 1, 4): (6806016, 0, 4218112, 802352, 2431488, 3260416),
    (64, 0, 1, 0): (44508160, 44508160, 42228224, 7957232, 1770240, 32121088),
    (64, 86, 5, 0): (50018816, 50018816, 42228224, 7957232, 7280896, 32121088),
    (64, 126, 1, 3): (57370368, 57370368, 46436864, 8746736, 10392064, 35312896),
    (64, 1024, 5, 5): (117430272, 0, 46432768, 8746736, 70454016, 35310848),
    (513, 4, 1, 1): (378873088, 378873088, 358841088, 67579168, 16554240, 272534528),
    (513, 86, 5, 0): (422153472, 422153472, 358836992, 67579168, 59836672, 272532480),
    (513, 460, 1, 2): (618595072, 0, 358845184, 67579168, 256274176, 272536576),
    (513, 1024, 5, 4): (922640384, 0, 363045632, 68368672, 556083200, 275724288),
}


@pytest.fixture(scope="module")
def layouts():
    """{shape: {layout: [offsets ..., total]}} and the sizeofs, from the stand-alone program."""
    deps = [SRC, os.path.join(CSRC, "avr_layout.h"), os.path.join(CSRC, "avr_k1p.h"), os.path.join(CSRC, "avr_chunk.h")]
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in deps):
        subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I" + CSRC, "-o", EXE, SRC], check=True)
    shapes = grid()
    text = "".join("%d %d %d %d %d %d %d %d\n" % ((s[0], s[1], s[2]) + plan_totals(s[0], s[3])) for s in shapes)
    out = subprocess.run([EXE], input=text, capture_output=True, text=True, check=True).stdout.split("\n")
    assert out[0].startswith("sizeof ") and len(out) == 1 + 5 * len(shapes) + 1
    sizes = dict(zip(("stretch", "entry", "totals", "summ"), map(int, out[0].split()[1:])))
    table = {}
    for i, s in enumerate(shapes):
        rows = [line.split() for line in out[1 + 5 * i:6 + 5 * i]]
        assert [r[0] for r in rows] == ["resolve", "code", "k1p", "k2p", "est"]
        table[s] = {r[0]: list(map(int, r[1:])) for r in rows}
    return table, sizes


def region_bytes(shape, sizes, lay):
    """What each region of each layout has to hold, restated from what the kernels index: {layout: [bytes per region]}."""
    n_slices, ns, n_groups, first = shape
    res_total, dig_total, chunks, _, out_total = plan_totals(n_slices, first)
    tiles = (chunks + 63) // 64 * 64 * 1024
    rows = 2 * ((chunks + 15) // 16)
    return {
        "resolve": [(chunks + 64) * 128, (chunks + 64) * ns * 2 + 256, chunks * ((ns + 3) // 4) * 4 + 16, chunks * sizes["stretch"],
                    256 + 2048 + 2048 + 128 * 511, n_slices * ns * 16 * sizes["summ"]],
        "code": [chunks * sizes["stretch"], chunks * sizes["entry"], n_slices * sizes["totals"], dig_total * 4 + 16, tiles],
        "k1p": [max(tiles, res_total + 32), lay["resolve"][-1], lay["code"][-1]],
        "k2p": [chunks * 8, chunks * 4, n_slices * 8, n_slices * 4, 4096, out_total * 4 + 64],
        "est": [4 * n_slices, 4 * n_groups, rows * 1028 * 4, rows * 1028 * 2],
    }


def test_regions_are_in_order_apart_aligned_and_end_at_the_total(layouts):
    table, sizes = layouts
    for shape, lay in table.items():
        need = region_bytes(shape, sizes, lay)
        for name, v in lay.items():
            starts, total = v[:-1], v[-1]
            if name == "resolve":
                assert starts[1] % 256 == 128, (shape, name)        # lend: 128 bytes into its region (the chain reads lend[-1])
                starts[1] -= 128
            assert len(starts) == len(need[name])
            ends = [a + n for a, n in zip(starts, need[name])]
            assert starts[0] == 0 and all(e <= a for e, a in zip(ends, starts[1:])), (shape, name, v)
            assert ends[-1] <= total < ends[-1] + 256, (shape, name, v)
            for k, a in enumerate(starts):
                if (name, k) != ("est", 3):                         # row16: directly behind row32, unrounded
                    assert a % 256 == 0, (shape, name, k)
        assert lay["est"][3] == lay["est"][2] + need["est"][2]
        assert lay["k1p"][2] == lay["k1p"][1] + lay["resolve"][-1]  # the code workspace begins at resolve.total


@pytest.mark.parametrize("build", ["product", "hooks"])
def test_totals_are_what_the_library_quotes(avr, layouts, build):
    L = ctypes.CDLL(avr.LIB_PATH if build == "product" else avr.HOOKS_LIB_PATH)
    table, _ = layouts
    for shape, lay in table.items():
        k1p = lay["k1p"][-1]
        want = (k1p, k1p if shape[1] <= MAX_STATES8 else 0, lay["k2p"][-1], lay["est"][-1], lay["resolve"][-1], lay["code"][-1])
        assert quotes(L, shape) == want, shape


@pytest.mark.parametrize("build", ["product", "hooks"])
def test_library_still_quotes_the_recorded_sizes(avr, build):
    L = ctypes.CDLL(avr.LIB_PATH if build == "product" else avr.HOOKS_LIB_PATH)
    assert len(RECORDED) >= 12
    for shape, want in RECORDED.items():
        assert quotes(L, shape) == want, shape


# The plan of three slices of 0xfffffff0 bins and an empty one (tests/test_plan.py: test_offsets_and_totals_above_4g), 86 contexts:
# res_total, dig_total, total_chunks, total_blocks, out_total, and what the library quotes for it -- K1p, K1p's phases B-D, K2p
FAR_TOTALS = (12884901904, 6442450952, 12582913, 3145729, 12884901904)
FAR_QUOTES = {"avr_cabac_chunked_workspace_bytes": 57428808960, "avr_cabac_resolved_workspace_bytes": 39208420352,
              "avr_range_chunked_workspace_bytes": 51690607872}


def far_quotes(L, res_total, dig_total, out_total):
    shape_plan = (res_total, dig_total) + FAR_TOTALS[2:4]

    class Plan(ctypes.Structure):
        _fields_ = [(name, ctypes.c_void_p) for name in ("res_off", "chunk_base", "chunk_slice", "blk_base", "blk_slice", "dig_off")]
        _fields_ += [("res_total", ctypes.c_uint64), ("dig_total", ctypes.c_uint64), ("total_chunks", ctypes.c_uint32),
                     ("total_blocks", ctypes.c_uint32)]
    plan = ctypes.byref(Plan(None, None, None, None, None, None, *shape_plan))
    z = ctypes.c_size_t
    for name in FAR_QUOTES:
        getattr(L, name).restype = z
    return {"avr_cabac_chunked_workspace_bytes": L.avr_cabac_chunked_workspace_bytes(z(4), z(86), plan),
            "avr_cabac_resolved_workspace_bytes": L.avr_cabac_resolved_workspace_bytes(z(4), plan),
            "avr_range_chunked_workspace_bytes": L.avr_range_chunked_workspace_bytes(z(4), plan, ctypes.c_uint64(out_total))}


@pytest.mark.parametrize("build", ["product", "hooks"])
def test_quotes_of_a_plan_above_4g(avr, build):
    """Totals that do not fit in 32 bits: the quotes are the recorded numbers, hold what the kernels index (the code buffer of
    res_total + 32 bytes, four bytes to a digit sum, four to a byte of out_total) and grow by exactly what a total grows by --
    a quote computed in 32 bits would wrap between one step and the next."""
    L = ctypes.CDLL(avr.LIB_PATH if build == "product" else avr.HOOKS_LIB_PATH)
    res_total, dig_total, _, _, out_total = FAR_TOTALS
    G = 1 << 32
    q = far_quotes(L, res_total, dig_total, out_total)
    assert q == FAR_QUOTES and all(v > G for v in q.values())
    assert q["avr_cabac_chunked_workspace_bytes"] >= res_total + 32 + q["avr_cabac_resolved_workspace_bytes"]
    assert q["avr_cabac_resolved_workspace_bytes"] >= 4 * dig_total + 16 and q["avr_range_chunked_workspace_bytes"] >= 4 * out_total + 64
    for step in (256, G - 256, G, 5 * G):                        # (multiples of 256: the regions are rounded to that)
        more_res = far_quotes(L, res_total + step, dig_total, out_total)
        more_dig = far_quotes(L, res_total, dig_total + step // 4, out_total)
        more_out = far_quotes(L, res_total, dig_total, out_total + step // 4)
        tiled = (FAR_TOTALS[2] + 63) // 64 * 64 * 1024             # the code buffer holds the larger of the tiled and the linear form
        linear = (res_total + step + 32 + 255) // 256 * 256
        assert tiled == 12884967424 and more_res["avr_cabac_chunked_workspace_bytes"] == q["avr_cabac_chunked_workspace_bytes"] - tiled + max(tiled, linear)
        assert more_dig["avr_cabac_chunked_workspace_bytes"] == q["avr_cabac_chunked_workspace_bytes"] + step
        assert more_dig["avr_cabac_resolved_workspace_bytes"] == q["avr_cabac_resolved_workspace_bytes"] + step
        assert more_out["avr_range_chunked_workspace_bytes"] == q["avr_range_chunked_workspace_bytes"] + step


if __name__ == "__main__":                                       # record: the table above, from the library given
    lib = ctypes.CDLL(sys.argv[1])
    picks = [s for s in grid() if (s[0], s[1], s[2], s[3]) in {
        (0, 0, 1, 0), (1, 1, 1, 0), (1, 4, 1, 1), (1, 86, 1, 5), (1, 1024, 5, 5), (3, 86, 1, 2), (3, 126, 5, 3), (3, 460, 1, 4),
        (64, 0, 1, 0), (64, 86, 5, 0), (64, 126, 1, 3), (64, 1024, 5, 5), (513, 4, 1, 1), (513, 86, 5, 0), (513, 460, 1, 2), (513, 1024, 5, 4)}]
    for s in picks:
        print("    %r: %r," % (s, quotes(lib, s)))
