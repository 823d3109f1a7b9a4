"""avr_multi's placement by units (csrc/avr_multi.h: avr::multi_place), a plain host function, against its Python twins.

tests/multi_plan_check.cpp is built with ASan + UBSan as a stand-alone program and run directly, nothing preloaded.  It places every
case below and checks what needs no twin (the loads add up, a group sits on one entry, no entry leads another by more than the heaviest
unit); this file compares the owners and loads it prints with sharding.lpt_assign_groups, and for one-slice units with the existing
sharding.lpt_assign.  The cases are seeded lists that include equal weights, zero weights, more entries than units, 1 and 64 entries,
groups of one slice and groups without slices."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from avrecode_ms_amd.sharding import lpt_assign, lpt_assign_groups

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "multi_plan_check.cpp")
SANITIZE = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def _groups(rng, n, n_groups, empty):
    """n_groups first-slice indices over n slices, the first 0; `empty`: some groups without slices (repeated indices)."""
    if n == 0:
        return [0] * n_groups
    cuts = sorted(rng.choice(np.arange(1, n), size=min(n_groups - 1, n - 1), replace=False).tolist()) if n > 1 and n_groups > 1 else []
    first = [0] + cuts
    if empty:
        for _ in range(3):
            at = int(rng.integers(0, len(first)))
            first.insert(at, first[at])                          # a group without slices in front of group `at`
        first.append(n)                                          # ... and one behind the last slice
    return first


def cases():
    rng = np.random.default_rng(20240611)
    out = []                                                     # (n_bins, group_first or None, n_entries)
    for world in (1, 2, 3, 4, 7, 64):
        for n in (0, 1, 2, 5, 40, 200):
            spread = rng.lognormal(7.5, 1.0, n).astype(np.int64).tolist()
            equal = [1000] * n
            zeros = [0 if i % 3 else int(v) for i, v in enumerate(spread)]
            few = rng.integers(0, 4, n).tolist()                 # many ties
            for bins in (spread, equal, zeros, few):
                out.append((bins, None, world))
                out.append((bins, list(range(n)), world))        # groups of one slice
                out.append((bins, _groups(rng, n, 7, False), world))
                out.append((bins, _groups(rng, n, 7, True), world))
    out.append(([0, 0, 0, 0], [0, 2], 3))                        # all weights zero: everything on entry 0
    out.append(([5, 5, 5], [0, 0, 0, 1, 3, 3], 64))              # more entries than units, empty groups around
    return out


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("multi_plan") / "multi_plan_check")
    subprocess.run([cxx] + SANITIZE + ["-std=c++17", "-Wall", "-Werror", "-o", exe, SRC], check=True)
    return exe


@pytest.fixture(scope="module")
def placed(program):
    """[(owners, loads)] of every case, from one run of the sanitized program."""
    cs = cases()
    lines = [str(len(cs))]
    for bins, first, world in cs:
        lines.append(f"{len(bins)} {-1 if first is None else len(first)} {world}")
        lines.append(" ".join(map(str, bins)))
        lines.append(" ".join(map(str, first or [])))
    p = subprocess.run([program], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert p.returncode == 0, p.stderr
    rows = p.stdout.split("\n")
    assert len(rows) >= 2 * len(cs)
    return [([int(x) for x in rows[2 * k].split()], [int(x) for x in rows[2 * k + 1].split()]) for k in range(len(cs))]


def test_the_cases_cover_what_they_name():
    cs = cases()
    assert any(w == 1 for _, _, w in cs) and any(w == 64 for _, _, w in cs)
    assert any(len(set(b)) == 1 and len(b) > 1 for b, _, _ in cs) and any(0 in b and any(b) for b, _, _ in cs)
    assert any(f is not None and len(set(f)) < len(f) for _, f, _ in cs)                       # groups without slices
    assert any(f is not None and f == list(range(len(b))) and len(b) > 1 for b, f, _ in cs)   # groups of one slice
    assert any(w > len(b) > 0 for b, _, w in cs)                                              # more entries than units


def test_groups_are_placed_as_the_python_twin_places_them(placed):
    n = 0
    for (bins, first, world), (owners, loads) in zip(cases(), placed):
        if first is None:
            continue
        want = lpt_assign_groups(bins, first, world)
        assert owners == want, (bins, first, world)
        assert loads == [sum(b for b, o in zip(bins, want) if o == e) for e in range(world)]
        n += 1
    assert n > 100


def test_slices_are_placed_as_lpt_assign_places_them(placed):
    """One-slice units, named as groups or not, are the existing rule element for element."""
    n = 0
    for (bins, first, world), (owners, loads) in zip(cases(), placed):
        if first is None or first == list(range(len(bins))):
            assert owners == lpt_assign(bins, world), (bins, first, world)
            assert sum(loads) == sum(bins) and len(loads) == world
            n += 1
    assert n > 100


def test_the_twin_keeps_a_group_together_and_skips_empty_ones():
    bins, first = [5, 1, 1, 9, 0, 3], [0, 0, 1, 3, 3, 4, 6]      # groups: {}, {0}, {1, 2}, {}, {3}, {4, 5}, {}
    assert lpt_assign_groups(bins, first, 2) == [1, 1, 1, 0, 1, 1]          # 9 -> 0; 5 -> 1; 3 -> 1 (5 < 9); 2 -> 1 (8 < 9)
    assert lpt_assign_groups(bins, first, 1) == [0] * 6
    assert lpt_assign_groups([], [0, 0], 3) == []
