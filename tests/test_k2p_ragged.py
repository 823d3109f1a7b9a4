"""The batches of tests/k2p_ragged.py held to their preconditions on the CPU, before tests/test_gpu_k2p_ragged.py takes them to the
device: the cut and the number of long slices each batch is built for, the lists that fill the hybrid's grid to its last block, both
sides of the cut present for every kind of special slice, the oracle's statuses for the planted slices -- and, by the CPU emulation of
K2p's double-precision walk (tests/k2p_emul.cpp), that a collapse hands its slice over at the planted bin while the certain records
do not.  cut() itself is held to the definition it restates, by trying every power of two.  These tests are what keeps the device
tests from quietly losing their mix when a builder is edited."""
import subprocess

import numpy as np
import pytest

import bad_records as br
import k2p_ragged as kr
from k2p_ragged import CHUNK_BINS
from test_k2p_emul import emul                                   # noqa: F401 (the fixture that builds tests/_k2p_emul.so)
from test_layouts import EXE, layouts                            # noqa: F401 (the fixture that builds tests/_layout_check)
from test_range_domain import fp_walk


def chunks(slices):
    return [kr.chunks_of(len(s)) for s in slices]


# ------------------------------------------------------------------ the rule

def brute_cut(chunks_, max_long):
    """The definition, tried power by power."""
    for k in range(32):
        long_ = [i for i, c in enumerate(chunks_) if c >= 1 << k]
        if len(long_) <= max_long:
            return 1 << k, long_
    return kr.NONE, []


def test_cut_is_the_smallest_power_of_two_that_fits():
    rng = np.random.default_rng(3190)
    cases = [([], 5), ([1], 0), ([1], 1), ([3, 3, 3], 2), ([3, 3, 3], 3), ([4, 4, 4, 3], 3), ([4, 4, 4, 3], 2), ([2, 1, 1], 1),
             ([1 << 31, 1 << 31, 1], 1), ([1 << 31, 1 << 31, 1], 2), ([(1 << 32) - 1] * 3, 2), ([1] * 70, 64), ([7] * 70, 70)]
    for _ in range(300):
        n = int(rng.integers(1, 400))
        top = int(rng.choice([1, 2, 3, 9, 40, 5000]))
        c = rng.integers(1, top + 1, n).tolist()
        if rng.random() < 0.3:
            c = [int(rng.choice([1, 2, 4, 8, 16]))] * n              # all equal, on a power of two
        max_long = int(rng.choice([0, 1, n // 2, n - 1, n, n + 3, sum(x >= 2 for x in c), sum(x >= 4 for x in c)]))
        cases.append((c, max_long))                                 # (the last two: a count of exactly max_long, where there is one)
    exact = 0
    for c, max_long in cases:
        t, long_ = kr.cut(c, max_long)
        assert (t, long_) == brute_cut(c, max_long), (c[:20], max_long)
        assert t == kr.NONE or (t & (t - 1) == 0 and len(long_) <= max_long)
        exact += len(long_) == max_long > 0
    assert exact > 30
    assert kr.cut([(1 << 32) - 1] * 3, 2) == (kr.NONE, []) and kr.cut([1 << 31] * 2 + [1 << 30], 2) == (1 << 31, [0, 1])
    assert kr.cut([4, 4, 4, 3], 3) == (4, [0, 1, 2]) and kr.cut([4, 4, 4, 3], 2) == (8, [])          # a tie does not split
    assert [kr.chunks_of(n) for n in (0, 1, CHUNK_BINS, CHUNK_BINS + 1, 2 * CHUNK_BINS)] == [1, 1, 1, 2, 2]


def test_shape_is_launch_k2ps_table():
    assert kr.shape(1024) == (16, 1008, "wave") and kr.shape(1025) == (17, 1007, "hybrid")
    assert kr.shape(kr.N_RAGGED) == (18, 1006, "hybrid")
    assert kr.shape(61440) == (960, 64, "hybrid") and kr.shape(61441) == (961, 63, "lane")
    assert [n for n in range(1, 70000) if kr.shape(n)[2] == "hybrid"] == list(range(1025, 61441))


def test_the_long_list_fits_its_region(layouts):                  # noqa: F811
    """threshold, count and the list: 2 + count words in the 4 096 bytes csrc/avr_layout.h reserves.  By shape the hybrid runs for
    1 025 .. 61 440 slices, where max_long is at most 1 007; forced by the hook k2p_wave = 3 on fewer slices, the count is at most the
    slice count up to 64 slices, and from 65 slices on at most max_long <= 1 022."""
    out = subprocess.run([EXE], input="1100 0 1 0 0 1300 0 2000000\n", capture_output=True, text=True, check=True).stdout.split("\n")
    k2p = [int(x) for x in next(line for line in out if line.startswith("k2p ")).split()[1:]]
    words = (k2p[5] - k2p[4]) // 4                                # long_chunks up to sums
    assert words == 1024
    for n in range(1025, 61441):
        assert kr.shape(n)[2] == "hybrid" and 2 + kr.shape(n)[1] <= words
    assert max(kr.shape(n)[1] for n in range(1025, 61441)) == 1007
    for n in range(1, 65):
        assert 2 + n <= words
    for n in range(65, 1025):
        assert kr.shape(n)[1] <= 1022 and 2 + kr.shape(n)[1] <= words


# ------------------------------------------------------------------ the batches

@pytest.mark.parametrize("name", kr.BATCHES)
def test_cut_and_count_are_what_the_batch_is_built_for(name):
    make, threshold, count = kr.BATCHES[name]
    slices, special = make()
    lane_blocks, max_long, form = kr.shape(len(slices))
    assert all(s.dtype == np.uint16 for s in slices)
    if threshold is None:
        assert form != "hybrid"
        return
    assert form == "hybrid"
    t, long_ = kr.cut_of(slices)
    print(f"{name}: {len(slices)} slices, {sum(len(s) for s in slices)} bins, threshold {t}, {len(long_)} long")
    assert (t, len(long_)) == (threshold, count)
    if name in ("brim", "wide"):
        assert lane_blocks + len(long_) == kr.GRID and long_[-1] == len(slices) - 1      # the grid's last block walks a listed slice
    if name in ("brim_plus_one", "wide_plus_one"):
        assert sum(c >= 2 for c in chunks(slices)) == max_long + 1                      # one too many for a cut of 2


def test_forms_at_their_boundaries():
    forms = kr.edge_forms()
    assert {n: kr.shape(n)[2] for n in forms} == {1024: "wave", 1025: "hybrid", 61440: "hybrid", 61441: "lane"}
    for n, ((slices, _), form) in forms.items():
        assert len(slices) == n and kr.shape(n)[2] == form
    a, b = forms[1024][0][0], forms[1025][0][0]
    assert all(x is y for x, y in zip(a, b))                      # the same slices, one fewer
    assert kr.chunks_of(len(b[1023])) > 1 and kr.chunks_of(len(b[1024])) > 1
    w, w1 = forms[61440][0][0], forms[61441][0][0]
    assert all(x is y for x, y in zip(w, w1)) and 0 < len(w1[-1]) < 9
    two = [i for i, c in enumerate(chunks(w)) if c == 2]
    assert len(two) == 64 and two[0] == 0 and two[-1] == 61439 and max(len(s) for i, s in enumerate(w) if i not in set(two)) <= 8
    assert len({i // 64 for i in two}) > 50                       # spread over the batch


def test_mixed_has_the_blocks_and_lengths_it_names():
    slices, special = kr.mixed()
    c, n = chunks(slices), [len(s) for s in slices]
    assert len(slices) == kr.N_RAGGED
    for i, v in kr.MIXED_FIXED.items():
        assert n[i] == v and i not in special
    assert set(kr.MIXED_LONG_FIXED) <= set(n) and max(c) == 16 and {2, 3, 9, 12} <= set(c)
    per_block = [sum(x >= 2 for x in c[b:b + 64]) for b in range(0, len(c), 64)]
    assert per_block[kr.MIXED_ALL_LONG] == 64 and per_block[kr.MIXED_ONE_LONG] == 1 and per_block[kr.MIXED_NO_LONG] == 0
    assert all(n[i] > 0 for i in range(64 * kr.MIXED_NO_LONG, 64 * kr.MIXED_NO_LONG + 64))   # the lanes of that block all walk
    assert c[0] >= 2 and c[-1] >= 2 and len(c) % 64 != 0                                     # slice 1 099: in the last, partial block
    one = [x for x, k in zip(n, c) if k == 1]
    assert 960 <= len(one) <= 1000 and sum(x < 200 for x in one) > 0.9 * len(one)
    assert sum(n) < 450_000


def test_cut4_has_the_lengths_it_names():
    slices, special = kr.cut4()
    c, n = chunks(slices), [len(s) for s in slices]
    assert len(slices) == kr.N_RAGGED and {3 * CHUNK_BINS, 3 * CHUNK_BINS + 1} <= set(n)
    assert min(c) == 2 and {2, 3, 4, 5, 7, 8, 9, 16} <= set(c)
    assert 1000 <= sum(k in (2, 3) for k in c) <= 1040 and sum(n) < 2_000_000
    for i, v in kr.CUT4_FIXED.items():
        assert n[i] == v and i not in special


@pytest.mark.parametrize("name", ["mixed", "cut4"])
def test_every_special_kind_on_both_sides_of_the_cut(name, oracle, emul):   # noqa: F811
    """A non-empty slice of every kind below the cut (a lane's) and at or above it (a wave's) -- but that in `mixed`, whose lane
    slices have one chunk, a collapse at bin 1 024 or 1 025 exists on the wave side only.  The oracle's statuses are the claims:
    both outcomes of a collapse on both sides, the malformed records seen by bad_records' rule.  The double-precision walk
    (k2p_emul_fp_walk: range_step_fp as the kernels run it) leaves at the planted collapse and nowhere else."""
    slices, special = kr.BATCHES[name][0]()
    threshold, long_ = kr.cut_of(slices)
    long_ = set(long_)
    seen = {"lane": {}, "wave": {}}
    for i, (kind, claim) in special.items():
        s = slices[i]
        side = "wave" if i in long_ else "lane"
        assert len(s) > 0 and kind not in seen[side]
        seen[side][kind] = claim
        bad = br.breaks_rule(br.KIND_RANGE, s)
        status = oracle.range_encode(s)[1]
        assert bad == (claim == "bad") and (bad or status == kr.STATUS_OF[claim]), (i, kind, claim, status)
        assert br.expected(br.KIND_RANGE, s)[0] == kr.STATUS_OF[claim]
        if kind.startswith("collapse@"):
            at = kind.split("@")[1]
            at = int(at) if at != "last" else max(k for k in range(len(s)) if not (s[k] >> 8) & 0x7f)
            assert (int(s[at]) & 0x7f01) == 0 and (int(s[at]) >> 1) & 0x7f and fp_walk(emul, s) == len(s) + 1 + at
            assert kind != "collapse@last" or kr.chunks_of(at + 1) == kr.chunks_of(len(s))
        elif not bad:
            assert fp_walk(emul, s) == len(s)                     # the pairs and the certain records: no hand-over
        if kind == "pairs":
            pos, neg = (s >> 1) & 0x7f, (s >> 8) & 0x7f
            assert pos.min() >= 1 and neg.min() >= 1 and (pos + neg).max() == 254    # on BOTH sides
            assert {(127, 127), (127, 1), (1, 127)} <= set(zip(pos.tolist(), neg.tolist()))
            assert side == "wave" or set(kr.CORNERS) <= set(s.tolist())   # (a short draw: the corners put in, either bin of each)
        if bad and side == "wave":                                # in a late chunk: a later segment under k2p_seg_len 1 and 3
            at = np.flatnonzero(((s & 0x8000) != 0) | ((s & 0x7ffe) == 0))
            assert at.size == 1 and at[0] >= 3 * CHUNK_BINS and kr.chunks_of(at[0] + 1) == kr.chunks_of(len(s))
    only_wave = {f"collapse@{CHUNK_BINS}", f"collapse@{CHUNK_BINS + 1}"} if name == "mixed" else set()
    assert set(seen["wave"]) == set(kr.KINDS) and set(seen["lane"]) == set(kr.KINDS) - only_wave
    for side in seen:
        outcomes = {claim for kind, claim in seen[side].items() if kind.startswith("collapse@")}
        assert outcomes == {"coded", "zero"}, side
    if name == "mixed":                                           # what the device test of short regions counts on
        lane, wave = kr.short_region_picks(slices, special, kr.wants(name, oracle))
        assert lane not in long_ and wave in long_ and not {lane, wave} & set(special)
    # every other slice is clean and coded
    rng = np.random.default_rng(1)
    for i in rng.choice(len(slices), 40, replace=False):
        if int(i) not in special:
            assert not br.breaks_rule(br.KIND_RANGE, slices[i]) and oracle.range_encode(slices[i])[1] == 0
