"""K2 batches for pass 1 of K2p where lanes and waves share a launch (k_k2p_ranges_hybrid, csrc/avr_k2p.hip), and the rule by which
the launch divides a batch -- restated here from what k_k2p_threshold promises, not from how it counts.

launch_k2p picks pass 1's form by the number of slices alone (shape()); the hybrid's grid is GRID blocks, the first ceil(n / 64)
walk a lane per slice, the others a wave per LONG slice.  A slice is long when it has at least `threshold` chunks, the threshold
being the smallest power of two at which the long slices fit the blocks left over (cut()).  The batches below are built around the
places where that can go wrong: the cut and its ties, a list that fills the grid to its last block, a 64-slice block whose lanes all
stand aside, and -- on BOTH sides of the cut -- slices over the whole (pos, neg) domain, slices the double-precision walk must hand to
the integer one, certain records it must keep, and malformed records (specials()).  tests/test_k2p_ragged.py holds every batch to
what its docstring claims, on the CPU; tests/test_gpu_k2p_ragged.py takes them to the device.  numpy, the oracle and the makers of
range_domain.py, bad_records.py and oracle_lib.py: nothing here touches a device."""
import functools

import numpy as np

import bad_records as br
import oracle_lib
import range_domain as rd
from bad_records import CHUNK_BINS                               # AVR_CHUNK_BINS, as the package reports it

GRID = 1024                                                      # launch_k2p's kSimds: the blocks of the hybrid's one grid
NONE = 0xffffffff                                                # the threshold when not even the top class fits
N_RAGGED, N_WIDE = 1100, 61440                                   # 18 lane blocks, 1 006 left; 960 lane blocks, 64 left
COLLAPSE_AT = (0, CHUNK_BINS - 1, CHUNK_BINS, CHUNK_BINS + 1, "last")   # around the first chunk's end; in the last chunk
KINDS = (("pairs",) + tuple(f"collapse@{at}" for at in COLLAPSE_AT)
         + ("certain bin 1", "certain bin 0", "bit 15", "total 0"))
STATUS_OF = {"clean": br.SLICE_OK, "coded": br.SLICE_OK, "zero": br.SLICE_ZERO_PROB, "bad": br.SLICE_BAD_RECORD}
WAVE_BINS = 4 * CHUNK_BINS + 300                                 # a special slice on the long side: five chunks, at or above both cuts


# ------------------------------------------------------------------ the rule

def chunks_of(n_bins):
    """A slice's chunk count: an empty slice still has its one chunk."""
    return max(1, -(-int(n_bins) // CHUNK_BINS))


def cut(chunks, max_long):
    """(threshold, the long slices in order): the smallest power of two 2^k such that at most max_long slices have 2^k chunks or
    more -- NONE if there is no such power below 2^32 -- and the slices that have.  Put by rank: with the chunk counts in falling
    order, the slice of rank max_long (from 0) is the first that must NOT be long, so the threshold is the first power of two above
    its count; if there is no such slice, every slice may be long and the threshold is 1."""
    chunks = [int(c) for c in chunks]
    ranked = sorted(chunks, reverse=True)
    if max_long >= len(ranked):
        threshold = 1
    else:
        threshold = 1 << ranked[max_long].bit_length()           # bit_length(c) = k <=> 2^(k-1) <= c < 2^k
        if threshold >= 1 << 32:
            return NONE, []
    return threshold, [i for i, c in enumerate(chunks) if c >= threshold]


def shape(n_slices):
    """(lane_blocks, max_long, form): how launch_k2p walks pass 1 for a batch of that many slices -- "wave" (a wave per slice),
    "hybrid" (lanes plus waves: max_long blocks are left for the long slices) or "lane" (a lane per slice)."""
    lane_blocks = (n_slices + 63) // 64
    form = "wave" if n_slices <= GRID else "hybrid" if lane_blocks + 64 <= GRID else "lane"
    return lane_blocks, GRID - lane_blocks, form


def cut_of(slices):
    """cut() for a batch as launch_k2p would ask it."""
    return cut([chunks_of(len(s)) for s in slices], shape(len(slices))[1])


# ------------------------------------------------------------------ streams

def _plain(rng, n, k):
    """A random stream of oracle_lib: the adaptive form (a Python loop a bin) for short slices only."""
    return oracle_lib.random_range_stream(rng, int(n), adaptive=bool(k % 3) and n <= 300)


def _domain(rng, n, mode="match"):
    """n records drawn over all of [1, 127]^2 (range_domain.all_pairs_slice, cut short)."""
    return rd.all_pairs_slice(rng, mode, 0)[:n].copy()


CORNERS = tuple(rd.rec(b, pos, neg) for pos, neg in ((127, 127), (127, 1), (1, 127)) for b in (1, 0))


def _corners(s):
    """The slice with the domain's corners written over six of its records, spread from front to back, either bin of each: a short
    draw holds (127, 127) only by luck, and a total of 254 is what reads the last entry of the tables by total."""
    for j, r in enumerate(CORNERS):
        s[(j + 1) * len(s) // (len(CORNERS) + 1)] = r
    return s


def _collapse(s, at, claim):
    """Plant `bin 0, pos p, neg 0` at `at`: the new range is range mod p.  p is chosen by the oracle on the slice's front so that the
    bin is coded (a remainder above 0) or is a bin of probability zero (a remainder of 0; p = 1 always gives one)."""
    for p in ((127, 77, 5, 3, 2) if claim == "coded" else (2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 16, 1)):
        s[at] = rd.rec(0, p, 0)
        if br.oracle().range_encode(s[:at + 1])[1] == STATUS_OF[claim]:
            return s
    raise AssertionError(f"no p makes the collapse at {at} {claim}")


def specials(rng, lane_bins):
    """[(side, kind, claim, records)]: every kind of KINDS once for the lane side (slices of lane_bins bins or fewer: below the
    batch's cut) and once for the wave side (WAVE_BINS bins, five chunks; the pairs slice all 16 129 pairs, 16 chunks).
      pairs           every (pos, neg) of [1, 127]^2 / a short draw from them with the corners (127, 127), (127, 1), (1, 127) put in
                      (_corners): a total of 254 on both sides
      collapse@at     `bin 0, pos p, neg 0` at bin 0, around the first chunk's end (COLLAPSE_AT) and in the slice's last chunk (a later segment under k2p_seg_len
                      1 and 3 on the wave side), where the slice has such a bin: the double-precision walk hands the slice to
                      k_k2p_ranges.  claim "coded": the oracle codes it; "zero": range mod p is 0, AVR_SLICE_ZERO_PROB.  The claims
                      alternate along COLLAPSE_AT, so both occur on both sides
      certain bin 1   `bin 1, neg 0`, and
      certain bin 0   `bin 0, pos 0`: the range stays, no hand-over, claim "clean"
      bit 15, total 0 a malformed record inside [0, n): AVR_SLICE_BAD_RECORD; on the wave side in the last chunk"""
    out = []
    for side, n in (("lane", lane_bins), ("wave", WAVE_BINS)):
        last = n - 6
        out.append((side, "pairs", "clean", _corners(_domain(rng, n - 37, "anti")) if side == "lane" else rd.all_pairs_slice(rng, "anti", 0)))
        for k, at in enumerate(COLLAPSE_AT):
            a = last if at == "last" else at
            if a < n:
                out.append((side, f"collapse@{at}", "zero" if k % 2 else "coded", _collapse(_domain(rng, n), a, "zero" if k % 2 else "coded")))
        out.append((side, "certain bin 1", "clean", br.spoil(_domain(rng, n - 1), last - 9, rd.rec(1, 77, 0))))
        out.append((side, "certain bin 0", "clean", br.spoil(_domain(rng, n - 2), last - 3, rd.rec(0, 0, 93))))
        out.append((side, "bit 15", "bad", br.spoil(_plain(rng, n - 3, 0), last - 5, 0x8000 | rd.rec(1, 5, 9))))
        out.append((side, "total 0", "bad", br.spoil(_plain(rng, n - 4, 0), last - 7, 0x0000)))
    return out


def _place(rng, slices, pool, lane_bins):
    """Replace slices of `pool` (ordinary ones) by the special slices: {slice: (kind, claim)}."""
    special = {}
    at = [int(i) for i in rng.permutation(sorted(pool))]
    for i, (_, kind, claim, recs) in zip(at, specials(rng, lane_bins)):
        slices[i] = recs.astype(np.uint16)
        special[i] = (kind, claim)
    return special


# ------------------------------------------------------------------ the batches

N_SCATTERED = 50
MIXED_FIXED = {10: 0, 11: 1, 12: 7, 13: 8, 14: 9, 15: CHUNK_BINS - 1, 16: CHUNK_BINS}                 # one chunk each
# the first scattered long slices: a bin into the second chunk, two chunks whole, a bin more, a bin into the ninth; the last: 12 chunks
MIXED_LONG_FIXED = (CHUNK_BINS + 1, 2 * CHUNK_BINS, 2 * CHUNK_BINS + 1, 8 * CHUNK_BINS + 1, 11 * CHUNK_BINS + 5)
MIXED_ALL_LONG, MIXED_ONE_LONG, MIXED_NO_LONG = 3, 5, 6                         # 64-slice blocks: slices 192-255, 320-383, 384-447


@functools.lru_cache(maxsize=None)
def mixed(seed=3101):
    """(slices, special): 1 100 slices, cut 2.  One-chunk slices, mostly under 200 bins, with 0, 1, 7, 8, 9 bins, a chunk less one bin
    and a whole chunk among them (MIXED_FIXED); 50 scattered slices of 2 to 12 chunks (MIXED_LONG_FIXED among them: a chunk and a bin,
    two chunks, two and a bin, eight and a bin); the whole block 192-255 long;
    slice 0 and slice 1 099 (in the last, partial block) long; block 320-383 with exactly one long slice, block 384-447 with none;
    then the special slices in place of ordinary ones outside those three blocks.  The long slices: 64 + 50 + 3 + the wave side's
    specials."""
    rng = np.random.default_rng(seed)
    n = N_RAGGED
    lengths = rng.integers(2, 200, n)
    some = rng.choice(n, 60, replace=False)
    lengths[some] = rng.integers(200, CHUNK_BINS + 1, some.size)
    for i, v in MIXED_FIXED.items():
        lengths[i] = v
    blocks = {b: set(range(64 * b, 64 * b + 64)) for b in (MIXED_ALL_LONG, MIXED_ONE_LONG, MIXED_NO_LONG)}
    kept = set(MIXED_FIXED) | {0, n - 1} | set().union(*blocks.values())
    free = [i for i in range(n) if i not in kept]
    scattered = sorted(int(i) for i in rng.choice(free, N_SCATTERED, replace=False))
    for k, i in enumerate(scattered):
        c = 2 + (int(rng.integers(1, 11)) if k % 5 == 0 else int(rng.integers(0, 2)))
        lengths[i] = MIXED_LONG_FIXED[k] if k < len(MIXED_LONG_FIXED) else (c - 1) * CHUNK_BINS + int(rng.integers(1, 200))
    for i in blocks[MIXED_ALL_LONG]:
        lengths[i] = rng.integers(CHUNK_BINS + 1, CHUNK_BINS + 300)
    lengths[0], lengths[n - 1] = 2 * CHUNK_BINS + 77, CHUNK_BINS + 1
    lengths[64 * MIXED_ONE_LONG + 41] = 3 * CHUNK_BINS + 9
    slices = [_plain(rng, v, i) for i, v in enumerate(lengths)]
    pool = [i for i in free if i not in scattered]
    return slices, _place(rng, slices, pool, CHUNK_BINS)


# three chunks whole: just below the cut; a bin more: just above; two chunks and four, whole and a bin more
CUT4_FIXED = {20: 3 * CHUNK_BINS, 21: 3 * CHUNK_BINS + 1, 22: 2 * CHUNK_BINS, 23: 2 * CHUNK_BINS + 1, 24: 4 * CHUNK_BINS, 25: 4 * CHUNK_BINS + 1}
CUT4_LONG = (4, 5, 4, 7, 4, 8, 5, 9, 4, 16, 4, 5)                                         # chunks of the long slices, in turn
N_CUT4_LONG = 70


@functools.lru_cache(maxsize=None)
def cut4(seed=3102):
    """(slices, special): 1 100 slices, cut 4.  Slices of 2 and 3 chunks, so that the lanes walk across chunk notes and segment seams
    (three whole chunks, just below the cut, among them); 70 slices of 4, 5, 7, 8, 9 and 16 chunks and those of CUT4_FIXED with three
    chunks and a bin, four chunks, and four and a bin above it; the special slices, the lane side's with 3 chunks."""
    rng = np.random.default_rng(seed)
    n = N_RAGGED
    lengths = np.where(rng.random(n) < 0.7, 1, 2) * CHUNK_BINS + rng.integers(1, 160, n)
    for i, v in CUT4_FIXED.items():
        lengths[i] = v
    free = [i for i in range(n) if i not in CUT4_FIXED]
    long_ = sorted(int(i) for i in rng.choice(free, N_CUT4_LONG, replace=False))
    for k, i in enumerate(long_):
        lengths[i] = (CUT4_LONG[k % len(CUT4_LONG)] - 1) * CHUNK_BINS + int(rng.integers(1, 100))
    slices = [_plain(rng, v, i) for i, v in enumerate(lengths)]
    return slices, _place(rng, slices, [i for i in free if i not in long_], 2 * CHUNK_BINS + 452)


def brim(n_two=1006, n_four=0):
    """(slices, {}): 1 100 slices, n_two of them of two chunks (slice 1 099 among them), the others of one; n_four of the two-chunk
    slices lengthened to four.  1 006: the cut is 2 and the list fills the grid to its last block.  1 007 (brim_plus_one): the cut
    moves to 4 and nothing is long -- or, with n_four = 7, those seven."""
    return _brim(n_two, n_four)


@functools.lru_cache(maxsize=None)
def _brim(n_two, n_four, seed=3103):
    rng = np.random.default_rng(seed)
    n = N_RAGGED
    two = [n - 1] + [int(i) for i in rng.permutation(n - 1)[:n_two - 1]]
    lengths = rng.integers(0, 200, n)
    lengths[two] = rng.integers(CHUNK_BINS + 1, CHUNK_BINS + 80, n_two)
    if n_four:
        lengths[two[3:3 + n_four]] = rng.integers(3 * CHUNK_BINS + 1, 3 * CHUNK_BINS + 80, n_four)
    return [_plain(rng, v, i) for i, v in enumerate(lengths)], {}


def brim_plus_one(n_four=0):
    return brim(1007, n_four)


def wide(n_two=64, more=0):
    """(slices, {}): 61 440 + more slices, n_two of them of two chunks spread over the batch (the first and slice 61 439 among
    them), all others of 0 to 8 bins.  64: the cut is 2 and the list fills the 64 blocks the lanes leave.  65 (wide_plus_one): cut 4,
    nothing long.  more = 1: one slice too many for the hybrid -- a lane per slice."""
    return _wide(n_two, more)


@functools.lru_cache(maxsize=None)
def _wide(n_two, more, seed=3104):
    rng = np.random.default_rng(seed)
    if more:
        return _wide(n_two, 0)[0] + [_plain(rng, 3 + k, 0) for k in range(more)], {}
    lengths = rng.integers(0, 9, N_WIDE)
    two = [0, N_WIDE - 1] + [int(i) for i in 1 + rng.permutation(N_WIDE - 2)[:n_two - 2]]
    lengths[two] = rng.integers(CHUNK_BINS + 1, CHUNK_BINS + 60, n_two)
    flat = oracle_lib.random_range_stream(rng, int(lengths.sum()), adaptive=False)
    return np.split(flat, np.cumsum(lengths)[:-1]), {}


def wide_plus_one():
    return wide(65)


@functools.lru_cache(maxsize=None)
def edge_1025(seed=3105):
    """(slices, {}): 1 025 slices -- the hybrid by shape, the last slice alone in block 16 -- ragged, 21 of them of 2 to 6 chunks,
    slices 1 023 and 1 024 among those.  Its first 1 024 slices are a wave per slice by shape."""
    rng = np.random.default_rng(seed)
    lengths = rng.integers(0, 300, 1025)
    long_ = [1023, 1024] + [int(i) for i in rng.permutation(1023)[:19]]
    lengths[long_] = rng.integers(1, 6, len(long_)) * CHUNK_BINS + rng.integers(1, 300, len(long_))
    return [_plain(rng, v, i) for i, v in enumerate(lengths)], {}


def edge_forms():
    """{slices: (batch, form)}: the forms' boundaries at 1 024 / 1 025 and 61 440 / 61 441 slices."""
    return {1024: ((edge_1025()[0][:1024], {}), "wave"), 1025: (edge_1025(), "hybrid"),
            N_WIDE: (wide(), "hybrid"), N_WIDE + 1: (wide(64, 1), "lane")}


# name: (the batch, the threshold, how many slices are long) -- None where the form does not ask
N_WAVE_SPECIALS = len(KINDS)
BATCHES = {
    "mixed": (mixed, 2, 64 + N_SCATTERED + 3 + N_WAVE_SPECIALS),
    "cut4": (cut4, 4, N_CUT4_LONG + 3 + N_WAVE_SPECIALS),         # + 3: those of CUT4_FIXED with four chunks or more
    "brim": (brim, 2, 1006),
    "brim_plus_one": (brim_plus_one, 4, 0),
    "brim_plus_one_seven": (lambda: brim_plus_one(7), 4, 7),
    "wide": (wide, 2, 64),
    "wide_plus_one": (wide_plus_one, 4, 0),
    "edge_1025": (edge_1025, 2, 21),
    "edge_1024": (lambda: edge_forms()[1024][0], None, None),
    "edge_61441": (lambda: edge_forms()[N_WIDE + 1][0], None, None),
}


def wants(name, oracle, threads=8):
    """[(bytes, status)] per slice: the oracle's, and AVR_SLICE_BAD_RECORD where a record breaks the rule of bad_records.py (the
    oracle does not look at bit 15).  The 61 440-slice batches through the threaded oracle."""
    slices, special = BATCHES[name][0]()
    if len(slices) > 4096:
        off = np.zeros(len(slices) + 1, np.uint64)
        off[1:] = np.cumsum([len(s) for s in slices])
        data, status = oracle.encode_batch(br.KIND_RANGE, np.concatenate(slices), off, None, 0, threads=threads)
        out = list(zip(data, status.tolist()))
    else:
        out = [oracle.range_encode(s) for s in slices]
    for i, (_, claim) in special.items():
        if claim == "bad":
            out[i] = (b"", br.SLICE_BAD_RECORD)
    return out


def short_region_picks(slices, special, wants_, need=80):
    """(a lane slice, a wave slice) for the device test that cuts two output regions to 64 bytes: the first clean, ordinary slice on
    either side of the cut that the oracle codes to `need` bytes or more (a one-chunk slice codes to under 100)."""
    long_ = set(cut_of(slices)[1])
    roomy = [i for i, (data, st) in enumerate(wants_) if st == br.SLICE_OK and len(data) >= need and i not in special]
    lane, wave = [i for i in roomy if i not in long_], [i for i in roomy if i in long_]
    assert lane and wave, f"no clean slice of {need} coded bytes on the {'wave' if lane else 'lane'} side of the cut"
    return lane[0], wave[0]
