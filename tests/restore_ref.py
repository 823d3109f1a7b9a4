"""The restore check's reference answer and its table of cases, for tests/test_restore_emul.py and tests/test_gpu_restore_check.py.

The answer is plain Python: avr.drop_stop_byte and avr.tail_patch (the helpers the decompressor itself calls, held to the oracle's by
tests/test_cabi.py), the tail patch fed what the compressor writes into the container -- the parity of the payload's length and, for
payloads of two bytes and more, its last byte -- then a first-difference loop.  Nothing of csrc/avr_restore.h is in here.

The rule is a function of bytes: `out` need not be a CABAC stream, so the cases are arbitrary byte strings."""
import numpy as np

VERIFY_NONE = 0xFFFFFFFF
EXPECT_NONE = 0xFFFFFFFF
FILL = 0xFF                                                  # what the regions hold past L and past E

LENGTHS = (0, 1, 2, 7, 8, 9, 511 * 8, 512 * 8, 512 * 8 + 1, 70001)
TAILS = ("80", "8080", "none")                               # the coded bytes end ...80, end ...80 80, or have no stop byte
POSITIONS = (0, 7, 8, 8 * 63, 8 * 64, "R-2", "R-1")          # where a single byte is changed


def restored(avr, out, expect):
    """What decompress writes for a slice whose coded bytes are `out` and whose container fields were taken from `expect`."""
    body = avr.drop_stop_byte(bytes(out))
    if len(expect) < 2:                                      # no last byte recorded for size <= 1: no patch
        return body
    return avr.tail_patch(body, len(expect) & 1, expect[-1])


def first_diff(avr, out, expect):
    r, e = restored(avr, out, expect), bytes(expect)
    n = min(len(r), len(e))
    if r[:n] != e[:n]:
        for j in range(n):
            if r[j] != e[j]:
                return j
    return n if len(r) != len(e) else VERIFY_NONE


class Case:
    """out: the coded bytes -- min(out_len, capacity) of them; out_len: what the encoder is said to have reported (beyond the capacity in
    the cases that ask for the clamp, else len(out))."""

    def __init__(self, name, out, expect, out_len=None):
        self.name, self.out, self.expect = name, bytes(out), bytes(expect)
        self.out_len = len(self.out) if out_len is None else out_len

    def __repr__(self):
        return self.name


def _coded(rng, L, tail):
    """L arbitrary bytes with the asked tail, or None where L is too short for it."""
    need = {"80": 1, "8080": 2, "none": 0}[tail]
    if L < need:
        return None
    b = bytearray(rng.integers(0, 256, L, dtype=np.uint8).tobytes())
    if tail == "none":
        if L and b[-1] == 0x80:
            b[-1] = 0x81
    else:
        b[L - need:] = b"\x80" * need
    return bytes(b)


def _flip(b, p):
    b = bytearray(b)
    b[p] ^= 0x5A
    return bytes(b)


def table():
    """Every case of the issue's table, the same list on every call (seeded).  Per coded string (a length, a tail), with L1 its length
    after finish:
      E in {0, 1, 2, L1 - 2 .. L1 + 2}: the expectation is the restored bytes cut or continued with arbitrary bytes to that length;
      the two expectations that restore exactly (E = L1, the last byte patched over; E = L1 + 1, the last byte appended), then
      with a single byte changed at each of POSITIONS -- in the expectation, and in the coded bytes -- and with two bytes changed."""
    rng = np.random.default_rng(20261019)
    cases = []
    for L in LENGTHS:
        for tail in TAILS:
            out = _coded(rng, L, tail)
            if out is None:
                continue
            L1 = L - 1 if L and out[-1] == 0x80 else L
            tag = f"L{L}-{tail}"
            more = rng.integers(0, 256, 4, dtype=np.uint8).tobytes()
            for E in sorted({0, 1, 2, L1 - 2, L1 - 1, L1, L1 + 1, L1 + 2}):
                if E >= 0:
                    cases.append(Case(f"{tag}-E{E}", out, (out[:L1] + more)[:E]))
            for E in (L1, L1 + 1):                           # R == E: patched in place, appended
                if E < 2:
                    continue
                clean = (out[:L1] + more)[:E]
                R = E
                places = sorted({p if isinstance(p, int) else R - int(p[2:]) for p in POSITIONS})
                places = [p for p in places if 0 <= p < R]
                for p in places:
                    cases.append(Case(f"{tag}-E{E}-exp@{p}", out, _flip(clean, p)))
                    if p < L:
                        cases.append(Case(f"{tag}-E{E}-out@{p}", _flip(out, p), clean))
                for a, b in {(places[0], places[-1]), (places[len(places) // 2], places[0]), (places[1 % len(places)], places[-2 % len(places)])}:
                    if a != b:                               # two planted differences, in either order: the answer is the smaller
                        cases.append(Case(f"{tag}-E{E}-exp@{a}+{b}", out, _flip(_flip(clean, a), b)))
            if L % 8 == 0 and L:                             # a reported length beyond the capacity means the whole region, not a byte more
                cases.append(Case(f"{tag}-claimed", out, out[:L1], out_len=L + 1000))
                cases.append(Case(f"{tag}-claimed-exp@{L1 - 1}", out, _flip(out[:L1], max(L1 - 2, 0)), out_len=0xFFFFFFFF))
    return cases


def layout(cases, far=0):
    """The cases as one batch in buffers of exactly the stated sizes: out regions of capacity align8(L) holding FILL past L (a case
    with a claimed length beyond its capacity: the whole region is its string), expectations padded to 8 with FILL.  far: added to
    every offset.
    Returns (out, out_off, out_len, expect, expect_off, expect_len) as numpy arrays, out and expect WITHOUT the far base in front."""
    n = len(cases)
    out_off, expect_off = np.zeros(n + 1, np.int64), np.zeros(n, np.int64)
    out_len, expect_len = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    at = 0
    for i, c in enumerate(cases):
        expect_off[i] = at
        out_off[i + 1] = out_off[i] + (len(c.out) + 7) // 8 * 8
        out_len[i], expect_len[i] = c.out_len, len(c.expect)
        at += (len(c.expect) + 7) // 8 * 8
    out, expect = np.full(int(out_off[-1]), FILL, np.uint8), np.full(at, FILL, np.uint8)
    for i, c in enumerate(cases):
        out[out_off[i]:out_off[i] + len(c.out)] = np.frombuffer(c.out, np.uint8)
        expect[expect_off[i]:expect_off[i] + len(c.expect)] = np.frombuffer(c.expect, np.uint8)
    return out, out_off + far, out_len, expect, expect_off + far, expect_len
