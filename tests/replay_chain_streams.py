"""Bin streams for the replay's state chain (replay_step8 of csrc/avr_k1p.h): the step reads bin j+1's state byte before bin j's
write-back and takes bin j's successor instead where the two bins share a slot of the lane's column, so what matters is WHICH bins
share a context and where in a group of eight they lie.  The streams are over 4 contexts plus bypass and terminate, where collisions
are the rule, as Stream of tests/b1walk_streams.py (symbols M, L, B, T0, T1; records and codes by a walk of the contexts' states).

tests/test_k1p_replay_step_emul.py gives them to the host build of the step, tests/test_gpu_k1p_replay_chain.py codes them on the
device."""
import numpy as np

import b1walk_streams as bs
from b1walk_streams import CHUNK, M, L, B, T0, T1, Stream

LENGTHS = (3 * CHUNK, 3 * CHUNK - 5, CHUNK + 9, 700, 5)
STATES4 = (10, 37, 62, 91)
QUIET = 80                                                       # bins behind a chunk's start without a coded LPS: the lane before walks them as its tail


def _syms(rng, n, p_lps=0.25, quiet_tails=False):
    s = bs.background(rng, n, p_lps=p_lps, p_bypass=0.0, p_term0=0.0)
    if quiet_tails:
        for c in range(CHUNK, n, CHUNK):
            s[c:c + QUIET] = M
    s[-1] = T1
    return s


def neighbours(rng, n, j, quiet_tails):
    """Contexts by turns (no two bins closer than four share one), and in every group of eight bins j and j+1 in the same context:
    j = 7 is the pair across the groups, which is also the pair across every 64-byte line of records and across the chunks."""
    ctx = np.arange(n) % 4
    at = np.arange(j, n - 1, 8)
    ctx[at + 1] = ctx[at]
    return Stream(f"neighbours-{j}-{n}{'-quiet' if quiet_tails else ''}", _syms(rng, n, quiet_tails=quiet_tails), ctx, STATES4)


def runs(rng):
    """One context 2, 3, 8, 9 and 17 bins long from every place of a group, other contexts by turns between the runs."""
    syms, ctx = [], []
    for length in (2, 3, 8, 9, 17):
        for start in range(8):
            while len(ctx) % 8 != start or len(ctx) < 8:
                ctx.append(1 + len(ctx) % 3)
            ctx += [0] * length
            ctx.append(1 + len(ctx) % 3)
    ctx = np.array(ctx)
    syms = _syms(rng, ctx.size, p_lps=0.35)
    return Stream("runs", syms, ctx, STATES4)


def edges():
    """Context 0 driven to pStateIdx 0 by a run of coded LPS bins and on through it (valMPS flips at every further one), each bin's
    successor used by the next; context 1 driven to pStateIdx 62 by a run of MPS bins and parked there, then an LPS and on."""
    syms = [L] * 48 + [M, L, M, M] + [M] * 130 + [L, M, L, L, M] + [T1]
    ctx = [0] * 52 + [1] * 135 + [2]
    return Stream("edges", syms, ctx, STATES4)


def pseudo(rng, n):
    """Bypass beside bypass, terminate behind a context bin and behind terminate, and the slice's last real bin an LPS in context 3:
    with four contexts the padding's slot is 7, whose place in a row of four is context 3's."""
    s = _syms(rng, n)
    ctx = np.arange(n) % 4
    reps = max(1, (n - 8) // 11)
    for g in range(reps):
        at, k = 11 * g, max(0, min(7, n - 2 - 11 * g))
        s[at:at + k] = [B, B, M, T0, L, T0, T0][:k]
    if n >= 2:
        s[-2], ctx[-2] = L, 3
    s[-1] = L                                                    # no terminate at the end: the last real bin is context 3's
    ctx[-1] = 3
    return Stream(f"pseudo-{n}", s, ctx, STATES4)


def all_states(sym):
    """126 contexts, context k in state k: every state once as bin j (an MPS or an LPS) with bin j+1 in the same context."""
    ctx = np.repeat(np.arange(126), 2)
    syms = np.tile([sym, M], 126)
    return Stream(f"all-states-{'LM'[sym == M]}", syms, ctx, np.arange(126))


def device_streams():
    """The streams both tests run (about 60: the device codes them as one batch)."""
    rng = np.random.default_rng(54001)
    out = []
    for j in range(8):
        out.append(neighbours(rng, LENGTHS[j % 4], j, quiet_tails=False))
        out.append(neighbours(rng, LENGTHS[(j + 1) % 4], j, quiet_tails=True))
    out.append(neighbours(rng, 3 * CHUNK - 5, 7, quiet_tails=True))             # (3 * CHUNK is among the above)
    out.append(neighbours(rng, CHUNK + 9, 7, quiet_tails=True))
    for n in LENGTHS:
        out.append(Stream(f"a-b-a-b-{n}", _syms(rng, n, p_lps=0.35), np.arange(n) % 2, STATES4))
        out.append(pseudo(rng, n))
    out.append(runs(rng))
    out.append(edges())
    out.append(all_states(M))
    out.append(all_states(L))
    for n in LENGTHS:
        for nk in (2, 86):
            s = bs.background(rng, n, p_lps=0.2)
            s[-1] = T1
            out.append(Stream(f"random-{nk}-{n}", s, rng.integers(0, nk, n), rng.integers(0, 126, nk)))
    return out


def long_random(nk, n=200_000):
    rng = np.random.default_rng(54100 + nk)
    s = bs.background(rng, n, p_lps=0.2)
    return Stream(f"random-{nk}-{n}", s, rng.integers(0, nk, n), rng.integers(0, 126, nk))
