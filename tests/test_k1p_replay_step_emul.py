"""The replay's state chain on the CPU: replay_step8 of avrecode-ms_amd/csrc/avr_k1p.h -- what k_k1p_replay's `eight` and `eight8`
call: bin j+1's state byte is read before bin j's write-back and bin j's successor handed on where the two share a slot -- compiled
for the host by tests/replay_step_emul.cpp, a stand-alone program built with AddressSanitizer and UBSan, and held group by group to
the plain loop per bin (state byte, table entry, write-back): every entry, every code and the whole column after every group, from
two-byte and from one-byte records.  A child process with this one's environment as it is: nothing sanitised is loaded into this
process.

The streams are those of tests/replay_chain_streams.py; that they still hold the cases they were made for is checked here, on the
contexts and the codes, so that a stream that stopped covering its case fails."""
import os
import struct
import subprocess

import numpy as np
import pytest

import replay_chain_streams as rs
from b1walk_streams import B, L, M, T0

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "avrecode-ms_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "replay_step_emul.cpp")
BIN = os.path.join(ROOT, "tests", "_replay_step_emul")
DEPS = [os.path.join(CSRC, h) for h in ("avr_k1p.h", "avr_chunk.h", "avr_tables.h")]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0")
EVERY_ROW = 132 * 2 * 9 * 8                                      # the program's own walk of the table: bins


@pytest.fixture(scope="module")
def program():
    if not os.path.exists(BIN) or any(os.path.getmtime(s) > os.path.getmtime(BIN) for s in [SRC] + DEPS):
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I" + CSRC, "-o", BIN, SRC], check=True)
    return BIN


@pytest.fixture(scope="module")
def mlps(avr):
    return list(avr.cabac_tables()[1])


def walk(program, tmp_path, mlps, streams):
    path = tmp_path / "streams.bin"
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(streams)))
        for s in streams:
            recs, codes = s.resolve(mlps)
            f.write(struct.pack("<II", recs.size, s.states.size) + s.states.tobytes() + recs.tobytes() + codes.tobytes())
    r = subprocess.run([program, str(path)], capture_output=True, text=True, env=ENV, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    # both record widths, whole groups of eight
    assert r.stdout.split() == ["ok", str(EVERY_ROW + 2 * sum(-(-s.syms.size // 8) * 8 for s in streams))]


def same_context_pairs(s, gap=1):
    """Places i where bins i and i + gap are context bins of one context."""
    ctx, real = s.ctx[:s.syms.size], s.syms <= L
    return np.flatnonzero((ctx[:-gap] == ctx[gap:]) & real[:-gap] & real[gap:])


def test_constructed_streams(program, tmp_path, mlps):
    streams = rs.device_streams()
    by_name = {s.name: s for s in streams}
    assert len(by_name) == len(streams)
    walk(program, tmp_path, mlps, streams)
    # equal neighbours at every place of a group, inside a chunk and inside the tail past it (the quiet bins behind a chunk's start)
    for j in range(8):
        for quiet in (False, True):
            s = next(s for s in streams if s.name.startswith(f"neighbours-{j}-") and s.name.endswith("-quiet") == quiet)
            at = same_context_pairs(s)
            assert set(at % 8) == {j} and at.size >= s.syms.size // 8 - 8
            if quiet and s.syms.size > rs.CHUNK:
                behind = min(rs.QUIET - 8, s.syms.size - 1 - rs.CHUNK)           # (the slice of CHUNK + 9 bins: one pair)
                assert ((at >= rs.CHUNK) & (at < rs.CHUNK + behind)).sum() >= max(1, behind // 8)
                assert not (s.syms[rs.CHUNK:rs.CHUNK + rs.QUIET] == L).any()
    across = same_context_pairs(by_name[f"neighbours-7-{3 * rs.CHUNK}-quiet"])
    assert {31, 63, rs.CHUNK - 1, 2 * rs.CHUNK - 1} <= set(across.tolist())      # across a line of records of either width, across the chunks
    # A B A B: the second A is two bins behind the first and never beside it
    s = by_name[f"a-b-a-b-{3 * rs.CHUNK}"]
    assert same_context_pairs(s).size == 0 and same_context_pairs(s, 2).size > 3000
    # runs of one context from every place of a group
    ctx = by_name["runs"].ctx
    starts = np.flatnonzero((ctx == 0) & (np.concatenate([[1], ctx[:-1]]) != 0))
    ends = np.flatnonzero((ctx == 0) & (np.concatenate([ctx[1:], [1]]) != 0))
    assert sorted(zip((ends - starts + 1).tolist(), (starts % 8).tolist())) == [(n, j) for n in (2, 3, 8, 9, 17) for j in range(8)]
    # the state machine's edges, each with the next bin in the same context
    s = by_name["edges"]
    _, codes = s.resolve(mlps)
    state, lps = codes >> 1, ((codes >> 1) ^ codes) & 1
    pairs = same_context_pairs(s)
    assert ((state[pairs] <= 1) & (lps[pairs] == 1)).sum() >= 4           # an LPS at pStateIdx 0: valMPS flips
    assert {0, 1} <= set(state[pairs][state[pairs] <= 1].tolist())
    assert ((state[pairs] >= 124) & (lps[pairs] == 0)).sum() >= 4          # an MPS at pStateIdx 62: parked
    assert ((state[pairs] >= 124) & (lps[pairs] == 1)).any()
    # pseudo contexts: bypass beside bypass, terminate behind a context bin and behind terminate; the last real bin context 3's
    for n in rs.LENGTHS:
        s = by_name[f"pseudo-{n}"]
        assert s.syms[-1] == L and s.ctx[-1] == 3 and len(rs.STATES4) + 3 == 7
        two = list(zip(s.syms[:-1].tolist(), s.syms[1:].tolist()))
        assert (B, B) in two and (n < 8 or {(M, T0), (L, T0), (T0, T0)} <= set(two))
    assert sum(by_name[f"pseudo-{n}"].syms.size % 8 != 0 for n in rs.LENGTHS) >= 4    # masked last groups
    # every state x bin as a bin whose successor is handed on
    seen = set()
    for name in ("all-states-M", "all-states-L"):
        s = by_name[name]
        _, codes = s.resolve(mlps)
        seen |= set(codes[same_context_pairs(s)].tolist())
    assert seen >= set(range(252))


@pytest.mark.parametrize("nk", [2, 86])
def test_random_streams(program, tmp_path, mlps, nk):
    """200 000 bins over 2 contexts (half of all neighbours share one) and over 86."""
    walk(program, tmp_path, mlps, [rs.long_random(nk)])
