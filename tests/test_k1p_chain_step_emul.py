"""The per-chunk step of K1p's context chains on the CPU: chain_step of avrecode-ms_amd/csrc/avr_k1p.h -- the function a lane of
k_k1p_ctxchain, k_k1p_chain_seg and k_k1p_chain_fix runs for every chunk -- compiled for the host by tests/chain_step_emul.cpp, with
the look-up table made by the function the device makes it with, against a walk of the transition table bin by bin.

The step takes a run's first (length % 8) bins through the table's section for that many bins and the rest as whole bytes through the
section for eight; the first 96 bins come out of a 128-bit window the caller loaded, what follows is fetched from the chunk's bit
string as it goes.  So a case is (state, where the run starts in its dword, how long it is, the bits): every state, every start,
every length up to 130 -- beyond the window -- and runs that end with the chunk's last bin, up to a whole chunk in one context."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import oracle_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "chain_step_emul.cpp")
CSRC = os.path.join(ROOT, "avrecode-ms_amd", "csrc")
N_STATES = 126                                                   # pStateIdx <= 62: pStateIdx 63 is never walked (its lanes get a run of 0 bins)


@pytest.fixture(scope="module")
def emul():
    so = os.path.join(ROOT, "tests", "_chain_step_emul.so")
    deps = [SRC] + [os.path.join(CSRC, h) for h in ("avr_k1p.h", "avr_chunk.h", "avr_tables.h", "avr_div.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I" + CSRC, "-o", so, SRC], check=True)
    lib = ctypes.CDLL(so)
    lib.chain_emul_chunk_bins.restype = ctypes.c_uint32
    lib.chain_emul_tn_bytes.restype = ctypes.c_uint32
    lib.tn = np.zeros(lib.chain_emul_tn_bytes(), np.uint8)
    lib.chain_emul_tn(oracle_lib.ptr(lib.tn))
    return lib


@pytest.fixture(scope="module")
def step_table(avr):
    """T[s, b]: the state after bin b in state s (cabac_code.h:43-47 on libavcodec's table), s < 128."""
    _, mlps = avr.cabac_tables()
    mlps = np.frombuffer(bytes(mlps), np.uint8).astype(np.uint32)
    s = np.arange(128)
    t = np.zeros((128, 2), np.uint32)
    for b in (0, 1):
        t[:, b] = np.where((s & 1) == b, mlps[128 + s], mlps[127 - s])
    return t


def bit_strings(chunk):
    """Bit strings of one chunk (a row each, a byte a bin): coin flips, biased either way, runs of one value, alternating."""
    rng = np.random.default_rng(4242)
    rows = [rng.integers(0, 2, chunk), rng.random(chunk) < 0.1, rng.random(chunk) < 0.9, np.zeros(chunk), np.ones(chunk), np.arange(chunk) & 1,
            (np.arange(chunk) // 13) & 1]
    return np.array(rows, np.uint8)


def pack(bins, chunk):
    """A row of bit_strings as the device keeps it: bin i in bit i % 32 of dword i / 32; four dwords behind it that are NOT the
    string's (all ones: a step that took bins from there would show)."""
    d = np.zeros(chunk // 32 + 4, np.uint32)
    d[:chunk // 32] = (bins.reshape(-1, 32).astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(axis=1).astype(np.uint32)
    d[chunk // 32:] = 0xffffffff
    return d


def walk(step_table, bins, pos, left, st):
    """Bin by bin: the states `st` after the runs bins[pos .. pos + left)."""
    st = st.copy()
    order = np.argsort(-left, kind="stable")                     # longest first: the runs that still have bin i are a prefix
    n_live = np.searchsorted(-left[order], -np.arange(int(left.max(initial=0))), side="left")
    for i, n in enumerate(n_live):
        live = order[:n]
        b = bins[pos[live] + i]
        st[live] = step_table[st[live], b if st.ndim == 1 else b[:, None]]
    return st


def run_cases(emul, step_table, bins, pos, left, ns):
    chunk = emul.chain_emul_chunk_bins()
    assert (pos + left <= chunk).all()
    pos, left = np.ascontiguousarray(pos, np.uint32), np.ascontiguousarray(left, np.uint32)
    n = pos.size
    first = np.arange(n) % N_STATES                              # every state in turn; walked beside it, one that differs
    st = first if ns == 1 else np.stack([first, (first * 7 + 3 + np.arange(n) // N_STATES) % N_STATES], axis=1)
    st = np.ascontiguousarray(st, np.uint32)
    want = walk(step_table, bins, pos.astype(np.int64), left.astype(np.int64), st)
    got = st.copy()
    P = oracle_lib.ptr
    emul.chain_emul_steps(P(emul.tn), P(pack(bins, chunk)), ctypes.c_uint64(n), P(pos), P(left), ctypes.c_uint32(ns), P(got))
    bad = np.flatnonzero((got != want).reshape(n, -1).any(axis=1))
    assert bad.size == 0, f"{bad.size} of {n} cases, first: pos {pos[bad[0]]} left {left[bad[0]]} from {st[bad[0]]}: {got[bad[0]]}, not {want[bad[0]]}"


def test_table_is_the_walk_of_its_index(emul, step_table):
    """tn[tn_section(n) + (s << n | bits)] is the state after the n bins `bits`, first bin in the low bit, n = 0 .. 8."""
    for n in range(9):
        s, bits = np.divmod(np.arange(128 << n), 1 << n)
        st = s.astype(np.uint32)
        for b in range(n):
            st = step_table[st, (bits >> b) & 1]
        assert (emul.tn[(128 << n) - 128:(128 << (n + 1)) - 128] == st).all(), n


@pytest.mark.parametrize("ns", [1, 2])
def test_every_state_start_and_length(emul, step_table, ns):
    """All 126 states x every start bit in a dword x run lengths 0 .. 130, on four kinds of bit string; which dword the run starts in
    moves with the case (the last ones included: the window then reaches past the string)."""
    chunk = emul.chain_emul_chunk_bins()
    sh, left, s = np.meshgrid(np.arange(32), np.arange(131), np.arange(N_STATES), indexing="ij")
    sh, left = sh.ravel(), left.ravel()                          # (the state is the case's number mod 126: run_cases)
    for row, bins in enumerate(bit_strings(chunk)[[0, 1, 4, 6]]):
        rng = np.random.default_rng(row)
        dword = rng.integers(0, chunk // 32, sh.size)
        pos = dword * 32 + sh
        pos = np.where(pos + left > chunk, (chunk - left) // 32 * 32 - 32 + sh, pos)      # the same start bit, in the last dword it fits
        run_cases(emul, step_table, bins, pos, left, ns)


@pytest.mark.parametrize("ns", [1, 2])
def test_runs_that_end_with_the_chunk(emul, step_table, ns):
    """Runs [chunk - n, chunk) for every n up to 130 and every 37th up to the whole chunk in one context, from every state: the last
    fetches of a long run are the string's last dwords."""
    chunk = emul.chain_emul_chunk_bins()
    left = np.repeat(np.concatenate([np.arange(131), np.arange(131, chunk, 37), [chunk]]), N_STATES)
    for bins in bit_strings(chunk):
        run_cases(emul, step_table, bins, chunk - left, left, ns)


def test_parked_states_stay_on_a_run_of_no_bins(emul, step_table):
    """The callers give a lane at pStateIdx 63 (states 126, 127) no bins: the step's one unconditional look-up is the identity."""
    chunk = emul.chain_emul_chunk_bins()
    st = np.ascontiguousarray(np.arange(128).repeat(32), np.uint32)
    pos = np.ascontiguousarray(np.tile(np.arange(32), 128) + 32 * 5, np.uint32)
    got = st.copy()
    P = oracle_lib.ptr
    emul.chain_emul_steps(P(emul.tn), P(pack(bit_strings(chunk)[0], chunk)), ctypes.c_uint64(st.size), P(pos), P(np.zeros(st.size, np.uint32)),
                          ctypes.c_uint32(1), P(got))
    assert (got == st).all()
