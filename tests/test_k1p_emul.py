"""K1p (intra-slice parallel CABAC encode) on the CPU: the product's per-lane functions
(avrecode-ms_amd/csrc/avr_k1p.h, the code the HIP kernels wrap) are compiled for the host by
tests/k1p_emul.cpp and run chunk by chunk, then compared with the oracle.  This checks the
decomposition itself -- stretch summaries, the 4->4 chain, digit sums, carries, finish() --
without a GPU; tests/test_gpu_k1p.py checks the kernels.

The same source is also built at two other chunk lengths (-DAVR_TEST_CHUNK_BINS, which csrc/avr_chunk.h honours in host-only
builds): 256 and 4096 bins.  The chunk length is defined once, so every use of it in avr_k1p.h must follow; one that stayed a
literal 1024 fails both (tried: `lo = chunk * 1024, limit = lo + 1024` in b1_stretch miscodes at 4096 and, at 256, codes right
with a quarter of the stretches: see active_stretches).  Those builds decline no stretch for its
length, as the resolved-code entry point of the library does not (launch_k1p_code): the limit is kMaxStretch = 16 chunks, so what it
declines depends on the chunk length by design, and the tests about declined streams stay at the shipped length."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import oracle_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "k1p_emul.cpp")
CSRC = os.path.join(ROOT, "avrecode-ms_amd", "csrc")
OTHER_CHUNK_BINS = (256, 4096)                                   # the shipped length is 1024


def build_emul(chunk_bins=None):
    """tests/k1p_emul.cpp at the shipped chunk length, or at `chunk_bins`."""
    so = os.path.join(ROOT, "tests", "_k1p_emul.so" if chunk_bins is None else f"_k1p_emul_{chunk_bins}.so")
    deps = [SRC] + [os.path.join(CSRC, h) for h in ("avr_k1p.h", "avr_chunk.h", "avr_tables.h", "avr_div.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        define = [] if chunk_bins is None else [f"-DAVR_TEST_CHUNK_BINS={chunk_bins}"]
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I" + CSRC] + define + ["-o", so, SRC], check=True)
    lib = ctypes.CDLL(so)
    lib.k1p_emul_encode_resolved.restype = ctypes.c_size_t
    lib.div_emul_check.restype = ctypes.c_uint64
    lib.div_emul_check.argtypes = [ctypes.c_uint64, ctypes.c_uint64]
    return lib


@pytest.fixture(scope="module")
def emul():
    return build_emul()


@pytest.fixture(scope="module", params=OTHER_CHUNK_BINS)
def emul_other(request):
    lib = build_emul(request.param)
    lib.k1p_emul_set_max_stretch(ctypes.c_uint32(0xFFFFFFFF))
    lib.chunk_bins = request.param                           # k1p() then also counts the stretches: see active_stretches
    return lib


def aligned(n):
    a = np.zeros(n + 64, np.uint8)
    o = (-a.ctypes.data) % 16
    return a[o:o + n + 16]


def active_stretches(codes, chunk_bins):
    """How many chunks of `chunk_bins` resolved codes open a stretch: chunk 0, and every later one that holds a coded LPS (a code with
    symbol ((c >> 1) ^ c) & 1 set that is no bypass bin, avr_k1p.h).  The bytes alone do not tell the chunk length the emulation cut
    the slice at -- any length gives the same bytes when every use of it agrees -- so the builds at other lengths are held to this."""
    c = np.asarray(codes, np.uint32)
    lps = ((((c >> 1) ^ c) & 1) == 1) & ((c >> 1) != 126)
    return 1 + sum(bool(lps[i:i + chunk_bins].any()) for i in range(chunk_bins, c.size, chunk_bins))


def k1p(emul, recs, states):
    """(bytes, final_states, info) or (None, None, rc)."""
    P = oracle_lib.ptr
    recs = np.ascontiguousarray(recs, dtype=np.uint16)
    st = np.array(states, dtype=np.uint8, copy=True)
    res = aligned(recs.size + 32)
    m = ctypes.c_size_t(0)
    rc = emul.k1p_emul_resolve(P(recs), ctypes.c_size_t(recs.size), P(st), ctypes.c_size_t(st.size), P(res), ctypes.byref(m))
    if rc:
        return None, None, rc
    out = np.zeros(recs.size + 64, np.uint8)
    info = np.zeros(8, np.uint32)
    n = emul.k1p_emul_encode_resolved(P(res), ctypes.c_size_t(m.value), P(out), ctypes.c_size_t(out.size), P(info))
    if getattr(emul, "chunk_bins", None):
        assert info[0] == active_stretches(res[:m.value], emul.chunk_bins), (info, emul.chunk_bins)
    return out[:n].tobytes(), st.tobytes(), info


def check_golden_vectors(emul):
    g = np.load(os.path.join(ROOT, "tests", "golden", "g3_cabac.npz"), allow_pickle=False)
    for i in range(int(g["n_cases"])):
        data, final, info = k1p(emul, g[f"recs_{i}"], g[f"states_{i}"])
        assert info[3] == 0
        assert data == g[f"bytes_{i}"].tobytes() and final == g[f"final_{i}"].tobytes(), f"case {i}"


def test_golden_vectors(emul):
    check_golden_vectors(emul)


def test_golden_vectors_at_other_chunk_lengths(emul_other):
    check_golden_vectors(emul_other)


def check_random_streams(emul, oracle, count):
    rng = np.random.default_rng(31)
    for t in range(count):
        n = int(rng.integers(0, 12000))
        nctx = int(rng.integers(1, 120))
        recs, states = oracle_lib.random_cabac_stream(rng, n, nctx, terminate=bool(t % 3))
        if t % 8 == 0:
            states[:] = rng.integers(0, 128, nctx)          # includes pStateIdx 63 (codes 254/255)
        want = oracle.cabac_encode(recs, states)
        data, final, info = k1p(emul, recs, states)
        assert info[3] == 0 and (data, final) == want[:2], f"stream {t} n={n} info={info}"


def test_random_streams_many_chunks(emul, oracle):
    check_random_streams(emul, oracle, 250)


def test_random_streams_at_other_chunk_lengths(emul_other, oracle):
    check_random_streams(emul_other, oracle, 100)


def test_hard_shapes(emul, oracle):
    rng = np.random.default_rng(32)
    n = 40000

    def mk(bins, sels):
        return (np.asarray(bins, np.uint16) | (np.asarray(sels, np.uint16) << 1)).astype(np.uint16)
    cases = [
        (mk(np.arange(n) & 1, np.zeros(n)), [0]),                                        # alternating bins, one context
        (mk(rng.integers(0, 2, n), np.zeros(n)), [60]),                                  # coin flips in one context
        (mk(rng.integers(0, 2, n), np.where(rng.random(n) < 0.97, 1024, 0)), [10]),      # almost all bypass
        (mk((rng.random(n) < 0.002).astype(int), np.zeros(n)), [124]),                   # an LPS every ~500 bins
        (mk((rng.random(n) < 0.5).astype(int), rng.integers(0, 3, n)), [125, 0, 63]),
    ]
    for k, (recs, st) in enumerate(cases):
        st = np.array(st, np.uint8)
        want = oracle.cabac_encode(recs, st)
        data, final, info = k1p(emul, recs, st)
        assert info[3] == 0 and (data, final) == want[:2], f"case {k} info={info}"


def test_streams_without_lps_are_declined_not_miscoded(emul):
    # no coded LPS for more than 16 chunks: the scheme flags the slice (the kernels then hand it to
    # the serial kernel); it must never return wrong bytes silently
    n = 20000
    recs = (np.ones(n, np.uint16) | (1024 << 1)).astype(np.uint16)                      # bypass only
    _, _, info = k1p(emul, recs, np.zeros(1, np.uint8))
    assert info[3] == 1
    recs = np.ones(50000, np.uint16)                                                      # all MPS at pStateIdx 62
    _, _, info = k1p(emul, recs, np.array([125], np.uint8))
    assert info[3] == 1


def test_synthetic_slices(emul, oracle, avr):
    for w, n in ((2, 1), (4, 2), (5, 30)):
        cfg = avr.synth_config(w, 1000, 0)
        nb = np.zeros(n, np.uint32)
        avr.lib().avr_synth_count_host(ctypes.byref(cfg), 0, n, nb.ctypes.data)
        off = np.zeros(n + 1, np.uint64)
        off[1:] = np.cumsum((nb.astype(np.uint64) + 7) // 8 * 8)
        recs = np.zeros(int(off[-1]), np.uint16)
        st = np.zeros(n * cfg.n_states, np.uint8)
        avr.lib().avr_synth_generate_host(ctypes.byref(cfg), 0, n, off.ctypes.data, recs.ctypes.data, st.ctypes.data)
        for i in range(n):
            r = recs[int(off[i]):int(off[i]) + int(nb[i])]
            s = st[i * cfg.n_states:(i + 1) * cfg.n_states]
            want = oracle.cabac_encode(r, s)
            data, final, info = k1p(emul, r, s)
            assert info[3] == 0 and (data, final) == want[:2], f"workload {w} slice {i}"


def test_state_transitions_are_monotone(avr):
    """What phase A's speculation rests on: in the order (62,MPS 0) < ... < (0,0) < (0,1) < ... < (62,1)
    both CABAC transition functions (cabac_code.h:43-47) are non-decreasing, so two state chains that
    have met stay together and bracket every chain started between them."""
    _, mlps = avr.cabac_tables()

    def sigma(s):
        return (s >> 1) if s & 1 else -1 - (s >> 1)

    def step(s, b):
        return mlps[128 + s] if b == (s & 1) else mlps[127 - s]
    states = sorted(range(126), key=sigma)                       # pStateIdx <= 62
    assert sigma(124) == min(map(sigma, states)) and sigma(125) == max(map(sigma, states))
    for b in (0, 1):
        images = [sigma(step(s, b)) for s in states]
        assert images == sorted(images), b
        assert all(step(s, b) < 126 for s in states)             # pStateIdx 63 is never entered
    for s in (126, 127):                                         # ... and never left
        assert step(s, 0) == s and step(s, 1) == s


def test_fp64_division_of_the_recoded_coder_is_exact(emul):
    """k_range_encode's range / total (recode.cpp:826) goes through the FP64 pipe (csrc/avr_div.h); the same function on
    the CPU against the integer divide: 200 000 dividends below 2^63 (edges, exact multiples, all-ones low words) times
    every divisor 1..255."""
    assert emul.div_emul_check(7, 200000) == 0


def check_long_carry_chains(emul, oracle, end):
    """Chains of 30 .. 20 000 16-bit digits (tests/carry_streams.py) -- past one of phase D's 33-digit segments, one of its
    8 448-digit tiles, two tiles -- that one carry turns from 0xff to 0x00 ("carry"), that stay 0xff ("none") or that
    finish() decides ("cut"): exact bytes and final states, and none of them declined."""
    import carry_streams
    for k, n_chain in enumerate((30, 70, 2200, 9000, 20000)):
        recs, st = carry_streams.carry_chain_cabac(np.random.default_rng(700 + k), 3 + 40 * k, n_chain, end)
        want = oracle.cabac_encode(recs, st)
        data, final, info = k1p(emul, recs, st)
        assert info[3] == 0 and (data, final) == want[:2], f"chain {n_chain} {end} info={info}"
        assert carry_streams.longest_run(data, 0 if end == "carry" else data[2 * (3 + 40 * k) + 8])[1] >= 2 * (n_chain - 3)


@pytest.mark.parametrize("end", ["carry", "none", "cut"])
def test_long_carry_chains(emul, oracle, end):
    check_long_carry_chains(emul, oracle, end)


@pytest.mark.parametrize("end", ["carry", "none", "cut"])
def test_long_carry_chains_at_other_chunk_lengths(emul_other, oracle, end):
    check_long_carry_chains(emul_other, oracle, end)


def test_long_carry_chain_without_lps_is_declined(emul, oracle):
    """A chain with no coded LPS for more than 16 chunks: declined (the kernels hand it to the serial kernel), not mis-coded."""
    import carry_streams
    recs, st = carry_streams.carry_chain_cabac(np.random.default_rng(77), 5, 3000, "carry", n_ctx=4, p_bypass=1.0,
                                               init_states=[124, 125, 124, 125])
    assert carry_streams.longest_run(oracle.cabac_encode(recs, st)[0], 0)[1] >= 2 * (3000 - 3)
    _, _, info = k1p(emul, recs, st)
    assert info[3] == 1
