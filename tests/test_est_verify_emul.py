"""The estimator checker (csrc/avr_est_verify.h: resolved K2 records held to their key records by the update rule, record by
record) emulated on the CPU by tests/est_verify_emul.cpp with the very functions the kernels run, against a plain statement of its
five conditions (tests/est_verify_ref.py).  Sound records come from the plain rule of tests/range_keys.py, never from the resolver.
Small chunks and spans put every kind of bin on, before and after a chunk, a span and a slice boundary.

The same walk runs once more under AddressSanitizer and UBSan in a stand-alone program of its own (tests/est_verify_check.cpp),
started as a child process."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import est_verify_ref as ref
import range_keys as rk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "avrecode-ms_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "est_verify_emul.cpp")
SO = os.path.join(ROOT, "tests", "_est_verify_emul.so")
CHECK_SRC = os.path.join(ROOT, "tests", "est_verify_check.cpp")
CHECK_BIN = os.path.join(ROOT, "tests", "_est_verify_check")
DEPS = [os.path.join(CSRC, h) for h in ("avr_est_verify.h", "avr_layout.h", "avr_k1p.h", "avr_chunk.h")]


def _stale(target, sources):
    return not os.path.exists(target) or any(os.path.getmtime(s) > os.path.getmtime(target) for s in sources)


@pytest.fixture(scope="module")
def emul():
    if _stale(SO, [SRC] + DEPS):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I" + CSRC, "-o", SO + ".tmp", SRC], check=True)
        os.replace(SO + ".tmp", SO)
    lib = ctypes.CDLL(SO)
    lib.estv_emul_workspace_bytes.restype = ctypes.c_uint64
    lib.estv_emul_workspace_bytes.argtypes = [ctypes.c_uint64] * 2
    lib.estv_emul_step.restype = ctypes.c_uint32
    lib.estv_emul_step.argtypes = [ctypes.c_uint32] * 2
    return lib


class Stream:
    """Key records in the slice-major layout with the records, padding and tables the plain rule gives for them."""

    def __init__(self, slices, group_first, tables=None, gap=0):
        self.slices, self.gf = slices, np.asarray(group_first, np.uint32)
        self.keys, self.rec_off, self.n_bins = rk.layout(slices, gap)
        want, tabs = rk.resolve(slices, group_first, tables)
        assert all(w is not None for w in want)
        self.recs, _ = rk.expected_layout(want, self.rec_off, self.n_bins)      # 0xabcd outside the documented extents
        self.est_in = None if tables is None else np.ascontiguousarray(np.stack(tables), np.uint8)
        self.est_out = np.ascontiguousarray(np.stack(tabs), np.uint8)
        self.status = np.zeros(len(slices), np.int32)


def run(emul, st, chunk, span, recs=None, est_out="own", status=None, poison=0xFF):
    recs = st.recs if recs is None else recs
    est_out = st.est_out if isinstance(est_out, str) else est_out
    status = (st.status if status is None else np.asarray(status, np.int32)).copy()
    first = np.full(len(st.slices), 0x55555555, np.uint32)
    info = (ctypes.c_uint32 * 4)()
    P = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    rc = emul.estv_emul_verify(P(st.keys), P(recs), P(st.rec_off), P(st.n_bins), ctypes.c_uint32(len(st.slices)), P(st.gf),
                               ctypes.c_uint32(st.gf.size - 1), P(st.est_in), P(est_out), ctypes.c_uint32(chunk), ctypes.c_uint32(span),
                               ctypes.c_uint32(poison), P(status), P(first), info)
    assert rc == 0
    return status.tolist(), first.tolist(), list(info)


def agree(emul, st, chunk, span, recs=None, est_out="own", status=None, poison=0xFF):
    """the emulation's answer is the reference's for the whole batch; returns the reference's"""
    recs = st.recs if recs is None else recs
    eo = st.est_out if isinstance(est_out, str) else est_out
    want = ref.expect(st.keys, recs, st.rec_off, st.n_bins, st.gf.tolist(), st.est_in, eo, status)
    got_status, got_first, info = run(emul, st, chunk, span, recs, est_out, status, poison)
    assert got_first == [f for _, f in want], f"chunk={chunk} span={span} info={info}"
    assert got_status == ref.expect_status(want, status)
    return want, info


def test_step_is_the_rule_of_range_keys(emul):
    """the checker's three lines against the rule as tests/range_keys.py states it, for every pair a record can carry"""
    for pos in range(0, 128):
        for neg in range(0, 256):
            for b in (0, 1):
                got = emul.estv_emul_step(pos | (neg << 8), b)
                assert got == int(ref.step(pos | (neg << 8), b))
                if 1 <= pos and 1 <= neg and pos + neg <= 0x60:
                    p, n = ref.step_plain(pos, neg, b)
                    assert got == p | (n << 8)
    # and the reference finds nothing in what range_keys.resolve makes
    rng = np.random.default_rng(1)
    slices = [rk.random_keys(rng, 3000, "skew") for _ in range(3)]
    st = Stream(slices, [0, 2, 3], [rk.random_table(rng), rk.random_table(rng)])
    assert ref.expect(st.keys, st.recs, st.rec_off, st.n_bins, [0, 2, 3], st.est_in, st.est_out) == [(False, ref.VERIFY_NONE)] * 3


@pytest.mark.parametrize("mode", ["one", "skew", "flat"])
@pytest.mark.parametrize("fresh", [True, False])
def test_sound_records_have_no_finding(emul, mode, fresh):
    rng = np.random.default_rng(300 + len(mode) + fresh)
    crossing = later = 0
    for chunk, span, scale in ((1024, 16, 30000), (64, 3, 900), (7, 2, 120), (1, 1, 40)):
        lens = [0 if rng.random() < 0.2 else int(rng.integers(1, scale)) for _ in range(9)]       # empty slices inside groups
        lens[4] = 3 * chunk * span - sum(lens[2:4])                   # slices 2..4: a group over three spans exactly when it starts on a boundary
        slices = [rk.random_keys(rng, max(n, 0), mode) for n in lens]
        for gf in ([0, 9], list(range(10)), [0, 2, 5, 5, 9], [0, 0, 3, 9, 9]):      # one group, a group a slice, groups without slices
            tables = None if fresh else [rk.random_table(rng) for _ in range(len(gf) - 1)]
            st = Stream(slices, gf, tables, gap=chunk % 2)
            for poison in (0x00, 0xFF, 0xA5):
                want, info = agree(emul, st, chunk, span, poison=poison)
                assert not any(f for f, _ in want)
            crossing += info[2]
            later += info[3]
    assert crossing > 0


def test_sound_group_that_ends_exactly_on_a_span_boundary_and_long_piece_chains(emul):
    rng = np.random.default_rng(17)
    chunk, span = 8, 2
    # slices of whole chunks: group 0 = chunks [0, 6) ends on the boundary of span 2; group 1 = [6, 6 + 2 * 70): 70 pieces, two blocks
    slices = [rk.random_keys(rng, 16, "skew"), rk.random_keys(rng, 32, "skew")] + [rk.random_keys(rng, 16, "skew") for _ in range(70)] + \
             [rk.random_keys(rng, 5, "flat")]
    st = Stream(slices, [0, 2, 72, 73], [rk.random_table(rng) for _ in range(3)])
    want, info = agree(emul, st, chunk, span)
    assert not any(f for f, _ in want) and info[3] >= 1
    # a corruption in the last piece of the long group, on a key met only in the first: the chain carries it across both blocks
    key = int(slices[2][0]) >> 1
    for s in slices[3:72]:
        s[(s >> 1) == key] = ((key + 1) % rk.N_KEYS) << 1
    slices[71][3] = key << 1
    st = Stream(slices, [0, 2, 72, 73], [rk.random_table(rng) for _ in range(3)])
    recs = st.recs.copy()
    recs[int(st.rec_off[71]) + 3] += 2
    want, _ = agree(emul, st, chunk, span, recs)
    assert want[71] == (True, 3)


def corruption_stream():
    """Three slices in two groups, small, with halvings: key 7 holds more than 100 bins, and equal keys sit side by side."""
    rng = np.random.default_rng(99)
    def make(n):
        key = np.where(rng.random(n) < 0.62, 7, rng.integers(0, 12, n))
        return ((key << 1) | (rng.random(n) < 0.7)).astype(np.uint16)
    slices = [make(83), make(70), make(45)]
    assert sum(int(((s >> 1) == 7).sum()) for s in slices[:2]) > 100
    return slices, [0, 2, 3]


@pytest.mark.parametrize("chunk,span", [(1024, 16), (16, 2), (5, 1)])
def test_every_corruption_of_every_record_is_reported_as_the_reference_says(emul, chunk, span):
    slices, gf = corruption_stream()
    rng = np.random.default_rng(5)
    st = Stream(slices, gf, [rk.random_table(rng), rk.random_table(rng)])
    agree(emul, st, chunk, span)
    found = 0
    for i in range(3):
        o, nb = int(st.rec_off[i]), int(st.n_bins[i])
        for j in range(nb):
            r = int(st.recs[o + j])
            pos, neg = (r >> 1) & 0x7F, r >> 8
            alts = [r + 2, r + 0x100, r ^ 1]
            if pos != neg:
                alts.append((r & 1) | (neg << 1) | (pos << 8))
            for alt in alts:
                recs = st.recs.copy()
                recs[o + j] = alt
                want, _ = agree(emul, st, chunk, span, recs)
                assert want[i] == (True, j)                            # found in its slice at that very bin
                found += 1
        for j in range(nb, (nb + 7) // 8 * 8):                         # every padding record
            recs = st.recs.copy()
            recs[o + j] = 1 + j
            want, _ = agree(emul, st, chunk, span, recs)
            assert want[i] == (True, nb)
    assert found > 700
    for g in range(2):                                                 # every est_out entry of a met key, one of an unmet key
        met = np.unique(np.concatenate([s >> 1 for s in slices[gf[g]:gf[g + 1]]]))
        for k in met.tolist() + [1000]:
            for part in (0, 1):
                eo = st.est_out.copy()
                eo[g, k, part] += 1
                want, _ = agree(emul, st, chunk, span, est_out=eo)
                last = gf[g + 1] - 1
                assert [f for f, _ in want] == [i == last for i in range(3)] and want[last][1] == int(st.n_bins[last])
    agree(emul, st, chunk, span, est_out=None)                         # est_out not given: not checked


def test_malformed_group_is_checked_up_to_the_bad_slice(emul):
    rng = np.random.default_rng(23)
    slices = [rk.random_keys(rng, int(rng.integers(40, 300)), "skew") for _ in range(7)]
    st = Stream(slices, [0, 2, 6, 7])
    status = [0, 0, 0, 0, rk.BAD_RECORD, rk.BAD_RECORD, 2]             # group 1 bad from slice 4 on; slice 6 overflowed: it takes part
    for chunk, span in ((1024, 16), (16, 2)):
        recs = st.recs.copy()
        recs[int(st.rec_off[4]):int(st.rec_off[6])] = 0xFFFF           # undefined records of the bad slices
        eo = st.est_out.copy()
        eo[1] = 0xCC                                                   # its table is undefined too
        want, _ = agree(emul, st, chunk, span, recs, eo, status)
        assert not any(f for f, _ in want)
        recs[int(st.rec_off[3]) + 9] ^= 0x200                          # a corruption before the bad slice is found
        recs[int(st.rec_off[6]) + 2] += 2                              # and one in a slice with another status: reported, status stays
        want, _ = agree(emul, st, chunk, span, recs, eo, status)
        assert want[3][0] and want[3][1] <= 9 and want[6] == (True, 2) and not want[4][0] and not want[5][0]
        krecs = st.keys.copy()                                         # a malformed key record in a slice that takes part: a finding there
        st2 = Stream(slices, [0, 2, 6, 7])
        st2.keys = krecs
        st2.keys[int(st.rec_off[1]) + 5] = 0x9000
        want, _ = agree(emul, st2, chunk, span)
        assert want[1][0] and want[1][1] <= 5


def test_workspace_formula_and_it_fits_in_the_resolvers(emul):
    import test_est_emul
    res = test_est_emul.emul.__wrapped__()
    for n, g, tc in ((1, 1, 1), (7, 3, 16), (1000, 10, 17), (1 << 20, 1 << 20, 1 << 20), (3, 1, 40000)):
        want = (4 * n + 255) // 256 * 256 + 2 * ((tc + 15) // 16) * 4112
        assert emul.estv_emul_workspace_bytes(n, tc) == want
        assert want <= res.est_emul_workspace_bytes(n, g, tc)


def test_the_sanitized_stand_alone_program():
    """tests/est_verify_check.cpp: the same walk on heap buffers of exactly the documented extents, sound and corrupted, under
    AddressSanitizer and UBSan.  A child process with this one's environment as it is: nothing is loaded into this process and
    nothing is preloaded into that one by the test."""
    if _stale(CHECK_BIN, [CHECK_SRC, SRC] + DEPS):
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + CSRC,
                        "-I" + os.path.join(ROOT, "tests"), "-o", CHECK_BIN + ".tmp", CHECK_SRC], check=True)
        os.replace(CHECK_BIN + ".tmp", CHECK_BIN)
    r = subprocess.run([CHECK_BIN], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-2000:] + r.stderr[-4000:]
