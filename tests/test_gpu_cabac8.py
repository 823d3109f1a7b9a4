"""K1 from one-byte records (AVR_KIND_CABAC8: bin | dense selector << 1) read natively on the device: the one-byte K1p call
(avr_cabac8_encode_chunked_device), the one-byte packer (avr_pack_tiles8_device) in front of the one-lane-per-slice coder, the
batch API on both paths and the multi-device batch -- every byte and final state against the oracle (cabac_code.h:33-67 on
arithmetic_code.h) and against the two-byte path on the same slices.  One-byte records have no no-op value, so every slice's
padding bytes hold garbage here that would change the bytes if it were coded."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import carry_streams
import oracle_lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TERM1 = (1025 << 1) | 1


def to8(recs):
    """Two-byte K1 records (selectors below 126, bypass, terminate) as one-byte records."""
    recs = np.asarray(recs, dtype=np.uint16)
    sel = (recs >> 1).astype(np.int64)
    sel8 = np.where(sel == 1024, 126, np.where(sel == 1025, 127, sel))
    assert ((sel8 >= 0) & (sel8 < 128)).all()
    return ((sel8 << 1) | (recs & 1)).astype(np.uint8)


def garbage(seed):
    return np.random.default_rng(seed).integers(0, 256, 4099).astype(np.uint8)


def chunked8(avr, slices, pad_seed=1, bad_offset=None):
    """(bytes, final states, statuses) of the slices through avr_cabac8_encode_chunked_device."""
    recs8 = [to8(r) if r.dtype == np.uint16 else r for r, _ in slices]
    w = avr.DeviceWorkload.from_host(avr.KIND_CABAC8, recs8, [s for _, s in slices], pad_bytes=garbage(pad_seed))
    if bad_offset is not None:                              # a slice whose offset is not a multiple of 16
        w.rec8_off[bad_offset] += 3
    w.status.zero_()                                        # what the packer found is not what is tested here: K1p validates by itself
    w.encode_chunked()
    return results(w)


def results(w):
    got, status = w.results()
    ns = w.n_states
    fs = w.final_states.cpu().numpy()
    return got, [fs[i * ns:(i + 1) * ns].tobytes() for i in range(w.n_slices)], status


def chunked16(avr, slices):
    w = avr.DeviceWorkload.from_host(avr.KIND_CABAC, [r for r, _ in slices], [s for _, s in slices])
    w.encode_chunked()
    return results(w)


def check(oracle, slices, got, what):
    data, states, status = got
    for i, (r, s) in enumerate(slices):
        assert (data[i], states[i], status[i]) == oracle.cabac_encode(r, s), f"{what}: slice {i} n={len(r)}"


def mixed_slices(rng, n_states):
    slices = []
    for n in (0, 1, 15, 16, 17, 1023, 1024, 1025):
        slices.append(oracle_lib.random_cabac_stream(rng, n, n_states, terminate=False))
        if n:
            slices.append(oracle_lib.random_cabac_stream(rng, n - 1, n_states, terminate=True))
    for n in (9000, 33333, 70001):                          # many chunks each, terminate-last and terminate-free
        slices.append(oracle_lib.random_cabac_stream(rng, n, n_states, terminate=True))
        slices.append(oracle_lib.random_cabac_stream(rng, n + 5, n_states, terminate=False))
    return slices


@pytest.mark.parametrize("n_states", [1, 37, 126])
def test_chunked_one_byte_entry_matches_oracle_and_two_byte_path(avr, oracle, n_states):
    slices = mixed_slices(np.random.default_rng(n_states), n_states)
    got = chunked8(avr, slices, pad_seed=n_states)
    check(oracle, slices, got, "one-byte chunked")
    assert got == chunked16(avr, slices)
    assert chunked8(avr, slices, pad_seed=n_states + 1000) == got           # other padding, same everything


def test_chunked_one_byte_bad_records_flag_their_slice_only(avr, oracle, hooks):
    rng = np.random.default_rng(77)
    ns = 40
    good = [oracle_lib.random_cabac_stream(rng, int(n), ns) for n in (5000, 3000, 12000, 7000, 2500)]
    recs8 = [to8(r) for r, _ in good]
    bad_sel = recs8[1].copy()
    bad_sel[1234] = (ns + 3) << 1                           # a selector in [n_states, 126): no context of the slice
    bad_term = recs8[2].copy()
    bad_term[5000] = (127 << 1) | 1                         # put_terminate(1) that is not the last bin
    slices = [(recs8[0], good[0][1]), (bad_sel, good[1][1]), (bad_term, good[2][1]), (recs8[3], good[3][1]), (recs8[4], good[4][1])]
    data, states, status = chunked8(avr, slices, pad_seed=5, bad_offset=3)
    assert status == [0, 3, 3, 3, 0]
    for i in (0, 4):
        assert (data[i], states[i], status[i]) == oracle.cabac_encode(*good[i])
    # the same slices (offsets all aligned) through a one-byte batch on the intra-slice parallel path, which has no packer in front
    hooks(k1_path=2)
    with avr.Batch(0, len(slices), sum(len(r) for r, _ in slices) + 64) as b:
        for r, s in slices:
            b.add_slice_cabac8(r, s)
        b.run()
        assert b.run_info()["chunked"] == 1
        assert [b.get(i)[1] for i in range(len(slices))] == [0, 3, 3, 0, 0]
        for i in (0, 3, 4):
            assert (b.get(i)[0], b.get_states(i), b.get(i)[1]) == oracle.cabac_encode(*good[i]), f"batch: slice {i}"


def hook_slices():
    rng = np.random.default_rng(4711)
    chains = [carry_streams.carry_chain_cabac(np.random.default_rng(300 + k), lead, n, end, n_ctx=100)
              for k, (lead, n, end) in enumerate([(3, 70, "carry"), (10, 2200, "none"), (0, 9000, "carry"), (20, 8448, "cut"),
                                                  (5, 20000, "carry")])]
    chains.append(carry_streams.carry_chain_cabac(np.random.default_rng(399), 5, 3000, "carry", n_ctx=100, p_bypass=1.0,
                                                  init_states=np.array([124, 125] * 50, np.uint8)))
    randoms = [oracle_lib.random_cabac_stream(rng, int(n), 100, terminate=bool(i % 3)) for i, n in enumerate(rng.integers(0, 20000, 8))]
    slices = []
    for k in range(max(len(chains), len(randoms))):         # chains and random neighbours, alternating
        slices += chains[k:k + 1] + randoms[k:k + 1]
    return slices


HOOKS = [dict(k1p_force_retry_every=3), dict(chain_segments=1), dict(chain_whole=1), dict(chain_segments=1, chain_force_redo=2),
         dict(local_waves=1), dict(local_waves=4)]


@pytest.fixture(scope="module")
def hooked(oracle):
    slices = hook_slices()
    return slices, [oracle.cabac_encode(r, s) for r, s in slices]


@pytest.mark.parametrize("setting", HOOKS, ids=lambda h: ",".join(f"{k}={v}" for k, v in h.items()))
def test_chunked_one_byte_rare_paths(avr, hooks, hooked, setting):
    """The hand-over of phase D to the serial coder (here: from the resolved codes, there being no two-byte records), the
    chains in segments, start to end and redone, k_k1p_local's workgroup sizes -- on carry-chain streams and random ones."""
    slices, wants = hooked
    hooks(**setting)
    data, states, status = chunked8(avr, slices, pad_seed=9)
    for i, want in enumerate(wants):
        assert (data[i], states[i], status[i]) == want, f"{setting}: slice {i}"


def test_pack_tiles8_then_tiles_coder(avr, oracle):
    rng = np.random.default_rng(88)
    ns = 60
    slices = [oracle_lib.random_cabac_stream(rng, int(n), ns, terminate=bool(i % 2)) for i, n in enumerate(rng.integers(0, 3000, 150))]
    slices += [(np.zeros(0, np.uint16), slices[0][1]), (np.array([TERM1], np.uint16), slices[0][1])]
    recs8 = [to8(r) for r, _ in slices]
    bad = recs8[7].copy()
    if bad.size:
        bad[bad.size // 2] = ((ns + 1) << 1) | 1
    recs8[7] = bad
    w = avr.DeviceWorkload.from_host(avr.KIND_CABAC8, recs8, [s for _, s in slices], pad_bytes=garbage(3))
    assert w.status.cpu().tolist()[7] == (3 if bad.size else 0)
    w.encode()
    data, states, status = results(w)
    for i, (r, s) in enumerate(slices):
        if i == 7 and bad.size:
            assert status[i] == 3 and data[i] == b""
            continue
        assert (data[i], states[i], status[i]) == oracle.cabac_encode(r, s), f"slice {i}"


# ---- real streams: the decompress-direction K1 records of the clips this repository has (tests/golden)

CLIPS = ("realshort.mp4", "cockatoo.mp4")


def _stream_records(host, data, residual, decompress, recoded=None, offered=None):
    """The clip's per-slice records through tests/_host_api.so's recorders (as tests/test_h264.py gets them)."""
    P = oracle_lib.ptr
    cap, slice_cap = 16 * len(data) + 4096, 4096
    recs, rec_end = np.zeros(cap, np.uint16), np.zeros(slice_cap, np.uint64)
    n = ctypes.c_uint64(0)
    pay, pay_end = np.zeros(len(data) + 64, np.uint8), np.zeros(slice_cap, np.uint64)
    first, n_states = np.zeros(slice_cap * 1024, np.uint8), np.zeros(slice_cap, np.int32)
    file = np.frombuffer(data, np.uint8).copy()
    if recoded is None:
        blob, off = np.zeros(1, np.uint8), np.zeros(1, np.uint64)
    else:
        blob = np.frombuffer(b"".join(recoded) + b"\0", np.uint8).copy()
        off = np.zeros(len(recoded) + 1, np.uint64)
        off[1:] = np.cumsum([len(x) for x in recoded])
    err = ctypes.create_string_buffer(512)
    flags = np.zeros(slice_cap, np.uint8)
    n_flags = ctypes.c_uint64(0)
    if offered is not None:
        flags[:len(offered)] = offered
        n_flags = ctypes.c_uint64(len(offered))
    rc = host.t_stream_records(P(file), ctypes.c_size_t(len(data)), int(residual), int(decompress), P(blob), P(off), P(recs), ctypes.c_size_t(cap),
                               P(rec_end), ctypes.c_size_t(slice_cap), ctypes.byref(n), P(pay), ctypes.c_size_t(pay.size), P(pay_end), P(first),
                               P(n_states), P(flags), ctypes.c_size_t(slice_cap), ctypes.byref(n_flags), err, ctypes.c_size_t(512))
    assert rc == 0, err.value.decode()
    ends = [0] + [int(e) for e in rec_end[:n.value]]
    slices = [recs[ends[i]:ends[i + 1]] for i in range(n.value)]
    if decompress:
        return slices, [first[1024 * i:1024 * i + int(n_states[i])] for i in range(n.value)]
    pe = [0] + [int(e) for e in pay_end[:n.value]]
    return slices, [pay[pe[i]:pe[i + 1]].tobytes() for i in range(n.value)], flags[:n_flags.value].copy()


def narrow(recs, first_states, n_states):
    """A slice's two-byte records with its contexts numbered by first appearance: (one-byte records, initial states)."""
    sel = (recs >> 1).astype(np.int64)
    ctx = sel < 1024
    order = list(dict.fromkeys(sel[ctx].tolist()))
    assert len(order) <= n_states
    ids = np.full(1024, 0, np.int64)
    ids[order] = np.arange(len(order))
    sel8 = np.where(ctx, ids[np.minimum(sel, 1023)], np.where(sel == 1024, 126, 127))
    states = np.zeros(n_states, np.uint8)
    states[:len(order)] = np.asarray(first_states, np.uint8)[order]
    return ((sel8 << 1) | (recs & 1)).astype(np.uint8), states


def host_api(avr):
    """tests/_host_api.so (tests/host_api.cpp on the host layer), built when it is older than its sources -- as tests/test_host.py builds it."""
    src, so = os.path.join(ROOT, "tests", "host_api.cpp"), os.path.join(ROOT, "tests", "_host_api.so")
    csrc = os.path.join(ROOT, "avrecode-ms_amd", "csrc")
    deps = [src, avr.LIB_PATH] + [os.path.join(csrc, "host", f) for f in ("avr_host.h", "avr_recode.h", "avr_model.h", "avr_h264.h", "avr_h264_tables.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.run(["g++", "-O2", "-pthread", "-std=c++17", "-fPIC", "-shared", "-I" + csrc, "-I/opt/rocm/include",
                        "-D__HIP_PLATFORM_AMD__", "-o", so, src, "-L" + os.path.dirname(avr.LIB_PATH), "-lavrecode_hip",
                        "-Wl,-rpath,$ORIGIN/../avrecode-ms_amd"], check=True)
    return ctypes.CDLL(so)


@pytest.fixture(scope="module")
def real_streams(avr, oracle):
    host = host_api(avr)
    out = {}
    for name in CLIPS:
        data = open(os.path.join(ROOT, "tests", "golden", name), "rb").read()
        k2, payloads, offered = _stream_records(host, data, 0, 0)
        recoded = [oracle.range_encode(r)[0] for r in k2]
        k1, first = _stream_records(host, data, 0, 1, recoded, offered)
        out[name] = (k1, first, payloads)
    return out


def contexts_of(recs):
    return len(set((recs[(recs >> 1) < 1024] >> 1).tolist()))


@pytest.mark.parametrize("name", CLIPS)
def test_real_streams_through_every_one_byte_path(avr, hooks, real_streams, name):
    """The slices of the clip whose contexts fit one byte (at most 126: 24 of realshort's 36 slices, 186 of cockatoo's 280 -- the
    others name up to 159 and 224 contexts and keep the two-byte form), narrowed with their contexts numbered by first appearance,
    through the one-byte chunked entry and a one-byte avr_batch on both paths: after drop_stop_byte + tail_patch every slice gives
    back its original payload."""
    k1, first, payloads = real_streams[name]
    keep = [i for i, r in enumerate(k1) if contexts_of(r) <= avr.MAX_STATES8]
    assert len(keep) >= len(k1) // 2
    k1, first, payloads = [k1[i] for i in keep], [first[i] for i in keep], [payloads[i] for i in keep]
    narrowed = [narrow(r, s, avr.MAX_STATES8) for r, s in zip(k1, first)]

    def back(data, i):
        return avr.tail_patch(avr.drop_stop_byte(data), len(payloads[i]) & 1, payloads[i][-1])

    data, _, status = chunked8(avr, narrowed, pad_seed=11)
    assert not any(status)
    for i in range(len(k1)):
        assert back(data[i], i) == payloads[i], f"{name}: one-byte chunked entry, slice {i}"
    for path in (1, 2):                                     # the batch API, serial and chunked
        hooks(k1_path=path)
        with avr.Batch(0, len(narrowed), sum(len(r) for r, _ in narrowed) + 64) as b:
            for r, s in narrowed:
                b.add_slice_cabac8(r, s)
            b.run()
            assert b.run_info()["chunked"] == path - 1
            for i in range(len(k1)):
                got, st = b.get(i)
                assert st == 0 and back(got, i) == payloads[i], f"{name}: batch k1_path={path}, slice {i}"


def test_full_size_config2_one_byte_equals_two_byte(avr):
    """BASELINE.json configs[1]: synthesised, densified (its contexts numbered 0 .. n-1), narrowed to one byte on the device --
    every one of the 512 slices' bytes, final states and statuses through the one-byte K1p call equal the two-byte one's."""
    import torch
    w = avr.DeviceWorkload.synth(2, 512, avr.KIND_CABAC, 0, 1000)
    w.densify()
    assert w.n_states <= avr.MAX_STATES8
    w8 = w.to_cabac8()
    w.encode_chunked()
    torch.cuda.synchronize()
    w.settle()
    want = results(w)
    w8.encode_chunked()
    got = results(w8)
    assert not any(got[2])
    assert got[2] == want[2]
    assert got[0] == want[0]
    assert got[1] == want[1]


def test_multibatch_add_slice_cabac8(avr, oracle):
    rng = np.random.default_rng(99)
    slices = [oracle_lib.random_cabac_stream(rng, int(n), 50) for n in rng.integers(0, 30000, 24)]
    with avr.MultiBatch([0], len(slices), sum(len(r) for r, _ in slices) + 64) as m:
        for r, s in slices:
            m.add_slice_cabac8(to8(r), s)
        m.run()
        for i, (r, s) in enumerate(slices):
            want = oracle.cabac_encode(r, s)
            assert m.get(i) == (want[0], want[2]), f"slice {i}"
