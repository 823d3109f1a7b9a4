"""GPU: K1p's context chains -- k_k1p_chain_seg / k_k1p_chain_fix for long slices, k_k1p_ctxchain start to end for short ones -- on the
step they share (chain_step of csrc/avr_k1p.h: a run's odd bins first, then whole bytes, each look-up taken only while some lane of the
wave has it) and the loop they share (ChainAhead: unrolled by the depth of its read-ahead).  What a wave does in a step now depends on
what its 64 lanes have in the chunk, so the batches here are made of contexts that differ: every batch is coded by the one-lane-per-slice
kernel and by the oracle once, and then by the intra-slice parallel kernels as the batch's shape has it, with the summaries of every third
pair distrusted (chain_force_redo), in segments whatever the shape, and start to end: bytes, lengths, statuses and final states are the
same every time.

The batches: slices long enough for the chains in segments, short ones for the start-to-end walk in groups of lanes and, past 129 024
pairs, in full waves; 1, 2, 63, 64 and 65 contexts (a wave is 64 pairs); every context hot (45 bins a chunk), every context cold and
equally so; and in the first batch two contexts with the same bins, two with 300 bins in one chunk each and none elsewhere (runs beyond
the 96 bins a window holds), one parked at pStateIdx 63, an empty slice and one with a bad record."""
import numpy as np
import pytest

import oracle_lib
from test_gpu_parity import to_records8

pytestmark = pytest.mark.gpu

CHUNK = 1024
# test hooks per mode: as shipped (the hooked build without a hook), every third pair's summaries distrusted, that in segments whatever the
# batch's shape, and every chain start to end
MODES = {"shipped": {}, "redo3": {"chain_force_redo": 3}, "segments-redo3": {"chain_segments": 1, "chain_force_redo": 3}, "whole": {"chain_whole": 1}}


def stream(rng, n, weights, p_bypass=0.1, terminate=True):
    """n bins whose contexts are drawn by `weights` (bypass bins among them), each context with a bias of its own."""
    weights = np.asarray(weights, float)
    n_ctx = weights.size
    sel = rng.choice(n_ctx, size=n, p=weights / weights.sum())
    bias = rng.random(n_ctx) ** 2
    bias = np.where(rng.random(n_ctx) < 0.5, bias, 1 - bias)
    bins = (rng.random(n) < bias[sel]).astype(np.uint16)
    sel = np.where(rng.random(n) < p_bypass, 1024, sel)
    recs = (bins | (sel << 1)).astype(np.uint16)
    if terminate:
        recs = np.concatenate([recs, np.array([1 | (1025 << 1)], np.uint16)])
    return recs, rng.integers(0, 126, n_ctx).astype(np.uint8)


def skewed(n_ctx, n_hot, ratio=12.0):
    w = np.ones(n_ctx)
    w[np.random.default_rng(n_ctx).choice(n_ctx, size=min(n_hot, n_ctx), replace=False)] = ratio
    return w


def batch_segments():
    """Five slices of 9 .. 40 chunks with 70 contexts, five of them hot, an empty slice and a slice with a bin behind put_terminate(1)."""
    rng = np.random.default_rng(9101)
    w = skewed(70, 5, 15.0)
    w[[11, 12, 30, 31, 40]] = 0                                  # placed by hand below
    slices = []
    for n_chunks in (40, 9, 38, 17, 30):
        n = n_chunks * CHUNK - int(rng.integers(1, 900))
        recs, st = stream(rng, n, w)
        free = np.flatnonzero((recs >> 1) < 1024)[:-1]
        # a tie: contexts 11 and 12 take the same bins at neighbouring places, two to a chunk each
        at = free[::500][: n // 520]
        recs[at] = (11 << 1) | (at & 1)
        recs[at + 1] = (12 << 1) | (at & 1)
        # contexts 30 and 31: 300 bins each in one chunk each, none elsewhere
        c = n_chunks // 2
        for ctx, chunk in ((30, c), (31, c + 1)):
            inside = chunk * CHUNK + rng.choice(CHUNK, size=300, replace=False)
            recs[inside] = (ctx << 1) | (rng.random(300) < 0.8)
        # context 40: parked at pStateIdx 63, a bin in a hundred
        st[40] = 126
        recs[free[7::100]] = 40 << 1
        slices.append((recs, st))
    slices.insert(2, (np.zeros(0, np.uint16), rng.integers(0, 126, 70).astype(np.uint8)))
    slices.insert(4, (np.array([1 | (1025 << 1), 0], np.uint16), rng.integers(0, 126, 70).astype(np.uint8)))
    return slices


def batch_short():
    """37 slices of up to three chunks: the chains start to end, a wave a group of a slice's contexts."""
    rng = np.random.default_rng(9102)
    w = skewed(70, 6)
    return [stream(rng, int(rng.integers(0, 3000)), w, terminate=bool(i % 3)) for i in range(37)]


def batch_many():
    """1 900 slices of one chunk, 70 contexts: 133 000 pairs, start to end in full waves across slices."""
    rng = np.random.default_rng(9103)
    w = skewed(70, 6)
    return [stream(rng, int(rng.integers(1, 260)), w, terminate=bool(i % 2)) for i in range(1900)]


def batch_contexts(n_ctx):
    rng = np.random.default_rng(9200 + n_ctx)
    w = skewed(n_ctx, max(1, n_ctx // 8))
    return [stream(rng, n, w) for n in (9 * CHUNK + 5, 12 * CHUNK - 1, 700, 10 * CHUNK)]


def batch_all_hot():
    """20 contexts with 45 bins a chunk each: every lane of every wave takes six look-ups or so a chunk."""
    rng = np.random.default_rng(9104)
    return [stream(rng, n, np.ones(20)) for n in (11 * CHUNK, 9 * CHUNK + 77, 16 * CHUNK - 3)]


def batch_all_cold():
    """200 contexts with the same four or five bins a chunk: every wave leaves the step after its first look-up."""
    rng = np.random.default_rng(9105)
    return [stream(rng, n, np.ones(200)) for n in (11 * CHUNK, 9 * CHUNK + 77, 16 * CHUNK - 3)]


BATCHES = {"segments": batch_segments, "short": batch_short, "many": batch_many, "all-hot": batch_all_hot, "all-cold": batch_all_cold,
           **{f"{n}-contexts": (lambda n=n: batch_contexts(n)) for n in (1, 2, 63, 64, 65)}}
_made = {}


def prepared(avr, oracle, name):
    """The batch, and what it codes to: by the oracle (bytes and final states of the slices it takes) and by the one-lane-per-slice
    kernel (bytes, statuses, lengths, final states) -- made once, shared by the tests, never changed."""
    if name not in _made:
        slices = BATCHES[name]()
        w = avr.DeviceWorkload.from_host(0, [r for r, _ in slices], [s for _, s in slices], 0)
        w.encode()
        data, status = w.results()
        serial = (data, list(status), w.out_len.cpu().numpy().copy(), w.final_states.cpu().numpy().copy())
        want = [oracle.cabac_encode(r, s) for r, s in slices]
        for i, (d, st) in enumerate(zip(data, status)):
            if st == 0:
                assert d == want[i][0], f"{name}: the one-lane-per-slice kernel and the oracle differ on slice {i}"
        _made[name] = (slices, serial, want)
    return _made[name]


def check_chunked(avr, oracle, name, w=None):
    slices, (data, status, out_len, final), want = prepared(avr, oracle, name)
    if w is None:
        w = avr.DeviceWorkload.from_host(0, [r for r, _ in slices], [s for _, s in slices], 0)
    w.encode_chunked()
    got, got_status = w.results()
    assert list(got_status) == status
    assert (w.out_len.cpu().numpy() == out_len).all()
    n_ctx = len(slices[0][1])
    got_final = w.final_states.cpu().numpy().reshape(len(slices), -1)
    for i in range(len(slices)):
        if status[i] == 0:
            assert got[i] == data[i] == want[i][0], f"{name}: slice {i}"
            assert got_final[i][:n_ctx].tobytes() == want[i][1], f"{name}: final states of slice {i}"
    assert (got_final == final.reshape(len(slices), -1))[np.array(status) == 0].all()
    return status


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", ["segments", "short", "many", "all-hot", "all-cold"])
def test_chains_code_the_same(avr, oracle, hooks, name, mode):
    hooks(**MODES[mode])
    status = check_chunked(avr, oracle, name)
    if name == "segments":
        assert status[4] == avr.SLICE_BAD_RECORD and sum(s != 0 for s in status) == 1


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("n_ctx", [1, 2, 63, 64, 65])
def test_context_counts_around_a_wave(avr, oracle, hooks, n_ctx, mode):
    hooks(**MODES[mode])
    check_chunked(avr, oracle, f"{n_ctx}-contexts")


@pytest.mark.parametrize("name", ["segments", "short", "many", "all-hot", "all-cold"])
def test_the_product_library_codes_the_same(avr, oracle, name):
    """No hook: the library as it ships."""
    check_chunked(avr, oracle, name)


def test_one_byte_records_take_the_same_step(avr, oracle, hooks):
    """AVR_KIND_CABAC8 (no renumbering: the dense ids are the selectors) through avr_cabac8_encode_chunked_device."""
    slices, _, _ = prepared(avr, oracle, "segments")
    good = [(r, s) for r, s in slices if r.size != 2]            # (the bad record is a two-byte one)
    want = [oracle.cabac_encode(r, s) for r, s in good]
    for mode in ("shipped", "redo3"):
        hooks(**MODES[mode])
        w = avr.DeviceWorkload.from_host(avr.KIND_CABAC8, [to_records8(r) for r, _ in good], [s for _, s in good], 0)
        w.encode_chunked()
        got, status = w.results()
        final = w.final_states.cpu().numpy().reshape(len(good), -1)
        for i in range(len(good)):
            assert status[i] == 0 and got[i] == want[i][0], f"slice {i} {mode}"
            assert final[i][:70].tobytes() == want[i][1], f"final states of slice {i} {mode}"
