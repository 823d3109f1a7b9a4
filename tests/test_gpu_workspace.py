"""GPU: every multi-kernel device path on DIRTY workspaces, in buffers of EXACTLY the quoted size, on a stream of the caller's own.

The intra-slice parallel paths (K1p in all its forms, K2p, the two-stage form) run many kernels in workspace memory the caller owns.
Several of those kernels add into words an earlier kernel of the same call must have zeroed, or read words no kernel of the call
writes; the layouts are sized by one count and indexed by another; and side streams must be joined back before the caller's stream
goes on.  DeviceWorkload takes every workspace from torch.empty(quoted + 256), which mostly holds zeros or a previous run's values,
and every other test runs on the null stream and synchronises the device -- so none of this was ever under test.  Here:

  A  every entry point equals the oracle (bad_records.expected: the oracle plus the library's rule for malformed records) with every
     workspace, the code buffer and out / out_len / final_states filled beforehand with 0x00, 0xFF, 0x5A -- and with what a
     DIFFERENT, larger batch left behind (A, B, A through one workspace sized for A).  A poison must not hide behind a hand-over:
     phase D of K1p gives a slice whose digit sums it cannot resolve to the serial kernel, which codes it right whatever the sums
     held.  So the set of slices that leave the parallel path (test hook k1p_keep_retry: they keep AVR_SLICE_RETRY_SERIAL) must be
     the same under every poison, and so must the number of slices left for the second pass (counts[1]).
  B  all of these runs use buffers of exactly the size the library quotes or the header documents (tests/guarded.py), a canary on
     both sides: the guards must be intact afterwards, and so must every byte of `out` outside the slices' own bytes.  The
     guard is a detector, not a fence (64 KiB a side: any off-by-a-row of the layouts; a wilder write leaves the tensor).
  C  the same calls on a non-blocking stream of the caller's own that is held up by a sleep kernel, the outputs copied to snapshots
     and the workspaces overwritten ON THAT STREAM right behind the call, and only that stream synchronised: a side stream that is
     not joined back, or a kernel that went to the null stream, gives wrong snapshots.

Every case asserts that the path it names ran, by what the library reports (settle(), the pinned counts, k1p_keep_retry) or, where it
reports nothing (the context chains' hooks), by what the path leaves in the workspace.  What a hook leaves no trace of at all
(local_waves, chain_force_redo, k2p_seg_len, k2p_wave) is asserted as far as the setter goes: an unknown hook is an error.

Batches: an empty slice, 1 bin, 1023 / 1024 / 1025 and 4095 / 4096 / 4097 bins, ragged lengths, long carry chains
(tests/carry_streams.py: they are what makes the digit sums and K2p's shared positions matter), slices the K1p scheme declines, a
malformed slice in the middle (length 0 on a poisoned out_len), and in the large batches one slice of more than 1024 chunks.

That these tests can fail was shown once on two builds with one initialisation store left out (values only, no index or bound):
k_k2p_zero's second loop -- every K2p case here fails, most on a length one byte too long, from 0xFF on (the handed-over slice
already under 0x00); k_k1p_b2's zeroing of the digit sums -- every K1p case fails on the oracle's lengths and bytes under 0xFF (the
sums do not slip out through phase D's hand-over: the comparison of bytes fails before the comparison of the hand-over sets).  The
suite as it was also caught both (43 and 79 failures): its workspaces come from the caching allocator's used blocks -- by accident
of test order, where these cases do it by construction."""
import ctypes
import time

import numpy as np
import pytest

import bad_records as br
import carry_streams
import guarded
import oracle_lib
from test_gpu_parity import compact, host_synth, to_records8

pytestmark = pytest.mark.gpu

POISONS = (0x00, 0xFF, 0x5A)
EDGES = (0, 1, 1023, 1024, 1025, 4095, 4096, 4097)
RETRY_SERIAL = 100                                           # AVR_SLICE_RETRY_SERIAL (csrc/avr_internal.h), visible under k1p_keep_retry only
LONG = 1024 * 1024 + 4500                                    # more than 1024 chunks


# ------------------------------------------------------------------ batches and their expected answers

def _exact(rng, n, n_ctx, terminate):
    """A random K1 stream of exactly n records."""
    if terminate and n:
        return oracle_lib.random_cabac_stream(rng, n - 1, n_ctx, terminate=True)
    return oracle_lib.random_cabac_stream(rng, n, n_ctx, terminate=False)


_cache = {}


def cabac_batch(seed, n_ctx, long_slice=False, ragged=6, top=20000, rare=False):
    """(slices [(recs, init_states)], wants [(status, bytes, final states)], named {"declined": [...], "bad": i}).
    rare: single bins in contexts nobody else uses (the sampled census misses them), n_ctx + 34 contexts declared."""
    key = (seed, n_ctx, long_slice, ragged, top, rare)
    if key in _cache:
        return _cache[key]
    rng = np.random.default_rng(seed)
    lengths = list(EDGES) + [int(x) for x in rng.integers(2, top, ragged)]
    slices = [_exact(rng, n, n_ctx, bool(i % 3)) for i, n in enumerate(lengths)]
    plain = [id(x[0]) for x in slices if len(x[0]) > 1000]
    if n_ctx >= 40:                                          # (a chain needs contexts to steer by)
        slices.insert(3, carry_streams.carry_chain_cabac(np.random.default_rng(seed + 1), 5, 2200, "carry", n_ctx=n_ctx))
        slices.insert(9, carry_streams.carry_chain_cabac(np.random.default_rng(seed + 2), 3, 6000, "none", n_ctx=n_ctx))
    named = {"declined": []}
    # slices the scheme declines (no coded LPS for more than 16 chunks): test_chunked_random_and_declined_slices
    named["declined"].append(len(slices))
    slices.append(((np.ones(40000, np.uint16) | (1024 << 1)).astype(np.uint16), rng.integers(0, 126, n_ctx).astype(np.uint8)))
    named["declined"].append(len(slices))
    slices.append((np.ones(60000, np.uint16), np.full(n_ctx, 125, np.uint8)))
    # a malformed slice in the middle
    r, s = _exact(rng, 7000, n_ctx, True)
    named["bad"] = len(slices) // 2
    slices.insert(named["bad"], (br.spoil(r, 3500, br.SEL_NOP << 1), s))
    named["declined"] = [i + 1 for i in named["declined"]]
    if long_slice:
        slices.append(_exact(rng, LONG, n_ctx, True))
    ns = n_ctx
    if rare:
        ns = n_ctx + 34
        slices = [(r, np.concatenate([s, rng.integers(0, 126, ns - n_ctx).astype(np.uint8)])) for r, s in slices]
        at = [i for i, x in enumerate(slices) if id(x[0]) in plain][:3]
        assert len(at) == 3
        for i, ctx in zip(at, (ns - 1, n_ctx + 7, n_ctx)):
            slices[i][0][999] = np.uint16((ctx << 1) | (i & 1))
    wants = [br.expected(br.KIND_CABAC, r, s) for r, s in slices]
    assert wants[named["bad"]][0] == br.SLICE_BAD_RECORD and sum(w[0] != 0 for w in wants) == 1
    _cache[key] = (slices, wants, named)
    return _cache[key]


def range_batch(seed, long_slice=False, ragged=5, top=20000):
    key = ("range", seed, long_slice, ragged, top)
    if key in _cache:
        return _cache[key]
    rng = np.random.default_rng(seed)
    lengths = list(EDGES) + [int(x) for x in rng.integers(2, top, ragged)]
    slices = [oracle_lib.random_range_stream(rng, n, adaptive=bool(i % 2)) for i, n in enumerate(lengths)]
    slices.insert(2, carry_streams.carry_chain_range(np.random.default_rng(seed + 1), 20, 4104, "carry"))
    slices.insert(7, carry_streams.carry_chain_range(np.random.default_rng(seed + 2), 7, 1500, "cut"))
    slices.insert(len(slices) // 2, br.spoil(oracle_lib.random_range_stream(rng, 6000), 3000, 0x8000 | (5 << 1) | (9 << 8)))
    collapse = oracle_lib.random_range_stream(rng, 9000)     # neg 0: the double-precision walk hands the slice to the integer one
    collapse[4321] = np.uint16(0 | (77 << 1) | (0 << 8))
    slices.append(collapse)
    if long_slice:
        slices.append(oracle_lib.random_range_stream(rng, LONG, adaptive=False))
    wants = [br.expected(br.KIND_RANGE, r) for r in slices]
    assert sum(w[0] != 0 for w in wants) == 1
    _cache[key] = (slices, wants, {})
    return _cache[key]


def make(avr, kind, slices):
    if kind == avr.KIND_RANGE:
        return avr.DeviceWorkload.from_host(avr.KIND_RANGE, slices, None, 0)
    if kind == avr.KIND_CABAC8:
        rng = np.random.default_rng(len(slices))
        return avr.DeviceWorkload.from_host(avr.KIND_CABAC8, [r for r, _ in slices], [s for _, s in slices], 0,
                                            pad_bytes=rng.integers(0, 256, 4096).astype(np.uint8))
    return avr.DeviceWorkload.from_host(avr.KIND_CABAC, [r for r, _ in slices], [s for _, s in slices], 0)


def narrow(slices, wants):
    """The batch as one-byte records: the same expected answers, restated by the one-byte rule."""
    s8 = []
    for r, s in slices:
        sel = r >> 1
        ok = (sel < 126) | (sel == 1024) | (sel == 1025)
        r8 = to_records8(np.where(ok, r, 0).astype(np.uint16))
        r8[~ok] = np.uint8(br.TERM1_8)                       # (the malformed record: a put_terminate(1) that is not last)
        s8.append((r8, s))
    w8 = [br.expected(br.KIND_CABAC8, r, s) for r, s in s8]
    assert [w[0] for w in w8] == [w[0] for w in wants]
    return s8, w8


# ------------------------------------------------------------------ comparing a run with the oracle

def snapshot(w):
    """The outputs on the host (after the caller has synchronised)."""
    fs = w.final_states.cpu().numpy().reshape(w.n_slices, -1) if w.final_states is not None else None
    return w.out.cpu().numpy(), w.out_len.cpu().numpy().astype(np.int64), w.status.cpu().numpy(), fs


def compare(snap, off, wants, what, poison=None, left=()):
    """Status, length, bytes and final states of every slice (those in `left` apart: they were left uncoded on purpose), and --
    with `poison` -- every byte of out that is not a slice's own still holds what it held before the call."""
    out, lens, status, fs = snap
    mine = np.zeros(out.size, bool)
    for i, (st, data, final) in enumerate(wants):
        if i in left:
            mine[off[i]:off[i + 1]] = True
            continue
        assert status[i] == st, f"{what}: status of slice {i}: {status[i]}, want {st}"
        if data is None:                                     # (ZERO_PROB: only the status is specified)
            mine[off[i]:off[i + 1]] = True
            continue
        assert lens[i] == len(data), f"{what}: length of slice {i}: {lens[i]}, want {len(data)}"
        got = out[off[i]:off[i] + len(data)].tobytes()
        if got != data:
            at = next(k for k in range(len(data)) if got[k] != data[k])
            raise AssertionError(f"{what}: slice {i} ({len(data)} bytes) differs from byte {at} on")
        mine[off[i]:off[i] + len(data)] = True
        if final is not None and fs is not None:
            assert fs[i][:len(final)].tobytes() == final, f"{what}: final states of slice {i}"
    if poison is not None:
        bad = np.flatnonzero(~mine & (out != poison))
        assert bad.size == 0, f"{what}: {bad.size} bytes of out written outside the slices' bytes, first at {bad[:6].tolist()}"


class Case:
    """A workload in guarded buffers of the exact sizes, with the packer's statuses kept for every further run."""

    def __init__(self, avr, kind, batch, at8=False, two_stage=False, parts=0, weights=None, plain=False):
        import torch
        self.avr, (self.slices, self.wants, self.named) = avr, batch
        self.w = make(avr, kind, self.slices)
        if parts:
            assert self.w.set_parts(parts, weights) == parts
        if plain:
            self.w._counts = None                            # avr_cabac_encode_chunked_device itself, not the hinted call
        self.bufs = guarded.install(avr, self.w, at8=at8, two_stage=two_stage)
        self.off = self.w.out_off.cpu().numpy()
        self.status0 = self.w.status.clone()
        torch.cuda.synchronize()

    def prepare(self, poison):
        self.bufs.poison(poison, self.w)
        self.w.status.copy_(self.status0)

    def verify(self, what, poison=None, left=()):
        import torch
        torch.cuda.synchronize()
        compare(snapshot(self.w), self.off, self.wants, what, poison, left)
        self.bufs.check()


def run_settled(w):
    """One encode_chunked() and what settle() says about it."""
    import torch
    w.encode_chunked()
    torch.cuda.synchronize()
    return w.settle()


# ------------------------------------------------------------------ A + B: K1p from two-byte records

@pytest.mark.parametrize("n_ctx,at8", [(1, False), (86, True), (460, False), (1024, True)])
def test_k1p_one_call(avr, n_ctx, at8):
    """avr_cabac_encode_chunked_device (the call that asks the device and waits) under every poison; 86 contexts: with the slice of
    more than 1024 chunks; regions at 0 and at 8 mod 16."""
    c = Case(avr, avr.KIND_CABAC, cabac_batch(100 + n_ctx, n_ctx, long_slice=n_ctx == 86), at8=at8, plain=True)
    for poison in POISONS:
        c.prepare(poison)
        c.w.encode_chunked()
        assert c.w._hinted_path is None
        c.verify(f"{n_ctx} contexts, poison {poison:#x}", poison)


@pytest.mark.parametrize("case", ["right", "too-small", "second-pass"])
def test_k1p_hinted(avr, hooks, case):
    """avr_cabac_encode_chunked_device_hinted: asked (no guess), then sized by the right guess; by a guess that is too small and the
    documented re-run; with a census that sees next to nothing, so that slices are left (counts[1] > 0) for
    avr_cabac_encode_chunked_second_pass_device, which runs in the workspace the first pass left.  Poisoned before every call."""
    import torch
    if case == "second-pass":
        hooks(census_stride=4099)
    c = Case(avr, avr.KIND_CABAC, cabac_batch(200, 86, long_slice=True, rare=case == "second-pass"), at8=case == "too-small")
    w, left_counts = c.w, []
    for poison in POISONS:
        what = f"{case}, poison {poison:#x}"
        w.rows_hint = 0
        c.prepare(poison)
        first = run_settled(w)
        assert first["hint"] == 0 and 1 <= first["rows"] <= w.n_states and w._hinted_path == "chunked"
        c.verify(what + ", asked", poison)
        if case == "too-small":
            w.rows_hint = 5
        hint = w.rows_hint
        assert hint
        c.prepare(poison)
        w.encode_chunked()
        torch.cuda.synchronize()
        rows, left = int(w._counts[0]), int(w._counts[1])
        assert rows == first["rows"]
        left_counts.append(left)
        second = w.settle()
        assert second["hint"] == hint
        if case == "right":
            assert rows <= hint and left == 0 and not second["redone"]
        elif case == "too-small":
            assert rows > hint and second["redone"]
        else:
            assert rows <= hint and left >= 3 and second["redone"]      # the three slices with a rare context at least
        c.verify(what + ", guessed", poison)
    assert len(set(left_counts)) == 1, f"slices left for the second pass depend on the poison: {left_counts}"


@pytest.mark.parametrize("parts,weights", [(2, [1, 8]), (3, [1, 4, 4])])
def test_k1p_parts(avr, parts, weights):
    """avr_cabac_encode_chunked_device_parts in 2 and 3 parts, every part's workspace poisoned: asked, then sized by the guess.  (The
    parts are cut by chunk counts: the slice of more than 1024 chunks, last in its batch, is most of the second of two parts.)"""
    c = Case(avr, avr.KIND_CABAC, cabac_batch(300 + parts, 86, long_slice=parts == 2), parts=parts, weights=weights, at8=parts == 3)
    assert len([k for k in c.bufs.all if k.startswith("ws_part")]) == parts
    for poison in POISONS:
        c.w.rows_hint = 0
        for run in ("asked", "guessed"):
            c.prepare(poison)
            info = run_settled(c.w)
            assert c.w._hinted_path == "parts" and info["parts"] == parts and not info["redone"]
            assert info["hint"] == (0 if run == "asked" else c.w.rows_hint) and (run == "asked" or info["hint"])
            c.verify(f"{parts} parts, poison {poison:#x}, {run}", poison)


@pytest.mark.parametrize("at8", [False, True])
def test_two_stage(avr, at8):
    """avr_cabac_resolve_device, then avr_cabac_encode_resolved_device: both workspaces and the code buffer (res_total + 32 bytes)
    poisoned before the first stage, nothing touched between the stages."""
    c = Case(avr, avr.KIND_CABAC, cabac_batch(400, 460 if at8 else 86, long_slice=not at8), two_stage=True, at8=at8)
    for poison in POISONS:
        c.prepare(poison)
        codes = c.w.resolve()
        assert codes.data_ptr() == c.bufs.all["codes"].view.data_ptr() and codes.numel() == c.w._plan["plan"].res_total + 32
        c.w.encode_resolved(codes)
        c.verify(f"two-stage, poison {poison:#x}", poison)


# ------------------------------------------------------------------ A + B: one-byte records

@pytest.mark.parametrize("n_ctx,at8", [(1, True), (126, False)])
def test_k1p_one_byte_records(avr, n_ctx, at8):
    """avr_cabac8_encode_chunked_device (avr_cabac8_chunked_workspace_bytes)."""
    c = Case(avr, avr.KIND_CABAC8, narrow(*cabac_batch(500 + n_ctx, n_ctx, long_slice=n_ctx == 126)[:2]) + ({},), at8=at8)
    for poison in POISONS:
        c.prepare(poison)
        c.w.encode_chunked()
        c.verify(f"one-byte records, {n_ctx} contexts, poison {poison:#x}", poison)


# ------------------------------------------------------------------ A + B: K2p

@pytest.mark.parametrize("wave", [1, 2, 3])
@pytest.mark.parametrize("seg_len", [0, 1, 3])
def test_k2p(avr, hooks, seg_len, wave):
    """avr_range_encode_chunked_device: the passes whole and in segments of 1 and 3 chunks (two streams), pass 1 by a wave, a lane,
    and both.  S is indexed by the caller's out_off: regions at 0 and at 8 mod 16."""
    hooks(k2p_seg_len=seg_len, k2p_wave=wave)
    big = seg_len == 1 and wave == 1
    c = Case(avr, avr.KIND_RANGE, range_batch(600, long_slice=big), at8=bool((seg_len + wave) % 2))
    for poison in POISONS:
        c.prepare(poison)
        c.w.encode_chunked()
        c.verify(f"K2p seg_len {seg_len} wave {wave}, poison {poison:#x}", poison)


# ------------------------------------------------------------------ A: what a different batch left behind

def _share(big, small, names):
    """The small case runs in the front of the big one's buffers `names`."""
    for n in names:
        assert small.bufs.all[n].n <= big.bufs.all[n].n, n
        small.bufs.all.pop(n)
    return big, small


@pytest.mark.parametrize("entry", ["k1p", "k1p-parts", "one-byte", "two-stage", "k2p"])
def test_what_a_different_batch_left_behind(avr, hooks, entry):
    """Batch A (more slices, more chunks, more contexts, a slice of more than 1024 chunks) and batch B (smaller, other lengths)
    alternately A, B, A, B through ONE workspace sized for A: B's plan points into the front of what A left, and A then finds what B
    left in its own front.  Nothing is cleared in between but the outputs."""
    import torch
    if entry == "k2p":
        hooks(k2p_seg_len=3)
        A = Case(avr, avr.KIND_RANGE, range_batch(700, long_slice=True, ragged=9))
        B = Case(avr, avr.KIND_RANGE, range_batch(701, ragged=2, top=9000))
        B.w._plan["ws_k2"] = A.w._plan["ws_k2"]
        _share(A, B, ["ws_k2"])
    elif entry == "one-byte":
        A = Case(avr, avr.KIND_CABAC8, narrow(*cabac_batch(710, 126, long_slice=True, ragged=9)[:2]) + ({},))
        B = Case(avr, avr.KIND_CABAC8, narrow(*cabac_batch(711, 40, ragged=2, top=9000)[:2]) + ({},))
        B.w._plan["ws"] = A.w._plan["ws"]
        _share(A, B, ["ws"])
    else:
        parts = 2 if entry == "k1p-parts" else 0
        kw = dict(two_stage=entry == "two-stage", parts=parts, weights=[1, 8] if parts else None)
        A = Case(avr, avr.KIND_CABAC, cabac_batch(720, 460, long_slice=True, ragged=9), **kw)
        B = Case(avr, avr.KIND_CABAC, cabac_batch(721, 40, ragged=2, top=9000), **kw)
        names = ["ws", "ws1", "ws2", "codes"] if entry == "two-stage" else ["ws", "ws_part0", "ws_part1"] if parts else ["ws"]
        for n in names:
            if n.startswith("ws_part"):
                B.w._parts[int(n[-1])]["ws"] = A.w._parts[int(n[-1])]["ws"]
            else:
                B.w._plan[n] = A.w._plan[n]
        _share(A, B, names)
    A.prepare(0xFF)
    B.prepare(0x00)
    for k, c in enumerate((A, B, A, B)):
        for name in ("out", "out_len", "final_states"):
            if name in c.bufs.all:
                c.bufs.all[name].view.fill_(0x5A)
        c.w.status.copy_(c.status0)
        if entry == "two-stage":
            c.w.encode_resolved(c.w.resolve())
        else:
            run_settled(c.w)
        c.verify(f"{entry}: run {k} ({'AB'[k % 2]})", 0x5A)
        torch.cuda.synchronize()


# ------------------------------------------------------------------ A: a poison must not hide behind a hand-over

@pytest.mark.parametrize("entry", ["k1p", "one-byte", "two-stage"])
def test_the_same_slices_leave_the_parallel_path_under_every_poison(avr, hooks, entry):
    """With the serial kernel behind phase D left out (test hook k1p_keep_retry) the slices that leave the parallel path -- declined
    by the scheme, or handed over by phase D because its digit sums do not resolve -- keep AVR_SLICE_RETRY_SERIAL: the same set
    under every poison, the declined slices in it where the path declines (two-byte records, one call), and every other slice the
    oracle's -- phase D's own work."""
    import torch
    hooks(k1p_keep_retry=1)
    batch = cabac_batch(800, 86, long_slice=True)
    if entry == "one-byte":
        batch = narrow(*batch[:2]) + (batch[2],)
    c = Case(avr, avr.KIND_CABAC8 if entry == "one-byte" else avr.KIND_CABAC, batch, two_stage=entry == "two-stage", plain=True)
    sets = []
    for poison in POISONS:
        c.prepare(poison)
        if entry == "two-stage":
            c.w.encode_resolved(c.w.resolve())
        else:
            c.w.encode_chunked()
        torch.cuda.synchronize()
        left = set(np.flatnonzero(c.w.status.cpu().numpy() == RETRY_SERIAL).tolist())
        sets.append(left)
        c.verify(f"{entry}, poison {poison:#x}, phase D alone", None, left)
    assert sets[1] == sets[0] and sets[2] == sets[0], f"the slices handed over depend on the poison: {sets}"
    if entry == "k1p":
        assert set(c.named["declined"]) <= sets[0], (c.named, sets[0])
    assert len(sets[0]) <= len(c.named["declined"]), f"phase D handed over slices of its own: {sets[0]}"


# ------------------------------------------------------------------ A: the rare paths that reuse regions (test hooks)

@pytest.mark.parametrize("every", [1, 3])
@pytest.mark.parametrize("entry", ["k1p", "one-byte", "two-stage"])
def test_forced_hand_over(avr, hooks, entry, every):
    """k1p_force_retry_every: phase D hands every n-th slice to the serial kernel, which writes where phase D would have.  First with
    k1p_keep_retry, to see that exactly those slices were handed over; then the whole call under every poison."""
    import torch
    batch = cabac_batch(900, 86)
    if entry == "one-byte":
        batch = narrow(*batch[:2]) + (batch[2],)
    c = Case(avr, avr.KIND_CABAC8 if entry == "one-byte" else avr.KIND_CABAC, batch, two_stage=entry == "two-stage", at8=every == 3)
    run = (lambda: c.w.encode_resolved(c.w.resolve())) if entry == "two-stage" else (lambda: run_settled(c.w))
    hooks(k1p_force_retry_every=every, k1p_keep_retry=1)
    c.prepare(0xFF)
    c.w._counts, counts = None, c.w._counts                  # (the asking call: a settle() would code nothing more)
    run()
    torch.cuda.synchronize()
    left = set(np.flatnonzero(c.w.status.cpu().numpy() == RETRY_SERIAL).tolist())
    forced = {i for i in range(c.w.n_slices) if i % every == 0 and c.wants[i][0] == 0}
    assert forced <= left and left <= forced | set(c.named["declined"]), (left, forced)
    c.w._counts = counts
    hooks(k1p_force_retry_every=every)
    for poison in POISONS:
        c.prepare(poison)
        run()
        c.verify(f"{entry}, every {every}, poison {poison:#x}", poison)


def test_context_chains_whole_and_in_segments(avr, hooks):
    """chain_whole / chain_segments / chain_nsegs / chain_force_redo: the chains start to end, or in segments whose summaries live in
    the LAST region of the resolver's workspace, which nothing else writes.  That the hooks took the paths they name shows in the
    workspace: under chain_whole that region keeps the poison, in segments it does not.  Then through the one call, whose workspace
    holds the same regions."""
    rng = np.random.default_rng(1000)
    slices = [_exact(rng, n, 30, True) for n in (65536, 40000, 8 * 1024, 5 * 1024 + 3, 131072 + 777)]
    slices.insert(2, carry_streams.carry_chain_cabac(np.random.default_rng(1001), 5, 3000, "carry", n_ctx=30))
    wants = [br.expected(br.KIND_CABAC, r, s) for r, s in slices]
    c = Case(avr, avr.KIND_CABAC, (slices, wants, {}), two_stage=True)
    ws1 = c.bufs.all["ws1"]
    extent = {}
    for mode, kw in (("whole", dict(chain_whole=1)), ("nsegs2", dict(chain_segments=1, chain_nsegs=2)),
                     ("segments", dict(chain_segments=1)), ("redo3", dict(chain_segments=1, chain_force_redo=3))):
        hooks(**kw)
        ext = []
        for poison in POISONS:
            c.prepare(poison)
            c.w.encode_resolved(c.w.resolve())
            c.verify(f"chains {mode}, poison {poison:#x}", poison)
            ext.append(ws1.extent(poison))
        extent[mode] = max(ext)
    print("touched extent of the resolver's workspace:", extent, "of", ws1.n)
    assert extent["whole"] < min(extent["nsegs2"], extent["segments"], extent["redo3"]) <= ws1.n, extent
    c2 = Case(avr, avr.KIND_CABAC, (slices, wants, {}), plain=True)
    for kw in (dict(chain_whole=1), dict(chain_segments=1, chain_force_redo=3)):
        hooks(**kw)
        for poison in POISONS:
            c2.prepare(poison)
            c2.w.encode_chunked()
            c2.verify(f"one call, chains {kw}, poison {poison:#x}", poison)


@pytest.mark.parametrize("waves", [1, 3, 8])
def test_local_waves(avr, hooks, waves):
    """local_waves: the chunk sort in workgroups of 1, 3 and 8 waves (the grid and the LDS rows follow the workgroup's size)."""
    hooks(local_waves=waves)
    c = Case(avr, avr.KIND_CABAC, cabac_batch(1100, 86), at8=waves == 3)
    for poison in POISONS:
        c.w.rows_hint = 0
        c.prepare(poison)
        run_settled(c.w)
        c.verify(f"local_waves {waves}, poison {poison:#x}", poison)


# ------------------------------------------------------------------ B: the packers' tiles and the resolver's records

def test_tiles_of_exactly_the_documented_size(avr):
    """avr_pack_tiles_device and avr_pack_tiles8_narrow_device into tile buffers of exactly tile_off[n_tiles] * 16 bytes.  One-byte
    tiles: "a lane writes its own slice's chunks only": the columns of shorter slices and of lanes past the last slice keep the canary."""
    import torch
    from avrecode_ms_amd.device import plan_tiles
    slices, wants, _ = cabac_batch(1200, 100, ragged=70, top=3000)
    L = avr.lib()
    sp = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    w = make(avr, avr.KIND_CABAC, slices)
    n_units = int(w.tile_off[-1])
    g = guarded.Guarded(n_units * 16, w.n_bins.device, "two-byte tiles")
    st = torch.zeros(w.n_slices, dtype=torch.int32, device=w.n_bins.device)
    assert L.avr_pack_tiles_device(0, sp, avr.KIND_CABAC, w.n_states, w.rec_flat.data_ptr(), w.rec_off.data_ptr(), w.n_bins.data_ptr(),
                                   w.order.data_ptr(), w.n_slices, w.tile_off.data_ptr(), g.view.data_ptr(), st.data_ptr()) == 0
    torch.cuda.synchronize()
    g.check()
    assert torch.equal(st, w.status)
    s8, _ = narrow(slices, wants)
    w8 = make(avr, avr.KIND_CABAC8, s8)
    order, tile_off = plan_tiles(w8.n_bins, 16)
    n_units = int(tile_off[-1])
    g = guarded.Guarded(n_units * 16, w8.n_bins.device, "one-byte tiles")
    assert L.avr_pack_tiles8_narrow_device(0, sp, w8.n_states, w8.rec8_flat.data_ptr(), w8.rec8_off.data_ptr(), w8.n_bins.data_ptr(),
                                           order.data_ptr(), w8.n_slices, tile_off.data_ptr(), g.view.data_ptr(), st.data_ptr()) == 0
    torch.cuda.synchronize()
    g.check()
    tiles = g.view.cpu().numpy().reshape(n_units, 16)
    written = np.zeros(n_units, bool)
    nb, order_h, toff = w8.n_bins.cpu().numpy(), order.cpu().numpy(), tile_off.cpu().numpy()
    flat, roff = w8.rec8_flat.cpu().numpy(), w8.rec8_off.cpu().numpy()
    for k, s in enumerate(order_h):
        chunks = (int(nb[s]) + 15) // 16
        at = int(toff[k // 64]) + np.arange(chunks) * 64 + k % 64
        written[at] = True
        assert np.array_equal(tiles[at].reshape(-1), flat[int(roff[s]):int(roff[s]) + 16 * chunks]), f"slice {s}"
    assert (~written).sum() > 1000 and (tiles[~written] == guarded.CANARY).all(), "a lane wrote outside its own slice's chunks"


def test_estimator_resolver_in_exact_buffers(avr, oracle):
    """avr_range_resolve_device: workspace, recs_out and est_out of exactly the quoted / documented sizes; "what lies between [a
    slice's next multiple of 8 records] and the next slice's rec_off is not touched": the gap records keep the canary."""
    import torch
    import range_keys as rk
    rng = np.random.default_rng(1300)
    slices = [rk.random_keys(rng, n, "skew") for n in (0, 1, 1023, 1024, 1025, 4097, 20000, 7, 3000)]
    gf = [0, 3, 3, 7, 9]
    want, want_tabs = rk.resolve(slices, gf)
    kw = avr.DeviceWorkload.from_host_keys(slices, gf, gap=2)
    dev = kw.n_bins.device
    p = kw._chunk_plan()
    p["ws_est_bytes"] = avr.lib().avr_range_resolve_workspace_bytes(kw.n_slices, kw.n_groups, ctypes.byref(p["plan"]))
    gs = [guarded.Guarded(p["ws_est_bytes"], dev, "ws_est"), guarded.Guarded(2 * int(kw.rec_off[-1]), dev, "recs_out"),
          guarded.Guarded(kw.n_groups * avr.EST_KEYS * 2, dev, "est_out")]
    p["ws_est"], kw.rec_flat, kw.est_out = gs[0].view, gs[1].as_dtype(torch.int16), gs[2].view
    rec_off, n_bins = kw.rec_off.cpu().numpy(), kw.n_bins.cpu().numpy()
    for poison in POISONS:
        gs[0].view.fill_(poison)
        gs[1].view.fill_(guarded.CANARY)
        gs[2].view.fill_(poison)
        kw.status.zero_()
        kw.resolve_keys()
        torch.cuda.synchronize()
        for g in gs:
            g.check()
        recs = kw.rec_flat.cpu().numpy().view(np.uint16)
        for i in range(kw.n_slices):
            o, nb = int(rec_off[i]), int(n_bins[i])
            pad = (o + nb + 7) // 8 * 8
            assert np.array_equal(recs[o:o + nb], want[i]) and not recs[o + nb:pad].any(), f"slice {i}, poison {poison:#x}"
            assert (recs[pad:int(rec_off[i + 1])] == guarded.CANARY * 0x0101).all() and int(rec_off[i + 1]) - pad == 16, f"gap behind slice {i}"
        est = kw.est_out.cpu().numpy().reshape(-1, rk.N_KEYS, 2)
        assert all(np.array_equal(est[g], want_tabs[g]) for g in range(kw.n_groups)) and not kw.status.any()


# ------------------------------------------------------------------ A + B at full size: config 2

def _config2_digest(avr, oracle, kind):
    import hashlib
    n = 512
    cfg, nbh, off, recs, states = host_synth(avr, 2, n, kind, 1000)
    flat, roff = compact(recs, off, nbh)
    want, st = oracle.encode_batch(kind, flat, roff, states if kind == avr.KIND_CABAC else None, cfg.n_states if kind == avr.KIND_CABAC else 0,
                                   threads=16)
    assert not st.any()
    dig = lambda chunks: hashlib.sha256(b"".join(hashlib.sha256(c).digest() for c in chunks)).hexdigest()
    return [len(x) for x in want], dig(want), dig


@pytest.mark.parametrize("path", ["parts", "k2p"])
def test_full_size_config2_poisoned(avr, oracle, path):
    """BASELINE.json configs[1] at its own 512 slices (where the parts fill workgroup rounds and K2p's passes run in segments by
    themselves), workspaces and outputs filled with 0xFF, exact sizes, every slice against the threaded oracle by a checksum of
    checksums.  (The touched extents it prints are what tools/workspace_extent.py records in profiles/workspace_extent.json.)"""
    import torch
    kind = avr.KIND_CABAC if path == "parts" else avr.KIND_RANGE
    w = avr.DeviceWorkload.synth(2, 512, kind, 0, 1000)
    if path == "parts":
        assert w.set_parts(0) == 2
    bufs = guarded.install(avr, w)
    off = w.out_off.cpu().numpy()
    runs = ("asked", "guessed") if path == "parts" else ("once",)
    for run in runs:
        bufs.poison(0xFF, w)
        w.status.zero_()
        info = run_settled(w)
        assert not info["redone"] and (path != "parts" or (w._hinted_path == "parts" and bool(info["hint"]) == (run == "guessed")))
    torch.cuda.synchronize()
    bufs.check()
    out, lens, status, _ = snapshot(w)
    assert not status.any()
    want_lens, want_dig, dig = _config2_digest(avr, oracle, kind)
    assert lens.tolist() == want_lens
    assert dig([out[off[i]:off[i] + lens[i]].tobytes() for i in range(512)]) == want_dig
    mine = np.zeros(out.size, bool)
    for i in range(512):
        mine[off[i]:off[i] + lens[i]] = True
    assert (out[~mine] == 0xFF).all()
    print({k: (g.extent(0xFF), g.n) for k, g in bufs.workspaces().items()}, "(touched, quoted) bytes of each workspace")


# ------------------------------------------------------------------ C: the caller's stream

@pytest.fixture(scope="module")
def hold():
    """hold(ms): a sleep kernel of about that long on the current stream."""
    import torch
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    torch.cuda._sleep(1_000_000)
    torch.cuda.synchronize()
    ev[0].record()
    torch.cuda._sleep(20_000_000)
    ev[1].record()
    torch.cuda.synchronize()
    per_ms = 20_000_000 / max(ev[0].elapsed_time(ev[1]), 1e-3)
    return lambda ms: torch.cuda._sleep(int(per_ms * ms))


def on_own_stream(c, stream, hold, call, never_blocks, what, ms=150):
    """The call behind a sleep on `stream`; right behind it, ON THE STREAM, the outputs copied to snapshots and every workspace
    overwritten; then that stream alone is synchronised and the snapshots are compared with the oracle."""
    import torch
    w = c.w
    keep = [t for t in (w.out, w.out_len, w.status, w.final_states) if t is not None]
    snaps = [torch.empty_like(t) for t in keep]
    with torch.cuda.stream(stream):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        hold(ms)
        ev[1].record()
        t0 = time.perf_counter()
        call()
        t1 = time.perf_counter()
        for s, t in zip(snaps, keep):
            s.copy_(t, non_blocking=True)
        for g in c.bufs.workspaces().values():
            g.view.fill_(0xFF)
        if "codes" in c.bufs.all:
            c.bufs.all["codes"].view.fill_(0xFF)
        stream.synchronize()
        host = [s.cpu().numpy() for s in snaps]
    slept = ev[0].elapsed_time(ev[1])
    assert slept > ms / 2, slept
    if never_blocks:
        assert (t1 - t0) * 1e3 < slept / 10, f"{what}: the call took {(t1 - t0) * 1e3:.1f} ms behind a sleep of {slept:.0f} ms"
    fs = host[3].reshape(w.n_slices, -1) if len(host) > 3 else None
    compare((host[0], host[1].astype(np.int64), host[2], fs), c.off, c.wants, what)
    c.bufs.check()


@pytest.mark.parametrize("entry", ["k1p", "k1p-parts2", "k1p-parts3", "one-byte", "k2p-segments"])
def test_on_a_stream_of_the_callers_own(avr, hooks, hold, entry):
    """K1p as one call and in parts with a small first part (part 0 runs on the caller's stream, which then runs dry long before the side
    streams do), the one-byte call, K2p in segments (a side stream of its own).  The K1p runs are the workload's SECOND one, sized by
    the guess: nothing of such a call waits, so all of it is still queued behind the sleep when the snapshot is enqueued -- and the
    calls that "never block" return while the sleep runs."""
    import torch
    stream = torch.cuda.Stream()
    if entry == "k2p-segments":
        hooks(k2p_seg_len=1)
        c = Case(avr, avr.KIND_RANGE, range_batch(600, long_slice=True))
    elif entry == "one-byte":
        c = Case(avr, avr.KIND_CABAC8, narrow(*cabac_batch(1400, 126, long_slice=True)[:2]) + ({},))
    else:
        parts = int(entry[-1]) if "parts" in entry else 0
        c = Case(avr, avr.KIND_CABAC, cabac_batch(1400, 86, long_slice=parts != 3), parts=parts,      # (three parts: cut by chunk counts, no slice may hold most of them)
                 weights=[1, 8] if parts == 2 else [1, 4, 4] if parts else None)
    never_blocks = entry != "k2p-segments"                   # (K2p does not wait either; the header lists the others)
    with torch.cuda.stream(stream):                          # the first run (K1p from two-byte records: it asks the device and waits on this stream)
        c.prepare(0x5A)
        c.w.encode_chunked()
        stream.synchronize()
        assert not c.w.settle()["redone"] and (c.w.kind != avr.KIND_CABAC or c.w.rows_hint)
    for rep in range(2):
        with torch.cuda.stream(stream):
            c.prepare(0xFF)
        on_own_stream(c, stream, hold, c.w.encode_chunked, never_blocks, f"{entry}, run {rep}")
        if c.w.kind == avr.KIND_CABAC:
            assert int(c.w._counts[0] if not getattr(c.w, "_parts", None) else c.w._part_counts[0]) <= c.w.rows_hint


@pytest.mark.parametrize("kind", ["k1", "k1-one-byte-tiles", "k2"])
def test_serial_paths_pack_then_encode_on_a_stream_of_the_callers_own(avr, hold, kind):
    """pack -> encode of the one-lane-per-slice paths on the caller's stream: the packer's tiles are the coder's input, with
    nothing but stream order between them.  avr_cabac8_encode_tiles_device never blocks."""
    import torch
    stream = torch.cuda.Stream()
    L = avr.lib()
    if kind == "k2":
        slices, wants, _ = range_batch(1500)
        w = make(avr, avr.KIND_RANGE, slices)
    else:
        slices, wants, _ = cabac_batch(1500, 100)
        if kind == "k1":
            w = make(avr, avr.KIND_CABAC, slices)
        else:
            slices, wants = narrow(slices, wants)
            w = avr.DeviceWorkload.from_host(avr.KIND_CABAC8, [r for r, _ in slices], [s for _, s in slices], 0, narrow_tiles=True)
    c = Case.__new__(Case)
    c.avr, c.slices, c.wants, c.named, c.w = avr, slices, wants, {}, w
    c.bufs = guarded.Buffers()
    tiles = c.bufs.add("ws_tiles", w.tiles.numel(), w.n_bins.device)       # (overwritten behind the call like a workspace)
    c.off = w.out_off.cpu().numpy()
    w.tiles = tiles.view
    torch.cuda.synchronize()

    def call():
        sp = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        assert sp.value == stream.cuda_stream
        if kind == "k1-one-byte-tiles":
            rc = L.avr_pack_tiles8_narrow_device(0, sp, w.n_states, w.rec8_flat.data_ptr(), w.rec8_off.data_ptr(), w.n_bins.data_ptr(),
                                                 w.order.data_ptr(), w.n_slices, w.tile_off.data_ptr(), w.tiles.data_ptr(), w.status.data_ptr())
        else:
            rc = L.avr_pack_tiles_device(0, sp, w.kind, w.n_states, w.rec_flat.data_ptr(), w.rec_off.data_ptr(), w.n_bins.data_ptr(),
                                         w.order.data_ptr(), w.n_slices, w.tile_off.data_ptr(), w.tiles.data_ptr(), w.status.data_ptr())
        assert rc == 0
        w.encode()

    with torch.cuda.stream(stream):                          # the first run (two-byte K1: it asks; the second is sized by its count)
        w.status.zero_()
        call()
        stream.synchronize()
        w.settle()
        assert kind != "k1" or w.rows_hint
    with torch.cuda.stream(stream):
        w.tiles.fill_(0x5A); w.out.fill_(0x5A); w.out_len.fill_(0x5A); w.status.zero_()
    on_own_stream(c, stream, hold, call, kind != "k2", kind)


def test_resolver_never_blocks_on_a_stream_of_the_callers_own(avr, oracle, hold):
    """avr_range_resolve_device and the K2p call behind it, on the caller's stream behind a sleep."""
    import torch
    import range_keys as rk
    rng = np.random.default_rng(1600)
    slices = [rk.random_keys(rng, n, "skew") for n in (30000, 0, 1025, 45000, 4096, 20001)]
    gf = [0, 2, 6]
    want, _ = rk.resolve(slices, gf)
    wants = [br.expected(br.KIND_RANGE, r) for r in want]
    kw = avr.DeviceWorkload.from_host_keys(slices, gf)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        rw = kw.resolve_range()                              # the first run: the plans and workspaces are made (DeviceWorkload itself waits for sizes)
        rw.encode_chunked()
        stream.synchronize()
        assert rw.rec_flat is kw.rec_flat
        out = torch.empty_like(rw.out)
        lens, status = torch.empty_like(rw.out_len), torch.empty_like(rw.status)
        kw._chunk_plan()["ws_est"].fill_(0xFF)
        kw.rec_flat.fill_(-1)
        rw.out.fill_(0x5A); rw.out_len.fill_(0x5A)
        kw.status.zero_(); rw.status.zero_()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        hold(150)
        ev[1].record()
        t0 = time.perf_counter()
        kw.resolve_keys()
        t1 = time.perf_counter()
        rw.encode_chunked()
        out.copy_(rw.out, non_blocking=True); lens.copy_(rw.out_len, non_blocking=True); status.copy_(rw.status, non_blocking=True)
        kw._chunk_plan()["ws_est"].fill_(0xFF)
        rw._chunk_plan()["ws_k2"].fill_(0xFF)
        stream.synchronize()
        snap = (out.cpu().numpy(), lens.cpu().numpy().astype(np.int64), status.cpu().numpy(), None)
    slept = ev[0].elapsed_time(ev[1])
    assert slept > 75 and (t1 - t0) * 1e3 < slept / 10, (t1 - t0, slept)
    compare(snap, rw.out_off.cpu().numpy(), wants, "resolver + K2p behind a sleep", 0x5A)


def test_two_workloads_on_two_streams_from_one_thread(avr, hooks, hold):
    """Two streams, one thread, the calls enqueued alternately (the header: one thread per stream): K1p in parts on one, K2p in
    segments on the other, then the one-byte call and K2p swapped over -- each stream's scratch, side streams and events are its own."""
    import torch
    hooks(k2p_seg_len=3)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    a = Case(avr, avr.KIND_CABAC, cabac_batch(1400, 86, long_slice=True), parts=2, weights=[1, 8])
    b = Case(avr, avr.KIND_RANGE, range_batch(600, long_slice=True))
    e = Case(avr, avr.KIND_CABAC8, narrow(*cabac_batch(1400, 126, long_slice=True)[:2]) + ({},))
    with torch.cuda.stream(s1):
        a.w.encode_chunked()
        s1.synchronize()
        assert not a.w.settle()["redone"]
    for first, second in (((a, s1), (b, s2)), ((b, s1), (e, s2)), ((a, s2), (b, s1))):
        for c, s in (first, second):
            with torch.cuda.stream(s):
                c.prepare(0xFF)
                hold(30)
        for rep in range(3):
            for c, s in (first, second):
                with torch.cuda.stream(s):
                    if rep:
                        c.w.status.copy_(c.status0)
                    c.w.encode_chunked()
        for c, s in (first, second):
            with torch.cuda.stream(s):
                s.synchronize()
                compare(snapshot(c.w), c.off, c.wants, f"kind {c.w.kind} on its own stream beside another", 0xFF)
                c.bufs.check()
