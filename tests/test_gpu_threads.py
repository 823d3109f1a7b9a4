"""GPU: the library from six host threads at once, each on a stream of its own (tests/threads.py has the crew).

include/avrecode_ms_amd.h promises: one avr_batch per host thread, calls on different batches independent, avr_last_error() the calling
thread's; and ONE THREAD PER STREAM -- what the library keeps between calls (the renumbering's scratch, K2p's side stream and events,
the part streams: StreamPool, csrc/avr_internal.h; K1p's constant table and its event; the kernels' dynamic-LDS attributes) is kept per
(device, stream), per device or per kernel, all of it made on first use.  Every other test calls from one thread.  Here:

  a  six device paths side by side, three rounds, the paths moving one worker on every round, so that every path runs on three
     threads and streams and every stream's scratch serves three batches: bytes, lengths, statuses and final states against the
     oracle, `out` untouched outside the slices' bytes, the guards intact.  The dense-count protocol degrades quietly by design -- a
     table another call overwrote turns into "contexts the census missed", which the serial kernel codes exactly -- so the PATH is
     compared too: each path runs alone first, and per round settle()'s rows and redone, the counts left for the second pass and
     (test hook k1p_keep_retry) the set of slices that leave the parallel path must be the lone run's; with census_stride = 1 the
     rows must be numpy's count of the contexts in use.
  b  six avr_batch objects side by side, four rounds of fill, run, collect, held to tests/batch_reuse.py's expectations and to what
     the same rounds report on a lone object (avr_batch_run_info).  All six pass a barrier in front of avr_batch_run.  Behind it
     one worker does not run at once: it destroys its batch and makes a new one (avr_batch_destroy: forget_part_streams,
     forget_stream) once a call of the five others is in flight, then fills and runs the new object; how many calls were in flight
     at the destroy is recorded and must be one at least in some round.  Another worker provokes a refusal every round and reads
     its own message behind the same barrier, while the others are inside avr_batch_run, and again behind its own run.
  c  the first use itself, which happens once per process: a child process (python tests/threads.py <first>) whose first library
     calls are made by six threads at the same moment.

Overlap is counted (threads.Crew): every round all six workers are inside it together, behind a sleep kernel each, and the calls
that block the calling thread overlap at least in pairs.  Test hooks are set in the main thread before the workers start."""
import copy
import json
import subprocess
import sys
import time

import numpy as np
import pytest

import batch_reuse as br
import test_gpu_workspace as ws
import threads
from test_gpu_workspace import hold                              # noqa: F401  (the sleep-kernel fixture)

pytestmark = pytest.mark.gpu

T = threads.T
POISONS = ws.POISONS


# ------------------------------------------------------------------ a. the device paths
class Path:
    """A Case and how one round of its path goes: steps(c, crew), each a call (or two) of the library on the current stream."""

    def __init__(self, name, c, steps, counted=False, k1p=False):
        import torch
        self.name, self.c, self.steps, self.counted, self.k1p = name, c, steps, counted, k1p
        w = c.w
        self.keep = [t for t in (w.out, w.out_len, w.status, w.final_states) if t is not None]
        self.snaps = [torch.empty_like(t) for t in self.keep]

    def _copy(self):
        for s, t in zip(self.snaps, self.keep):
            s.copy_(t, non_blocking=True)

    def finish(self, stream):
        """Behind a step: the outputs copied on the stream, the stream synchronised, what the device reported (settle() runs the
        second pass where slices were left for it, in the workspace as the call left it), the snapshot on the host."""
        w = self.c.w
        self._copy()
        stream.synchronize()
        parts = getattr(w, "_parts", None)
        if parts:
            left = [int(w._part_counts[2 * i + 1]) for i in range(w.n_parts)]
        else:
            left = [int(w._counts[1])] if w._counts is not None and w._hinted_path else [0]
        info = w.settle(stream)                                  # (waits for this stream alone, never for the device)
        if info["redone"]:
            self._copy()
            stream.synchronize()
        host = [s.cpu().numpy() for s in self.snaps]
        fs = host[3].reshape(w.n_slices, -1) if len(host) > 3 else None
        return (host[0], host[1].astype(np.int64), host[2], fs), {"rows": info["rows"], "redone": bool(info["redone"]), "left": left}

    def play(self, crew, stream, poison):
        """One round on the current stream (poisoned by the caller): [(snapshot, info)] of every step."""
        got = []
        for k, step in enumerate(self.steps):
            if k:
                # The one thing a worker does besides calling the library, copying snapshots and synchronising its stream: between
                # the two calls of a two-step path the buffers are poisoned and the packer's statuses put back -- tensor fills and
                # a copy, enqueued on the worker's own stream, in order between its two calls.  The main thread cannot do it: the
                # second call is sized by what the first one reported in this round, on this stream.
                self.c.prepare(poison)
            step(self.c, crew)
            got.append(self.finish(stream))
        return got


def tiles_asked(c, crew):
    c.w.rows_hint = 0
    with crew.blocking:                                          # asks the device for the context count and waits
        c.w.encode()
    assert c.w._hinted_path == "tiles"


def tiles_hinted(c, crew):
    assert c.w.rows_hint
    c.w.encode()


def chunked(c, crew):
    assert c.w.kind != c.avr.KIND_CABAC or c.w.rows_hint       # two-byte records: sized by the lone run's count, nothing waits
    c.w.encode_chunked()


def two_stage(c, crew):
    with crew.blocking:
        codes = c.w.resolve()
    c.w.encode_resolved(codes)


def make_paths(avr):
    C = ws.Case
    wide = ws.cabac_batch(2100, 215)
    rare = ws.cabac_batch(2102, 86, rare=True)
    return [
        # two-byte K1 tiles, asked, 215 contexts: 189 to 236 rows are four waves of more than 48 KiB of dynamic LDS (launch_cabac_encode)
        Path("k1-tiles-215-asked", C(avr, avr.KIND_CABAC, wide), [tiles_asked], counted=True),
        Path("k1-tiles-86-asked-hinted", C(avr, avr.KIND_CABAC, ws.cabac_batch(2101, 86)), [tiles_asked, tiles_hinted], counted=True),
        Path("k1p-2-parts-rare", C(avr, avr.KIND_CABAC, rare, parts=2, weights=[1, 2]), [chunked], counted=True, k1p=True),
        Path("k1p-one-byte-126", C(avr, avr.KIND_CABAC8, ws.narrow(*ws.cabac_batch(2103, 126)[:2]) + ({},), at8=True), [chunked], k1p=True),
        Path("k2p-segments-of-3", C(avr, avr.KIND_RANGE, ws.range_batch(2104)), [chunked]),
        Path("two-stage", C(avr, avr.KIND_CABAC, ws.cabac_batch(2105, 86), two_stage=True), [two_stage], k1p=True),
    ]


def hold_to_oracle(p, got, what, poison, mode):
    """Every step's snapshot against the oracle; returns what is compared between the lone run and the rounds: [(info, left set)]."""
    seen = []
    for k, (snap, info) in enumerate(got):
        left = set(np.flatnonzero(snap[2] == ws.RETRY_SERIAL).tolist())
        assert mode == "hand-over" or not left, f"{what}: slices {sorted(left)} were left uncoded"
        assert p.k1p or not left
        ws.compare(snap, p.c.off, p.c.wants, f"{what}, step {k}", poison, left)
        seen.append((info, left))
    return seen


MODES = {"paths": {}, "exact-census": {"census_stride": 1}, "hand-over": {"k1p_keep_retry": 1}}


@pytest.mark.parametrize("mode", list(MODES))
def test_device_paths_side_by_side(avr, hooks, hold, mode):                 # noqa: F811
    import torch
    hooks(k2p_seg_len=3, **MODES[mode])                          # in the main thread, before any worker exists
    paths = make_paths(avr)
    assert len(paths) == T
    crew = threads.Crew(hold)
    own = torch.cuda.Stream()
    assert own.cuda_stream not in [s.cuda_stream for s in crew.streams]
    lone, t0 = {}, time.perf_counter()
    # every path alone, in the main thread on a stream of its own: what it reports under every poison
    with torch.cuda.stream(own):
        for p in paths:
            w = p.c.w
            if p.name.startswith("k1p-2-parts"):             # the asking call once: the rounds are sized by its count
                p.c.prepare(0x5A)
                w.encode_chunked()
                own.synchronize()
                first = w.settle(own)
                assert w._hinted_path == "parts" and first["hint"] == 0 and first["parts"] == 2 and w.rows_hint
            lone[p.name] = []
            for poison in POISONS:
                p.c.prepare(poison)
                lone[p.name].append(hold_to_oracle(p, p.play(crew, own, poison), f"{p.name} alone, poison {poison:#x}", poison, mode))
            p.c.bufs.check()
            infos = [[s[0] for s in per] for per in lone[p.name]]
            lefts = [[s[1] for s in per] for per in lone[p.name]]
            assert infos[1] == infos[0] and infos[2] == infos[0], f"{p.name} alone: what the device reports depends on the poison: {infos}"
            assert lefts[1] == lefts[0] and lefts[2] == lefts[0], f"{p.name} alone: the slices handed over depend on the poison: {lefts}"
            rows = infos[0][0]["rows"]
            if p.name == "k1-tiles-215-asked" and mode != "hand-over":
                lds = 4 * ((rows + 7) // 4) * 256
                assert 48 * 1024 < lds <= 60 * 1024, f"{rows} rows: {lds} bytes of LDS do not go through hipFuncSetAttribute in four waves"
            if p.counted and mode == "exact-census":
                parts = getattr(w, "_parts", None) or [{"first": 0, "n": w.n_slices}]
                want = max(threads.contexts_in_use(p.c.slices[q["first"]:q["first"] + q["n"]], w.n_states) for q in parts)
                assert [i["rows"] for i in infos[0]] == [want] * len(infos[0]), f"{p.name}: rows {infos[0]}, contexts in use {want}"
            if p.name.startswith("k1p-2-parts"):
                if mode == "paths":                          # the sampled census misses a rare context: slices are left, settle() runs their second pass
                    assert sum(infos[0][0]["left"]) >= 1 and infos[0][0]["redone"], infos[0]
                if mode == "exact-census":
                    assert sum(infos[0][0]["left"]) == 0 and not infos[0][0]["redone"], infos[0]
                if mode == "hand-over":
                    assert set(p.c.named["declined"]) <= lefts[0][0], (p.c.named, lefts[0])
    torch.cuda.synchronize()
    lone_s = time.perf_counter() - t0
    crew.blocking.reset()

    def between(r):
        for p in paths:
            p.c.prepare(POISONS[r])
        torch.cuda.synchronize()

    def work(t, r, crew):
        return paths[(t - r) % T].play(crew, crew.streams[t], POISONS[r])      # path k on worker (k + r) % T

    try:
        results = crew.run(len(POISONS), work, between)
    finally:
        torch.cuda.synchronize()
    print(f"mode {mode}: inside-a-round peaks {crew.round_peaks}, blocking calls at once {crew.blocking.peak}, the lone runs {lone_s:.2f} s")
    for r, poison in enumerate(POISONS):
        for t in range(T):
            p = paths[(t - r) % T]
            what = f"{p.name} on worker {t}, round {r}, poison {poison:#x}"
            seen = hold_to_oracle(p, results[t][r], what, poison, mode)
            assert [s[0] for s in seen] == [s[0] for s in lone[p.name][r]], f"{what}: the device reports {[s[0] for s in seen]}, alone {[s[0] for s in lone[p.name][r]]}"
            assert [s[1] for s in seen] == [s[1] for s in lone[p.name][r]], f"{what}: slices {[sorted(s[1]) for s in seen]} left the parallel path, alone {[sorted(s[1]) for s in lone[p.name][r]]}"
    for p in paths:
        p.c.bufs.check()
    assert crew.blocking.peak >= 2, f"the blocking calls never overlapped: at most {crew.blocking.peak} at once"


# ------------------------------------------------------------------ b. the batch objects
def batch_runs():
    """Six runs, a worker each: two-byte K1 with set_verify_k1 and an expectation a slice; two-byte K1 plain; one-byte K1; codes; K2
    tiles (its worker provokes a refusal a round); K2p from key records in two groups with set_verify.  On the test build the
    k1_path hook sends all of them through the intra-slice parallel kernels.  DESTROYER: whose object goes and comes."""
    return [br.make_run("threads-cabac-checked", "cabac", "lanes", 8100, n_slices=40, n_states=60, n_ctx=50, verify=True, expect="right"),
            br.make_run("threads-cabac-plain", "cabac", "lanes", 8101, n_slices=50, n_states=100, n_ctx=90),
            br.make_run("threads-cabac8", "cabac8", "lanes", 8102, n_slices=45, n_states=64, n_ctx=60),
            br.make_run("threads-codes", "codes", "lanes", 8103, n_slices=48, n_states=70),
            br.make_run("threads-range", "range", "lanes", 8104, n_slices=60),
            br.make_run("threads-keys", "keys", "chunked", 8105, n_slices=3, groups=2, given=(1,), verify=True)]


CHECKED, REFUSER = 0, 4
# The worker whose object goes and comes is one whose stream HAS entries in the pools: on the product library the plain two-byte K1
# worker (one lane per slice: the renumbering's scratch), on the test build, where k1_path sends K1 through the kernels that keep
# nothing per stream, the key-record worker (K2p: the side stream and its events).
DESTROYER = {"product": 1, "hooks": 5}
ROUNDS = 4


@pytest.mark.parametrize("build", ["product", "hooks"])
def test_batches_side_by_side(avr, hooks, hold, build):                     # noqa: F811
    if build == "hooks":
        hooks(k1_path=2)                                         # in the main thread, before any worker exists
    runs = batch_runs()
    assert len(runs) == T
    wants = []
    for run in runs:
        want = copy.copy(br.expected(run))
        if build == "hooks":
            want.chunked = 1
        wants.append(want)
    rooms = [(len(run.slices), run.total + 64) if t == REFUSER else br.room(run) for t, run in enumerate(runs)]
    # every run alone first, four rounds on one object: what avr_batch_run_info reports single-threaded
    lone = []
    for t, run in enumerate(runs):
        b, infos = avr.Batch(0, *rooms[t]), []
        try:
            for r in range(ROUNDS):
                if r:
                    b.reset()
                br.fill(b, run)
                b.run()
                br.compare(br.collect(b, run), wants[t], "alone, round %d" % r, run)
                infos.append(b.run_info())
        finally:
            b.close()
        lone.append(infos)
    assert all(i["rows_guessed"] > 0 and not i["ran_again"] & 1 for i in lone[CHECKED][1:]), lone[CHECKED]
    assert lone[CHECKED][0]["rows_guessed"] == 0
    made = [avr.Batch(0, *rooms[t]) for t in range(T)]
    crew = threads.Crew(hold)
    destroyer = DESTROYER[build]
    messages, beside = [], []

    def others_inside():
        """Behind the workers' barrier: how many avr_batch_run calls are in flight, once there is one (the others are on their way
        in; the loop gives the interpreter lock away and waits for nothing; it gives up after two seconds and reports none)."""
        until = time.perf_counter() + 2.0
        while crew.blocking.now == 0 and time.perf_counter() < until:
            time.sleep(0)
        return crew.blocking.now

    def work(t, r, crew):
        run = runs[t]
        destroys = r and t == destroyer
        if r and not destroys:
            made[t].reset()
        if not destroys:
            br.fill(made[t], run)
        raised = behind = None
        if t == REFUSER:                                         # a slice beyond capacity
            try:
                made[t].add_slice_range(run.slices[0][:1])
            except avr.AvrError as exc:
                raised = str(exc)
        crew.together.wait()                                     # all six go on at the same moment: five into avr_batch_run ...
        if destroys:
            # ... and this one into avr_batch_destroy (forget_part_streams, forget_stream) and avr_batch_create, while the five are
            # inside avr_batch_run and its launchers' pools; then its own fill and run on the new object
            before = others_inside()
            made[t].close()
            during = crew.blocking.now
            made[t] = avr.Batch(0, *rooms[t])
            beside.append((r, before, during, crew.blocking.now))
            br.fill(made[t], run)
        if t == REFUSER:                                         # its message, read while the others are inside avr_batch_run
            inside = others_inside()
            behind = (made[t]._L.avr_last_error().decode(), min(inside, crew.blocking.now))
        b = made[t]
        with crew.blocking:
            b.run()
        if t == REFUSER:                                         # ... and once more behind its own successful run, which leaves it in place
            messages.append((r, raised, behind, b._L.avr_last_error().decode()))
        return br.collect(b, run), b.run_info()

    try:
        results = crew.run(ROUNDS, work)
    finally:
        for b in made:
            b.close()
    print(f"build {build}: inside-a-round peaks {crew.round_peaks}, avr_batch_run calls at once {crew.blocking.peak}")
    for t, run in enumerate(runs):
        for r in range(ROUNDS):
            got, info = results[t][r]
            what = "worker %d, round %d" % (t, r)
            br.compare(got, wants[t], what, run)
            alone = lone[t][0 if t == destroyer else r]
            assert info == alone, "%s: run %s: avr_batch_run_info %r, alone %r" % (what, run.name, info, alone)
    text = "batch holds max_slices=%d slices" % len(runs[REFUSER].slices)
    assert len(messages) == ROUNDS and all(raised and text in raised and behind[0] == text and last == text
                                           for _, raised, behind, last in messages), (text, messages)
    print(f"avr_batch_run calls in flight (round, at avr_batch_destroy, behind it, behind avr_batch_create): {beside}; "
          f"at the refusing worker's read: {[m[2][1] for m in messages]}")
    assert len(beside) == ROUNDS - 1 and max(b[1] for b in beside) >= 1, f"no avr_batch_destroy began while another worker was inside avr_batch_run: {beside}"
    assert max(m[2][1] for m in messages) >= 1, f"the refusing worker never read its message while another was inside avr_batch_run: {messages}"
    assert crew.blocking.peak >= 2, f"avr_batch_run never overlapped: at most {crew.blocking.peak} calls at once"


# ------------------------------------------------------------------ c. the first use of everything, in a fresh process
# Measured on an MI355X: a child takes 2.8 (batch), 3.1 (k2p), 3.3 (k1p) and 3.9 s (parts) from start to exit -- import torch, load
# the library, the first kernels' code objects; the two rounds themselves 0.2 to 0.4 s.  The limit is ten times the slowest, since
# import and first-load times vary on a shared machine.  A child that runs into it counts as hung.
COLD_MEASURED_S = 3.9
COLD_LIMIT_S = 10 * COLD_MEASURED_S


@pytest.mark.parametrize("first", threads.FIRSTS)
def test_cold_start(first):
    t0 = time.perf_counter()
    child = subprocess.run([sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [threads.__file__, first],
                           capture_output=True, text=True, timeout=COLD_LIMIT_S)
    took = time.perf_counter() - t0
    lines = child.stdout.strip().splitlines()
    assert lines, f"the child wrote nothing; exit status {child.returncode}; {child.stderr[-3000:]}"
    verdict = json.loads(lines[-1])
    print(f"cold start {first}: the child took {took:.1f} s; {verdict}")
    assert child.returncode == 0 and verdict["ok"], f"exit status {child.returncode}: {verdict}; {child.stderr[-3000:]}"
    assert verdict["inside_peaks"] == [T, T], verdict
    if first != "k2p":                                           # (K2p never blocks the calling thread)
        assert verdict["blocking_peak"] >= 2, verdict
