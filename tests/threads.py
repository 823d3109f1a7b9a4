"""Host threads that call the library side by side, each on a stream of its own: the crew of tests/test_gpu_threads.py, and -- as a
program -- the child process of its cold start.

The header's contract (include/avrecode_ms_amd.h, Threading and ONE THREAD PER STREAM): one avr_batch per host thread, one host thread
per stream.  Crew runs T workers through rounds.  Each worker enters a torch stream of its own inside its thread (the current stream
is thread-local, and DeviceWorkload takes it from there), and every round is: a barrier, a sleep kernel on the worker's stream, the
worker's calls behind it, that stream synchronised.  That the workers were inside a round together is counted, not hoped for: a
counter under a lock, whose peak the tests hold to T for every round; a second counter goes around the calls that block (the K1
calls that ask the device for the context count, avr_batch_run).  A worker that fails stores its exception, sets the stop flag and
breaks the barriers; nobody starts anything on the GPU after that, and the main thread raises the first exception stored.

As a program (python tests/threads.py <first>): a fresh process, in which everything the library makes on first use -- the stream
pools, K1p's constant table and the event the other streams wait for, the kernels' attributes, the environment switches -- is made
by six threads at the same moment.  It initialises torch, builds its inputs with torch and numpy alone, loads the library and makes
no avr_* call; then the six workers pass a barrier and make the process's first library calls together, for two rounds, held to the
oracle.  One JSON line with the verdict and the overlap peaks; exit status 1 on any difference."""
import json
import os
import sys
import threading
import time

import numpy as np

T = 6                                                            # fewer than the CPUs a command gets, more than the hardware queues a process opens
HOLD_MS = 30
BARRIER_S = 120.0
FIRSTS = ("k1p", "k2p", "parts", "batch")


class Counter:
    """How many threads are inside at once, and the most there were since reset()."""

    def __init__(self):
        self.lock, self.now, self.peak = threading.Lock(), 0, 0

    def reset(self):
        with self.lock:
            self.peak = self.now

    def __enter__(self):
        with self.lock:
            self.now += 1
            self.peak = max(self.peak, self.now)

    def __exit__(self, *exc):
        with self.lock:
            self.now -= 1


def make_hold():
    """hold(ms): a sleep kernel of about that long on the current stream (as the fixture of tests/test_gpu_workspace.py)."""
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


def contexts_in_use(slices, n_states):
    """numpy's count of the distinct selectors below n_states in [(records, states)]: the rows a census that misses nothing reports."""
    sel = np.unique(np.concatenate([r.astype(np.uint16) >> 1 for r, _ in slices] + [np.zeros(0, np.uint16)]))
    return int((sel < n_states).sum())


class Crew:
    """T workers with a stream each.  run(n_rounds, work, between): `between(r)` in the main thread before round r (every worker is
    behind its stream's synchronise then), work(t, r, crew) in worker t inside its stream; returns results[t][r]."""

    def __init__(self, hold, n=T):
        import torch
        self.n, self.hold = n, hold
        self.streams = [torch.cuda.Stream() for _ in range(n)]
        handles = [s.cuda_stream for s in self.streams]
        # torch hands streams out of a pool: two workers on one handle would break the header's contract in the test itself
        assert len(set(handles)) == n and 0 not in handles, "the workers' streams are not pairwise different: %r" % (handles,)
        self.inside, self.blocking = Counter(), Counter()
        self.round_peaks, self.errors = [], []
        self.stop = threading.Event()
        self.start = threading.Barrier(n + 1, timeout=BARRIER_S)
        self.done = threading.Barrier(n + 1, timeout=BARRIER_S)
        self.together = threading.Barrier(n, timeout=BARRIER_S)  # the workers alone: right in front of a call all of them make

    def _fail(self, t, exc):
        self.errors.append((t, exc))
        self.stop.set()
        for b in (self.start, self.done, self.together):
            b.abort()

    def _worker(self, t, n_rounds, work, results):
        import torch
        try:
            with torch.cuda.stream(self.streams[t]):
                assert torch.cuda.current_stream().cuda_stream == self.streams[t].cuda_stream
                for r in range(n_rounds):
                    self.start.wait()
                    if self.stop.is_set():
                        return
                    with self.inside:
                        self.hold(HOLD_MS)
                        results[t][r] = work(t, r, self)
                        self.streams[t].synchronize()
                    self.done.wait()
        except BaseException as exc:                             # (a broken barrier included: the first one stored is the cause)
            self._fail(t, exc)

    def run(self, n_rounds, work, between=None):
        results = [[None] * n_rounds for _ in range(self.n)]
        threads = [threading.Thread(target=self._worker, args=(t, n_rounds, work, results), name="worker-%d" % t) for t in range(self.n)]
        for th in threads:
            th.start()
        try:
            for r in range(n_rounds):
                if between is not None:
                    between(r)
                self.inside.reset()
                self.start.wait()
                self.done.wait()
                self.round_peaks.append(self.inside.peak)
        except BaseException as exc:
            self._fail("main", exc)
        for th in threads:
            th.join(2 * BARRIER_S)
        assert not any(th.is_alive() for th in threads), "a worker did not come back"
        if self.errors:
            who, exc = self.errors[0]
            raise AssertionError("worker %s failed first (%d failures in all): %r" % (who, len(self.errors), exc)) from exc
        assert self.round_peaks == [self.n] * n_rounds, "workers inside each round at once: %r, meant %d every round" % (self.round_peaks, self.n)
        return results


# ------------------------------------------------------------------ a DeviceWorkload made without a call into the library
def raw_workload(avr, kind, slices):
    """DeviceWorkload.from_host() without its packer call: the slice-major records, the counts and the states uploaded by torch; no
    tiles (the intra-slice parallel paths read none).  The status starts at zero: those paths find a malformed record themselves."""
    import torch
    from avrecode_ms_amd.device import DeviceWorkload, plan_tiles
    cabac = kind == avr.KIND_CABAC
    recs = [s[0] for s in slices] if cabac else list(slices)
    dev = torch.device("cuda", 0)
    nb = np.array([len(r) for r in recs], dtype=np.int32)
    rec_off = np.zeros(len(recs) + 1, dtype=np.int64)
    rec_off[1:] = np.cumsum((nb.astype(np.int64) + 7) // 8 * 8)
    flat = np.full(int(rec_off[-1]) + 8, avr.NOP_CABAC if cabac else avr.NOP_RANGE, dtype=np.uint16)
    for i, r in enumerate(recs):
        flat[rec_off[i]:rec_off[i] + len(r)] = r
    n_bins = torch.from_numpy(nb).to(dev)
    order, tile_off = plan_tiles(n_bins)
    init = torch.from_numpy(np.concatenate([np.asarray(s[1], np.uint8) for s in slices])).to(dev) if cabac else None
    w = DeviceWorkload(kind, 0, n_bins, order, tile_off, torch.zeros(16, dtype=torch.uint8, device=dev), init, len(slices[0][1]) if cabac else 0)
    w.rec_flat, w.rec_off = torch.from_numpy(flat.view(np.int16)).to(dev), torch.from_numpy(rec_off).to(dev)
    return w


# ------------------------------------------------------------------ the cold start
def cold_start(first):
    import torch
    torch.cuda.init()
    import avrecode_ms_amd as avr
    import batch_reuse as br
    import test_gpu_workspace as ws
    hold = make_hold()
    crew = Crew(hold)
    poison = 0x5A
    if first == "batch":
        kinds = [("cabac", "lanes", 100), ("keys", "chunked", 0), ("cabac8", "lanes", 60), ("range", "chunked", 0), ("cabac", "chunked", 40), ("codes", "lanes", 50)]
        runs = [br.make_run("cold-%d-%s-%s" % (t, k, p), k, p, 9100 + t, n_slices=40 if p == "lanes" else 3, n_states=ns, groups=2, verify=k == "keys")
                for t, (k, p, ns) in enumerate(kinds)]
        wants = [br.expected(r) for r in runs]
        made = [None] * T
    else:
        if first == "k2p":
            batches = [ws.range_batch(9200 + t) for t in range(T)]
            loads = [raw_workload(avr, avr.KIND_RANGE, b[0]) for b in batches]
        else:
            batches = [ws.cabac_batch(9300 + t, 86) for t in range(T)]
            loads = [raw_workload(avr, avr.KIND_CABAC, b[0]) for b in batches]
        offs = [w.out_off.cpu().numpy() for w in loads]
    avr.lib()                                                    # loaded and bound; nothing called

    def between(r):
        """In the main thread, before every round: the outputs poisoned anew (a second call that coded nothing must not pass on
        the first one's bytes), the statuses cleared."""
        if first != "batch":
            for w in loads:
                w.out.fill_(poison)
                w.out_len.fill_(poison)
                w.status.zero_()
                if w.final_states is not None:
                    w.final_states.fill_(poison)
        torch.cuda.synchronize()

    def work(t, r, crew):
        if first == "batch":
            run = runs[t]
            if r == 0:
                made[t] = avr.Batch(0, *br.room(run))
            else:
                made[t].reset()
            br.fill(made[t], run)
            crew.together.wait()
            with crew.blocking:
                made[t].run()
            return br.collect(made[t], run)
        w = loads[t]
        if first == "parts" and r == 0:
            assert w.set_parts(3) == 3
        if w.kind == avr.KIND_CABAC and not w.rows_hint:
            with crew.blocking:                                  # no guess yet: the call asks the device and waits
                w.encode_chunked()
        else:
            w.encode_chunked()
        crew.streams[t].synchronize()
        left = []                                                # the slices left for a second pass, as the device reported them
        if w.kind == avr.KIND_CABAC:
            left = [int(w._part_counts[2 * i + 1]) for i in range(w.n_parts)] if first == "parts" else [int(w._counts[1])]
        info = w.settle(crew.streams[t])
        return ws.snapshot(w), dict(info, left=left)

    t0 = time.perf_counter()
    try:
        results = crew.run(2, work, between)
    finally:
        torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    for t in range(T):
        for r in range(2):
            what = "cold start %s: worker %d, round %d" % (first, t, r)
            if first == "batch":
                br.compare(results[t][r], wants[t], what, runs[t])
                continue
            snap, info = results[t][r]
            ws.compare(snap, offs[t], batches[t][1], what, poison)
            if loads[t].kind == avr.KIND_CABAC:
                # The path, as far as a process without a lone run can hold it: no slice left for a second pass, nothing run again --
                # so the census missed no context, and the rows it reports are the contexts numpy counts in the batch (in parts: in
                # the part that uses the most) -- in both rounds, the second sized by the first one's count.
                w, slices = loads[t], batches[t][0]
                parts = w._parts if first == "parts" else [{"first": 0, "n": w.n_slices}]
                rows = max(contexts_in_use(slices[q["first"]:q["first"] + q["n"]], w.n_states) for q in parts)
                assert info["left"] == [0] * len(parts) and not info["redone"], (what, info)
                assert info["rows"] == rows and info["hint"] == (min(w.n_states, rows + 8) if r else 0), (what, info, rows)
    if first == "batch":
        for b in made:
            b.close()
    return {"first": first, "inside_peaks": crew.round_peaks, "blocking_peak": crew.blocking.peak, "rounds_s": round(seconds, 3)}


def main(argv):
    if len(argv) != 2 or argv[1] not in FIRSTS:
        print("usage: threads.py " + "|".join(FIRSTS), file=sys.stderr)
        return 2
    here = os.path.dirname(os.path.abspath(__file__))
    for p in (os.path.dirname(here), here):
        if p not in sys.path:
            sys.path.insert(0, p)
    t0 = time.perf_counter()
    try:
        verdict = dict(cold_start(argv[1]), ok=True)
    except BaseException as exc:
        verdict = {"first": argv[1], "ok": False, "error": repr(exc)[:2000]}
    verdict["seconds"] = round(time.perf_counter() - t0, 3)
    print(json.dumps(verdict), flush=True)
    return 0 if verdict["ok"] else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv))
