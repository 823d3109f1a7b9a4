"""Runs of a reused avr_batch and what each must give, for tests/test_gpu_batch_reuse.py (the library, on the device) and
tests/test_batch_reuse_model.py (tests/cpu_batch.cpp, the CPU stand-in, for the kinds it has).

A Run describes one filling of a batch object: the kind, the shape (which picks the path: avr::want_chunked, csrc/avr_plan.h), n_states,
the checks, how the slices go in (add_* or reserve), a malformed record, a fault hook of the test build.  expected() works out what
such a run must hand back with nothing of the library under test: bytes, statuses and final states from the oracle
(oracle/avr_oracle.c) under the rule of tests/bad_records.py, resolved records and tables from tests/range_keys.py, the restore answer
from tests/restore_ref.py, the verifiers' answers under a fault hook from the oracle's decoders the way tests/cli_verify_faults.py
works them out.  No GPU and no torch in here; the driver (fill / collect / compare) takes any object with avr.Batch's methods."""
import ctypes

import numpy as np

import bad_records
import cabac_verify_streams as cvs
import cli_verify_faults as cvf
import oracle_lib
import range_keys
import restore_ref
import verify_streams

NONE = 0xFFFFFFFF
OK, BAD_RECORD, VERIFY_FAILED = 0, 3, 4
KIND = {"cabac": 0, "range": 1, "codes": 2, "cabac8": 3, "keys": 4}           # AVR_KIND_*
KINDS = ("cabac", "cabac8", "codes", "range", "keys")
K1 = ("cabac", "cabac8", "codes")
PATHS = ("lanes", "chunked")
RUN_TYPES = [(k, p) for k in KINDS for p in PATHS]
EDGE_LENGTHS = (0, 1, 7, 8, 9, 15, 16, 17, 1023, 1024, 1025)
CHUNKED_LENGTHS = {3: (12289, 0, 20001), 4: (12289, 20001, 0, 8192), 5: (30011, 0, 20001, 12289, 24000)}


def want_chunked(lengths):
    """avr::want_chunked, restated: few slices, long on average."""
    n = len(lengths)
    return 0 < n <= 32768 and sum(lengths) // n >= 8192


class Run:
    """slices: what the library is given (uint16 records, one-byte records or codes).  two / states: for the K1 kinds the two-byte
    records and initial states the slices stand for (states: n_states bytes a slice; for codes, the states the codes were resolved
    from).  group_first / tables: key records -- the first slice of each group (a group may hold no slice) and its start table or
    None.  verify: the verifier of the kind's direction (and for key records the estimator checker).  expects: per slice the payload
    it is expected to restore, or None.  hook: the fault point set while the run is in flight, on a build that has fault points."""

    def __init__(self, name, kind, path, slices, n_states=0, two=None, states=None, group_first=None, tables=None, verify=False,
                 expects=None, hook=None, method="add"):
        self.name, self.kind, self.path, self.slices, self.n_states = name, kind, path, slices, n_states
        self.two, self.states, self.group_first, self.tables = two, states, group_first, tables
        self.verify, self.expects, self.hook, self.method = verify, expects, dict(hook or {}), method
        self.lengths = [len(s) for s in slices]
        assert want_chunked(self.lengths) == (path == "chunked"), name
        self._want = {}

    def __repr__(self):
        return self.name

    @property
    def total(self):
        return sum(self.lengths)


class Want:
    """What a run hands back.  None stands for "not specified" (tests/bad_records.py): the final states and the estimator checker's
    answer of a slice with a malformed record, the table of a group with one."""

    def __init__(self, n):
        self.out, self.states = [None] * n, [None] * n
        self.verify, self.verify_est, self.restore = [NONE] * n, [NONE] * n, [NONE] * n
        self.tables, self.chunked = [], 0


# ------------------------------------------------------------------------------------------------ slices
def _k1_slice(rng, n, n_ctx, n_states):
    """n two-byte records over the first n_ctx of n_states contexts (most slices end in put_terminate(1), a slice of one record is
    that alone) and n_states initial states."""
    states = rng.integers(0, 126, n_states).astype(np.uint8)
    if n == 0:
        return np.zeros(0, np.uint16), states
    if n_ctx == 0:                                               # no contexts: bypass bins and put_terminate(0)
        sel = np.where(rng.random(n - 1) < 0.9, 1024, 1025)
        bins = np.where(sel == 1025, 0, rng.integers(0, 2, n - 1))
        recs = np.concatenate([(bins | (sel << 1)), [1 | (1025 << 1)]]).astype(np.uint16)
        return recs, states
    if n > 1 and rng.random() < 0.2:                             # no closing terminate
        recs, st = oracle_lib.random_cabac_stream(rng, n, n_ctx, terminate=False)
    else:
        recs, st = oracle_lib.random_cabac_stream(rng, n - 1, n_ctx, terminate=True)
    states[:n_ctx] = st
    return recs, states


def lane_lengths(rng, n_slices, top=1500):
    """The lengths at which the lane kernels change their step, then random ones; a single slice is a short random one."""
    if n_slices < len(EDGE_LENGTHS):
        return [int(rng.integers(20, top)) for _ in range(n_slices)]
    more = [int(rng.integers(0, top)) for _ in range(n_slices - len(EDGE_LENGTHS))]
    lengths = list(EDGE_LENGTHS) + more
    return [lengths[i] for i in rng.permutation(n_slices)]


def encode_codes(codes):
    """oracle/avr_oracle.c's coder from resolved codes: (bytes, status)."""
    o = oracle_lib.load_oracle()
    codes = np.ascontiguousarray(codes, np.uint8)
    out = np.zeros(2 * codes.size + 64, np.uint8)
    status = ctypes.c_int(0)
    o.L.avr_oracle_cabac_encode_codes.restype = ctypes.c_size_t
    n = o.L.avr_oracle_cabac_encode_codes(oracle_lib.ptr(codes), ctypes.c_size_t(codes.size), oracle_lib.ptr(out), ctypes.c_size_t(out.size),
                                          ctypes.byref(status))
    return (out[:n].tobytes() if status.value == OK else b""), status.value


def make_run(name, kind, path, seed, n_slices=None, n_states=0, n_ctx=None, lengths=None, groups=1, given=(), empty_groups=(),
             verify=False, expect=None, malformed=False, hook=False, method="add"):
    """A seeded run.  lanes: n_slices slices of lane_lengths(); chunked: CHUNKED_LENGTHS[n_slices].  K1 kinds: n_ctx contexts in use of
    n_states (codes: n_states is not given to the library).  Key records: `groups` groups of about equal size, those in `given` with a
    caller's start table, those in `empty_groups` without a slice (0 < g: it begins where the next one does).  expect: None, "right"
    (every slice restores its expectation) or "mixed" (every fifth is wrong: a byte changed, cut short, or a byte too long).
    malformed: one slice holds a record no recorder writes.  hook: the fault point of the kind, at a slice with coded bytes."""
    rng = np.random.default_rng(seed)
    if lengths is None:
        lengths = list(CHUNKED_LENGTHS[n_slices]) if path == "chunked" else lane_lengths(rng, n_slices)
    n = len(lengths)
    n_ctx = n_states if n_ctx is None else n_ctx
    o = oracle_lib.load_oracle()
    two = states = group_first = tables = None
    if kind in K1:
        pairs = [_k1_slice(rng, m, n_ctx, max(n_states, n_ctx)) for m in lengths]
        two, states = [p[0] for p in pairs], [p[1] for p in pairs]
        if kind == "cabac":
            slices = [t.copy() for t in two]
        elif kind == "cabac8":
            slices = [cvs.narrowed(t) for t in two]
        else:
            mlps = o.tables()[1]
            slices = [cvs.codes_of(t, s, mlps) for t, s in zip(two, states)]
    elif kind == "range":
        slices = [oracle_lib.random_range_stream(rng, m, adaptive=False) for m in lengths]
    else:
        slices = [range_keys.random_keys(rng, m, "skew" if i % 3 else "flat") for i, m in enumerate(lengths)]
        real = [g for g in range(groups) if g not in empty_groups]
        cuts = [n * j // len(real) for j in range(len(real))]
        group_first, j = [], 0
        for g in range(groups):
            if g in empty_groups:
                group_first.append(cuts[j] if j < len(cuts) else n)
            else:
                group_first.append(cuts[j])
                j += 1
        tables = [range_keys.random_table(rng) if g in given else None for g in range(groups)]
    long_ones = [i for i in range(n) if lengths[i] >= 40]
    run = Run(name, kind, path, slices, n_states if kind in ("cabac", "cabac8") else 0, two, states, group_first, tables, verify, None, None, method)
    # Resolved codes have no bad value (include/avrecode_ms_amd.h, "Malformed records"): the device's coders from codes trust them, and
    # a bin behind a put_terminate(1) is the caller's mistake, not a status.  A run of codes has no malformed record.
    if malformed and kind != "codes":                            # the last long slice: a group of key records loses few others
        i = long_ones[-1]
        at = lengths[i] // 2
        bad = {"cabac": bad_records.SEL_NOP << 1, "cabac8": bad_records.TERM1_8, "range": 0x0000, "keys": 1027 << 1}[kind]
        run.slices[i] = bad_records.spoil(run.slices[i], at, bad)
        long_ones = long_ones[:-1]
    if expect:
        sound = expected(run).out
        run.expects = []
        for i in range(n):
            data = sound[i][0]
            right = restore_ref.restored(o, data, b"\x55\xaa" if len(data) % 2 else b"\x55\xaa\x33")     # any parity, a last byte
            if restore_ref.first_diff(o, data, right) != NONE:   # (too short for a patch: what the stop byte's removal leaves)
                right = restore_ref.restored(o, data, b"")
            assert restore_ref.first_diff(o, data, right) == NONE, (name, i)
            if expect == "mixed" and i % 5 == 2:
                right = [right[:len(right) // 2] + bytes([right[len(right) // 2] ^ 0x21]) + right[len(right) // 2 + 1:] if right else b"\x01",
                         right[:-1], right + b"\x00"][(i // 5) % 3]
            run.expects.append(right)
        run._want = {}
    if hook:
        k = long_ones[len(long_ones) // 2] + 1
        if kind == "keys":
            run.hook = {"est_flip": k, "est_flip_bin": min(lengths[k - 1] - 1, 7 * k + 1)}
        else:
            run.hook = {"verify_flip" if verify else "restore_flip": k}
    return run


# ------------------------------------------------------------------------------------------------ what a run must give
def _first_bad(o, run, i, data, resolved=None):
    """The verifier's answer for slice i over `data`, by the oracle's decoder of the kind (K2: against the range records the encoder
    read -- for key records the resolved ones)."""
    if run.kind in ("range", "keys"):
        return verify_streams.first_bad(o, data, resolved)
    if run.kind == "codes":
        return cvf.first_bad_codes(o, data, run.slices[i]) if len(run.slices[i]) else NONE
    recs = run.two[i]
    if recs.size == 0:
        return NONE
    bins, final = o.spec_cabac_decode(bytes(data), recs, run.states[i])
    diff = np.nonzero(bins != (recs & 1).astype(np.uint8))[0]
    if diff.size:
        return int(diff[0])
    return NONE if final == o.cabac_encode(recs, run.states[i])[1] else int(recs.size)        # only the final states differ: n_bins


def expected(run, hooked=False):
    """The Want of a run; hooked: on a build with fault points, run.hook set."""
    if hooked in run._want:
        return run._want[hooked]
    o = oracle_lib.load_oracle()
    hook = run.hook if hooked else {}
    n = len(run.slices)
    w = Want(n)
    w.chunked = int(run.path == "chunked")
    resolved = run.slices
    if run.kind == "keys":
        gf = list(run.group_first) + [n]
        resolved, tabs = range_keys.resolve(run.slices, gf, run.tables)
        w.tables = tabs
        k = hook.get("est_flip", 0)
        if run.verify and 0 < k <= n:
            m = hook.get("est_flip_bin", 0)
            assert resolved[k - 1] is not None and m < len(resolved[k - 1])
            resolved[k - 1] = resolved[k - 1].copy()
            resolved[k - 1][m] += 0x100
            w.verify_est[k - 1] = m
    for i in range(n):
        if run.kind in ("range", "keys"):
            st, data, final = (BAD_RECORD, b"", None) if resolved[i] is None else bad_records.expected(bad_records.KIND_RANGE, resolved[i])
        elif run.kind == "cabac":
            st, data, final = bad_records.expected(bad_records.KIND_CABAC, run.slices[i], run.states[i][:run.n_states])
        elif run.kind == "cabac8":
            st, data, final = bad_records.expected(bad_records.KIND_CABAC8, run.slices[i], run.states[i][:run.n_states])
        else:
            data, st = encode_codes(run.slices[i])
            final = b""
        assert data is not None and st in (OK, BAD_RECORD), (run.name, i, st)
        w.out[i], w.states[i] = [data, st], final
        if st == BAD_RECORD:
            w.verify_est[i] = None
    if run.kind == "keys":
        k = hook.get("est_flip", 0)
        if k and w.verify_est[k - 1] not in (None, NONE):
            w.out[k - 1][1] = VERIFY_FAILED
    def flip(i):                                                 # bit 7 of byte 0 of the slice's coded bytes, as the fault points do
        assert w.out[i][1] in (OK, VERIFY_FAILED) and len(w.out[i][0]) >= 3, (run.name, i)
        w.out[i][0] = bytes([w.out[i][0][0] ^ 0x80]) + w.out[i][0][1:]
    k = hook.get("verify_flip", 0) if run.verify else 0
    if 0 < k <= n:
        flip(k - 1)
        w.verify[k - 1] = _first_bad(o, run, k - 1, w.out[k - 1][0], resolved[k - 1])
        assert w.verify[k - 1] != NONE, "the flipped byte of slice %d of %s is not found by the oracle's decoder" % (k - 1, run.name)
        w.out[k - 1][1] = VERIFY_FAILED
    k = hook.get("restore_flip", 0) if run.expects else 0        # the restore check runs behind the verifier, over what it left
    if 0 < k <= n:
        flip(k - 1)
    if run.expects:
        for i in range(n):
            if run.expects[i] is None or w.out[i][1] not in (OK, VERIFY_FAILED):
                continue
            w.restore[i] = restore_ref.first_diff(o, w.out[i][0], run.expects[i])
            if w.restore[i] != NONE:
                w.out[i][1] = VERIFY_FAILED
    w.out = [tuple(x) for x in w.out]
    run._want[hooked] = w
    return w


# ------------------------------------------------------------------------------------------------ the driver
def fill(b, run, settings=True, method=None):
    """The run's slices, groups and expectations into an open batch; settings: the two verify switches as the run wants them."""
    if settings:
        b.set_verify(bool(run.verify and run.kind not in K1))
        b.set_verify_k1(bool(run.verify and run.kind in K1))
    method = method or run.method
    groups = {}
    for g, f in enumerate(run.group_first or []):
        groups.setdefault(f, []).append(g)
    for i, s in enumerate(run.slices):
        for g in groups.get(i, []):
            assert b.begin_group(run.tables[g]) == g
        st = run.states[i][:run.n_states] if run.kind in ("cabac", "cabac8") else None
        if method == "reserve" and hasattr(b, "reserve"):        # (the stand-in has no zero-copy add)
            idx, view = b.reserve(KIND[run.kind], len(s), st)
            view[:] = s
        elif run.kind == "cabac":
            idx = b.add_slice_cabac(s, st)
        elif run.kind == "cabac8":
            idx = b.add_slice_cabac8(s, st)
        elif run.kind == "codes":
            idx = b.add_codes(s)
        elif run.kind == "range":
            idx = b.add_slice_range(s)
        else:
            idx = b.add_slice_range_keys(s)
        assert idx == i
        if run.expects and run.expects[i] is not None:
            b.expect(i, run.expects[i])
    for g in groups.get(len(run.slices), []):                    # trailing groups without a slice
        assert b.begin_group(run.tables[g]) == g


class Got:
    pass


def collect(b, run):
    """Everything the getters give for a run, in Want's form (tables: every group's)."""
    n = len(run.slices)
    g = Got()
    g.out = [b.get(i) for i in range(n)]
    g.states = [b.get_states(i) if run.kind in ("cabac", "cabac8") else b"" for i in range(n)]
    g.verify = [b.get_verify(i) for i in range(n)]
    g.verify_est = [b.get_verify_est(i) for i in range(n)]
    g.restore = [b.get_restore(i) for i in range(n)]
    g.tables = [np.asarray(b.get_estimators(j), np.uint8).reshape(-1, 2) for j in range(len(run.group_first or []))]
    g.chunked = b.run_info()["chunked"] if hasattr(b, "run_info") else None
    g.ms = (b.verify_ms(), b.verify_est_ms(), b.restore_ms())
    return g


def compare(got, want, label, run):
    """got against a Want (None: not specified) or against another Got (a fresh object's: everything the contract defines)."""
    where = "%s: run %s" % (label, run.name)
    if got.chunked is not None and want.chunked is not None:
        assert got.chunked == want.chunked, "%s: chunked %r, meant %r" % (where, got.chunked, want.chunked)
    n, firsts = len(run.slices), list(run.group_first or [])
    ends = firsts[1:] + [n]                                      # a group with a malformed key: its table is not specified
    undefined_groups = {j for j in range(len(firsts)) if any(tuple(want.out[i])[1] == BAD_RECORD for i in range(firsts[j], ends[j]))}
    for i in range(len(run.slices)):
        at = "%s, slice %d of %d (%d bins)" % (where, i, len(run.slices), run.lengths[i])
        w_out = tuple(want.out[i])
        assert got.out[i][1] == w_out[1], "%s: status %d, expected %d" % (at, got.out[i][1], w_out[1])
        assert got.out[i][0] == w_out[0], "%s: %d coded bytes differ from the %d expected" % (at, len(got.out[i][0]), len(w_out[0]))
        # a slice with a malformed record: its final states and the estimator checker's answer are not specified; no decoder and no
        # restore check runs on it, so those two answer VERIFY_NONE whatever an earlier run left in their arrays
        if want.states[i] is not None and w_out[1] != BAD_RECORD:
            assert got.states[i] == want.states[i], "%s: final states differ" % at
        assert got.verify[i] == want.verify[i], "%s: get_verify %#x, expected %#x" % (at, got.verify[i], want.verify[i])
        if want.verify_est[i] is not None and w_out[1] != BAD_RECORD:
            assert got.verify_est[i] == want.verify_est[i], "%s: get_verify_est %#x, expected %#x" % (at, got.verify_est[i], want.verify_est[i])
        assert got.restore[i] == want.restore[i], "%s: get_restore %#x, expected %#x" % (at, got.restore[i], want.restore[i])
    for j, t in enumerate(want.tables):
        if t is None or j in undefined_groups:
            continue
        assert np.array_equal(got.tables[j], np.asarray(t, np.uint8).reshape(-1, 2)), "%s: the table of group %d differs" % (where, j)


def check_times(got, run, where):
    """A check that did not run took 0.0 ms; one that ran took more."""
    on = (bool(run.verify), bool(run.verify and run.kind == "keys"), bool(run.expects))
    for name, ms, ran in zip(("verify_ms", "verify_est_ms", "restore_ms"), got.ms, on):
        assert (ms > 0.0) == ran, "%s: run %s: %s = %r with the check %s" % (where, run.name, name, ms, "on" if ran else "off")


def set_hooks(setter, run=None):
    """The fault points of `run` (none: all off) through setter(name, value) -- avr_test_hook_set of either build with fault points."""
    setter("reset", 0)
    for name, value in (run.hook if run is not None else {}).items():
        setter(name, value)


def run_and_check(b, run, label, hooked=False, fresh=None, again=True):
    """b holds the run's slices: run it, hold it to expected() and to `fresh` (a fresh object's Got), then once more as it is."""
    want = expected(run, hooked)
    got = None
    for turn in ("", " (submitted again)") if again else ("",):
        b.submit()
        b.wait()
        got = collect(b, run)
        compare(got, want, label + turn, run)
        check_times(got, run, label + turn)
        if fresh is not None:
            compare(got, fresh, label + turn + " against a fresh object", run)
    return got


# ------------------------------------------------------------------------------------------------ the ten run types, dirty and small
_cache = {}


def run_type(kind, path, size):
    """size "A": the dirty run -- 130 slices (5 chunked), the most contexts, its kind's verifier on, K1: an expectation a slice, some
    wrong; key records: five groups, three with start tables; a malformed record; the kind's fault hook.  size "B": the small run
    behind it -- 60 to 65 slices (3 or 4 chunked), few contexts, checks off except where noted below."""
    key = (kind, path, size)
    if key in _cache:
        return _cache[key]
    t = RUN_TYPES.index((kind, path))
    name = "%s-%s-%s" % (size, kind, path)
    if size == "A":
        ns, nc = {"cabac": (460, 300), "cabac8": (126, 120), "codes": (200, 200)}.get(kind, (0, 0))
        run = make_run(name, kind, path, 7100 + t, n_slices=130 if path == "lanes" else 5, n_states=ns, n_ctx=nc, groups=5, given=(0, 2, 3),
                       verify=True, expect="mixed" if kind in K1 else None, malformed=True, hook=True, method="reserve" if t % 2 else "add")
    else:
        ns, nc = {"cabac": (40, 30), "cabac8": (20, 15), "codes": (30, 30)}.get(kind, (0, 0))
        n_slices = (60, 63, 64, 65, 61)[KINDS.index(kind)] if path == "lanes" else (3, 4, 3, 4, 3)[KINDS.index(kind)]
        # B's rows with a check on: codes-lanes restores right expectations, keys-chunked is verified (a start table given), range-lanes too
        run = make_run(name, kind, path, 7200 + t, n_slices=n_slices, n_states=ns, n_ctx=nc, groups=2, given=(1,) if path == "chunked" else (),
                       verify=(kind, path) in (("keys", "chunked"), ("range", "lanes")), expect="right" if (kind, path) == ("codes", "lanes") else None,
                       method="add" if t % 2 else "reserve")
    _cache[key] = run
    return run


# ------------------------------------------------------------------------------------------------ the sequences
# new_batch(max_slices, max_bins) -> an object with avr.Batch's methods; setter: avr_test_hook_set of a build with fault points, or
# None on the product library (no fault is forced there: only the restore check can have a finding).
def refused(call, *args):
    try:
        call(*args)
    except RuntimeError:
        return True
    return False


def fresh(new_batch, run):
    """The run on an object that has seen nothing else, no fault point set."""
    b = new_batch(len(run.slices) + 1, run.total + 8)
    try:
        fill(b, run)
        b.run()
        return collect(b, run)
    finally:
        b.close()


def room(*runs):
    return max(len(r.slices) for r in runs) + 8, max(r.total for r in runs) + 64


def dirty(b, setter, A):
    """The dirty run, held to its expectation too: what it leaves behind is what was meant."""
    if setter:
        set_hooks(setter, A)
    fill(b, A)
    run_and_check(b, A, "the dirty run", hooked=setter is not None, again=False)
    if setter:
        set_hooks(setter, None)


def seq_pair(new_batch, setter, A, B, fresh_B):
    """(a): A, reset, B, B again as it is."""
    b = new_batch(*room(A, B))
    try:
        dirty(b, setter, A)
        b.reset()
        fill(b, B)
        run_and_check(b, B, "after run %s and reset" % A.name, fresh=fresh_B)
    finally:
        b.close()
        if setter:
            set_hooks(setter, None)


def seq_runs(new_batch, runs, label):
    """(b): the runs one after the other on one object, each held to its expectation and run again as it is."""
    b = new_batch(*room(*runs))
    try:
        before = "nothing"
        for r in runs:
            b.reset()
            fill(b, r)
            run_and_check(b, r, "%s: after run %s" % (label, before))
            before = r.name
    finally:
        b.close()


# The verify switch of consecutive runs is the same in both states (on, on; off, off; ...): seq_checks() sets it only where it changes, so
# that the runs in between show it surviving reset().  The other switch of a family changes with every run.
CHECK_PATTERNS = ((1, 1), (1, 0), (0, 0), (0, 1), (1, 1), (1, 0), (0, 1), (0, 0))
CHECK_SLICES, CHECK_AT = 62, 14                                  # every run of (c): this many slices, the forced finding in slice CHECK_AT - 1


def check_runs(family, kinds):
    """(c): eight runs over every on/off pattern of the family's two switches -- K1: (set_verify_k1, expectations), K2: (set_verify, key
    records) -- each with a finding forced in every check it has; then the family's fullest run with every finding forced in slice
    CHECK_AT - 1, and right behind it the same kind of run without any fault."""
    key = (family, tuple(kinds))
    if key in _cache:
        return _cache[key]
    rng = np.random.default_rng(7300)
    runs = []
    for j, (first, second) in enumerate(CHECK_PATTERNS + ((1, 1), (1, 1))):
        fault = j <= len(CHECK_PATTERNS)
        lengths = lane_lengths(rng, CHECK_SLICES, 700)
        lengths[CHECK_AT - 1] = 300 + j
        if family == "k1":
            kind = kinds[j % len(kinds)] if fault else runs[-1].kind
            ns = {"cabac": (12, 9, 300, 8, 0, 40, 9, 8, 20, 11)[j], "cabac8": (30, 5, 126, 0, 17, 64, 8, 9, 20, 11)[j], "codes": 50}[kind]
            r = make_run("c%d-%s-%s%s" % (j, kind, "verify" if first else "plain", "-expect" if second else ""), kind, "lanes", 7310 + j,
                         n_states=ns, lengths=lengths, verify=bool(first), expect=("mixed" if fault else "right") if second else None)
            if fault and (first or second):
                r.hook = {"verify_flip" if first else "restore_flip": CHECK_AT}
        else:
            kind = "keys" if second else "range"
            r = make_run("c%d-%s-%s" % (j, kind, "verify" if first else "plain"), kind, "lanes", 7330 + j, lengths=lengths,
                         groups=3, given=(1,) if j % 2 else (), verify=bool(first))
            if fault and first:
                r.hook = {"verify_flip": CHECK_AT} if kind == "range" else {"est_flip": CHECK_AT, "est_flip_bin": 40 + j}
                if kind == "keys" and j in (4, 8):
                    r.hook["verify_flip"] = CHECK_AT             # both faults in one slice: the decoder reads the altered records
        r._want = {}
        runs.append(r)
    _cache[key] = runs
    return runs


def seq_checks(new_batch, setter, runs):
    """(c) on one object.  A run whose switches are the previous run's does not set them again: only reset() lies between, and the run's
    forced verifier finding (switch on) or its VERIFY_NONE and 0.0 ms everywhere (switch off) show that the setting survived it."""
    b = new_batch(*room(*runs))
    try:
        before, settings, survived = None, None, set()
        for r in runs:
            now = (bool(r.verify and r.kind not in K1), bool(r.verify and r.kind in K1))
            set_hooks(setter, r)
            b.reset()
            fill(b, r, settings=now != settings)
            if now == settings:
                survived.add(bool(r.verify))
            settings = now
            label = "after run %s" % (before.name if before else "nothing")
            got = run_and_check(b, r, label, hooked=True, again=False)
            for name, on, answers in (("verifier", r.verify, got.verify), ("estimator checker", r.verify and r.kind == "keys", got.verify_est),
                                      ("restore check", r.expects, got.restore)):
                if not on:                                       # ... and check_times() has seen its 0.0 ms
                    assert answers == [NONE] * len(r.slices), "%s: run %s has no %s and reports %r" % (label, r.name, name, [a for a in answers if a != NONE])
            if not (r.verify or r.expects):
                assert all(st != VERIFY_FAILED for _, st in got.out), "%s: run %s has no check and a slice failed one" % (label, r.name)
            if r.hook:
                assert got.out[CHECK_AT - 1][1] == VERIFY_FAILED, "%s: run %s: the forced finding is missing" % (label, r.name)
            before = r
        assert survived == {True, False}, "the sequence must leave the verify switch alone across a reset in both of its states"
        last = runs[-1]                                          # checks on, no fault, behind a reset behind findings of every check in slice CHECK_AT - 1
        assert not last.hook and all(st == OK for _, st in got.out) and before is last
        found = expected(runs[-2], True)
        assert runs[-2].hook and (found.verify[CHECK_AT - 1] != NONE) and (found.verify_est[CHECK_AT - 1] != NONE or last.kind != "keys") \
            and (found.restore[CHECK_AT - 1] != NONE or not last.expects), "the run before the last must find something in every check"
        hooked_last = Run(last.name + "-faulted", last.kind, last.path, last.slices, last.n_states, last.two, last.states, last.group_first, last.tables,
                          last.verify, last.expects, runs[-2].hook, last.method)
        for r in (hooked_last, last):                            # the same slices submitted again: with the fault, then without
            set_hooks(setter, r)
            run_and_check(b, r, "submitted again after run %s" % before.name, hooked=True, again=False)
            before = r
    finally:
        b.close()
        set_hooks(setter, None)


def seq_empty(new_batch, setter, A, B, fresh_B):
    """(d): a run without a slice behind a dirty one reports nothing of it, and the run behind it is a fresh object's."""
    b = new_batch(*room(A, B))
    try:
        dirty(b, setter, A)
        b.reset()
        b.run()
        where = "the empty run after run %s" % A.name
        assert refused(b.get, 0), "%s: get(0) is not refused" % where
        if hasattr(b, "run_info"):
            assert b.run_info() == {"chunked": 0, "rows_guessed": 0, "contexts_seen": 0, "ran_again": 0}, "%s: run_info() = %r" % (where, b.run_info())
            assert list(b.timings().values()) == [0.0] * 4, "%s: timings() = %r" % (where, b.timings())
        ms = (b.verify_ms(), b.verify_est_ms(), b.restore_ms())
        assert ms == (0.0, 0.0, 0.0), "%s: verify_ms, verify_est_ms, restore_ms = %r" % (where, ms)
        b.reset()
        fill(b, B)
        run_and_check(b, B, "after run %s and an empty run" % A.name, fresh=fresh_B)
    finally:
        b.close()
        if setter:
            set_hooks(setter, None)


def seq_refused(new_batch, run, fresh_run):
    """(d): a submit refused for the other direction's verify switch leaves a sound object."""
    b = new_batch(*room(run))
    wrong, right = (b.set_verify, b.set_verify_k1) if run.kind in K1 else (b.set_verify_k1, b.set_verify)
    try:
        wrong(True)
        right(bool(run.verify))
        fill(b, run, settings=False)
        assert refused(b.submit), "run %s: submit with the other direction's verify switch on is not refused" % run.name
        assert refused(b.get, 0), "run %s: get(0) behind a refused submit is not refused" % run.name
        wrong(False)
        run_and_check(b, run, "after a refused submit", fresh=fresh_run)
    finally:
        b.close()


def seq_capacity(new_batch, run):
    """(d): a batch filled to exactly max_slices slices and max_bins bins refuses one more slice and one more bin, and the refused add
    leaves no trace."""
    n, total = len(run.slices), run.total
    extra = run.slices[next(i for i in range(n) if run.lengths[i])][:1]
    st = run.states[0][:run.n_states] if run.kind in ("cabac", "cabac8") else None
    add = {"cabac": lambda b, s: b.add_slice_cabac(s, st), "cabac8": lambda b, s: b.add_slice_cabac8(s, st), "codes": lambda b, s: b.add_codes(s),
           "range": lambda b, s: b.add_slice_range(s), "keys": lambda b, s: b.add_slice_range_keys(s)}[run.kind]
    for slices_room, what in ((0, "one more slice"), (1, "one more bin")):
        b = new_batch(n + slices_room, total)
        try:
            fill(b, run)
            assert refused(add, b, extra if slices_room else extra[:0]), "run %s: %s than the batch was made for is not refused" % (run.name, what)
            if slices_room and hasattr(b, "reserve"):
                assert refused(b.reserve, KIND[run.kind], 1, st), "run %s: one more bin through reserve is not refused" % run.name
            if run.expects:                                      # (an expectation behind the refused add belongs to no slice)
                assert refused(b.expect, n, b"\x01\x02")
            run_and_check(b, run, "filled to the brim, %s refused" % what)
        finally:
            b.close()
