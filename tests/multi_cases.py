"""What tests/test_gpu_multi.py shares: a batch described once as the calls a caller makes, given word for word to a MultiBatch and to
one Batch on device 0 (their methods carry the same names), and everything the equivalence rule names read back from either."""
import numpy as np

import oracle_lib
import range_keys
from cabac_verify_streams import codes_of, narrowed

VERIFY_NONE = 0xFFFFFFFF
SLICE_OK, SLICE_BAD_RECORD, SLICE_VERIFY_FAILED = 0, 3, 4
K1 = ("cabac", "cabac8", "codes")


class Case:
    """kind: 'cabac' | 'cabac8' | 'codes' | 'range' | 'keys'.  slices: the record (code) arrays; states: the initial states of the record
    kinds of K1; groups: [(first slice, start table or None)] for key records; expects: {slice: payload}."""

    def __init__(self, kind, slices, states=None, groups=(), expects=None, verify=False, verify_k1=False):
        self.kind, self.slices, self.states = kind, list(slices), states
        self.groups, self.expects = list(groups), dict(expects or {})
        self.verify, self.verify_k1 = verify, verify_k1

    def __len__(self):
        return len(self.slices)

    @property
    def n_bins(self):
        return [len(s) for s in self.slices]

    @property
    def group_first(self):
        return [f for f, _ in self.groups]

    def share(self, only):
        """The case an entry's sub-batch is given: the slices `only`, the groups that hold one of them, their expectations."""
        index = {i: j for j, i in enumerate(only)}
        bounds = self.group_first + [len(self)]
        groups = [(index[f], t) for g, (f, t) in enumerate(self.groups) if f < bounds[g + 1] and f in index]
        return Case(self.kind, [self.slices[i] for i in only], None if self.states is None else [self.states[i] for i in only], groups,
                    {index[i]: p for i, p in self.expects.items() if i in index}, self.verify, self.verify_k1)


def feed(obj, case):
    """The caller's calls, the same for a Batch and a MultiBatch."""
    groups = {}
    for f, t in case.groups:
        groups.setdefault(f, []).append(t)
    for i in range(len(case) + 1):
        for t in groups.get(i, ()):
            obj.begin_group(t)
        if i == len(case):
            break
        s = case.slices[i]
        if case.kind == "cabac":
            idx = obj.add_slice_cabac(s, case.states[i])
        elif case.kind == "cabac8":
            idx = obj.add_slice_cabac8(s, case.states[i])
        elif case.kind == "codes":
            idx = obj.add_codes(s)
        elif case.kind == "range":
            idx = obj.add_slice_range(s)
        else:
            idx = obj.add_slice_range_keys(s)
        assert idx == i
    for i, payload in sorted(case.expects.items()):
        obj.expect(i, payload)


def settings(obj, case):
    obj.set_verify(case.verify)
    obj.set_verify_k1(case.verify_k1)


def answers(obj, case):
    """([(bytes, status, final states or None, first_bad, first_bad_est, first_diff)] per slice, [table] per group) after a run."""
    with_states = case.kind in ("cabac", "cabac8")
    per_slice = []
    for i in range(len(case)):
        data, status = obj.get(i)
        per_slice.append((data, status, obj.get_states(i) if with_states else None, obj.get_verify(i), obj.get_verify_est(i), obj.get_restore(i)))
    return per_slice, [obj.get_estimators(g) for g in range(len(case.groups))]


def capacity(case):
    return max(len(case), len(case.groups), 1), sum(case.n_bins) + 8           # (a batch holds at most max_slices groups as well)


def run_single(avr, case):
    with avr.Batch(0, *capacity(case)) as b:
        settings(b, case)
        feed(b, case)
        b.run()
        return answers(b, case)


def run_multi(avr, case, entries, how="run"):
    """(answers, owners, loads, [entry_info]) of one MultiBatch run of the case."""
    with avr.MultiBatch(entries, *capacity(case)) as m:
        return run_on(m, case, how)


def run_on(m, case, how="run"):
    settings(m, case)
    feed(m, case)
    if how == "run":
        m.run()
    else:
        m.submit()
        m.wait()
    return answers(m, case), [m.placement(i) for i in range(len(case))], m.load(), [m.entry_info(e) for e in range(len(m.devices))]


def same(got, want, what, skip_groups=()):
    """The multi's answers against the single batch's: every slice, every group's table but the ones with a malformed record."""
    assert len(got[0]) == len(want[0]) and len(got[1]) == len(want[1]), what
    for i, (g, w) in enumerate(zip(got[0], want[0])):
        assert g == w, f"{what}: slice {i}: status {g[1]} / {w[1]}, {len(g[0])} / {len(w[0])} bytes, answers {g[3:]} / {w[3:]}"
    for k, (g, w) in enumerate(zip(got[1], want[1])):
        if k not in skip_groups:
            assert np.array_equal(g, w), f"{what}: the table of group {k}"


def oracle_answers(oracle, case):
    """[(bytes, status, final states or None)] by the oracle; key records through the Python rule (tests/range_keys.py) in front of it,
    a slice the rule calls malformed (and the rest of its group) as (b"", AVR_SLICE_BAD_RECORD).  Tables: the rule's, None where undefined."""
    out, tables = [], []
    if case.kind == "keys":
        bounds = case.group_first + [len(case)]
        for g, (first, table) in enumerate(case.groups):
            recs, after = range_keys.resolve_group(case.slices[first:bounds[g + 1]], table)
            out += [(b"", SLICE_BAD_RECORD, None) if r is None else oracle.range_encode(r) + (None,) for r in recs]
            tables.append(after)
        return out, tables
    for i, s in enumerate(case.slices):
        if case.kind == "range":
            out.append(oracle.range_encode(s) + (None,))
        elif case.kind == "codes":
            out.append(case.codes_truth[i] + (None,))
        else:
            recs = s if case.kind == "cabac" else case.wide[i]
            data, final, status = oracle.cabac_encode(recs, case.states[i])
            out.append((data, status, final))
    return out, tables


def against_oracle(oracle, got, case, what, failed=()):
    want, tables = oracle_answers(oracle, case)
    for i, (g, w) in enumerate(zip(got[0], want)):
        status = SLICE_VERIFY_FAILED if i in failed else w[1]
        assert (g[0], g[1]) == (w[0], status), f"{what}: slice {i} against the oracle"
        if w[2] is not None:
            assert g[2] == w[2], f"{what}: final states of slice {i} against the oracle"
    for k, t in enumerate(tables):
        if t is not None:
            assert np.array_equal(got[1][k], t), f"{what}: the table of group {k} against the rule"


# ------------------------------------------------------------------ the batches

def k1_case(oracle, kind, streams, **kw):
    """streams: [(two-byte records, initial states)] -- given as two-byte records, one-byte records or resolved codes."""
    if kind == "cabac":
        return Case(kind, [r for r, _ in streams], [s for _, s in streams], **kw)
    if kind == "cabac8":
        c = Case(kind, [narrowed(r) for r, _ in streams], [s for _, s in streams], **kw)
        c.wide = [r for r, _ in streams]
        return c
    mlps = oracle.tables()[1]
    c = Case(kind, [codes_of(r, s, mlps) for r, s in streams], **kw)
    c.codes_truth = [oracle.cabac_encode(r, s)[::2] for r, s in streams]     # (bytes, status): the coder from codes codes what the records code
    return c


def mixed_lengths(rng, n):
    """About n slices with lengths lognormal(7.5, 1), plus empty and one-bin slices."""
    lens = [int(x) for x in rng.lognormal(7.5, 1.0, n)]
    for at, v in ((0, 0), (4, 1), (8, 0), (n - 1, 1)):          # (k1_streams ends slice i with a terminate unless i % 4 == 0)
        lens[at] = v
    return lens


def k1_streams(rng, lens, n_ctx=120):
    return [oracle_lib.random_cabac_stream(rng, n, n_ctx, terminate=bool(i % 4)) for i, n in enumerate(lens)]


def seven_groups(rng, malformed=True, hi=3000):
    """Key records in seven groups: 0 fresh (3 slices), 1 from a table (2), 2 fresh with a malformed key in its second slice (3),
    3 without slices, 4 from a table (1), 5 fresh with an empty slice (4), 6 fresh (2).  Slices of 0 to `hi` bins."""
    counts, slices, groups = (3, 2, 3, 0, 1, 4, 2), [], []
    for g, count in enumerate(counts):
        groups.append((len(slices), range_keys.random_table(rng) if g in (1, 4) else None))
        for j in range(count):
            n = 0 if (g, j) == (5, 1) else int(rng.integers(1, hi + 1))
            slices.append(range_keys.random_keys(rng, n, "skew"))
    if malformed:
        bad = slices[groups[2][0] + 1]
        if len(bad) < 8:
            bad = slices[groups[2][0] + 1] = range_keys.random_keys(rng, 100, "skew")
        bad[len(bad) // 2] = (range_keys.N_KEYS + 1) << 1
    return Case("keys", slices, groups=groups)


def local_slice(owners, entries, k):
    """The caller's slices that are local slice k of their entry (entries that hold fewer have none)."""
    out = []
    for e in range(entries):
        mine = [i for i, o in enumerate(owners) if o == e]
        if len(mine) > k:
            out.append(mine[k])
    return out
