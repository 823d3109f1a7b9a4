"""A reused avr_batch (csrc/avr_api.cpp): every kind, path and check after any other.

avr_batch_reset keeps every pinned and device buffer and clears a hand-kept list of fields; `recode test <dir>` takes a whole directory
through two such objects.  The property throughout: a run on a reused object gives exactly what tests/batch_reuse.py expects of it --
the oracle's bytes, statuses and final states, the resolved tables, the checks' answers -- and exactly what the same slices give on a
fresh object.  The runs, the expectations and the sequences are tests/batch_reuse.py's (held to the CPU stand-in by
tests/test_batch_reuse_model.py); this module runs them on the product library and, where a verifier's finding has to be forced, on
the test build with its fault points."""
import numpy as np
import pytest

import batch_reuse as br

pytestmark = pytest.mark.gpu

IDS = lambda t: "%s-%s" % t
_fresh = {}


@pytest.fixture
def device(avr, hooks):
    """device(build) -> (new_batch, setter): "product" -- the library as shipped, no fault points (setter None); "hooks" -- the test
    build, its fault points set through avr_test_hook_set."""
    made = []

    def choose(build):
        setter = None
        if build == "hooks":
            hooks()

            def setter(name, value):
                assert avr.lib().avr_test_hook_set(name.encode(), int(value)) == 0, avr.lib().avr_last_error()

        def new_batch(max_slices, max_bins):
            assert len([b for b in made if b._h]) < 3, "no more than three objects alive at once"
            made.append(avr.Batch(0, max_slices, max_bins))
            return made[-1]

        def fresh_of(run):
            if (build, run.name) not in _fresh:
                _fresh[build, run.name] = br.fresh(new_batch, run)
            return _fresh[build, run.name]
        return new_batch, setter, fresh_of
    yield choose
    for b in made:
        b.close()


# ------------------------------------------------------------------ a. every ordered pair
@pytest.mark.parametrize("b_type", br.RUN_TYPES, ids=lambda t: "B-%s-%s" % t)
@pytest.mark.parametrize("a_type", br.RUN_TYPES, ids=lambda t: "A-%s-%s" % t)
@pytest.mark.parametrize("build", ("product", "hooks"))
def test_every_ordered_pair(device, build, a_type, b_type):
    """A, the dirty run (larger in slices -- where the paths allow --, bins, contexts and n_states; its verifier on; K1: an expectation a
    slice, some wrong; key records: five groups, three start tables; a malformed record; on the test build the fault hook of its kind),
    reset(), then B, and B again as it is.  On the product library only A's restore check has findings."""
    new_batch, setter, fresh_of = device(build)
    A, B = br.run_type(*a_type, "A"), br.run_type(*b_type, "B")
    br.seq_pair(new_batch, setter, A, B, fresh_of(B))


# ------------------------------------------------------------------ b. shrink after grow, same kind
def shrink_runs(kind):
    """130 -> 1 -> 64 -> 65 -> 63 slices, then chunked and lanes again; n_states 460 -> 4 -> 0 -> 126 -> 9 -> 8 (two-byte records: the
    renumbering starts above 8) and 126 -> 5 -> 0 (one-byte records); key records: 5 -> 1 -> 3 groups, start tables given -> none ->
    given, then a group of empty slices only and a trailing group without a slice, both with start tables."""
    counts = (130, 1, 64, 65, 63)
    n_states = {"cabac": (460, 4, 0, 126, 9, 8, 40), "cabac8": (126, 5, 0, 64, 9, 8, 30), "codes": (200, 20, 50, 120, 9, 8, 40)}.get(kind, (0,) * 7)
    groups = ((5, (0, 2, 4)), (1, ()), (3, (1,)), (2, ()), (4, (0, 3)))
    runs = []
    for j, n in enumerate(counts):
        runs.append(br.make_run("shrink%d-%s-%d-slices" % (j, kind, n), kind, "lanes", 7400 + 10 * br.KINDS.index(kind) + j, n_slices=n,
                                n_states=n_states[j], groups=groups[j][0], given=groups[j][1], method="reserve" if j % 2 else "add"))
    runs.append(br.make_run("shrink5-%s-chunked" % kind, kind, "chunked", 7405 + 10 * br.KINDS.index(kind), n_slices=4, n_states=n_states[5], groups=2, given=(0,)))
    rng = np.random.default_rng(7406)
    lengths = br.lane_lengths(rng, 60, 900)
    lengths[20:25] = [0] * 5
    last = br.make_run("shrink6-%s-lanes" % kind, kind, "lanes", 7406 + 10 * br.KINDS.index(kind), lengths=lengths, n_states=n_states[6], groups=4, given=(1, 3))
    if kind == "keys":
        last.group_first = [0, 20, 25, 60]                       # group 1: empty slices only; group 3: no slice at all
    runs.append(last)
    return runs


@pytest.mark.parametrize("kind", br.KINDS)
def test_shrink_after_grow(device, kind):
    new_batch, _, _ = device("product")
    runs = shrink_runs(kind)
    br.seq_runs(new_batch, runs, "shrink after grow")
    if kind == "keys":                                           # a group with no bins hands its start table back
        last, want = runs[-1], br.expected(runs[-1])
        assert np.array_equal(want.tables[1], last.tables[1]) and np.array_equal(want.tables[3], last.tables[3])


# ------------------------------------------------------------------ c. the checks across runs
@pytest.mark.parametrize("family,kinds", [("k1", ("cabac", "cabac8", "codes")), ("k2", ())])
def test_the_checks_across_runs(device, family, kinds):
    """One object through eight runs over every on/off pattern of its two switches (K1: set_verify_k1, expectations; K2: set_verify, key
    records -- the estimator checker rides on verify), a finding forced in every check a run has; a run without a check reports
    VERIFY_NONE for every slice, 0.0 ms and no VERIFY_FAILED.  Consecutive runs share the verify switch in both of its states and do not
    set it again: it survives reset(); the expectations do not.  Then a run with every check finding something in one slice, and behind
    a reset the checks on and no fault: nothing is found; the same slices submitted again as they are, with the fault and without."""
    new_batch, setter, _ = device("hooks")
    br.seq_checks(new_batch, setter, br.check_runs(family, kinds))


# ------------------------------------------------------------------ d. empty runs and refusals in between
@pytest.mark.parametrize("a_type", br.RUN_TYPES, ids=lambda t: "A-%s-%s" % t)
def test_an_empty_run_reports_nothing_of_the_run_before(device, a_type):
    new_batch, setter, fresh_of = device("product")
    A = br.run_type(*a_type, "A")
    B = br.run_type(*br.RUN_TYPES[(br.RUN_TYPES.index(a_type) + 3) % len(br.RUN_TYPES)], "B")
    br.seq_empty(new_batch, setter, A, B, fresh_of(B))


@pytest.mark.parametrize("kind", br.KINDS)
def test_a_refused_submit_leaves_a_sound_object(device, kind):
    new_batch, _, fresh_of = device("product")
    B = br.run_type(kind, "lanes", "B")
    br.seq_refused(new_batch, B, fresh_of(B))


@pytest.mark.parametrize("kind", br.KINDS + ("codes-tight",))
def test_a_refused_add_leaves_no_trace(device, kind):
    """Exactly max_slices slices and max_bins bins; for codes also 64 slices of one code, whose padding takes the most of the padded
    code buffer a batch of that size can ask for."""
    new_batch, _, _ = device("product")
    if kind == "codes-tight":
        run = br.make_run("tight-codes", "codes", "lanes", 7500, lengths=[1] * 64, n_states=4)
    else:
        run = br.run_type(kind, "lanes", "B")
    br.seq_capacity(new_batch, run)


# ------------------------------------------------------------------ e. objects coming and going
def test_objects_come_and_go(device):
    """Twenty rounds of create, fill, run, destroy over the ten run types (the stream pools are keyed by stream handles, which a
    process gets back); then two objects in flight together, of different kinds."""
    new_batch, _, _ = device("product")
    for k in range(20):
        run = br.run_type(*br.RUN_TYPES[(3 * k) % len(br.RUN_TYPES)], "B")
        b = new_batch(len(run.slices), run.total)
        try:
            br.fill(b, run, method=("add", "reserve")[k % 2])
            br.run_and_check(b, run, "round %d of create and destroy" % k, again=k % 4 == 0)
        finally:
            b.close()
    for one, other in ((("cabac", "lanes"), ("range", "chunked")), (("keys", "chunked"), ("cabac8", "lanes")), (("codes", "chunked"), ("keys", "lanes"))):
        r1, r2 = br.run_type(*one, "B"), br.run_type(*other, "B")
        assert one != ("cabac", "lanes") or r1.n_states > 8
        b1, b2 = new_batch(*br.room(r1)), new_batch(*br.room(r2))
        try:
            for turn in range(2):
                if turn:
                    b1.reset()
                    b2.reset()
                br.fill(b1, r1)
                br.fill(b2, r2)
                b1.submit()
                b2.submit()
                b1.wait()
                b2.wait()
                for b, r, beside in ((b1, r1, r2), (b2, r2, r1)):
                    got = br.collect(b, r)
                    br.compare(got, br.expected(r), "in flight beside run %s, turn %d" % (beside.name, turn), r)
        finally:
            b1.close()
            b2.close()
