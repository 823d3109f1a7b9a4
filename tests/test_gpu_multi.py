"""avr_multi at the level of avr_batch: key-record groups, the three checks, final states, submit / wait and reuse.

The rule every case is held to: slice by slice and group by group, a MultiBatch over any device list gives what ONE Batch on device 0
given the same calls gives -- bytes, statuses, final states, first_bad of either verifier and of the estimator checker, first_diff of the
restore check, every group's table -- and both give what the oracle gives.  The entries are GPU 0 named two to four times: as many
sub-batches, each with its own host thread, stream and staging.  tests/multi_cases.py describes a batch once and makes the same calls
on either object."""
import numpy as np
import pytest

import multi_cases as mc
import oracle_lib
import range_keys
import restore_ref
from avrecode_ms_amd.sharding import lpt_assign, lpt_assign_groups

pytestmark = pytest.mark.gpu

ERR_INVALID = "avr error -1"


def held_to_one_batch(avr, oracle, case, entries, what, skip_groups=(), how="run"):
    got, owners, load, info = mc.run_multi(avr, case, entries, how)
    mc.same(got, mc.run_single(avr, case), what, skip_groups)
    mc.against_oracle(oracle, got, case, what)
    assert sum(load) == sum(case.n_bins) and load == [sum(n for n, o in zip(case.n_bins, owners) if o == e) for e in range(len(entries))]
    return got, owners, info


# ------------------------------------------------------------------ 1. every kind

@pytest.fixture(scope="module")
def streams60():
    rng = np.random.default_rng(7101)
    return mc.k1_streams(rng, mc.mixed_lengths(rng, 60))


@pytest.mark.parametrize("kind", ["cabac", "cabac8", "codes", "range"])
def test_every_kind_over_three_entries(avr, oracle, streams60, kind):
    if kind == "range":
        rng = np.random.default_rng(7102)
        case = mc.Case("range", [oracle_lib.random_range_stream(rng, n) for n in mc.mixed_lengths(rng, 60)])
    else:
        case = mc.k1_case(oracle, kind, streams60)
    got, owners, _ = held_to_one_batch(avr, oracle, case, [0, 0, 0], kind)
    assert set(owners) == {0, 1, 2} and owners == lpt_assign(case.n_bins, 3)
    assert all(g[1] == 0 for g in got[0])
    if kind in ("cabac", "cabac8"):
        assert all(len(g[2]) == 120 for g in got[0])             # final states, one array a slice


# ------------------------------------------------------------------ 2. the intra-slice parallel path inside sub-batches

@pytest.mark.parametrize("kind", ["cabac", "codes", "range"])
def test_sub_batches_on_the_intra_slice_parallel_path(avr, oracle, kind):
    rng = np.random.default_rng(7200)
    lens = [int(n) for n in rng.integers(9000, 20001, 8)]
    if kind == "range":
        case = mc.Case("range", [oracle_lib.random_range_stream(rng, n) for n in lens])
    else:
        case = mc.k1_case(oracle, kind, mc.k1_streams(rng, lens), verify_k1=True)
    got, owners, info = held_to_one_batch(avr, oracle, case, [0, 0], kind)
    assert [i[0] for i in info] == [1, 1], info                  # both sub-batches chose it, each from its own share
    assert set(owners) == {0, 1} and all(g[1] == 0 and g[3] == mc.VERIFY_NONE for g in got[0])


# ------------------------------------------------------------------ 3. key records

@pytest.mark.parametrize("verify", [False, True])
def test_key_records_in_seven_groups(avr, oracle, verify):
    case = mc.seven_groups(np.random.default_rng(7300))
    case.verify = verify
    got, owners, _ = held_to_one_batch(avr, oracle, case, [0, 0, 0], f"key records, verify {verify}", skip_groups=(2,))
    first = case.group_first
    assert owners == lpt_assign_groups(case.n_bins, first, 3) and set(owners) == {0, 1, 2}
    for g in range(7):                                           # every slice of a group on one entry
        assert len(set(owners[first[g]:(first + [len(case)])[g + 1]])) <= 1
    bad = first[2] + 1                                           # the malformed slice and the rest of its group, and nothing else
    assert [i for i, s in enumerate(got[0]) if s[1] != 0] == [bad, bad + 1]
    assert all(got[0][i][:2] == (b"", mc.SLICE_BAD_RECORD) for i in (bad, bad + 1))
    assert np.array_equal(got[1][3], range_keys.fresh_table())   # the group without slices: its start table
    well_formed = [i for i in range(len(case)) if not first[2] <= i < first[3]]
    assert all(got[0][i][3:] == (mc.VERIFY_NONE,) * 3 for i in well_formed)       # no finding of the decoder or of the estimator checker


def test_an_empty_group_begun_from_a_table_gives_that_table(avr):
    rng = np.random.default_rng(7301)
    table = range_keys.random_table(rng)
    case = mc.Case("keys", [range_keys.random_keys(rng, 500, "skew") for _ in range(3)], groups=[(0, None), (2, table), (2, None), (3, table)])
    got, owners, _, _ = mc.run_multi(avr, case, [0, 0])
    mc.same(got, mc.run_single(avr, case), "empty groups from tables")
    assert np.array_equal(got[1][1], table) and np.array_equal(got[1][3], table)


def test_a_group_split_over_two_multis(avr, oracle):
    rng = np.random.default_rng(7302)
    slices = [range_keys.random_keys(rng, int(rng.integers(1, 3000)), "skew") for _ in range(6)]
    whole = mc.Case("keys", slices, groups=[(0, None)])
    want = mc.run_single(avr, whole)
    first, _, _, _ = mc.run_multi(avr, mc.Case("keys", slices[:3], groups=[(0, None)]), [0, 0, 0])
    second, _, _, _ = mc.run_multi(avr, mc.Case("keys", slices[3:], groups=[(0, first[1][0])]), [0, 0, 0])
    assert first[0] + second[0] == want[0]
    assert np.array_equal(second[1][0], want[1][0])
    mc.against_oracle(oracle, (first[0] + second[0], [second[1][0]]), whole, "the split group")


# ------------------------------------------------------------------ 4. findings, on the hooks build

def flipped(data):
    return bytes([data[0] ^ 0x80]) + data[1:]


@pytest.mark.parametrize("fault", ["verify_k2", "verify_k1", "est", "restore"])
def test_a_finding_in_local_slice_1_of_every_entry(avr, oracle, hooks, fault):
    """verify_flip, est_flip and restore_flip address each (sub-)batch's own slice K - 1: local slice 1 of every entry, and only those,
    come back AVR_SLICE_VERIFY_FAILED, with the first_bad / first_diff a single Batch holding that entry's slices reports; lengths are
    unchanged, and so are the bytes but for the bit the hook complements behind the encode."""
    rng = np.random.default_rng(7400)
    entries = [0, 0, 0]
    if fault == "verify_k2":
        case = mc.Case("range", [oracle_lib.random_range_stream(rng, int(n)) for n in rng.integers(60, 2500, 20)], verify=True)
        hooks(verify_flip=2)
    elif fault == "verify_k1":
        case = mc.k1_case(oracle, "cabac", mc.k1_streams(rng, [int(n) for n in rng.integers(60, 2500, 20)]), verify_k1=True)
        hooks(verify_flip=2)
    elif fault == "est":
        groups = [(2 * g, range_keys.random_table(rng) if g == 5 else None) for g in range(8)]
        case = mc.Case("keys", [range_keys.random_keys(rng, int(n), "skew") for n in rng.integers(60, 2500, 16)], groups=groups, verify=True)
        hooks(est_flip=2, est_flip_bin=5)
    else:
        streams = mc.k1_streams(rng, [int(n) for n in rng.integers(200, 2500, 20)])
        case = mc.k1_case(oracle, "codes", streams)
        case.expects = {i: avr.drop_stop_byte(oracle.cabac_encode(r, s)[0]) for i, (r, s) in enumerate(streams)}
        hooks(restore_flip=2)
    got, owners, _, _ = mc.run_multi(avr, case, entries)
    hit = mc.local_slice(owners, len(entries), 1)
    assert len(hit) == 3
    assert [i for i, g in enumerate(got[0]) if g[1] != 0] == sorted(hit)
    for e in range(len(entries)):
        mine = [i for i, o in enumerate(owners) if o == e]
        want = mc.run_single(avr, case.share(mine))
        mc.same(([got[0][i] for i in mine], []), (want[0], []), f"{fault}: entry {e} against a batch of its slices")
    truth, _ = mc.oracle_answers(oracle, case)
    which = {"verify_k2": 3, "verify_k1": 3, "est": 4, "restore": 5}[fault]
    for i, g in enumerate(got[0]):
        data = truth[i][0]
        if i in hit:
            assert g[1] == mc.SLICE_VERIFY_FAILED and g[which] != mc.VERIFY_NONE, (fault, i, g[1:])
            assert all(g[k] == mc.VERIFY_NONE for k in (3, 4, 5) if k != which)
            if fault == "est":
                assert g[4] == 5                                 # the estimator checker names the planted bin; the bytes are the flipped record's
                continue
            data = flipped(data)
        else:
            assert g[3:] == (mc.VERIFY_NONE,) * 3, (fault, i, g[3:])
        assert g[0] == data, (fault, i)                          # the length unchanged, the bytes but for the complemented bit
    if fault == "restore":
        assert all(got[0][i][5] == 0 for i in hit)               # byte 0 differs


# ------------------------------------------------------------------ 5. expectations without hooks

def test_expectations_right_and_wrong(avr, oracle):
    rng = np.random.default_rng(7500)
    streams = mc.k1_streams(rng, [int(n) for n in rng.integers(200, 2500, 24)])
    case = mc.k1_case(oracle, "codes", streams)
    coded = [oracle.cabac_encode(r, s)[0] for r, s in streams]
    for i, raw in enumerate(coded):
        if i % 4 == 3:
            continue                                             # several slices have none
        want = avr.drop_stop_byte(raw)
        assert restore_ref.first_diff(avr, raw, want) == restore_ref.VERIFY_NONE
        if i == 1:
            want = want[:-1]                                     # shorter
        elif i == 5:
            want = want + b"\x5a\x5a"                            # longer (one byte more is what the tail patch itself restores)
        elif i == 9:
            want = want[:len(want) // 2] + bytes([want[len(want) // 2] ^ 0x10]) + want[len(want) // 2 + 1:]
        case.expects[i] = want
    got, owners, _ = held_to_one_batch_with_findings(avr, oracle, case, [0, 0, 0], {1, 5, 9})
    for i, raw in enumerate(coded):
        want = restore_ref.first_diff(avr, raw, case.expects[i]) if i in case.expects else restore_ref.VERIFY_NONE
        assert got[0][i][5] == want, f"slice {i}: first_diff {got[0][i][5]}, the reference rule says {want}"
        assert (want != restore_ref.VERIFY_NONE) == (i in (1, 5, 9))


def held_to_one_batch_with_findings(avr, oracle, case, entries, failed):
    got, owners, _, info = mc.run_multi(avr, case, entries)
    mc.same(got, mc.run_single(avr, case), "expectations")
    mc.against_oracle(oracle, got, case, "expectations", failed=failed)
    return got, owners, info


# ------------------------------------------------------------------ 6. refusals and reuse

def test_the_wrong_direction_is_refused_and_the_object_stays_usable(avr, oracle, streams60):
    case = mc.k1_case(oracle, "cabac", streams60[:20])
    with avr.MultiBatch([0, 0], *mc.capacity(case)) as m:
        m.set_verify(True)
        mc.feed(m, case)
        for call in (m.submit, m.run):
            with pytest.raises(avr.AvrError, match="compress direction only"):
                call()
        assert m.created() == 0                                  # refused before any sub-batch was touched
        m.set_verify(False)
        m.run()
        mc.same(mc.answers(m, case), mc.run_single(avr, case), "after the refusal")
    keys = mc.seven_groups(np.random.default_rng(7600), malformed=False, hi=800)
    with avr.MultiBatch([0, 0], 64, 1 << 20) as m:
        m.set_verify_k1(True)
        mc.feed(m, keys)
        with pytest.raises(avr.AvrError, match="decompress direction only"):
            m.submit()
        m.reset()                                                # ... or reset: the setting stays, so K1 slices now run verified
        case.verify_k1 = True
        mc.feed(m, case)
        m.run()
        mc.same(mc.answers(m, case), mc.run_single(avr, case), "after the refusal and a reset")


def test_one_object_through_every_kind(avr, oracle, streams60):
    """CABAC, reset, key records with verify, reset, codes with expectations and the K1 verifier, reset, a run without slices, reset,
    CABAC8: every step equal to a fresh object's (and so to one Batch's); the same slices a second time create no sub-batch."""
    rng = np.random.default_rng(7601)
    cabac = mc.k1_case(oracle, "cabac", streams60[:30])
    keys = mc.seven_groups(rng, hi=1500)
    keys.verify = True
    codes = mc.k1_case(oracle, "codes", streams60[10:40], verify_k1=True)
    codes.expects = {i: avr.drop_stop_byte(oracle.cabac_encode(*streams60[10 + i])[0]) for i in range(0, 30, 3) if len(streams60[10 + i][0]) > 100}
    codes.expects[2] = b"\x01\x02\x03"                           # one that is wrong
    nothing = mc.Case("range", [])
    cabac8 = mc.k1_case(oracle, "cabac8", streams60[20:50])
    entries = [0, 0, 0]
    with avr.MultiBatch(entries, 64, 1 << 20) as m:
        for step, case in enumerate((cabac, keys, codes, nothing, cabac8, cabac8)):
            before = m.created()
            got = mc.run_on(m, case, "submit" if step % 2 else "run")
            fresh = mc.run_multi(avr, case, entries)
            skip = (2,) if case is keys else ()
            mc.same(got[0], fresh[0], f"step {step} against a fresh object", skip)
            assert got[1:3] == fresh[1:3]
            mc.same(got[0], mc.run_single(avr, case), f"step {step} against one batch", skip)
            mc.against_oracle(oracle, got[0], case, f"step {step}", failed={2} if case is codes else ())
            if case is nothing:
                assert got[3] == [[0, 0, 0, 0]] * 3 and m.entry_ms(0) == [0.0] * 7
            if step == 5:
                assert m.created() == before                     # the same slices again: every sub-batch reused
            m.reset()
            with pytest.raises(avr.AvrError, match="has not run"):
                m.get(0)
        assert 3 <= m.created() <= 3 * 4


def test_getters_before_a_run_and_out_of_range(avr, oracle, streams60):
    case = mc.k1_case(oracle, "cabac", streams60[:8])
    with avr.MultiBatch([0, 0], *mc.capacity(case)) as m:
        mc.feed(m, case)
        for call in (lambda: m.get(0), lambda: m.get_states(0), lambda: m.get_verify(0), lambda: m.get_verify_est(0), lambda: m.get_restore(0),
                     lambda: m.get_estimators(0), lambda: m.entry_info(0), lambda: m.entry_ms(0), lambda: m.placement(0), m.load, m.wait):
            with pytest.raises(avr.AvrError, match=ERR_INVALID):
                call()
        m.run()
        for call in (lambda: m.get(8), lambda: m.get_states(8), lambda: m.get_verify(8), lambda: m.get_verify_est(8), lambda: m.get_restore(8),
                     lambda: m.entry_info(2), lambda: m.entry_ms(2), lambda: m.placement(8), lambda: m.get_estimators(0)):
            with pytest.raises(avr.AvrError, match=ERR_INVALID):
                call()
        with pytest.raises(avr.AvrError, match="batch already ran"):
            m.submit()
        ms = m.entry_ms(0)
        assert len(ms) == 7 and ms[0] > 0 and ms[2] > 0 and ms[4:] == [0.0] * 3


# ------------------------------------------------------------------ 7. submit / wait

def test_two_multis_in_turn(avr, oracle):
    """Two MultiBatch objects used in turn over five rounds -- submit the next, wait for the previous -- and between submit and wait
    add, get, reset and expect are refused and disturb nothing."""
    rng = np.random.default_rng(7700)
    rounds = []
    for k in range(5):
        n_ctx = (40, 40, 300, 40, 120)[k]
        lens = [int(n) for n in (rng.integers(0, 1500, 50) if k != 3 else rng.integers(9000, 14000, 6))]
        rounds.append(mc.k1_case(oracle, "cabac" if k % 2 == 0 else "codes", [oracle_lib.random_cabac_stream(rng, n, n_ctx) for n in lens]))
    pair = [avr.MultiBatch([0, 0, 0], 64, 1 << 20) for _ in range(2)]
    extra = rounds[0].slices[0], rounds[0].states[0]
    try:
        def begin(k):
            m = pair[k % 2]
            mc.feed(m, rounds[k])
            m.submit()
            for call in (lambda: m.add_slice_cabac(*extra), lambda: m.add_codes(rounds[1].slices[0]), lambda: m.get(0), m.reset,
                         lambda: m.expect(0, b"abc"), m.submit, lambda: m.set_verify_k1(True), lambda: m.begin_group(), lambda: m.get_states(0),
                         lambda: m.placement(0), lambda: m.entry_info(0)):
                with pytest.raises(avr.AvrError, match=ERR_INVALID):
                    call()

        def end(k):
            m = pair[k % 2]
            m.wait()
            got = mc.answers(m, rounds[k])
            mc.against_oracle(oracle, got, rounds[k], f"round {k}")
            assert all(g[3:] == (mc.VERIFY_NONE,) * 3 for g in got[0])
            m.reset()
        begin(0)
        for k in range(1, 5):
            begin(k)
            end(k - 1)
        end(4)
        with pytest.raises(avr.AvrError, match="has not been submitted"):
            pair[0].wait()
    finally:
        for m in pair:
            m.close()
