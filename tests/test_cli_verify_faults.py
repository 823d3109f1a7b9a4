"""The command line when a verify switch finds a fault (README: `Verify error: ... (slice N, bin M)`, exit status 1, nothing written),
on the CPU: the stand-in for the batch calls (tests/cpu_batch.cpp: the oracle codes and verifies, with the fault points of the
device's test build) linked with the real csrc/host/recode_main.cpp, under ASan + UBSan, and once more under ThreadSanitizer.  Stand-
alone programs started as child processes, nothing preloaded.

What is held here is the host code between a verifier's finding and that promise: compressor::take_from, decompressor::take_from,
take_restore_from (csrc/host/avr_recode.h), run_compress / run_decompress / roundtrip and the window driver of `recode test <dir>`
(recode_main.cpp), where the slices of all files of a window share one batch and a finding at batch slice first + i must fail the owning
file only, under its own index i.  The K1-verifier branch of take_restore_from is not reachable from the command line (no restore batch
of the CLI has the K1 verifier on): tests/restore_host.cpp has it.

What these tests found when they were written, fixed in recode_main.cpp: `roundtrip <in> <out>` and the loop of AVR_TEST_SEQUENTIAL=1
opened (and so created) the output file before the run, so a file that ended in `Verify error` left an empty one behind.

AVR_CLI_FAULTS_RECORD=<path>: the case table (case -> status, message, files written) as JSON (profiles/cli_verify_faults.json is
such a run)."""
import json
import os

import pytest

import cli_verify_faults as cvf
import cpu_recode

ROWS = []


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    d = tmp_path_factory.mktemp("cli_verify_faults")

    class Cli:
        asan = cpu_recode.build(d, sanitize=True)
        work = d
        _sound = {}

        def sound(self, clip="realshort", model_hooks=0):
            if (clip, model_hooks) not in self._sound:
                self._sound[clip, model_hooks] = cvf.Sound(self.asan, d, clip, model_hooks)
            return self._sound[clip, model_hooks]

    yield Cli()
    path = os.environ.get("AVR_CLI_FAULTS_RECORD")
    if path:
        with open(path, "w") as f:
            json.dump({"build": "tests/cpu_batch.cpp + csrc/host/recode_main.cpp, ASan + UBSan", "rows": ROWS}, f, indent=1)


def clean(o):
    assert "AddressSanitizer" not in o.stderr and "runtime error" not in o.stderr, o.stderr[-3000:]


def record(case, status, messages, written):
    ROWS.append(dict(case=case, status=status, messages=messages, written=written))


def source(cli, clip, command, model_hooks=0):
    return cli.sound(clip, model_hooks).path if command == "decompress" else os.path.join(cpu_recode.GOLDEN, clip + ".mp4")


def sound_product(cli, clip, command, model_hooks=0):
    """What a sound run of `command` writes: the clip for decompress, the container for compress and roundtrip."""
    return cpu_recode.golden(clip) if command == "decompress" else cli.sound(clip, model_hooks).container


def one_fault(cli, tmp_path, clip, kind, command, j, env, case):
    s = cli.sound(clip)
    out = tmp_path / "out"
    o = cpu_recode.run(cli.asan, command, source(cli, clip, command), out, 0, env=env)
    print(case, "->", o.status, o.messages)
    clean(o)
    record(case, o.status, o.messages, out.exists())
    assert o.status == 1, o.stderr[-2000:]
    assert o.messages == [s.message(kind, j)]
    assert not out.exists(), "a file at the output path beside exit status 1"


# ------------------------------------------------------------------------------------------------ a. sound input, every switch set
@pytest.mark.parametrize("model_hooks", (0, 1))
@pytest.mark.parametrize("switches", cvf.switch_subsets(), ids=lambda s: "+".join(x[4:] for x in s) or "none")
def test_compress_writes_the_same_bytes_under_every_switch_set(cli, tmp_path, switches, model_hooks):
    env = dict({s: "1" for s in switches}, AVR_TIMING="1")
    out = tmp_path / "out.recode"
    o = cpu_recode.run(cli.asan, "compress", source(cli, "realshort", "compress"), out, model_hooks, env=env)
    clean(o)
    record("sound compress %s hooks=%d" % ("+".join(switches) or "no switch", model_hooks), o.status, o.messages, out.exists())
    assert o.status == 0 and o.messages == [] and out.read_bytes() == cli.sound("realshort", model_hooks).container, o.stderr[-2000:]
    for switch, lines in cvf.TIMING_LINES.items():           # the verifier lines the README names: there exactly when their switch is on
        for line in lines:
            assert (("[timing] " + line) in o.stderr) == (switch in switches), (line, o.stderr)
    est = "AVR_VERIFY" in switches and "AVR_DEVICE_ESTIMATORS" in switches and not model_hooks
    assert (cvf.EST_TIMING_LINE in o.stderr) == est, o.stderr


@pytest.mark.parametrize("model_hooks", (0, 1))
@pytest.mark.parametrize("verify_k1", (0, 1))
def test_decompress_gives_back_the_clip_with_and_without_the_k1_verifier(cli, tmp_path, verify_k1, model_hooks):
    env = dict({"AVR_VERIFY_K1": "1"} if verify_k1 else {}, AVR_TIMING="1")
    out = tmp_path / "back.mp4"
    o = cpu_recode.run(cli.asan, "decompress", cli.sound("realshort", model_hooks).path, out, model_hooks, env=env)
    clean(o)
    assert o.status == 0 and o.messages == [] and out.read_bytes() == cpu_recode.golden("realshort"), o.stderr[-2000:]
    assert (("[timing] " + cvf.TIMING_LINES["AVR_VERIFY_K1"][0]) in o.stderr) == bool(verify_k1), o.stderr


def test_roundtrip_with_every_switch_on_writes_the_same_bytes(cli, tmp_path):
    out = tmp_path / "out.recode"
    env = {"AVR_DEVICE_ESTIMATORS": "1", "AVR_VERIFY": "1", "AVR_VERIFY_RESTORE": "1", "AVR_VERIFY_K1": "1"}
    o = cpu_recode.run(cli.asan, "roundtrip", source(cli, "realshort", "roundtrip"), out, 0, env=env)
    clean(o)
    assert o.status == 0 and o.messages == [] and out.read_bytes() == cli.sound().container, o.stderr[-2000:]


# ------------------------------------------------------------------------------------------------ b. one fault, one message
@pytest.mark.parametrize("place", (0, 1, 2), ids=("first", "middle", "last"))
@pytest.mark.parametrize("through", ("own", "roundtrip"))
@pytest.mark.parametrize("kind", sorted(cvf.KINDS))
def test_one_fault_one_message(cli, tmp_path, kind, through, place):
    s = cli.sound()
    j = s.places(kind)[place]
    command = cvf.KINDS[kind]["command"] if through == "own" else "roundtrip"
    one_fault(cli, tmp_path, "realshort", kind, command, j, cvf.fault_env(kind, j + 1, s.est_bin(j)), "%s %s slice %d" % (kind, command, j))


@pytest.mark.parametrize("kind", sorted(cvf.KINDS))
def test_one_fault_one_message_on_the_long_clip(cli, tmp_path, kind):
    s = cli.sound("cockatoo")
    j = s.places(kind)[1]
    one_fault(cli, tmp_path, "cockatoo", kind, cvf.KINDS[kind]["command"], j, cvf.fault_env(kind, j + 1, s.est_bin(j)),
              "%s %s cockatoo slice %d" % (kind, cvf.KINDS[kind]["command"], j))


@pytest.mark.parametrize("how", ("past the last slice", "switch off"))
@pytest.mark.parametrize("through", ("own", "roundtrip"))
@pytest.mark.parametrize("kind", sorted(cvf.KINDS))
def test_a_fault_that_addresses_nothing_changes_nothing(cli, tmp_path, kind, through, how):
    s = cli.sound()
    command = cvf.KINDS[kind]["command"] if through == "own" else "roundtrip"
    if how == "past the last slice":
        env = cvf.fault_env(kind, s.n + 1, 0)
    else:
        j = s.places(kind)[1]
        env = cvf.without_switches(cvf.fault_env(kind, j + 1, s.est_bin(j)))
        if kind == "est":                                    # the estimators on the device, nothing verified: the hook is not read
            env["AVR_DEVICE_ESTIMATORS"] = "1"
    out = tmp_path / "out"
    o = cpu_recode.run(cli.asan, command, source(cli, "realshort", command), out, 0, env=env)
    clean(o)
    record("%s %s, %s" % (kind, command, how), o.status, o.messages, out.exists())
    assert o.status == 0 and o.messages == [] and out.read_bytes() == sound_product(cli, "realshort", command), o.stderr[-2000:]


# ------------------------------------------------------------------------------------------------ c. which finding wins
def test_the_estimator_finding_is_shown_where_the_decoder_is_content_and_the_decoder_wins_where_both_find(cli, tmp_path):
    s = cli.sound()
    j = s.places("est")[1]
    out = tmp_path / "out.recode"
    o = cpu_recode.run(cli.asan, "compress", source(cli, "realshort", "compress"), out, 0, env=cvf.fault_env("est", j + 1, s.est_bin(j)))
    clean(o)
    assert (o.status, o.messages, out.exists()) == (1, [s.message("est", j)], False)
    # Both on one slice.  The decoder reads the bumped record too, so its first bad bin is the oracle's over the bytes the encoder makes of
    # those records: not the sound run's.  The sentence and the slice are held here, the bin against the oracle with those very records.
    import oracle_lib
    import verify_streams
    oracle = oracle_lib.load_oracle()
    recs = s.slices["est"][j]["data"].copy()
    recs[s.est_bin(j)] += 0x100
    coded, status = oracle.range_encode(recs, cap=2 * recs.size + 64)
    assert status == 0
    m = verify_streams.first_bad(oracle, bytes([coded[0] ^ 0x80]) + coded[1:], recs)
    assert m != cvf.VERIFY_NONE
    o = cpu_recode.run(cli.asan, "compress", source(cli, "realshort", "compress"), out, 0, env=cvf.fault_env("est", j + 1, s.est_bin(j), both=True))
    clean(o)
    record("est + k2 on slice %d" % j, o.status, o.messages, out.exists())
    assert (o.status, o.messages, out.exists()) == (1, [cvf.EXCEPTION + cvf.KINDS["k2"]["sentence"] % (j, m)], False)


# ------------------------------------------------------------------------------------------------ d. the window driver on real clips
@pytest.fixture(scope="module")
def sound_directory(cli):
    """`recode test <dir>` over five copies of the short clip, no switch, the default window: the outputs every other run is held to."""
    d = cvf.make_directory(cli.work / "sound_dir")
    status, stdout, stderr, per_file, rows, files = cvf.run_test(cli.asan, d, {})
    assert status == 0 and "AddressSanitizer" not in stderr and "runtime error" not in stderr, stderr[-3000:]
    assert "failed on" not in stdout and len(rows) == 5 and sorted(files) == sorted(cvf.COPIES)
    return files


@pytest.mark.parametrize("setting", ({"AVR_TEST_WINDOW": "64"}, {"AVR_TEST_WINDOW": "2"}, {"AVR_TEST_WINDOW": "1"}, {"AVR_TEST_SEQUENTIAL": "1"}),
                         ids=("window64", "window2", "window1", "sequential"))
def test_every_window_setting_writes_the_same_outputs_and_they_restore_the_clip(cli, tmp_path, sound_directory, setting):
    status, stdout, stderr, per_file, rows, files = cvf.run_test(cli.asan, cvf.make_directory(tmp_path / "dir"), setting)
    assert "AddressSanitizer" not in stderr and "runtime error" not in stderr, stderr[-3000:]
    assert status == 0 and "failed on" not in stdout and len(rows) == 5 and len(per_file) == 5
    assert files == sound_directory and all(b == cli.sound().container for b in files.values())
    back = tmp_path / "back.mp4"                             # (the five are one container: it restores the clip)
    o = cpu_recode.run(cli.asan, "decompress", tmp_path / "dir" / "output" / cvf.COPIES[3], back, 0)
    assert o.status == 0 and back.read_bytes() == cpu_recode.golden("realshort")


def window_fault(cli, tmp_path, sound_directory, kind, k, setting, case):
    s = cli.sound()
    window = int(setting.get("AVR_TEST_WINDOW", 64)) if "AVR_TEST_SEQUENTIAL" not in setting else 1
    hit = cvf.owners(k, window, s.n)
    j = (k - 1) % s.n
    env = dict(cvf.fault_env(kind, k, s.est_bin(j)), **setting)
    status, stdout, stderr, per_file, rows, files = cvf.run_test(cli.asan, cvf.make_directory(tmp_path / "dir"), env)
    print(case, "->", status, stdout.splitlines()[-1:], {i: cvf.exception_lines(t) for i, t in enumerate(per_file)})
    record(case, status, [l for t in per_file for l in cvf.exception_lines(t)], sorted(files))
    assert "AddressSanitizer" not in stderr and "runtime error" not in stderr, stderr[-3000:]
    assert status == 0 and len(per_file) == 5
    for i, text in enumerate(per_file):                      # the owning file fails under its own index; the others say nothing
        assert cvf.exception_lines(text) == ([s.message(kind, hit[i])] if i in hit else []), (i, text)
    assert stdout.rstrip().endswith("failed on %d / 5 files" % len(hit)), stdout
    assert sorted(files) == sorted(n for i, n in enumerate(cvf.COPIES) if i not in hit)
    assert len(rows) == 5 - len(hit)
    assert all(files[n] == sound_directory[n] for n in files)
    return hit


@pytest.mark.parametrize("place", ("second file", "first slice of a file", "last slice of the batch"))
@pytest.mark.parametrize("kind", sorted(cvf.KINDS))
def test_a_window_loses_only_the_file_that_owns_the_slice(cli, tmp_path, sound_directory, kind, place):
    s = cli.sound()
    first, middle, last = s.places(kind)
    k = {"second file": s.n + middle + 1, "first slice of a file": 2 * s.n + first + 1, "last slice of the batch": 4 * s.n + last + 1}[place]
    if place == "first slice of a file":
        assert first == 0
    if place == "last slice of the batch":
        assert last == s.n - 1 and k == 5 * s.n
    hit = window_fault(cli, tmp_path, sound_directory, kind, k, {"AVR_TEST_WINDOW": "64"}, "test <dir> window 64, %s, %s" % (kind, place))
    assert len(hit) == 1


@pytest.mark.parametrize("where", ("second file", "first file"))
@pytest.mark.parametrize("kind", sorted(cvf.KINDS))
def test_with_a_window_of_two_the_fault_hits_a_file_of_every_window_that_has_the_slice(cli, tmp_path, sound_directory, kind, where):
    """The hook addresses the slice per batch, and every window has a batch of its own: windows {a, b}, {c, d}, {e}.  A slice of a
    window's first file is in all three (three files fail), one of its second file in the two windows that have a second file."""
    s = cli.sound()
    middle = s.places(kind)[1]
    k = middle + 1 + (s.n if where == "second file" else 0)
    hit = window_fault(cli, tmp_path, sound_directory, kind, k, {"AVR_TEST_WINDOW": "2"}, "test <dir> window 2, %s, %s" % (kind, where))
    assert sorted(hit) == ([1, 3] if where == "second file" else [0, 2, 4]) and set(hit.values()) == {middle}


def test_the_sequential_loop_loses_every_file_and_leaves_no_output_behind(cli, tmp_path, sound_directory):
    """AVR_TEST_SEQUENTIAL=1 is a batch a file: the fault hits slice k - 1 of each of the five, and none of them leaves a file."""
    s = cli.sound()
    k = s.places("k2")[1] + 1
    hit = window_fault(cli, tmp_path, sound_directory, "k2", k, {"AVR_TEST_SEQUENTIAL": "1"}, "test <dir> sequential, k2")
    assert len(hit) == 5


# ------------------------------------------------------------------------------------------------ e. threads
@pytest.fixture(scope="module")
def tsan(cli):
    return cvf.build_tsan(cli.work)


def test_the_parse_threads_and_the_files_threads_are_clean_under_tsan(cli, tsan, tmp_path):
    """The same command line under ThreadSanitizer (a stand-alone program): compress with 1, 2 and 16 parse threads writes the same
    bytes with no report, and so does `test <dir>` with a window of two, one file a thread."""
    made = {}
    for threads in (1, 2, 16):
        out = tmp_path / ("out.%d" % threads)
        o = cpu_recode.run(tsan, "compress", source(cli, "realshort", "compress"), out, 0, env={"AVR_PARSE_THREADS": str(threads), "AVR_TIMING": "1"})
        assert "ThreadSanitizer" not in o.stderr and o.status == 0, o.stderr[-3000:]
        made[threads] = out.read_bytes()
    assert made[1] == made[2] == made[16] == cli.sound().container
    status, stdout, stderr, per_file, rows, files = cvf.run_test(tsan, cvf.make_directory(tmp_path / "dir"), {"AVR_TEST_WINDOW": "2"})
    assert "ThreadSanitizer" not in stderr and status == 0 and "failed on" not in stdout, stderr[-3000:]
    assert sorted(files) == sorted(cvf.COPIES) and all(b == cli.sound().container for b in files.values())
