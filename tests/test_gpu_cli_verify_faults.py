"""The command line on the device when a verify switch finds a fault, against the CPU stand-in (tests/cpu_batch.cpp: the same host
code, the oracle coding and verifying the batches) given the same fault.

  a. the product (no hooks) on sound input, every switch set, both clips: the stand-in's bytes, and the clip back under AVR_VERIFY_K1=1;
  b. the hooked test build (tests/recode_hooked.cpp on libavrecode_hip_hooks.so) with a fault point set, against the stand-in with the
     same one: same exit status, the same single message -- so the device verifier's bin is the oracle's -- and nothing written; once
     per message on the other kernel path (K2p / K1p, the k1_path hook);
  c. `recode test <dir>` on the hooked build, the fault in the second file of a window: the same files fail with the same log lines,
     the other outputs are the stand-in's byte for byte;
  d. a hook set with its switch off: the product's sound bytes.

These inputs are not meant to fault anything: a fault point complements one bit of one output byte, or adds one to one estimator
field, between two kernels, and both verifiers decode arbitrary bytes inside their own regions -- with these very hooks at batch level
(test_a_flipped_byte_comes_back_through_the_batch_api).  All the same, one child process per case under a time limit, and a case that
ends by signal or at its limit stops the module: nothing more is started on the device behind it.  The stand-in is built here without
sanitizers."""
import os
import subprocess

import pytest

import cli_verify_faults as cvf
import cpu_recode

pytestmark = pytest.mark.gpu

STOPPED = []
K1P = {"k1_path": 2}                                         # pick_chunked: the intra-slice parallel path, in both directions


@pytest.fixture(scope="module")
def product(avr):
    return avr.build_recode()


@pytest.fixture(scope="module")
def hooked(avr):
    return cvf.build_hooked(avr)


@pytest.fixture(scope="module")
def stand_in():
    return cpu_recode.build_cached()


@pytest.fixture(scope="module")
def sound(stand_in, tmp_path_factory):
    d, made = tmp_path_factory.mktemp("sound"), {}

    def get(clip="realshort", model_hooks=0):
        if (clip, model_hooks) not in made:
            made[clip, model_hooks] = cvf.Sound(stand_in, d, clip, model_hooks)
        return made[clip, model_hooks]
    return get


def stop_unless_clean(what, status, stderr):
    if status not in (0, 1):
        STOPPED.append("%s ended with status %d" % (what, status))
        pytest.fail(STOPPED[0] + "\n" + stderr[-3000:])


def child(exe, command, src, dst, model_hooks, env=None):
    if STOPPED:
        pytest.skip("nothing more is started on the device: " + STOPPED[0])
    try:
        o = cpu_recode.run(exe, command, src, dst, model_hooks, env=env)
    except subprocess.TimeoutExpired:
        STOPPED.append("%s %s reached its time limit" % (os.path.basename(exe), command))
        raise
    stop_unless_clean("%s %s" % (os.path.basename(exe), command), o.status, o.stderr)
    return o


def child_test(exe, directory, env):
    if STOPPED:
        pytest.skip("nothing more is started on the device: " + STOPPED[0])
    try:
        r = cvf.run_test(exe, directory, env)
    except subprocess.TimeoutExpired:
        STOPPED.append("%s test reached its time limit" % os.path.basename(exe))
        raise
    stop_unless_clean("%s test" % os.path.basename(exe), r[0], r[2])
    return r


def source(sound, clip, command, model_hooks=0):
    return sound(clip, model_hooks).path if command == "decompress" else os.path.join(cpu_recode.GOLDEN, clip + ".mp4")


# ------------------------------------------------------------------------------------------------ a. the product on sound input
@pytest.mark.parametrize("model_hooks", (0, 1))
@pytest.mark.parametrize("switches", cvf.switch_subsets(), ids=lambda s: "+".join(x[4:] for x in s) or "none")
@pytest.mark.parametrize("clip", ("realshort", "cockatoo"))
def test_the_product_writes_the_stand_ins_bytes_under_every_switch_set(product, sound, tmp_path, clip, switches, model_hooks):
    out = tmp_path / "out.recode"
    o = child(product, "compress", source(sound, clip, "compress"), out, model_hooks, env={s: "1" for s in switches})
    assert o.status == 0 and o.messages == [], o.stderr[-2000:]
    assert out.read_bytes() == sound(clip, model_hooks).container


@pytest.mark.parametrize("model_hooks", (0, 1))
@pytest.mark.parametrize("clip", ("realshort", "cockatoo"))
def test_the_product_restores_the_stand_ins_container_under_the_k1_verifier(product, sound, tmp_path, clip, model_hooks):
    out = tmp_path / "back.mp4"
    o = child(product, "decompress", sound(clip, model_hooks).path, out, model_hooks, env={"AVR_VERIFY_K1": "1"})
    assert o.status == 0 and o.messages == [], o.stderr[-2000:]
    assert out.read_bytes() == cpu_recode.golden(clip)


# ------------------------------------------------------------------------------------------------ b. the same fault on both
def same_end(hooked, stand_in, sound, tmp_path, kind, command, j, more_hooks=None, both=False):
    s = sound()
    ends = {}
    for tag, exe, is_hooked in (("stand-in", stand_in, False), ("hooked", hooked, True)):
        out = tmp_path / (tag + ".out")
        env = cvf.fault_env(kind, j + 1, s.est_bin(j), hooked=is_hooked, more_hooks=more_hooks if is_hooked else None, both=both)
        o = child(exe, command, source(sound, "realshort", command), out, 0, env=env)
        print(tag, kind, command, j, "->", o.status, o.messages)
        ends[tag] = (o.status, o.messages, out.exists())
    assert ends["hooked"] == ends["stand-in"]
    return ends["hooked"]


@pytest.mark.parametrize("place", (0, 1, 2), ids=("first", "middle", "last"))
@pytest.mark.parametrize("through", ("own", "roundtrip"))
@pytest.mark.parametrize("kind", sorted(cvf.KINDS))
def test_one_fault_ends_the_hooked_build_as_it_ends_the_stand_in(hooked, stand_in, sound, tmp_path, kind, through, place):
    j = sound().places(kind)[place]
    command = cvf.KINDS[kind]["command"] if through == "own" else "roundtrip"
    assert same_end(hooked, stand_in, sound, tmp_path, kind, command, j) == (1, [sound().message(kind, j)], False)


@pytest.mark.parametrize("kind", sorted(cvf.KINDS))
def test_one_fault_on_the_intra_slice_parallel_path_ends_the_same_way(hooked, stand_in, sound, tmp_path, kind):
    """k1_path = 2: K2p codes the compress direction's batch (behind the resolver, for key records), K1p the restore batch and the
    decompress direction's -- the verifiers then read the slice-major records, and the restore check follows K1p."""
    j = sound().places(kind)[1]
    assert same_end(hooked, stand_in, sound, tmp_path, kind, cvf.KINDS[kind]["command"], j, more_hooks=K1P) == (1, [sound().message(kind, j)], False)


def test_the_decoders_finding_wins_over_the_estimator_checkers_on_the_device_too(hooked, stand_in, sound, tmp_path):
    j = sound().places("est")[1]
    status, messages, written = same_end(hooked, stand_in, sound, tmp_path, "est", "compress", j, both=True)
    assert status == 1 and not written and len(messages) == 1 and "recoded block does not decode" in messages[0] and "(slice %d, " % j in messages[0]


# ------------------------------------------------------------------------------------------------ c. recode test <dir>
@pytest.fixture(scope="module")
def sound_directory(stand_in, tmp_path_factory):
    status, stdout, stderr, per_file, rows, files = cvf.run_test(stand_in, cvf.make_directory(tmp_path_factory.mktemp("sound_dir") / "dir"), {})
    assert status == 0 and "failed on" not in stdout and sorted(files) == sorted(cvf.COPIES)
    return files


@pytest.mark.parametrize("window", (64, 2))
@pytest.mark.parametrize("kind", sorted(cvf.KINDS))
def test_a_window_on_the_device_loses_the_files_the_stand_in_loses(hooked, stand_in, sound, sound_directory, tmp_path, kind, window):
    s = sound()
    j = s.places(kind)[1]
    k = s.n + j + 1                                          # the second file of a window
    hit = cvf.owners(k, window, s.n)
    assert sorted(hit) == ([1] if window == 64 else [1, 3])
    ends = {}
    for tag, exe, is_hooked in (("stand-in", stand_in, False), ("hooked", hooked, True)):
        env = dict(cvf.fault_env(kind, k, s.est_bin(j), hooked=is_hooked), AVR_TEST_WINDOW=str(window))
        run = child_test if is_hooked else cvf.run_test
        status, stdout, stderr, per_file, rows, files = run(exe, cvf.make_directory(tmp_path / tag), env)
        ends[tag] = (status, stdout.splitlines()[-1], [cvf.exception_lines(t) for t in per_file], len(rows), files)
        print(tag, ends[tag][:4])
    assert ends["hooked"] == ends["stand-in"]
    status, last_line, lines, n_rows, files = ends["hooked"]
    assert status == 0 and last_line.endswith("failed on %d / 5 files" % len(hit)) and n_rows == 5 - len(hit)
    assert lines == [[s.message(kind, hit[i])] if i in hit else [] for i in range(5)]
    assert sorted(files) == sorted(n for i, n in enumerate(cvf.COPIES) if i not in hit) and all(files[n] == sound_directory[n] for n in files)


# ------------------------------------------------------------------------------------------------ d. a hook without its switch
@pytest.mark.parametrize("kind", sorted(cvf.KINDS))
def test_a_hook_is_inert_outside_a_verified_run(hooked, sound, tmp_path, kind):
    s = sound()
    j = s.places(kind)[1]
    command = cvf.KINDS[kind]["command"]
    env = cvf.without_switches(cvf.fault_env(kind, j + 1, s.est_bin(j), hooked=True))
    if kind == "est":
        env["AVR_DEVICE_ESTIMATORS"] = "1"                   # the resolver runs, nothing is verified: the hook is not read
    out = tmp_path / "out"
    o = child(hooked, command, source(sound, "realshort", command), out, 0, env=env)
    assert o.status == 0 and o.messages == [], o.stderr[-2000:]
    assert out.read_bytes() == (cpu_recode.golden("realshort") if command == "decompress" else s.container)
