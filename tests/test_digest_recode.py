"""The optional digest of a .recode file on the CPU: the command line on the stand-in for the batch calls (tests/cpu_batch.cpp, coded
by oracle/), under AddressSanitizer and UBSan, every run a child process with nothing preloaded.

`AVR_DIGEST=1` puts Recoded.metadata at the head of the archive -- the SHA-256 and the length of the original -- and every route that
restores an archive holds the assembled file to it before a byte is written.  What is pinned here:
  * the format: the archive is tests/digest_recode.py's prefix (hashlib's digest, this side's varints) plus the archive without the
    switch, byte for byte; `decompress` restores it; `check` vouches for it, and says that it cannot for an archive without a digest;
  * no silent difference is left: over the whole damaged-container corpus of tests/damaged_recode.py, each case behind the prefix,
    exit status 0 means the original came back, with no case left out -- and the cases profiles/damaged_recode.json records as
    restoring another file with exit status 0 now end with the digest message;
  * damage to the prefix itself ends the same way;
  * `recode test <dir>` writes the archives `compress` writes, windowed and a file at a time.
"""
import os
import shutil
import subprocess

import pytest

import cpu_recode
import damaged_recode as dmg
import digest_recode as dig

CLIPS = ("realshort", "cockatoo")


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    """The sanitized stand-in command line, and per (clip, hooks setting) the archive without and with the digest, made once."""
    d = tmp_path_factory.mktemp("digest_recode")

    class Cli:
        asan = cpu_recode.build(d, sanitize=True)
        work = d
        _made = {}

        def archives(self, clip, model_hooks):
            key = (clip, model_hooks)
            if key not in self._made:
                src = os.path.join(cpu_recode.GOLDEN, clip + ".mp4")
                files = {}
                for tag, env in (("unset", {}), ("0", {"AVR_DIGEST": "0"}), ("1", {"AVR_DIGEST": "1"})):
                    dst = d / ("%s.%d.%s.recode" % (clip, model_hooks, tag))
                    o = run(self.asan, "compress", src, dst, model_hooks, env)
                    assert o.status == 0 and not o.messages, o.stderr[-2000:]
                    files[tag] = dst
                plain = files["unset"].read_bytes()
                self._made[key] = dict(files=files, plain=plain, cases=None)
            return self._made[key]

        def cases(self, clip, model_hooks):
            a = self.archives(clip, model_hooks)
            if a["cases"] is None:
                a["cases"] = dict(dmg.container_cases(a["plain"]))
            return a["cases"]

    return Cli()


def run(exe, command, src, dst, model_hooks, env=None):
    """cpu_recode.run with AVR_DIGEST as `env` has it and unset otherwise, whatever this process inherited (the child starts from
    this process's environment)."""
    saved = os.environ.pop("AVR_DIGEST", None)
    try:
        return cpu_recode.run(exe, command, src, dst, model_hooks, env=env)
    finally:
        if saved is not None:
            os.environ["AVR_DIGEST"] = saved


def check(exe, archive, model_hooks, cwd=None):
    """`recode check <archive>`: (exit status, stdout, the Exception lines, stderr).  No output path: the command takes none."""
    e = dict(os.environ, AVR_MODEL_HOOKS=str(int(model_hooks)), ASAN_OPTIONS="detect_leaks=0:abort_on_error=0")
    for k in ("AVR_VERIFY", "AVR_VERIFY_K1", "AVR_VERIFY_RESTORE", "AVR_DEVICE_ESTIMATORS", "AVR_TIMING", "AVR_DIGEST"):
        e.pop(k, None)
    p = subprocess.run([exe, "check", str(archive)], capture_output=True, env=e, timeout=cpu_recode.TIMEOUT, cwd=cwd)
    stderr = p.stderr.decode("utf-8", "replace")
    return p.returncode, p.stdout.decode("utf-8", "replace"), [l for l in stderr.splitlines() if l.startswith("Exception (")], stderr


def clean(outcome):
    """The rule of tests/test_damaged_recode.py: exit status 0, or 1 with exactly one `Exception (` line; no signal, no sanitizer report."""
    assert "AddressSanitizer" not in outcome.stderr and "runtime error" not in outcome.stderr, outcome.stderr[-3000:]
    assert outcome.status in (0, 1), "ended with status %d\n%s" % (outcome.status, outcome.stderr[-2000:])
    assert len(outcome.messages) == (1 if outcome.status else 0), outcome.stderr[-2000:]


# ------------------------------------------------------------------------------------------------ the format
@pytest.mark.parametrize("clip,model_hooks", [("realshort", 0), ("realshort", 1), ("cockatoo", 0)])
def test_the_archive_is_the_prefix_and_the_plain_archive(cli, tmp_path, clip, model_hooks):
    a = cli.archives(clip, model_hooks)
    original = cpu_recode.golden(clip)
    assert a["files"]["0"].read_bytes() == a["plain"]                                   # off is off, however it is said
    assert dmg.serialise(dmg.parse(a["plain"])) == a["plain"]                           # ... and what the reference's schema describes
    with_digest = a["files"]["1"].read_bytes()
    assert with_digest == dig.prefix(original) + a["plain"]
    assert with_digest[:4] == b"\x0a" + bytes([len(dig.metadata(original))]) + b"\x2a\x20"
    back = tmp_path / "back.mp4"
    o = run(cli.asan, "decompress", a["files"]["1"], back, model_hooks)
    clean(o)
    assert o.status == 0 and back.read_bytes() == original, o.stderr[-2000:]
    empty = tmp_path / "empty"
    empty.mkdir()
    status, stdout, messages, stderr = check(cli.asan, a["files"]["1"], model_hooks, cwd=str(empty))
    assert (status, stdout, messages) == (0, "Digest OK: %d bytes\n" % len(original), []), stderr[-2000:]
    assert "AddressSanitizer" not in stderr and "runtime error" not in stderr
    status, stdout, messages, stderr = check(cli.asan, a["files"]["unset"], model_hooks, cwd=str(empty))
    assert (status, stdout, messages) == (1, "No digest in this archive: %d bytes restored, not checked\n" % len(original), []), stderr[-2000:]
    assert os.listdir(str(empty)) == []                                                 # check writes nothing


def test_the_phase_lines_and_roundtrip(cli, tmp_path):
    """AVR_TIMING=1 names the two phases; `roundtrip` with the switch writes the same archive as `compress` (its second half is the
    decompress route, digest check included)."""
    a = cli.archives("realshort", 0)
    src, dst = os.path.join(cpu_recode.GOLDEN, "realshort.mp4"), tmp_path / "roundtrip.recode"
    o = run(cli.asan, "roundtrip", src, dst, 0, {"AVR_DIGEST": "1", "AVR_TIMING": "1"})
    clean(o)
    assert o.status == 0 and dst.read_bytes() == a["files"]["1"].read_bytes(), o.stderr[-2000:]
    assert "[timing] compress: digest" in o.stderr and "[timing] decompress: digest" in o.stderr
    o = run(cli.asan, "roundtrip", src, dst, 0, {"AVR_TIMING": "1"})
    assert o.status == 0 and dst.read_bytes() == a["plain"] and "[timing] compress: digest" not in o.stderr and "[timing] decompress: digest" not in o.stderr, o.stderr[-2000:]


# ------------------------------------------------------------------------------------------------ no silent difference is left
def damaged(cli, tmp_path, clip, model_hooks, case):
    original = cpu_recode.golden(clip)
    src, dst = tmp_path / "damaged.recode", tmp_path / "restored.mp4"
    src.write_bytes(dig.prefix(original) + cli.cases(clip, model_hooks)[case])
    o = run(cli.asan, "decompress", src, dst, model_hooks)
    print(case, clip, model_hooks, "->", o.status, o.messages)
    clean(o)
    if o.status == 0:
        assert dst.read_bytes() == original, "exit status 0 and a file that is not the original"
    else:
        assert not dst.exists(), "an output file beside exit status 1"
    if case in dmg.MUST_RESTORE:
        assert o.status == 0, o.stderr[-2000:]
    return o, original


@pytest.mark.parametrize("case", dmg.CONTAINER_CASE_NAMES)
@pytest.mark.parametrize("model_hooks", (0, 1))
def test_no_damaged_container_restores_another_file_in_silence(cli, tmp_path, model_hooks, case):
    o, original = damaged(cli, tmp_path, "realshort", model_hooks, case)
    if case in dig.SILENT[model_hooks]:
        assert o.status == 1 and o.messages[0].startswith(dig.EXCEPTION + "Verify error: restored file does not match the archive's digest ("), o.stderr[-2000:]
        assert o.messages[0].endswith(" bytes restored, %d recorded)" % len(original))


@pytest.mark.parametrize("case", dmg.ONE_PER_FAMILY)
@pytest.mark.parametrize("model_hooks", (0, 1))
def test_no_damaged_container_of_the_long_clip_restores_another_file_in_silence(cli, tmp_path, model_hooks, case):
    damaged(cli, tmp_path, "cockatoo", model_hooks, case)


# ------------------------------------------------------------------------------------------------ damage inside the prefix
@pytest.mark.parametrize("case", dig.PREFIX_CASE_NAMES)
@pytest.mark.parametrize("model_hooks", (0, 1))
def test_a_damaged_prefix_ends_cleanly(cli, tmp_path, model_hooks, case):
    original = cpu_recode.golden("realshort")
    head, end, recorded = dig.prefix_cases(original)[case]
    src, dst = tmp_path / "damaged.recode", tmp_path / "restored.mp4"
    src.write_bytes(head + cli.archives("realshort", model_hooks)["plain"])
    o = run(cli.asan, "decompress", src, dst, model_hooks)
    print(case, model_hooks, "->", o.status, o.messages)
    clean(o)
    if o.status == 0:
        assert dst.read_bytes() == original
    else:
        assert not dst.exists()
    if end == dig.RESTORES:
        assert o.status == 0, o.stderr[-2000:]
    elif end == dig.DIGEST:
        assert o.status == 1 and o.messages == [dig.EXCEPTION + dig.MESSAGE % (len(original), recorded)], o.stderr[-2000:]
    else:
        assert o.status == 1 and o.messages == [dig.NOT_PARSED], o.stderr[-2000:]
    status, stdout, messages, stderr = check(cli.asan, src, model_hooks)                 # the same archive through `check`
    assert "AddressSanitizer" not in stderr and "runtime error" not in stderr, stderr[-3000:]
    if end != dig.RESTORES:
        assert (status, stdout, messages) == (1, "", o.messages), stderr[-2000:]
    elif case in ("tag_metadata_unknown", "tag_digest_unknown"):                          # restored, and nothing to vouch with
        assert (status, stdout, messages) == (1, "No digest in this archive: %d bytes restored, not checked\n" % len(original), []), stderr[-2000:]
    else:
        assert (status, stdout, messages) == (0, "Digest OK: %d bytes\n" % len(original), []), stderr[-2000:]


# ------------------------------------------------------------------------------------------------ recode test <dir>
@pytest.mark.parametrize("sequential", (False, True))
def test_recode_test_directory_writes_the_archives_of_compress(cli, tmp_path, sequential):
    """Two copies of each clip (the directory of tests/test_h264.py's cross-file test, kept small), the files of the window in one batch
    per direction or a file at a time: every output archive carries its own file's digest and is `compress`'s, byte for byte."""
    d = tmp_path / "clips"
    d.mkdir()
    names = {}
    for k in range(2):
        for clip in CLIPS:
            names["%02d_%s.mp4" % (k, clip)] = clip
            shutil.copy(os.path.join(cpu_recode.GOLDEN, clip + ".mp4"), d / ("%02d_%s.mp4" % (k, clip)))
    e = dict(os.environ, AVR_MODEL_HOOKS="0", AVR_DIGEST="1", ASAN_OPTIONS="detect_leaks=0:abort_on_error=0")
    for k in ("AVR_VERIFY", "AVR_VERIFY_K1", "AVR_VERIFY_RESTORE", "AVR_DEVICE_ESTIMATORS", "AVR_TIMING", "AVR_TEST_WINDOW", "AVR_TEST_SEQUENTIAL"):
        e.pop(k, None)
    if sequential:
        e["AVR_TEST_SEQUENTIAL"] = "1"
    p = subprocess.run([cli.asan, "test", str(d)], capture_output=True, text=True, env=e, timeout=4 * cpu_recode.TIMEOUT)
    assert "AddressSanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-3000:]
    assert p.returncode == 0 and "failed on" not in p.stdout, p.stdout + p.stderr[-2000:]
    log = (d / "output" / "log.txt").read_text()
    assert log.count("Compress-decompress roundtrip succeeded:") == len(names) and "Exception (" not in log
    assert len((d / "output" / "metrics.csv").read_text().strip().splitlines()) == 1 + len(names)
    for name, clip in names.items():
        got = (d / "output" / name).read_bytes()
        assert got.startswith(dig.prefix(cpu_recode.golden(clip))), name
        assert got == cli.archives(clip, 0)["files"]["1"].read_bytes(), name
