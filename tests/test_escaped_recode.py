"""Escaped blocks on the CPU: slices whose NAL unit carries an emulation_prevention_three_byte inside the payload, coded with
`AVR_ESCAPED=1` (Block field 7, csrc/host/avr_host.h: escape) where they stay literal otherwise.  The command line on the stand-in
for the batch calls (tests/cpu_batch.cpp, coded by oracle/), under AddressSanitizer and UBSan, every run a child process with nothing
preloaded; tests/escaped_check.cpp is a sanitized stand-alone program of its own.

cockatoo.mp4 has 13 such slices among its 280, one escape each.  With the switch all 280 are coded blocks, 13 of them escaped, and
the file comes back byte for byte; without it the archive is what it was."""
import os
import shutil
import subprocess

import pytest

import cpu_recode
import damaged_recode as dmg
import finish_ref
import h264_corpus as corpus
import h264_walker as hw

F_SIZE, F_LITERAL, F_SKIP, F_CABAC, F_ESCAPED = 1, 2, 3, 4, 7
ON = {"AVR_ESCAPED": "1"}


def run(exe, command, src, dst, model_hooks=False, env=None):
    """cpu_recode.run with AVR_ESCAPED and AVR_DIGEST as `env` has them and unset otherwise, whatever this process inherited."""
    saved = {k: os.environ.pop(k) for k in ("AVR_ESCAPED", "AVR_DIGEST") if k in os.environ}
    try:
        return cpu_recode.run(exe, command, src, dst, model_hooks, env=env)
    finally:
        os.environ.update(saved)


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    return cpu_recode.build(tmp_path_factory.mktemp("escaped_recode"), sanitize=True)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return cpu_recode.build_program(tmp_path_factory.mktemp("escaped_check"), "escaped_check", os.path.join(cpu_recode.ROOT, "tests", "escaped_check.cpp"))


def compress(cli, src, dst, env=None, model_hooks=False):
    o = run(cli, "compress", src, dst, model_hooks, env)
    assert o.status == 0 and not o.messages, o.stderr[-2000:]
    return dst.read_bytes()


def restores(cli, archive, original, tmp_path, model_hooks=False, env=None):
    back = tmp_path / "back.bin"
    if back.exists():
        back.unlink()
    o = run(cli, "decompress", archive, back, model_hooks, env)
    assert o.status == 0 and not o.messages, o.stderr[-2000:]
    assert back.read_bytes() == original


def kinds(archive):
    """(blocks with cabac, blocks with field 7, skip_coded blocks without field 7) of an archive without metadata."""
    blocks = dmg.parse(archive)
    for b in blocks:
        if dmg.has(b, F_ESCAPED):
            assert dmg.get(b, F_ESCAPED) == 1 and dmg.has(b, F_CABAC) and dmg.get(b, F_SKIP) == 0        # the pair a reader without field 7 refuses
            assert [f for f, _, _ in b] == sorted(f for f, _, _ in b)                                  # in field-number order
    return (sum(dmg.has(b, F_CABAC) for b in blocks), sum(dmg.has(b, F_ESCAPED) for b in blocks),
            sum(dmg.has(b, F_SKIP) and not dmg.has(b, F_ESCAPED) for b in blocks))


@pytest.fixture(scope="module")
def cockatoo(cli, tmp_path_factory):
    d = tmp_path_factory.mktemp("cockatoo")
    src = os.path.join(cpu_recode.GOLDEN, "cockatoo.mp4")
    return {tag: (d / (tag + ".recode"), compress(cli, src, d / (tag + ".recode"), env))
            for tag, env in (("unset", None), ("0", {"AVR_ESCAPED": "0"}), ("1", ON))}


def test_cockatoo_codes_its_thirteen_escaped_slices(cli, cockatoo, tmp_path):
    """Fails without the feature: the switch does nothing there and the 13 slices stay skip_coded blocks."""
    original = cpu_recode.golden("cockatoo")
    assert kinds(cockatoo["1"][1]) == (280, 13, 0)
    assert kinds(cockatoo["unset"][1]) == (267, 0, 13) and cockatoo["unset"][1] == cockatoo["0"][1]
    restores(cli, cockatoo["1"][0], original, tmp_path)
    restores(cli, cockatoo["unset"][0], original, tmp_path)
    src = os.path.join(cpu_recode.GOLDEN, "cockatoo.mp4")
    for env in (dict(ON, AVR_DIGEST="1"), dict(ON, AVR_VERIFY_RESTORE="1")):
        archive = tmp_path / "switches.recode"
        made = compress(cli, src, archive, env)
        assert made.endswith(cockatoo["1"][1]) and (len(made) > len(cockatoo["1"][1])) == ("AVR_DIGEST" in env)
        restores(cli, archive, original, tmp_path)
    o = run(cli, "roundtrip", src, tmp_path / "roundtrip.recode", env=dict(ON, AVR_VERIFY_RESTORE="1"))
    assert o.status == 0 and not o.messages and "Compress-decompress roundtrip succeeded:" in o.stderr, o.stderr[-2000:]
    assert (tmp_path / "roundtrip.recode").read_bytes() == cockatoo["1"][1]


def test_realshort_has_none_and_its_archive_does_not_change(cli, tmp_path):
    src = os.path.join(cpu_recode.GOLDEN, "realshort.mp4")
    assert compress(cli, src, tmp_path / "on.recode", ON) == compress(cli, src, tmp_path / "off.recode")


def test_test_dir_writes_the_archives_compress_writes(cli, cockatoo, tmp_path):
    d = tmp_path / "clips"
    d.mkdir()
    shutil.copy(os.path.join(cpu_recode.GOLDEN, "cockatoo.mp4"), d / "00_cockatoo.mp4")
    shutil.copy(os.path.join(cpu_recode.GOLDEN, "realshort.mp4"), d / "01_realshort.mp4")
    e = dict(os.environ, AVR_MODEL_HOOKS="0", AVR_ESCAPED="1", AVR_VERIFY_RESTORE="1", ASAN_OPTIONS="detect_leaks=0:abort_on_error=0")
    for k in ("AVR_VERIFY", "AVR_VERIFY_K1", "AVR_DEVICE_ESTIMATORS", "AVR_TIMING", "AVR_TEST_WINDOW", "AVR_TEST_SEQUENTIAL", "AVR_DIGEST"):
        e.pop(k, None)
    p = subprocess.run([cli, "test", str(d)], capture_output=True, text=True, env=e, timeout=4 * cpu_recode.TIMEOUT)
    assert "AddressSanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-3000:]
    assert p.returncode == 0 and "failed on" not in p.stdout, p.stdout + p.stderr[-2000:]
    assert (d / "output" / "log.txt").read_text().count("Compress-decompress roundtrip succeeded:") == 2
    assert (d / "output" / "00_cockatoo.mp4").read_bytes() == cockatoo["1"][1]


@pytest.fixture(scope="module")
def files(oracle, avr):
    from test_host import host as host_fixture
    host = host_fixture.__wrapped__(avr)
    host.t_init_states.restype = None
    return {name: corpus.build(name, oracle, host) for name in corpus.CASE_NAMES}


@pytest.mark.parametrize("name", corpus.CASE_NAMES)
def test_the_corpus_with_the_switch(cli, files, tmp_path, name):
    """Every slice the parser gets through (`expect` empty) is a coded block with the switch -- without it the escaped ones are not --
    and every file round-trips as Annex B, with the residual hooks off and on."""
    data, slices = files[name]
    src = tmp_path / (name + ".264")
    src.write_bytes(data)
    on, off = compress(cli, src, tmp_path / "on.recode", ON), compress(cli, src, tmp_path / "off.recode")
    coded, escaped, skipped = kinds(on)
    parsed = sum(1 for e in slices if not e["expect"])
    assert coded == parsed and skipped == len([e for e in slices if e["fields"] is not None]) - parsed
    assert kinds(off)[0] == coded - escaped and (on == off) == (escaped == 0)
    if name == "emulation":
        assert escaped >= 2
    restores(cli, tmp_path / "on.recode", data, tmp_path)
    compress(cli, src, tmp_path / "hooks.recode", ON, model_hooks=True)
    restores(cli, tmp_path / "hooks.recode", data, tmp_path, model_hooks=True)


def test_z_is_read_from_the_file_on_both_sides(program):
    """tests/escaped_check.cpp z: payloads behind 0, 1 and 2 zero bytes, beginning with a byte <= 3 and with one above."""
    r = subprocess.run([program, "z"], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0"), timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok 12 slices"), r.stdout[-2000:] + r.stderr[-4000:]


def rewritten(archive, change):
    """The archive with change(block) -> block applied to every block (the wire bytes made again by tests/damaged_recode.py)."""
    return dmg.serialise([change(b) for b in dmg.parse(archive)])


def refused(cli, archive, tmp_path, needle):
    src, dst = tmp_path / "rewritten.recode", tmp_path / "restored.bin"
    src.write_bytes(archive)
    o = run(cli, "decompress", src, dst)
    assert o.status == 1 and len(o.messages) == 1 and needle in o.messages[0], o.stderr[-2000:]
    assert not dst.exists()


def test_a_reader_that_does_not_know_field_7_refuses_the_archive(cli, cockatoo, tmp_path):
    """What an older reader sees is the archive without field 7: cabac and skip_coded = false on one block.  It ends with the message
    that reader has for it, exit status 1, nothing written -- it does not restore the unescaped bytes in silence."""
    old = rewritten(cockatoo["1"][1], lambda b: dmg.without(b, F_ESCAPED))
    assert old != cockatoo["1"][1]
    refused(cli, old, tmp_path, "must have exactly one type")


def test_field_7_on_a_literal_block_is_refused(cli, cockatoo, tmp_path):
    first = [True]

    def mark(b):
        if dmg.has(b, F_LITERAL) and first[0]:
            first[0] = False
            return b + [(F_ESCAPED, 0, 1)]
        return b
    refused(cli, rewritten(cockatoo["unset"][1], mark), tmp_path, "Invalid input block: escaped without cabac")
    # ... and on a coded block that does not say skip_coded = false
    refused(cli, rewritten(cockatoo["1"][1], lambda b: dmg.without(b, F_SKIP) if dmg.has(b, F_ESCAPED) else b), tmp_path,
            "Invalid input block: escaped without cabac")


def test_a_wrong_size_on_an_escaped_block_is_a_clean_error(cli, files, tmp_path):
    """Annex B has no length prefixes: a surrogate one byte longer is a NAL unit one byte longer, the parse goes through, and the block
    then escapes to a length that is not its size.  One error, nothing written."""
    data, _ = files["emulation"]
    src = tmp_path / "emulation.264"
    src.write_bytes(data)
    archive = compress(cli, src, tmp_path / "on.recode", ON)
    done = [False]

    def longer(b):
        if dmg.has(b, F_ESCAPED) and not done[0]:
            done[0] = True
            return dmg.replace(b, F_SIZE, dmg.get(b, F_SIZE) + 1)
        return b
    refused(cli, rewritten(archive, longer), tmp_path, "Escaped block restores to")
    assert done[0]


def python_escape(p, z):
    """The rule, written once more: a byte at a time."""
    s, out = z, bytearray()
    for b in p:
        if s == 2 and b <= 3:
            out.append(3)
            s = 0
        out.append(b)
        s = s + 1 if b == 0 else 0
    return bytes(out)


def test_escape_over_every_short_string(program, tmp_path):
    """host::escape over every string of length <= 8 over {0, 1, 3, 4, 0x80}, times z, in the sanitized program (which also holds
    h264::unescape to undo it): against the rule above and against the walker's escape() of the zeros and the string -- which
    knows no z and adds 7.4.1's 0x03 behind a final zero, not part of this rule."""
    out = tmp_path / "strings.bin"
    r = subprocess.run([program, "strings", str(out)], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0"),
                       timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok 1464843 cases"), r.stdout[-2000:] + r.stderr[-4000:]
    got, at, cases = out.read_bytes(), 0, 0
    for n in range(9):
        for code in range(5 ** n):
            p = bytes(finish_ref.ALPHABET[code // 5 ** j % 5] for j in range(n))
            for z in range(3):
                e = got[at + 1:at + 1 + got[at]]
                at += 1 + got[at]
                assert e == python_escape(p, z), (p.hex(), z)
                walker = hw.escape(bytes(z) + p)
                assert e == (walker[:-1] if (bytes(z) + p).endswith(b"\0") else walker)[z:], (p.hex(), z)
                cases += 1
    assert at == len(got) and cases == 1464843
