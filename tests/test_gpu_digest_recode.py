"""The optional digest of a .recode file on the device: the product command line held to the CPU stand-in (tests/cpu_batch.cpp: the
same host code, the oracle coding the batches), case by case -- exit status, message line, output bytes.

The digest itself is host code (csrc/host/avr_sha256.h), the same in both programs; what differs is what stands between the archive
and the bytes it is held to: K1 on the device here, the oracle's coder there.  `compress` with AVR_DIGEST=1 writes the stand-in's
bytes (tests/digest_recode.py's prefix in front), `decompress` and `check` take them back, a handful of the damaged-container
corpus behind the prefix ends as on the stand-in, and one `roundtrip` of the long clip runs with the digest and the K1 verifier
together.

One child process per run, under a time limit, as tests/test_gpu_damaged_recode.py does it: a run that ends by signal or at its
limit stops the module, and nothing more is started on the device behind it.
"""
import os
import subprocess

import pytest

import cpu_recode
import damaged_recode as dmg
import digest_recode as dig

pytestmark = pytest.mark.gpu

CASES = ("bits-mid-flip_byte0", "fields-last_byte_changed", "literal-pps", "structure-dropped", "structure-cut_0")
STOPPED = []


@pytest.fixture(scope="module")
def product(avr):
    return avr.build_recode()


@pytest.fixture(scope="module")
def stand_in():
    return cpu_recode.build_cached()


def started(what, run):
    """run() unless the module has stopped; a signal or the time limit stops it."""
    if STOPPED:
        pytest.skip("nothing more is started on the device: " + STOPPED[0])
    try:
        status, result = run()
    except subprocess.TimeoutExpired:
        STOPPED.append("%s reached its time limit" % what)
        raise
    if status not in (0, 1):
        STOPPED.append("%s ended with status %d" % (what, status))
        pytest.fail(STOPPED[0])
    return result


def environment(env):
    e = dict(os.environ, AVR_MODEL_HOOKS="0")
    for k in ("AVR_VERIFY", "AVR_VERIFY_K1", "AVR_VERIFY_RESTORE", "AVR_DEVICE_ESTIMATORS", "AVR_TIMING", "AVR_DIGEST"):
        e.pop(k, None)
    e.update(env or {})
    return e


def child(exe, command, src, dst, env=None):
    def run():
        p = subprocess.run([exe, command, str(src), str(dst)], capture_output=True, env=environment(env), timeout=cpu_recode.TIMEOUT)
        stderr = p.stderr.decode("utf-8", "replace")
        return p.returncode, (p.returncode, [l for l in stderr.splitlines() if l.startswith("Exception (")], stderr)
    return started("%s %s" % (os.path.basename(exe), command), run)


def check(exe, archive):
    def run():
        p = subprocess.run([exe, "check", str(archive)], capture_output=True, env=environment(None), timeout=cpu_recode.TIMEOUT)
        stderr = p.stderr.decode("utf-8", "replace")
        return p.returncode, (p.returncode, p.stdout.decode("utf-8", "replace"), [l for l in stderr.splitlines() if l.startswith("Exception (")])
    return started("%s check" % os.path.basename(exe), run)


@pytest.fixture(scope="module")
def sound(stand_in, tmp_path_factory):
    """realshort.mp4 through the stand-in, without and with the digest, and the corpus cases of the plain archive."""
    d = tmp_path_factory.mktemp("sound")
    src, made = os.path.join(cpu_recode.GOLDEN, "realshort.mp4"), {}
    for tag, env in (("plain", None), ("digest", {"AVR_DIGEST": "1"})):
        status, messages, stderr = child(stand_in, "compress", src, d / (tag + ".recode"), env)
        assert status == 0, stderr
        made[tag] = d / (tag + ".recode")
    original = cpu_recode.golden("realshort")
    assert made["digest"].read_bytes() == dig.prefix(original) + made["plain"].read_bytes()
    return dict(made, original=original, cases=dict(dmg.container_cases(made["plain"].read_bytes())))


def test_compress_on_the_device_writes_the_stand_ins_archive_and_takes_it_back(product, stand_in, sound, tmp_path):
    src = os.path.join(cpu_recode.GOLDEN, "realshort.mp4")
    status, messages, stderr = child(product, "compress", src, tmp_path / "product.recode", {"AVR_DIGEST": "1"})
    assert status == 0, stderr
    assert (tmp_path / "product.recode").read_bytes() == sound["digest"].read_bytes()
    for tag, exe in (("stand-in", stand_in), ("product", product)):
        back = tmp_path / (tag + ".back")
        status, messages, stderr = child(exe, "decompress", sound["digest"], back)
        assert (status, messages) == (0, []) and back.read_bytes() == sound["original"], (tag, stderr[-2000:])
        assert check(exe, sound["digest"]) == (0, "Digest OK: %d bytes\n" % len(sound["original"]), []), tag
        assert check(exe, sound["plain"]) == (1, "No digest in this archive: %d bytes restored, not checked\n" % len(sound["original"]), []), tag


@pytest.mark.parametrize("case", CASES)
def test_a_damaged_archive_with_a_digest_ends_on_the_device_as_on_the_stand_in(product, stand_in, sound, tmp_path, case):
    src = tmp_path / "damaged.recode"
    src.write_bytes(dig.prefix(sound["original"]) + sound["cases"][case])
    ends = {}
    for tag, exe in (("stand-in", stand_in), ("product", product)):
        dst = tmp_path / (tag + ".restored")
        status, messages, stderr = child(exe, "decompress", src, dst)
        assert len(messages) == (1 if status else 0) and (status == 0) == dst.exists(), (tag, stderr[-2000:])
        ends[tag] = (status, messages, dst.read_bytes() if status == 0 else None, check(exe, src))
        print(tag, "->", status, messages, ends[tag][3])
    assert ends["product"] == ends["stand-in"]
    if ends["product"][0] == 0:
        assert ends["product"][2] == sound["original"]
    if case in dig.SILENT[0]:
        assert ends["product"][0] == 1 and ends["product"][1][0].startswith(dig.EXCEPTION + "Verify error: restored file does not match the archive's digest (")


def test_roundtrip_of_the_long_clip_with_the_digest_and_the_k1_verifier(product, stand_in, tmp_path):
    src, original = os.path.join(cpu_recode.GOLDEN, "cockatoo.mp4"), cpu_recode.golden("cockatoo")
    status, messages, stderr = child(product, "roundtrip", src, tmp_path / "product.recode", {"AVR_DIGEST": "1", "AVR_VERIFY_K1": "1", "AVR_TIMING": "1"})
    assert (status, messages) == (0, []), stderr[-2000:]
    assert "Compress-decompress roundtrip succeeded:" in stderr and "[timing] decompress: digest" in stderr and "[timing] decompress: GPU verify (K1)" in stderr
    got = (tmp_path / "product.recode").read_bytes()
    assert got.startswith(dig.prefix(original))
    status, messages, stderr = child(stand_in, "compress", src, tmp_path / "stand-in.recode", {"AVR_DIGEST": "1"})
    assert status == 0 and got == (tmp_path / "stand-in.recode").read_bytes(), stderr[-2000:]
