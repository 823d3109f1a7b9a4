"""The product command line on the device against the CPU stand-in (tests/cpu_batch.cpp: the same host code, the oracle coding the
batches), on sound clips and on the damaged containers of tests/damaged_recode.py.

The stand-in is the plain reference of the whole command (every route of it: tests/test_gpu_cli_verify_faults.py holds the verify
switches to it); here, of the decompress direction on damaged input: `compress` must write the same .recode bytes on both (both clips, both
hook settings -- which is also what proves the stand-in codes what the device codes), and on every damaged container `decompress`
must end the same way on both: exit status, message line, and the output's bytes when the status is 0.  Once more with
AVR_VERIFY_K1=1 on the product only: the verifier decodes what K1 coded from the recorder's codes, so it finds nothing in a run the
plain one accepted, and the outcome is the same.

These inputs are not meant to fault anything: the device only ever sees code bytes that decompress_recorder wrote, and its worst
case, a bin behind a put_terminate(1), is a status the kernels return (tests/test_gpu_bad_records.py).  All the same, one child
process per case under a time limit, and a case that ends by signal or at its limit stops the module: nothing more is started on the
device behind it.  The stand-in is built here without sanitizers; everything is generated on the machine that runs the test.
"""
import os
import subprocess

import pytest

import cpu_recode
import damaged_recode as dmg

pytestmark = pytest.mark.gpu

# The container cases that tests/test_damaged_recode.py found to end within its limit on the CPU: all of them.  A case that did not
# would be named here with the reason, and not run on the device.
LEFT_OUT = {}
CASES = [n for n in dmg.CONTAINER_CASE_NAMES if n not in LEFT_OUT]
STOPPED = []


@pytest.fixture(scope="module")
def product(avr):
    return avr.build_recode()


@pytest.fixture(scope="module")
def stand_in():
    return cpu_recode.build_cached()


def child(exe, command, src, dst, model_hooks, env=None):
    if STOPPED:
        pytest.skip("nothing more is started on the device: " + STOPPED[0])
    try:
        o = cpu_recode.run(exe, command, src, dst, model_hooks, env=env)
    except subprocess.TimeoutExpired:
        STOPPED.append("%s %s reached its time limit" % (os.path.basename(exe), command))
        raise
    if o.status not in (0, 1):
        STOPPED.append("%s %s ended with status %d" % (os.path.basename(exe), command, o.status))
        pytest.fail(STOPPED[0] + "\n" + o.stderr[-3000:])
    return o


@pytest.fixture(scope="module")
def sound(stand_in, tmp_path_factory):
    """The sound container of realshort.mp4 per hooks setting, written by the stand-in, and its damaged variants."""
    d, made = tmp_path_factory.mktemp("sound"), {}

    def get(model_hooks):
        if model_hooks not in made:
            dst = d / ("realshort.%d.recode" % model_hooks)
            o = child(stand_in, "compress", os.path.join(cpu_recode.GOLDEN, "realshort.mp4"), dst, model_hooks)
            assert o.status == 0, o.stderr
            made[model_hooks] = dict(dmg.container_cases(dst.read_bytes()))
        return made[model_hooks]
    return get


@pytest.mark.parametrize("model_hooks", (0, 1))
@pytest.mark.parametrize("clip", ("realshort", "cockatoo"))
def test_compress_on_the_device_writes_the_stand_ins_bytes(product, stand_in, tmp_path, clip, model_hooks):
    src, files = os.path.join(cpu_recode.GOLDEN, clip + ".mp4"), {}
    for tag, exe in (("stand-in", stand_in), ("product", product)):
        o = child(exe, "compress", src, tmp_path / tag, model_hooks)
        assert o.status == 0, o.stderr
        files[tag] = (tmp_path / tag).read_bytes()
    assert len(files["product"]) > 0 and files["product"] == files["stand-in"]
    back = tmp_path / "back"                             # and the device restores what the stand-in wrote
    assert child(product, "decompress", tmp_path / "stand-in", back, model_hooks).status == 0 and back.read_bytes() == cpu_recode.golden(clip)


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("model_hooks", (0, 1))
def test_decompress_on_the_device_ends_as_the_stand_in_does(product, stand_in, sound, tmp_path, model_hooks, case):
    src = tmp_path / "damaged.recode"
    src.write_bytes(sound(model_hooks)[case])
    ends = {}
    for k, (tag, exe, env) in enumerate((("stand-in", stand_in, None), ("product", product, None), ("product, AVR_VERIFY_K1=1", product, {"AVR_VERIFY_K1": "1"}))):
        dst = tmp_path / ("restored.%d" % k)
        o = child(exe, "decompress", src, dst, model_hooks, env=env)
        assert len(o.messages) == (1 if o.status else 0) and (o.status == 0) == dst.exists(), (tag, o.stderr[-2000:])
        ends[tag] = (o.status, o.messages, dst.read_bytes() if o.status == 0 else None)
        print(tag, "->", o.status, o.messages)
    assert ends["product"] == ends["stand-in"]
    assert ends["product, AVR_VERIFY_K1=1"] == ends["stand-in"]
    if case in dmg.MUST_RESTORE:
        assert ends["product"] == (0, [], cpu_recode.golden("realshort"))
