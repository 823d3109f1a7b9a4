"""Escaped blocks on the device: the product command line with `AVR_ESCAPED=1` held to the CPU stand-in (tests/cpu_batch.cpp: the
same host code, the oracle coding the batches) on cockatoo.mp4 -- 13 of its 280 slices carry an escape -- and on the generated
`emulation` case of tests/h264_corpus.py: `compress` writes the stand-in's archive byte for byte, `decompress`, `roundtrip` and
`test <dir>` bring the files back, once with every verifier on.

One child process per run, under a time limit, as tests/test_gpu_digest_recode.py does it: a run that ends by signal or at its limit
stops the module, and nothing more is started on the device behind it."""
import os
import shutil
import subprocess

import pytest

import cpu_recode
import h264_corpus as corpus
from test_escaped_recode import kinds
from test_gpu_digest_recode import child, environment, started

pytestmark = pytest.mark.gpu

ON = {"AVR_ESCAPED": "1"}
VERIFIED = dict(ON, AVR_VERIFY="1", AVR_VERIFY_K1="1", AVR_VERIFY_RESTORE="1")


@pytest.fixture(scope="module")
def product(avr):
    return avr.build_recode()


@pytest.fixture(scope="module")
def stand_in():
    return cpu_recode.build_cached()


@pytest.fixture(scope="module")
def clips(oracle, avr, tmp_path_factory):
    """name -> (path, bytes): the golden clip, and the generated case as an Annex B file."""
    from test_host import host as host_fixture
    host = host_fixture.__wrapped__(avr)
    host.t_init_states.restype = None
    d = tmp_path_factory.mktemp("clips")
    data, _ = corpus.build("emulation", oracle, host)
    (d / "emulation.264").write_bytes(data)
    return {"cockatoo": (os.path.join(cpu_recode.GOLDEN, "cockatoo.mp4"), cpu_recode.golden("cockatoo")), "emulation": (str(d / "emulation.264"), data)}


@pytest.fixture(scope="module")
def expected(stand_in, clips, tmp_path_factory):
    """name -> the stand-in's archive with the switch."""
    d, out = tmp_path_factory.mktemp("expected"), {}
    for name, (src, _) in clips.items():
        status, messages, stderr = child(stand_in, "compress", src, d / (name + ".recode"), ON)
        assert status == 0, stderr[-2000:]
        out[name] = (d / (name + ".recode")).read_bytes()
    assert kinds(out["cockatoo"]) == (280, 13, 0) and kinds(out["emulation"])[1] >= 2
    return out


@pytest.mark.parametrize("name", ["cockatoo", "emulation"])
def test_compress_and_decompress(product, clips, expected, tmp_path, name):
    src, original = clips[name]
    status, messages, stderr = child(product, "compress", src, tmp_path / "product.recode", ON)
    assert (status, messages) == (0, []), stderr[-2000:]
    assert (tmp_path / "product.recode").read_bytes() == expected[name]
    status, messages, stderr = child(product, "decompress", tmp_path / "product.recode", tmp_path / "back.bin")
    assert (status, messages) == (0, []) and (tmp_path / "back.bin").read_bytes() == original, stderr[-2000:]


@pytest.mark.parametrize("name", ["cockatoo", "emulation"])
def test_roundtrip_with_every_verifier(product, clips, expected, tmp_path, name):
    src, _ = clips[name]
    status, messages, stderr = child(product, "roundtrip", src, tmp_path / "product.recode", VERIFIED)
    assert (status, messages) == (0, []) and "Compress-decompress roundtrip succeeded:" in stderr, stderr[-2000:]
    assert (tmp_path / "product.recode").read_bytes() == expected[name]


def test_test_dir_over_both(product, clips, expected, tmp_path):
    d = tmp_path / "clips"
    d.mkdir()
    names = {}
    for name, (src, _) in clips.items():
        names[os.path.basename(src)] = name
        shutil.copy(src, d / os.path.basename(src))

    def run():
        e = environment(ON)
        for k in ("AVR_TEST_WINDOW", "AVR_TEST_SEQUENTIAL"):
            e.pop(k, None)
        p = subprocess.run([product, "test", str(d)], capture_output=True, text=True, env=e, timeout=4 * cpu_recode.TIMEOUT)
        return p.returncode, p
    p = started("recode test", run)
    assert p.returncode == 0 and "failed on" not in p.stdout, p.stdout + p.stderr[-2000:]
    log = (d / "output" / "log.txt").read_text()
    assert log.count("Compress-decompress roundtrip succeeded:") == len(names) and "Exception (" not in log
    for file, name in names.items():
        assert (d / "output" / file).read_bytes() == expected[name], file
