"""GPU: the generated H.264 streams of tests/h264_corpus.py through the `recode` command line, and the walker's own record streams
-- true H.264 context structure over 1024 states -- through the batch API on both K1 paths."""
import os
import subprocess

import numpy as np
import pytest

import h264_corpus as corpus

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recode(avr):
    return avr.build_recode()


@pytest.fixture(scope="module")
def files(avr, oracle):
    from test_host import host as host_fixture
    host = host_fixture.__wrapped__(avr)
    host.t_init_states.restype = None
    return {name: corpus.build(name, oracle, host) for name in corpus.CASE_NAMES}


@pytest.mark.parametrize("name", corpus.CASE_NAMES)
def test_cli_round_trips_every_generated_file(recode, files, tmp_path, name):
    """`recode roundtrip` restores the file byte for byte with AVR_MODEL_HOOKS 0 and 1, and `recode compress` with
    AVR_DEVICE_ESTIMATORS=1 writes the same .recode bytes as without."""
    src = tmp_path / (name + ".264")
    src.write_bytes(files[name][0])
    for all_hooks in ("0", "1"):
        env = dict(os.environ, AVR_MODEL_HOOKS=all_hooks)
        comp, back = tmp_path / f"{name}.{all_hooks}.recode", tmp_path / f"{name}.{all_hooks}.back"
        out = subprocess.run([recode, "roundtrip", str(src), str(comp)], capture_output=True, text=True, timeout=300, env=env)
        assert out.returncode == 0 and "Compress-decompress roundtrip succeeded:" in out.stderr, out.stderr
        assert subprocess.run([recode, "decompress", str(comp), str(back)], timeout=300, env=env).returncode == 0
        assert back.read_bytes() == files[name][0]
    made = {}
    for on in ("0", "1"):
        out = tmp_path / f"{name}.est{on}.recode"
        run = subprocess.run([recode, "compress", str(src), str(out)], capture_output=True, text=True, timeout=300,
                             env=dict(os.environ, AVR_DEVICE_ESTIMATORS=on))
        assert run.returncode == 0, run.stderr
        made[on] = out.read_bytes()
    assert made["0"] == made["1"] and len(made["0"]) > 0


@pytest.mark.parametrize("path", [1, 2])
def test_walker_record_streams_through_the_batch_api(avr, oracle, hooks, files, path):
    """Every coded slice of the corpus as the walker logged it, with the parser's initial states: the device's bytes after
    drop_stop_byte + tail_patch are the payload the 9.3.4.2 encoder wrote, and the final states are the oracle's."""
    hooks(k1_path=path)
    slices = [e for name in corpus.CASE_NAMES for e in files[name][1] if e["fields"] is not None and not e.get("pcm")]
    assert len(slices) > 150 and max(len(set((e["log"] >> 1).tolist())) for e in slices) > 300
    with avr.Batch(0, len(slices), sum(len(e["log"]) for e in slices) + 64) as b:
        for e in slices:
            b.add_slice_cabac(e["log"], e["states"])
        b.run()
        assert b.run_info()["chunked"] == path - 1
        for i, e in enumerate(slices):
            got, st = b.get(i)
            want, final, _ = oracle.spec_cabac_encode(e["log"], e["states"])
            assert st == 0 and b.get_states(i) == final, f"{e['case']}: slice {i}"
            assert avr.tail_patch(avr.drop_stop_byte(got), len(e["payload"]) & 1, e["payload"][-1]) == e["payload"] == want, f"{e['case']}: slice {i}"
