"""f4: the bin-stream source without FFmpeg (avrecode-ms_amd/csrc/host/avr_h264.h) and the `recode` command line on top of it.

The real-stream fixtures are two CABAC H.264 MP4s from imageio's standard images, kept in tests/golden/:
    realshort.mp4   High profile 4:2:0, 8x8 transform, I / P slices, 36 slices of 300 macroblocks
    cockatoo.mp4    High 4:4:4 Predictive (x264 build 142), weighted prediction, 3-4 references, I / P / B slices,
                    280 slices of 3600 macroblocks

What parsing them to the end pins: the slice-data syntax and every context derivation of the parser, and -- because a wrong
(m, n) of a context a stream uses derails the arithmetic decoder within a few bins -- the initialisation values typed
into avr_h264_tables.h for the contexts these streams use (I slices and cabac_init_idc 0), and with them, once more, the
rangeTabLPS / transIdx tables of avr_tables.h against streams made by real encoders.
"""
import json
import os
import shutil
import subprocess

import pytest

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CLIPS = {"realshort.mp4": (36, 300), "cockatoo.mp4": (280, 3600)}


@pytest.fixture(scope="module")
def recode(avr):
    return avr.build_recode()


def clip(name):
    return os.path.join(GOLD, name)


@pytest.mark.parametrize("name", sorted(CLIPS))
def test_every_slice_of_the_real_streams_parses_to_its_end(recode, name):
    """Each slice must end on end_of_slice_flag = 1 at its last macroblock, with the arithmetic decoder having pulled in
    exactly the bits up to the rbsp_stop_one_bit in the payload's last byte (h264_stream_decoder::payload_decodes)."""
    out = subprocess.run([recode, "probe", clip(name)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    res = json.loads(out.stdout)
    assert res == {"slices": CLIPS[name][0], "parse_to_the_end": CLIPS[name][0], "fail": 0, "unsupported": 0, "header_failures": 0,
                   "literal_reasons": {}}, out.stderr


from stream_records import stream_records as _stream_records  # noqa: E402  (other test files import it from here)


@pytest.mark.parametrize("name", sorted(CLIPS))
def test_real_streams_round_trip_through_the_model_with_all_eleven_hooks(avr, oracle, name):
    """Rows a13 / f3 end to end on real streams, on the CPU: the build's syntax parser drives the hook table over the clip with
    (a) frame_spec / mb_xy only, as the reference's fork is annotated, and (b) all eleven hooks (begin / end_sub_mb and
    PIP_SIGNIFICANCE_MAP around every residual block: h264_stream_decoder::residual_hooks).  Compress recorder -> K2 records ->
    the reference's range coder (oracle) -> decompress recorder answering the same parser's bin requests from those bytes -> K1
    records -> cabac::encoder (oracle) -> drop-0x80 + tail patch must give back every slice's payload bit for bit, in both modes;
    a slice with a block whose nonzero count does not fit the reference's 2 / 4 / 6-bit field stays literal (realshort: 4 of 36).
    What the significance-map model buys is reported, not demanded: 2.1 % fewer bytes on realshort.mp4 (4:2:0, I / P), 0.3 % MORE
    on cockatoo.mp4 (4:4:4, B frames) -- the reference's own verdict on this model is "FIXME: why doesn't this prior help at all"
    (recode.cpp:793, :811)."""
    from test_host import host as host_fixture
    host = host_fixture.__wrapped__(avr)
    data = open(clip(name), "rb").read()
    totals = {}
    for residual in (0, 1):
        k2, payloads, offered = _stream_records(host, data, residual, 0)
        assert len(offered) == CLIPS[name][0] and len(k2) == int(offered.sum())
        if not residual:
            assert len(k2) == CLIPS[name][0]
        else:                                                # slices with a block whose count does not fit the reference's field stay literal
            assert len(k2) >= 0.5 * CLIPS[name][0], (len(k2), CLIPS[name][0])
        recoded = []
        for r in k2:
            coded, st = oracle.range_encode(r)
            assert st == 0
            recoded.append(coded)
        k1, first_states = _stream_records(host, data, residual, 1, recoded, offered)
        assert len(k1) == len(k2)
        for i, (r, states) in enumerate(zip(k1, first_states)):
            raw, _, st = oracle.cabac_encode(r, states)
            assert st == 0
            back = oracle.tail_patch(oracle.drop_stop_byte(raw), len(payloads[i]) & 1, payloads[i][-1])     # recode.cpp:1508-1512, 1354-1360
            assert back == payloads[i], f"{name} slice {i} residual_hooks={residual}"
        totals[residual] = (sum(len(x) for x in recoded), sum(len(x) for x in payloads), sum(len(r) for r in k2), len(k2))
    print(name, "(recoded bytes, payload bytes, K2 records, slices hooked) by residual_hooks:", totals)
    # what the significance-map model buys, on the slices it coded: recoded / payload bytes, within a percent or two either way
    gain = totals[0][0] / totals[0][1] - totals[1][0] / totals[1][1]
    assert -0.01 < gain < 0.05, totals
    if name == "realshort.mp4":
        assert gain > 0.01, totals


def test_cli_surface(recode, tmp_path):
    """recode.cpp:1646-1675: usage and unknown commands exit 1 with the reference's messages; a file without any H.264 in it
    needs no GPU (nothing to code) and round-trips as one literal block."""
    out = subprocess.run([recode], capture_output=True, text=True)
    assert out.returncode == 1 and "[compress|decompress|roundtrip|test] <input> [output]" in out.stderr
    out = subprocess.run([recode, "frobnicate", "x"], capture_output=True, text=True)
    assert out.returncode == 1 and "Unknown command: frobnicate" in out.stderr and out.stderr.startswith("Exception (")
    out = subprocess.run([recode, "compress", str(tmp_path / "missing")], capture_output=True, text=True)
    assert out.returncode == 1 and "Exception (" in out.stderr
    plain = tmp_path / "plain.bin"
    plain.write_bytes(bytes(range(256)) * 40)
    comp, back = tmp_path / "plain.recode", tmp_path / "plain.out"
    assert subprocess.run([recode, "compress", str(plain), str(comp)]).returncode == 0
    assert subprocess.run([recode, "decompress", str(comp), str(back)]).returncode == 0
    assert back.read_bytes() == plain.read_bytes()
    out = subprocess.run([recode, "roundtrip", str(plain)], capture_output=True, text=True)
    assert out.returncode == 0 and "Compress-decompress roundtrip succeeded:" in out.stderr and " compression ratio: " in out.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("all_hooks", [0, 1])
@pytest.mark.parametrize("name", sorted(CLIPS))
def test_roundtrip_of_a_real_file(recode, tmp_path, name, all_hooks):
    """BASELINE.json configs[0] (`./recode roundtrip <clip>`, README.md:24) on the clips this image has: compress (syntax parser
    -> eleven hooks -> K2 on the GPU), decompress (K3 on the CPU, K1 on the GPU from resolved codes), byte-compare.
    all_hooks = 1 (AVR_MODEL_HOOKS=1): begin / end_sub_mb and begin / end_coding_type fire too -- h264_model's significance-map
    keys, the recorders' queueing and the nonzero counts sent ahead are live on the product path (rows a13 / f3)."""
    src = clip(name)
    comp = tmp_path / (name + ".recode")
    env = dict(os.environ, AVR_MODEL_HOOKS=str(all_hooks))
    out = subprocess.run([recode, "roundtrip", src, str(comp)], capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0, out.stderr
    assert "Compress-decompress roundtrip succeeded:" in out.stderr
    # With frame_spec / mb_xy the only model hooks firing (what the reference's source says of its FFmpeg fork, recode.cpp:173-215)
    # the model is one adaptive {pos, neg} estimator per context: about CABAC's own efficiency, plus the container's framing.
    ratio = float(out.stderr.split("compression ratio: ")[1].split("%")[0])
    assert 90.0 < ratio < 102.0, out.stderr
    # the two halves on their own, through files
    back = tmp_path / (name + ".back")
    assert subprocess.run([recode, "decompress", str(comp), str(back)], timeout=600, env=env).returncode == 0
    assert back.read_bytes() == open(src, "rb").read()
    # the container holds one coded block per slice the compressor could place (unescaped payloads are found in the file)
    import avrecode_ms_amd  # noqa: F401  (path set-up)
    from test_host import recoded_message_classes
    msg = recoded_message_classes()()
    msg.ParseFromString(comp.read_bytes())
    coded = sum(1 for b in msg.block if b.HasField("cabac"))
    skipped = sum(1 for b in msg.block if b.HasField("skip_coded"))
    assert coded + skipped == CLIPS[name][0] and coded >= 0.8 * CLIPS[name][0]


@pytest.mark.gpu
def test_recode_test_directory(recode, tmp_path):
    """`recode test <dir>` (test.cpp:113-148): every regular file round-trips, output/ gets the compressed files, the log and
    metrics.csv with the reference's columns (test.cpp:32)."""
    for name in CLIPS:
        shutil.copy(clip(name), tmp_path / name)
    out = subprocess.run([recode, "test", str(tmp_path)], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr
    assert "failed on" not in out.stdout
    rows = (tmp_path / "output" / "metrics.csv").read_text().strip().splitlines()
    assert rows[0].startswith("File,Duration,Initial size (MB),Compressed size (MB),Compression rate (%),Space saving (%),Total time (ms)")
    assert len(rows) == 1 + len(CLIPS)
    log = (tmp_path / "output" / "log.txt").read_text()
    assert log.count("Compress-decompress roundtrip succeeded:") == len(CLIPS)
    for name in CLIPS:
        assert (tmp_path / "output" / name).stat().st_size > 0


@pytest.mark.gpu
def test_recode_test_directory_batches_across_files(recode, tmp_path):
    """`recode test <dir>` over a directory of 16 copies of each of the image's two clips: the files of the directory go through the two
    directions together -- host sides one file per thread, the slices of ALL files in one GPU batch per direction (K2 in, K1 out) -- and
    write exactly the files the reference's loop writes (AVR_TEST_SEQUENTIAL=1: a file at a time, a batch per file and direction, as
    rounds 1-3 ran it); every output file decompresses back to its clip.  The two wall times go to gpurun_out/ (profiles/r04_cli_timing.txt)."""
    import time
    a, b = tmp_path / "batched", tmp_path / "sequential"
    for d in (a, b):
        d.mkdir()
        for k in range(16):
            for name in CLIPS:
                shutil.copy(clip(name), d / f"{k:02d}_{name}")
    t0 = time.perf_counter()
    out = subprocess.run([recode, "test", str(a)], capture_output=True, text=True, timeout=1800)
    t_batched = time.perf_counter() - t0
    assert out.returncode == 0 and "failed on" not in out.stdout, out.stderr + out.stdout
    t0 = time.perf_counter()
    seq = subprocess.run([recode, "test", str(b)], capture_output=True, text=True, timeout=1800, env=dict(os.environ, AVR_TEST_SEQUENTIAL="1"))
    t_seq = time.perf_counter() - t0
    assert seq.returncode == 0 and "failed on" not in seq.stdout, seq.stderr + seq.stdout
    names = sorted(p.name for p in a.iterdir() if p.is_file())
    assert len(names) == 16 * len(CLIPS)
    for name in names:
        got, want = (a / "output" / name).read_bytes(), (b / "output" / name).read_bytes()
        assert got == want and len(got) > 0, name
    for name in names[:2] + names[-2:]:                      # ... and they are what `recode decompress` turns back into the clip
        back = subprocess.run([recode, "decompress", str(a / "output" / name)], capture_output=True, timeout=600)
        assert back.returncode == 0 and back.stdout == (a / name).read_bytes(), name
    rows = (a / "output" / "metrics.csv").read_text().strip().splitlines()
    assert len(rows) == 1 + len(names)
    assert (a / "output" / "log.txt").read_text().count("Compress-decompress roundtrip succeeded:") == len(names)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if os.path.isdir(os.path.join(root, "gpurun_out")):
        with open(os.path.join(root, "gpurun_out", "cli_directory_timing.txt"), "w") as f:
            f.write(f"recode test <dir>, {len(names)} files ({sum((a / n).stat().st_size for n in names)} bytes): "
                    f"batched across files {t_batched:.2f} s, a file at a time {t_seq:.2f} s, ratio {t_seq / t_batched:.2f}\n")
    assert t_batched < t_seq
