"""Phase B1 as the kernels walk it, on the CPU: B1Walk of avrecode-ms_amd/csrc/avr_k1p.h -- what a lane of k_k1p_replay and k_k1p_b1
runs, eight bins at a time: the merged step, the branch-free candidate step, the opening group, the tail past the chunk, and the
bin-by-bin form left for what is rare -- compiled for the host by tests/b1walk_emul.cpp, a stand-alone program built with
AddressSanitizer and UBSan, and held to b1_stretch, the CPU's statement of a chunk's stretch summary: first, end, exit_q, t_exit[4],
r_exit[4] and too_long are equal for every chunk of every stream, walked as a lane alone and as a lane beside one that is still
looking.  A child process with this one's environment as it is: nothing sanitised is loaded into this process.

The streams are those of tests/b1walk_streams.py, where the coded LPS bins are placed bin by bin; what the program reports about
each stream's middle chunk is held to what the stream was made for, so that a stream that stopped covering its case fails here."""
import os
import struct
import subprocess

import pytest

import b1walk_streams as bs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "avrecode-ms_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "b1walk_emul.cpp")
BIN = os.path.join(ROOT, "tests", "_b1walk_emul")
DEPS = [os.path.join(CSRC, h) for h in ("avr_k1p.h", "avr_chunk.h", "avr_tables.h")]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0")
CHUNK, NONE = bs.CHUNK, 0xFFFFFFFF


@pytest.fixture(scope="module")
def program():
    if not os.path.exists(BIN) or any(os.path.getmtime(s) > os.path.getmtime(BIN) for s in [SRC] + DEPS):
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I" + CSRC, "-o", BIN, SRC], check=True)
    return BIN


@pytest.fixture(scope="module")
def tables(avr):
    lps_range, mlps = avr.cabac_tables()
    return list(lps_range), list(mlps)


def walk(program, tmp_path, tables, streams):
    """Every chunk of every stream through the program; {name: (chunks, first, end, meet, too_long) of the middle chunk}."""
    path = tmp_path / "streams.bin"
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(streams)))
        for s in streams:
            _, codes = s.resolve(tables[1])
            f.write(struct.pack("<II", codes.size, s.max_stretch) + codes.tobytes())
    r = subprocess.run([program, str(path)], capture_output=True, text=True, env=ENV, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.split("\n")
    assert lines[len(streams)].startswith("ok ")
    assert int(lines[len(streams)].split()[1]) == 2 * sum(-(-s.syms.size // CHUNK) for s in streams)
    seen = {}
    for s, line in zip(streams, lines):
        w = line.split()
        seen[s.name] = tuple(int(x) if x != "-" else None for x in w[1:])
    return seen


def test_constructed_streams(program, tmp_path, tables):
    streams = bs.constructed(*tables)
    seen = walk(program, tmp_path, tables, streams)
    n = 3 * CHUNK
    for later in (0, 1):
        for j in range(8):
            opens, closes = 40 * later + j, 24 * later + 7 - j
            assert seen[f"open{opens}-close{closes}"][:3] == (3, CHUNK + opens, 2 * CHUNK + closes + 1)
    assert seen["no-lps-in-chunk"][1] == NONE
    assert seen["never-closes"][1:3] == (CHUNK + 3, n) and seen["never-closes"][4] == 0
    assert seen["closes-with-the-slice"][1:3] == (CHUNK + 3, n) and seen["closes-with-the-slice"][4] == 0
    for ms in (100, CHUNK - 1, CHUNK, CHUNK + 3, 1500, 2 * CHUNK - 5):
        assert seen[f"too-long-{ms}"][2] == CHUNK + max(ms + 1, CHUNK) + 1 and seen[f"too-long-{ms}"][4] == 1
    assert seen["closes-before-too-long"][2] == 2 * CHUNK + 6 and seen["closes-before-too-long"][4] == 0
    assert seen["closes-at-too-long"][2] == 2 * CHUNK + 6 and seen["closes-at-too-long"][4] == 0
    first, end, meet = seen["never-meet"][1:4]
    assert (first, end) == (CHUNK + 21, 2 * CHUNK + 12) and (meet == NONE or meet >= end - 1)        # four candidates at the closing bin
    for opens in (16, 50):
        first, _, meet = seen[f"meet-in-group-{opens}"][1:4]
        assert first == CHUNK + opens and meet <= (first | 7)
    for name in ("bypass", "terminate"):
        for opens, closes in ((4, 3), (8, 7), (15, 0)):
            assert seen[f"between-{name}-{opens}-{closes}"][1:3] == (CHUNK + opens, 2 * CHUNK + closes + 1)
    assert seen["closes-in-partial-group"][1:3] == (2 * CHUNK - 24, 3 * CHUNK - 7)
    assert seen["opens-at-last-bin"][1:3] == (2 * CHUNK - 1, 3 * CHUNK - 5)
    assert seen["short-second-chunk"][:3] == (2, CHUNK + 2, CHUNK + 9)
    assert seen["five-bins"][0] == 1 and seen["one-bin"][0] == 1
    # among the streams whose candidates were left to chance: some meet inside the chunk and behind the opening group
    meets = [seen[f"open{40 * later + j}-close{24 * later + 7 - j}"] for later in (0, 1) for j in range(8)]
    assert any((first | 7) < meet < 2 * CHUNK for _, first, _, meet, _ in meets)


@pytest.mark.parametrize("rate", [0.02, 0.12, 0.40])
def test_random_streams(program, tmp_path, tables, rate):
    """Coded LPS bins at 2 %, 12 % and 40 % of the bins: openings late and at once, candidates on four ranges for long and not at all."""
    streams = bs.random_streams(seed=int(rate * 1000), per_rate=24, rates=(rate,))
    walk(program, tmp_path, tables, streams)


def test_the_wave_mixing_slices(program, tmp_path, tables):
    """The 64 slices the device test codes as one batch; every eighth one opens its chunks at bin 300 or later."""
    streams = bs.wave_mix()
    seen = walk(program, tmp_path, tables, streams)
    for i in range(7, 64, 8):
        chunks, first = seen[f"mix-{i}"][:2]
        assert chunks == 1 or first == NONE or first >= CHUNK + 300
