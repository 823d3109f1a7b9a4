"""`recode decompress` on .recode files that are not the ones `compress` wrote, and `compress` on damaged MP4s: on the CPU, under
AddressSanitizer and UBSan, with the oracle coding the batches (tests/cpu_batch.cpp) in place of the device.

In this direction every step is driven by data from the file: the host range decoder (K3), the adaptive model, decompress_recorder,
and from its bins the H.264 slice-data parser, whose records K1 then codes.  The container carries no checksum (the format is the
reference's), so damage ends in one of two ways and no third: a clean error -- exit status 1, one `Exception (...)` line, nothing
written -- or exit status 0 with a file that may differ from the original.  Never a signal, a sanitizer report or a hang.

The corpus is tests/damaged_recode.py: every case on realshort.mp4 (36 slices) with AVR_MODEL_HOOKS 0 and 1, one case per family on
cockatoo.mp4.  What it found when it was written, each fixed in csrc/host:
  * every case that throws inside a slice (most of the `bits`, `length` and `literal` families): ~cabac_decoder pushed into its
    owner's pending_ after that vector had been destroyed -- heap use after free in ~decompressor.  tests/unwind_check.cpp is the same
    unwind without the command line, in both classes.
  * fields-size_2p31 .. 2p64m1 (and 2p31m1): open_block allocated a surrogate of the size the file asked for.
  * any case that ends in an exception: main had opened (and so emptied or created) the output path before it knew.
AVR_DAMAGED_RECORD=<path>: the outcomes seen, one row per case and hooks setting, as JSON (profiles/damaged_recode.json is such a run).
"""
import json
import os
import subprocess

import numpy as np
import pytest

import cpu_recode
import damaged_recode as dmg
import oracle_lib

CLIPS = ("realshort", "cockatoo")
SEL_BYPASS, SEL_TERMINATE = 1024, 1025
ROWS = []


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    """The stand-in command line, twice: with ASan + UBSan (what the corpus runs on) and plain (for the address-space limit, which a
    sanitized program cannot carry).  Also the sound containers, made once by the sanitized build, and how long their decompress
    takes on it (the unit of the recorded wall times)."""
    d = tmp_path_factory.mktemp("cpu_recode")

    class Cli:
        asan = cpu_recode.build(d, sanitize=True)
        plain = cpu_recode.build(d, sanitize=False)
        work = d
        _sound = {}

        def sound(self, clip, model_hooks):
            key = (clip, model_hooks)
            if key not in self._sound:
                src, dst, back = os.path.join(cpu_recode.GOLDEN, clip + ".mp4"), d / ("%s.%d.recode" % key), d / ("%s.%d.back" % key)
                c = cpu_recode.run(self.asan, "compress", src, dst, model_hooks)
                assert c.status == 0 and "AddressSanitizer" not in c.stderr and "runtime error" not in c.stderr, c.stderr[-2000:]
                r = cpu_recode.run(self.asan, "decompress", dst, back, model_hooks)
                assert r.status == 0 and "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-2000:]
                container = dst.read_bytes()
                self._sound[key] = dict(container=container, restored=back.read_bytes(), seconds=r.seconds, pending=r.pending,
                                        cases=dict(dmg.container_cases(container)))
            return self._sound[key]

    yield Cli()
    path = os.environ.get("AVR_DAMAGED_RECORD")
    if path:
        with open(path, "w") as f:
            json.dump({"unit": "wall time of decompress on the sound container, same build (ASan + UBSan), same clip and hooks setting", "rows": ROWS},
                      f, indent=1)


def clean(outcome):
    """Rule 1: exit status 0, or 1 with exactly one `Exception (` line; never a signal; no sanitizer report."""
    assert "AddressSanitizer" not in outcome.stderr and "runtime error" not in outcome.stderr, outcome.stderr[-3000:]
    assert outcome.status in (0, 1), "ended with status %d\n%s" % (outcome.status, outcome.stderr[-2000:])
    assert len(outcome.messages) == (1 if outcome.status else 0), outcome.stderr[-2000:]


def record(case, clip, model_hooks, outcome, dst, unit):
    ROWS.append(dict(case=case, clip=clip, model_hooks=model_hooks, status=outcome.status, message=outcome.messages[0] if outcome.messages else None,
                     sha256=cpu_recode.digest(dst) if outcome.status == 0 else None, wall_ratio=round(outcome.seconds / unit, 2), pending=outcome.pending))


# ------------------------------------------------------------------------------------------------ the stand-in is sound
def codes_of(recs, states, mlps_state):
    """The resolved codes of a record stream: what decompress_recorder writes beside its records (AVR_CODE_* of the header)."""
    st, codes = list(states), []
    for r in recs.tolist():
        b, sel = r & 1, r >> 1
        if sel == SEL_BYPASS:
            codes.append(252 | b)
        elif sel == SEL_TERMINATE:
            codes.append(255 - b)
        else:
            s = st[sel]
            codes.append(255 - ((b ^ s) & 1) if s >= 126 else (s << 1) | b)
            st[sel] = mlps_state[127 - s] if b != (s & 1) else mlps_state[128 + s]
    return np.array(codes, dtype=np.uint8)


def encode_codes(oracle, codes):
    import ctypes
    out = np.zeros(2 * codes.size + 64, np.uint8)
    status = ctypes.c_int(0)
    oracle.L.avr_oracle_cabac_encode_codes.restype = ctypes.c_size_t
    n = oracle.L.avr_oracle_cabac_encode_codes(oracle_lib.ptr(codes), ctypes.c_size_t(codes.size), oracle_lib.ptr(out), ctypes.c_size_t(out.size),
                                               ctypes.byref(status))
    return out[:n].tobytes(), status.value


@pytest.mark.parametrize("seed", range(6))
def test_the_coder_from_codes_is_the_coder_from_records(oracle, seed):
    """oracle/avr_oracle.c: avr_oracle_cabac_encode_codes against avr_oracle_cabac_encode on random streams (contexts in every state a
    slice can hold, 0 .. 125; bypass and terminate bins; with and without the closing put_terminate(1); the empty stream)."""
    rng = np.random.default_rng(seed)
    mlps = oracle.tables()[1]
    for n in (0, 1, 7, 300, 5000):
        n_states = int(rng.integers(1, 400))
        states = rng.integers(0, 126, n_states).astype(np.uint8)
        sel = rng.integers(0, n_states, n)
        kind = rng.random(n)
        sel[kind < 0.25] = SEL_BYPASS
        sel[kind < 0.03] = SEL_TERMINATE
        bins = (rng.random(n) < rng.choice([0.1, 0.5, 0.9])).astype(np.int64)
        bins[sel == SEL_TERMINATE] = 0
        recs = (bins | sel << 1).astype(np.uint16)
        for closing in ([], [1 | SEL_TERMINATE << 1]):
            r = np.concatenate([recs, np.array(closing, np.uint16)])
            want, _, status = oracle.cabac_encode(r, states, cap=2 * r.size + 64)
            assert (want, status) == encode_codes(oracle, codes_of(r, states, mlps)), (seed, n, closing)
    # a bin behind put_terminate(1): the status of the records coder (and of the device)
    r = np.array([2, 1 | SEL_TERMINATE << 1, 3], np.uint16)
    assert oracle.cabac_encode(r, np.zeros(4, np.uint8))[2] == encode_codes(oracle, codes_of(r, [0] * 4, mlps))[1] == 3


@pytest.mark.parametrize("model_hooks", (0, 1))
@pytest.mark.parametrize("clip", CLIPS)
def test_the_stand_in_restores_the_clip_and_its_container_reads_back(cli, clip, model_hooks):
    s = cli.sound(clip, model_hooks)
    assert s["restored"] == cpu_recode.golden(clip)
    blocks = dmg.parse(s["container"])                   # the reader of the damage module, independent of the C++ one
    assert dmg.serialise(blocks) == s["container"]
    assert len(dmg.coded_blocks(blocks)) >= 3 and s["pending"].startswith("%d slices" % len(dmg.coded_blocks(blocks)))


# ------------------------------------------------------------------------------------------------ damaged containers
def damaged_container(cli, tmp_path, clip, model_hooks, case):
    s = cli.sound(clip, model_hooks)
    src, dst = tmp_path / "damaged.recode", tmp_path / "restored.mp4"
    src.write_bytes(s["cases"][case])
    o = cpu_recode.run(cli.asan, "decompress", src, dst, model_hooks)
    print(case, clip, model_hooks, "->", o.status, o.messages, "%.2f x the sound file" % (o.seconds / s["seconds"]), o.pending)
    clean(o)
    if o.status:
        assert not dst.exists(), "an output file beside exit status 1"                      # rule 2
    record(case, clip, model_hooks, o, dst, s["seconds"])
    if case in dmg.MUST_RESTORE:                                                                # rule 3
        assert o.status == 0 and dst.read_bytes() == cpu_recode.golden(clip), o.stderr[-2000:]
    size = dmg.UNUSABLE_SIZES.get(case[len("fields-size_"):]) if case.startswith("fields-size_") else None
    if size is not None:                                                                        # rule 5, the message; the allocation: below
        assert o.status == 1 and "size" in o.messages[0] and str(size) in o.messages[0], o.stderr[-2000:]


@pytest.mark.parametrize("case", dmg.CONTAINER_CASE_NAMES)
@pytest.mark.parametrize("model_hooks", (0, 1))
def test_damaged_container_ends_cleanly(cli, tmp_path, model_hooks, case):
    damaged_container(cli, tmp_path, "realshort", model_hooks, case)


@pytest.mark.parametrize("case", dmg.ONE_PER_FAMILY)
@pytest.mark.parametrize("model_hooks", (0, 1))
def test_damaged_container_of_the_long_clip_ends_cleanly(cli, tmp_path, model_hooks, case):
    damaged_container(cli, tmp_path, "cockatoo", model_hooks, case)


@pytest.mark.parametrize("name", sorted(dmg.UNUSABLE_SIZES))
def test_an_unusable_size_is_refused_before_it_is_allocated(cli, tmp_path, name):
    """A size that is negative as int64 or above INT_MAX can never be recognised (recognize_coded_block compares it with an int): it is
    refused by name, and before make_surrogate_block allocates it -- the plain build under an address-space limit of 1 GiB, where an
    allocation of 2 GiB and more ends in std::bad_alloc, a message that names no size."""
    s = cli.sound("realshort", 0)
    src, dst = tmp_path / "damaged.recode", tmp_path / "restored.mp4"
    src.write_bytes(s["cases"]["fields-size_" + name])
    o = cpu_recode.run(cli.plain, "decompress", src, dst, 0, limit_address_space=1 << 30)
    clean(o)
    assert o.status == 1 and "size" in o.messages[0] and str(dmg.UNUSABLE_SIZES[name]) in o.messages[0] and "bad_alloc" not in o.stderr, o.stderr[-2000:]
    assert not dst.exists()
    sound = tmp_path / "sound.recode"                    # the limit itself leaves a sound file alone
    sound.write_bytes(s["container"])
    o = cpu_recode.run(cli.plain, "decompress", sound, dst, 0, limit_address_space=1 << 30)
    assert o.status == 0 and dst.read_bytes() == cpu_recode.golden("realshort"), o.stderr[-2000:]


# ------------------------------------------------------------------------------------------------ damaged input to compress
@pytest.fixture(scope="module")
def damaged_mp4s():
    return dict(dmg.mp4_cases(cpu_recode.golden("realshort")))


@pytest.mark.parametrize("case", dmg.MP4_CASE_NAMES)
@pytest.mark.parametrize("model_hooks", (0, 1))
def test_damaged_mp4_compresses_to_what_restores_it_or_is_refused(cli, damaged_mp4s, tmp_path, model_hooks, case):
    """Rule 6: compress exits 0 and decompress then restores the DAMAGED input exactly (what does not parse stays literal), or compress
    exits 1 with a message."""
    src, recoded, back = tmp_path / "damaged.mp4", tmp_path / "damaged.recode", tmp_path / "back.mp4"
    src.write_bytes(damaged_mp4s[case])
    c = cpu_recode.run(cli.asan, "compress", src, recoded, model_hooks)
    print(case, model_hooks, "compress ->", c.status, c.messages, c.pending)
    clean(c)
    if c.status:
        assert not recoded.exists()
        record(case, "realshort", model_hooks, c, recoded, cli.sound("realshort", model_hooks)["seconds"])
        return
    d = cpu_recode.run(cli.asan, "decompress", recoded, back, model_hooks)
    print(case, model_hooks, "decompress ->", d.status, d.messages, d.pending)
    clean(d)
    record(case, "realshort", model_hooks, d, back, cli.sound("realshort", model_hooks)["seconds"])
    assert d.status == 0 and back.read_bytes() == damaged_mp4s[case], d.stderr[-2000:]


# ------------------------------------------------------------------------------------------------ the unwind itself
def test_compressor_and_decompressor_are_safe_to_destroy_after_a_throw(cli):
    """tests/unwind_check.cpp under ASan + UBSan: a throw after init_decoder inside the first, a middle and the last slice, in
    compressor (with and without the restore check's second vector) and decompressor; then fresh objects for a whole run."""
    exe = cpu_recode.build_program(cli.work, "unwind_check", os.path.join(cpu_recode.ROOT, "tests", "unwind_check.cpp"))
    p = subprocess.run([exe], capture_output=True, text=True, timeout=cpu_recode.TIMEOUT, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0"))
    assert "AddressSanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-3000:]
    assert p.returncode == 0 and p.stdout.rstrip().endswith("unwind ok") and p.stdout.count("destroyed") == 9, p.stdout + p.stderr[-2000:]
