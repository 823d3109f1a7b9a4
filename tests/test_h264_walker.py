"""The H.264 slice parser (avrecode-ms_amd/csrc/host/avr_h264.h) against tests/h264_walker.py, an independent reading of the
slice_data() syntax and of every ctxIdx derivation (see that module's docstring for what it is written from and what it cannot prove:
the initial-state tables of cabac_init_idc 1 / 2 stay unverified).

a. replay: on the two real clips the walker derives, from the bins alone, the ctxIdx the parser used for every bin -- the anchor that
   entitles it to judge the parser where no real stream does;
b. generated streams (tests/h264_corpus.py) through `recode probe` and the parser's trace, header field by header field and bin for bin;
c. the corpus reaches every context of the frame-coded syntax and every mb_type / sub_mb_type (a condition on the generator alone);
d. slices that must stay literal (I_PCM, CAVLC, field coding, slice groups, cabac_zero_words) say why, their neighbours are coded;
e. both directions of the model chain on the CPU for every generated file.
"""
import json
import os
import subprocess
import time

import numpy as np
import pytest

import h264_corpus as corpus
import h264_walker as hw
from stream_records import stream_records

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
COCKATOO_EVERY = 7                                           # cockatoo.mp4: every I slice, and every 7th slice in stream order


@pytest.fixture(scope="module")
def recode(avr):
    return avr.build_recode()


@pytest.fixture(scope="module")
def host(avr):
    from test_host import host as host_fixture
    lib = host_fixture.__wrapped__(avr)
    lib.t_init_states.restype = None
    return lib


@pytest.fixture(scope="module")
def files(oracle, host):
    """name -> (bytes, slices) of every case, built once."""
    t0 = time.time()
    out = {name: corpus.build(name, oracle, host) for name in corpus.CASE_NAMES}
    print(f"corpus: {sum(len(s) for _, s in out.values())} slices, {sum(len(e['log']) for _, s in out.values() for e in s)} bins, "
          f"generated in {time.time() - t0:.1f} s")
    return out


# ------------------------------------------------------------------------------------------------ a. replay on real streams
@pytest.mark.parametrize("name,n_slices", [("realshort.mp4", 36), ("cockatoo.mp4", 280)])
def test_replay_of_the_real_clips_derives_the_parsers_contexts(host, name, n_slices):
    data = open(os.path.join(GOLD, name), "rb").read()
    trace = corpus.parse_trace(host, data)
    assert len(trace) == n_slices
    pic, replayed, bins, sid = None, 0, 0, 0
    for i, (f, recs, why) in enumerate(trace):
        assert f["status"] == 0 and f["clean_end"] == 1 and why == "", (i, why)
        if pic is None or f["first_mb"] == 0:
            pic = hw.Picture(f["width"], f["height"], f["chroma"])
        sid += 1
        if name == "cockatoo.mp4" and f["type"] != hw.SLICE_I and i % COCKATOO_EVERY:
            continue                                         # sampled by index only; a slice needs nothing of the slices before it
        w = hw.Walker(pic, sid, f["type"], f["first_mb"], (f["refs0"], f["refs1"]), f["t8_mode"], f["d8_inference"],
                      old_x264_444=bool(f["old_x264_444"]), recs=recs.tolist())
        n = w.run()
        assert w.pos == len(recs), f"{name} slice {i}: the walker ended on bin {w.pos} of {len(recs)}"
        assert n == f["macroblocks"]
        replayed += 1
        bins += len(recs)
    print(f"{name}: {replayed} of {n_slices} slices replayed, {bins} bins")
    if name == "realshort.mp4":
        assert replayed == 36
    else:
        i_slices = sum(1 for f, _, _ in trace if f["type"] == hw.SLICE_I)
        assert replayed == len({i for i, (f, _, _) in enumerate(trace) if f["type"] == hw.SLICE_I or i % COCKATOO_EVERY == 0}) >= 40 + i_slices // 2


# ------------------------------------------------------------------------------------------------ c. coverage, from the walker's own log
# every ctxIdx of Table 9-34 except, with the reason:
UNREACHABLE = [(0, 2, "mb_type of SI slices (SP / SI slices are not parsed)"),
               (70, 72, "mb_field_decoding_flag: MBAFF only"),
               (276, 276, "the terminate bin has no context variable"),
               (277, 398, "significant / last_significant_coeff_flag of field-coded blocks, ctxBlockCat 0-4"),
               (436, 459, "... of field-coded 8x8 luma blocks"),
               (675, 689, "significant_coeff_flag of field-coded Cb 8x8 blocks"), (699, 707, "last_significant_coeff_flag of the same"),
               (733, 747, "significant_coeff_flag of field-coded Cr 8x8 blocks"), (757, 765, "last_significant_coeff_flag of the same"),
               (776, 951, "significant / last_significant_coeff_flag of field-coded Cb / Cr blocks, ctxBlockCat 6-8, 10-12")]
# inside the frame-coded tables: ctxBlockCat 1, 4, 7 and 11 (AC blocks, 15 coefficients) use 14 of their 15 map contexts -- Table 9-34's
# ranges leave no gap for that, the fifteenth index of one category is the first of the next -- and ctxBlockCat 3 uses 9 of 10 level contexts
# (its ctxIdxInc stops at 5 + 3), the tenth being the first of ctxBlockCat 4.  So nothing more is excluded.


def test_the_corpus_reaches_every_frame_coded_context_and_every_macroblock_type(files):
    want = set(range(1024))
    for lo, hi, _ in UNREACHABLE:
        want -= set(range(lo, hi + 1))
    seen, mb_types, sub_types = set(), set(), set()
    for name, (_, slices) in files.items():
        for e in slices:
            sel = e["log"] >> 1
            seen |= set(sel[sel < 1024].tolist())
            mb_types |= e["mb_types"]
            sub_types |= e["sub_types"]
    print(f"distinct contexts: {len(seen)} of {len(want)} wanted")
    assert not (want - seen), f"contexts never drawn: {sorted(want - seen)}"
    assert not (seen - want), f"contexts the syntax should not reach: {sorted(seen - want)}"
    assert {t for k, t in mb_types if k == "I"} == set(range(26))                # Table 7-11 (I_PCM in case `literal`)
    assert {t for k, t in mb_types if k == "P"} >= set(range(4)) | set(range(5, 30))            # Table 7-13 and the intra types at 5 ...
    assert {t for k, t in mb_types if k == "B"} >= set(range(23)) | set(range(23, 48))          # Table 7-14 and the intra types at 23 ...
    assert {t for k, t in sub_types if k == "P"} == set(range(4)) and {t for k, t in sub_types if k == "B"} == set(range(13))


# ------------------------------------------------------------------------------------------------ b, d. the parser on generated streams
def first_difference(got, want, se):
    n = min(len(got), len(want))
    diff = np.flatnonzero(got[:n] != want[:n])
    at = int(diff[0]) if diff.size else n
    where = se[at] if at < len(se) else "the end"
    g = f"{got[at] >> 1}:{got[at] & 1}" if at < len(got) else "nothing"
    w = f"{want[at] >> 1}:{want[at] & 1}" if at < len(want) else "nothing"
    return f"first difference at bin {at} of {len(want)} (parser read {len(got)}): parser {g}, walker {w}, in {where}"


@pytest.mark.parametrize("name", corpus.CASE_NAMES)
def test_generated_streams_parse_bin_for_bin(files, host, recode, tmp_path, name):
    data, slices = files[name]
    path = tmp_path / (name + ".264")
    path.write_bytes(data)
    out = subprocess.run([recode, "probe", str(path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    res = json.loads(out.stdout)
    reasons, counters = {}, {"fail": 0, "unsupported": 0}
    for e in slices:
        if e["expect"]:
            counters[e["expect"][0]] += 1
            reasons[e["expect"][1]] = reasons.get(e["expect"][1], 0) + 1
    assert res == {"slices": len(slices), "parse_to_the_end": len(slices) - sum(counters.values()), "fail": counters["fail"],
                   "unsupported": counters["unsupported"], "header_failures": 0, "literal_reasons": reasons}, out.stderr
    if name != "literal" and name != "emulation":
        assert not reasons
    trace = corpus.parse_trace(host, data)
    assert len(trace) == len(slices)
    for i, ((f, recs, why), e) in enumerate(zip(trace, slices)):
        what = f"{name} slice {i}"
        if e["fields"] is None:                              # refused by its header, for the stated reason
            assert f["status"] == 1 and why == e["expect"][1], (what, why)
            continue
        assert {k: f[k] for k in e["fields"]} == e["fields"], what
        assert np.array_equal(recs, e["log"]), what + ": " + first_difference(recs, e["log"], e["se"])
        if e.get("pcm"):
            assert f["status"] == 1 and why == "I_PCM macroblock", (what, why)
        else:
            assert f["status"] == 0 and why == "" and f["clean_end"] == (0 if e["zero_words"] else 1), (what, why)
    if name == "emulation":                                  # the case is about escaped payloads: some must be
        assert sum(1 for e in slices if e.get("escaped")) >= 2


# ------------------------------------------------------------------------------------------------ e. both directions on the CPU
@pytest.mark.parametrize("name", corpus.CASE_NAMES)
def test_generated_streams_round_trip_through_the_model(files, host, oracle, name):
    """The chain of test_h264.py's test_real_streams_round_trip_through_the_model_with_all_eleven_hooks on every generated file, with the
    residual hooks off and on; with them on, once as generated -- a slice is refused exactly when the walker saw a block with a full nonzero
    count in it -- and once generated with counts kept below count_limit(), where every slice must be offered."""
    def chain(data, slices, residual, all_offered):
        k2, payloads, offered = stream_records(host, data, residual, 0)
        headers_ok = [e for e in slices if e["fields"] is not None]
        assert len(offered) == len(headers_ok)
        for e, o in zip(headers_ok, offered):
            refused = bool(e["expect"]) or (residual and e["full_blocks"] > 0)
            assert bool(o) == (not refused), (name, residual, e["expect"], e["full_blocks"])
        if all_offered:
            assert all(bool(o) for e, o in zip(headers_ok, offered) if not e["expect"])
        kept = [e for e, o in zip(headers_ok, offered) if o]
        assert len(k2) == len(kept) and [e["payload"] for e in kept] == payloads
        recoded = []
        for r in k2:
            coded, st = oracle.range_encode(r)
            assert st == 0
            recoded.append(coded)
        k1, first_states = stream_records(host, data, residual, 1, recoded, offered)
        assert len(k1) == len(k2)
        for i, (r, states) in enumerate(zip(k1, first_states)):
            raw, _, st = oracle.cabac_encode(r, states)
            assert st == 0
            back = oracle.tail_patch(oracle.drop_stop_byte(raw), len(payloads[i]) & 1, payloads[i][-1])
            assert back == payloads[i], f"{name} slice {i} residual_hooks={residual}"
    data, slices = files[name]
    chain(data, slices, 0, True)
    chain(data, slices, 1, False)
    data, slices = corpus.build(name, oracle, host, no_full_blocks=True)
    assert all(e["full_blocks"] == 0 for e in slices)
    chain(data, slices, 1, True)
