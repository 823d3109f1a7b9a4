"""The seeded corpus of generated H.264 streams for tests/test_h264_walker.py (CPU) and tests/test_gpu_h264_walker.py: Annex B files
written by tests/h264_walker.py, one per case, each a few small pictures.  Nothing binary is committed; the same seed gives the same
file.  Also the ctypes front of tests/host_api.cpp's t_parse_trace / t_init_states."""
import ctypes
import random

import numpy as np

import h264_walker as hw
import oracle_lib
from h264_walker import SLICE_B as B, SLICE_I as I, SLICE_P as P

P_ = oracle_lib.ptr
FIELDS = ("status", "first_mb", "type", "qp", "cabac_init_idc", "refs0", "refs1", "data_offset", "chroma", "t8_mode", "d8_inference",
          "width", "height", "old_x264_444", "macroblocks", "clean_end")
ZERO_WORDS_REASON = "the payload does not end on end_of_slice_flag in its last byte"


def parse_trace(host, data):
    """[(fields dict, records uint16[], reason str)] per slice of `data`, as the parser read it."""
    cap, slice_cap = 16 * len(data) + 4096, 4096
    recs, rec_end = np.zeros(cap, np.uint16), np.zeros(slice_cap, np.uint64)
    fields = np.zeros(16 * slice_cap, np.int32)
    reasons, err = ctypes.create_string_buffer(256 * slice_cap), ctypes.create_string_buffer(512)
    n = ctypes.c_uint64(0)
    file = np.frombuffer(data, np.uint8).copy()
    rc = host.t_parse_trace(P_(file), ctypes.c_size_t(len(data)), P_(recs), ctypes.c_size_t(cap), P_(rec_end), P_(fields), reasons,
                            ctypes.c_size_t(len(reasons)), ctypes.c_size_t(slice_cap), ctypes.byref(n), err, ctypes.c_size_t(512))
    assert rc == 0, err.value.decode()
    why = reasons.value.decode().split("\n")
    ends = [0] + [int(e) for e in rec_end[:n.value]]
    return [(dict(zip(FIELDS, fields[16 * i:16 * i + 16].tolist())), recs[ends[i]:ends[i + 1]].copy(), why[i]) for i in range(n.value)]


def init_states(host, intra, qp, idc):
    out = np.zeros(1024, np.uint8)
    host.t_init_states(int(intra), int(qp), int(idc), P_(out))
    return out


def S(slice_type, n, **kw):
    return dict(type=slice_type, n=n, **kw)


def seg(sps, ppss, pictures, profile=None):
    return dict(sps=sps, ppss=ppss, pictures=pictures, profile=profile or {})


def ipb(w, h, split=True):
    """An I, a P and a B picture of w x h macroblocks, each in two slices (the first ends mid-row when the picture has rows to end in)."""
    n = w * h
    a = n // 2 + (1 if w > 1 and split else 0)
    return [[S(t, a), S(t, n - a)] for t in (I, P, B)]


LONG_BLOCKS = dict(p_last=0.03, p_sig=0.7, p_cbp=0.8, p_cbf=0.9)     # blocks that run to their last positions
SCALING = ["full", None, "short", "default", "full", "short", "full", "default"]
HEADER_SEGMENTS = {
    "poc1": (dict(poc_type=1), dict(bottom_poc=1), {}),
    "poc1_zero": (dict(poc_type=1, delta_always_zero=1), dict(bottom_poc=1), {}),
    "poc2": (dict(poc_type=2), {}, {}),
    "bottom_poc": (dict(log2_poc_lsb=11), dict(bottom_poc=1), dict(poc_lsb=1234)),
    "redundant": ({}, dict(redundant=1), dict(redundant_cnt=5)),
    "override": ({}, dict(refs=(3, 2)), dict(refs=(7, 5))),
    "rplm": ({}, dict(refs=(2, 2)), dict(rplm=(((0, 3), (1, 0), (2, 1)), ((1, 2),)))),
    "weighted": ({}, dict(refs=(3, 2), weighted=1, bipred=1), {}),
    "bipred2": ({}, dict(refs=(2, 2), weighted=0, bipred=2), {}),
    "mmco": ({}, {}, dict(mmco=(1, 2, 3, 4, 6, 5))),
    "deblock0": ({}, dict(deblock=1), dict(deblock_idc=0)),
    "deblock1": ({}, dict(deblock=1), dict(deblock_idc=1)),
    "deblock2": ({}, dict(deblock=1), dict(deblock_idc=2)),
    "scaling_sps": (dict(scaling=SCALING), dict(t8=1), {}),
    "scaling_pps": ({}, dict(t8=1, scaling=SCALING), {}),
    "scaling_pps_4x4": ({}, dict(t8=0, scaling=SCALING), {}),
    "scaling_444": (dict(chroma=3, scaling=SCALING), dict(t8=1, scaling=SCALING), {}),
    "non_ref_plus5": ({}, {}, dict(ref_idc=0, type_plus5=1)),
    "wide_fields": (dict(log2_frame_num=16, log2_poc_lsb=16), {}, dict(frame_num=0, poc_lsb=0)),       # 32 zero bits: emulation prevention in the header
    "all": (dict(poc_type=1, scaling=SCALING, log2_frame_num=9),
            dict(bottom_poc=1, redundant=1, refs=(3, 2), weighted=1, bipred=1, deblock=1, t8=1, scaling=SCALING, init_qp=31),
            dict(redundant_cnt=2, refs=(5, 4), rplm=(((0, 1),), ((2, 0), (1, 1))), mmco=(3, 1, 0 + 4), deblock_idc=2, frame_num=300)),
}


def cases():
    """name -> list of segments.  A segment sends its SPS and PPSs, then its pictures; a slice is S(type, macroblocks, ...)."""
    c = {}
    c["multislice"] = [seg(dict(chroma=1, width=5, height=4), [dict(id=0, t8=1, refs=(2, 3)), dict(id=1, refs=(1, 1), init_qp=30)],
                           [[S(I, 7), S(I, 5, pps=1), S(I, 8)], [S(P, 5), S(B, 5, pps=1), S(I, 3), S(P, 7, pps=1)],
                            [S(B, 4, pps=k % 2) for k in range(5)], [S(P, 10, pps=1), S(B, 10)]])]
    c["yuv444_std"] = [seg(dict(chroma=3, width=6, height=4), [dict(t8=1, refs=(2, 2))],
                           [[S(I, 12), S(I, 12)], [S(P, 24)], [S(B, 10), S(B, 14)], [S(I, 9), S(P, 15)], [S(B, 24)],
                            [S(I, 12, profile=LONG_BLOCKS), S(P, 12, profile=LONG_BLOCKS)],
                            [S(I, 12, profile=dict(LONG_BLOCKS, i16_only=True)), S(I, 12, profile=dict(LONG_BLOCKS, i16_only=True, levels=[0, 0, 0, 1]))]])]
    c["yuv422"] = [seg(dict(chroma=2, width=5, height=4), [dict(t8=1, refs=(2, 2))], ipb(5, 4) + ipb(5, 4) + [[S(I, 10, profile=LONG_BLOCKS), S(P, 10, profile=LONG_BLOCKS)]])]
    c["mono"] = [seg(dict(chroma=0, width=5, height=4), [dict(t8=1, refs=(2, 2))], ipb(5, 4))]
    for k in (1, 2):
        c[f"idc{k}"] = [seg(dict(chroma=1, width=5, height=4), [dict(t8=1, refs=(2, 2))],
                            [[S(I, 20)], [S(P, 10, qp=0, idc=k), S(P, 10, qp=51, idc=k)], [S(B, 10, qp=51, idc=k), S(B, 10, qp=0, idc=k)],
                             [S(P, 8, qp=33, idc=k), S(B, 12, qp=17, idc=k)]])]
    big = dict(chroma=1, width=8, height=6)
    c["b_all"] = [seg(big, [dict(t8=1, refs=(32, 32))], [[S(I, 48)]] + [[S(B, 48)]] * 3 + [[S(B, 48, profile=dict(p_intra=0.8))]],
                      dict(refs_high=True, p_intra=0.1, p_skip=0.05))]
    c["p_all"] = [seg(big, [dict(t8=1, refs=(32, 1))], [[S(I, 48)]] + [[S(P, 48)]] * 2 + [[S(P, 48, profile=dict(p_intra=0.8))]],
                      dict(refs_high=True, p_intra=0.1, p_skip=0.05))]
    c["i16_all"] = [seg(big, [dict(t8=1)], [[S(I, 30), S(I, 18)], [S(I, 48)], [S(P, 24), S(B, 24)]], dict(i16_only=True, p_intra=0.6))]
    c["escapes"] = [seg(dict(chroma=1, width=5, height=4), [dict(refs=(2, 2))], ipb(5, 4) + ipb(5, 4)[1:],
                        dict(mvd=[0, 1, 2, 1, 2, 3, 15, 16, 17, 31, 32, 33, 34, 8, 9, 10, 64, 65, 200, 4000, 8000],
                             levels=[0, 0, 1, 2, 12, 13, 14, 15, 16, 30, 100, 1000, 40000], qp=[0, 1, 5, 30, 51, 52], p_skip=0.05))]
    c["t8x8_inter"] = [seg(dict(chroma=1, width=5, height=4, direct_8x8=d), [dict(t8=1, refs=(2, 2))], ipb(5, 4)[1:] + ipb(5, 4)[1:],
                           dict(p_cbp=0.8, p_intra=0.1)) for d in (0, 1)]
    c["narrow"] = [seg(dict(chroma=1, width=w, height=h), [dict(t8=1, refs=(2, 2))], ipb(w, h, split=False)) for w, h in ((1, 7), (7, 1))]
    c["headers"] = []
    for name, (sps, pps, hdr) in HEADER_SEGMENTS.items():
        sps = dict(dict(chroma=1, width=3, height=2), **sps)
        c["headers"].append(seg(sps, [dict(dict(refs=(1, 1)), **pps)],
                                [[S(I, 6, hdr=hdr)], [S(P, 2, hdr=hdr), S(P, 4, hdr=hdr)], [S(B, 6, hdr=hdr)]]))
    c["emulation"] = [seg(dict(chroma=1, width=4, height=3, log2_frame_num=16, log2_poc_lsb=16), [dict(refs=(1, 1))],
                          ipb(4, 3) + [[S(I, 12, zero_words=2)]] + ipb(4, 3)[1:],
                          dict(levels=[0, 14 + (1 << 20) - 1, 14 + (1 << 22) - 1, 14 + (1 << 23) - 1], mvd=[0, 9 + 8 * ((1 << 14) - 1), 1], p_skip=0.05))]
    # what stays literal, between slices that are coded
    normal, cavlc, groups = dict(id=0, t8=1, refs=(2, 2)), dict(id=1, cabac=0), dict(id=3, slice_groups=2)
    frame = dict(chroma=1, width=5, height=4)
    c["literal"] = [
        seg(frame, [normal, cavlc], [[S(I, 10), S(I, 10)],
                                     [S(P, 7), S(I, 6, profile=dict(pcm=True, pcm_once=True), expect=("fail", "I_PCM macroblock")), S(B, 7)],
                                     [S(I, 10, pps=1, garbage=True, expect=("unsupported", "CAVLC slice")),
                                      S(I, 10, pps=1, garbage=True, expect=("unsupported", "CAVLC slice"))],
                                     [S(P, 20)]]),
        seg(dict(frame, id=1, frame_mbs_only=0), [dict(id=2)], [[S(I, 20, garbage=True, expect=("unsupported", "field / MBAFF coding"))]]),
        seg(frame, [normal, groups], [[S(P, 10), S(P, 10, pps=1, garbage=True, expect=("unsupported", "slice groups"))], [S(B, 12), S(I, 8)]])]
    return c


CASE_NAMES = ["multislice", "yuv444_std", "yuv422", "mono", "idc1", "idc2", "b_all", "p_all", "i16_all", "escapes", "t8x8_inter", "narrow",
              "headers", "emulation", "literal"]


def encode_payload(oracle, log, states, pcm_at, pcm_bytes, rng):
    """slice_data() bytes from the walker's log: 9.3.4.2 by the oracle; at an I_PCM the flushed engine's bytes, the raw samples, and
    a freshly initialised engine that carries the context states on."""
    out, at, st = b"", 0, states
    for cut in list(pcm_at) + [len(log)]:
        data, final, status = oracle.spec_cabac_encode(np.array(log[at:cut], np.uint16), st)
        assert status == 0
        out += data
        st = np.frombuffer(final, np.uint8)
        if cut != len(log):
            out += bytes(rng.randrange(1, 256) for _ in range(pcm_bytes))
        at = cut
    return out


def build(name, oracle, host, no_full_blocks=False, seed=0):
    """(file bytes, [slice dict]) of one case.  Per slice: log (uint16 records), se (the syntax element of each), states (initial),
    payload, fields (what the header says, by the names of FIELDS), expect (None: coded; (probe counter, literal reason) otherwise),
    mb_types / sub_types seen, full_blocks."""
    rng = random.Random(f"{name}/{seed}")
    out, slices, sid, decks, n_nal = b"", [], 0, {}, 0
    for sg in cases()[name]:
        sps = sg["sps"]
        out += hw.nal(3, 7, hw.write_sps(sps, rng), True)
        for pps in sg["ppss"]:
            out += hw.nal(3, 8, hw.write_pps(pps, sps, rng), pps.get("id", 0) % 2 == 0)
        for pi, picture in enumerate(sg["pictures"]):
            pic = hw.Picture(sps["width"], sps["height"], sps["chroma"])
            first = 0
            idr = pi == 0 and all(s["type"] == I for s in picture)
            for s in picture:
                pps = sg["ppss"][s.get("pps", 0)]
                hdr = dict(first_mb=first, type=s["type"], qp=s.get("qp", pps.get("init_qp", 26) + rng.randint(-5, 5)), idr=idr,
                           ref_idc=3 if idr else 1, cabac_init_idc=s.get("idc", 0))
                hdr.update(s.get("hdr", {}))
                if idr:
                    hdr["ref_idc"] = max(hdr["ref_idc"], 1)
                bits, refs = hw.write_slice_header(hdr, sps, pps, rng)
                entry = dict(case=name, expect=s.get("expect"), zero_words=s.get("zero_words", 0))
                if s.get("garbage"):
                    bits.b += [rng.getrandbits(1) for _ in range(300)]
                    rbsp = bits.trailing().bytes()
                    entry.update(log=np.zeros(0, np.uint16), se=[], payload=b"", states=None, fields=None, mb_types=set(), sub_types=set(), full_blocks=0)
                else:
                    profile = dict(sg["profile"], no_full_blocks=no_full_blocks)
                    profile.update(s.get("profile", {}))
                    gen = hw.Generator(rng.getrandbits(32), profile, decks)
                    w = hw.Walker(pic, sid, s["type"], first, refs, pps.get("t8", 0), sps.get("direct_8x8", 1), gen=gen, keep_se=True)
                    assert w.run(s["n"]) == s["n"]
                    assert not gen.q                                     # nothing of the last element may be left over
                    idc = hdr["cabac_init_idc"] if s["type"] != I else 0
                    states = init_states(host, s["type"] == I, hdr["qp"], idc)
                    pcm_bytes = 256 + 2 * 64 * {0: 0, 1: 1, 2: 2, 3: 4}[sps["chroma"]]
                    payload = encode_payload(oracle, w.log, states, w.pcm_at, pcm_bytes, rng)
                    head = bits.bytes()
                    rbsp = head + payload + b"\0\0" * entry["zero_words"]
                    if entry["zero_words"]:
                        entry["expect"] = ("fail", ZERO_WORDS_REASON)
                    log = np.array(w.log[:w.pcm_at[0]] if w.pcm_at else w.log, np.uint16)       # the parser stops at an I_PCM
                    entry.update(log=log, se=w.se_log, payload=payload, states=states, mb_types=w.seen_mb_types, sub_types=w.seen_sub_types,
                                 full_blocks=w.full_blocks, pcm=bool(w.pcm_at), escaped=hw.escape(rbsp[len(head):]) != rbsp[len(head):],
                                 fields=dict(first_mb=first, type=s["type"], qp=hdr["qp"], cabac_init_idc=idc, refs0=refs[0], refs1=refs[1],
                                             data_offset=len(head), chroma=sps["chroma"], t8_mode=pps.get("t8", 0),
                                             d8_inference=sps.get("direct_8x8", 1), width=sps["width"], height=sps["height"], old_x264_444=0))
                out += hw.nal(hdr["ref_idc"], 5 if idr else 1, rbsp, n_nal % 3 == 0)
                slices.append(entry)
                n_nal += 1
                sid += 1
                first += s["n"]
    return out, slices
