"""Damage to a .recode container (and to the MP4 that goes into one), stated once and deterministic.

What storage does to an archive -- flipped, missing, repeated bytes -- and what a hostile or confused writer could put into the six
fields of a block, as a named list of variants of ONE sound container: container_cases(sound) -> [(name, bytes)], the names fixed
(CONTAINER_CASE_NAMES, usable as pytest ids before any container exists), the draws seeded per case.  mp4_cases(mp4) is the other
side: the input of `recode compress` with bytes changed inside mdat.

The container is read and written here by a proto2 reader of this module's own (recode.proto: Recoded { repeated Block block = 2 },
Block { int64 size = 1; bytes literal = 2; bool skip_coded = 3; bytes cabac = 4; bool length_parity = 5; bytes last_byte = 6 }),
independent of the C++ one in csrc/host/avr_host.h: a block is the ordered list of its fields as they stand in the file, so a sound
file re-serialises byte for byte (serialise(parse(x)) == x is part of the tests) and a damaged one says exactly what it holds.

Pure Python with numpy.  Nothing here runs the product.
"""
import struct

import numpy as np

F_SIZE, F_LITERAL, F_SKIP, F_CABAC, F_PARITY, F_LAST = 1, 2, 3, 4, 5, 6


# ------------------------------------------------------------------------------------------------ proto2 wire format
def put_varint(v):
    v &= (1 << 64) - 1
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7f) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def get_varint(data, at):
    v = shift = 0
    while True:
        if at >= len(data) or shift >= 70:
            raise ValueError("truncated varint")
        c = data[at]
        at += 1
        v |= (c & 0x7f) << shift
        shift += 7
        if not c & 0x80:
            return v, at


def parse_fields(data):
    """[(field, wire, value)] in file order: value an int for wire 0, bytes for wire 1, 2 and 5."""
    fields, at = [], 0
    while at < len(data):
        tag, at = get_varint(data, at)
        field, wire = tag >> 3, tag & 7
        if wire == 0:
            v, at = get_varint(data, at)
        elif wire == 2:
            n, at = get_varint(data, at)
            if at + n > len(data):
                raise ValueError("truncated bytes field")
            v, at = bytes(data[at:at + n]), at + n
        elif wire in (1, 5):
            n = 8 if wire == 1 else 4
            if at + n > len(data):
                raise ValueError("truncated fixed field")
            v, at = bytes(data[at:at + n]), at + n
        else:
            raise ValueError("wire type %d" % wire)
        fields.append((field, wire, v))
    return fields


def put_fields(fields):
    out = bytearray()
    for field, wire, v in fields:
        out += put_varint(field << 3 | wire)
        if wire == 0:
            out += put_varint(v)
        elif wire == 2:
            out += put_varint(len(v)) + v
        else:
            out += v
    return bytes(out)


def parse(data):
    """The container as a list of blocks, each the list of its fields."""
    blocks = []
    for field, wire, v in parse_fields(data):
        if (field, wire) != (2, 2):
            raise ValueError("top-level field %d / wire %d" % (field, wire))
        blocks.append(parse_fields(v))
    return blocks


def serialise(blocks):
    return put_fields([(2, 2, put_fields(b)) for b in blocks])


def get(block, field):
    for f, _, v in block:
        if f == field:
            return v
    return None


def has(block, field):
    return get(block, field) is not None


def replace(block, field, value):
    return [(f, w, value if f == field else v) for f, w, v in block]


def without(block, field):
    return [e for e in block if e[0] != field]


def coded_blocks(blocks):
    return [i for i, b in enumerate(blocks) if has(b, F_CABAC)]


# ------------------------------------------------------------------------------------------------ H.264 headers, as far as the damage needs them
class BitReader:
    """Over a NAL unit with its emulation prevention bytes taken out (7.4.1); bit positions are handed back as positions in the
    unit as it lies in the file, so that a flip lands on the bit that was read."""
    def __init__(self, nal, at=0):
        self.d, self.raw, zeros = bytearray(), [], 0
        for i, b in enumerate(nal):
            if zeros >= 2 and b == 3:
                zeros = 0
                continue
            self.d.append(b)
            self.raw.append(i)
            zeros = zeros + 1 if b == 0 else 0
        self.at = at * 8

    def where(self, bit):
        return self.raw[bit >> 3] * 8 + (bit & 7)

    def u(self, n):
        v = 0
        for _ in range(n):
            v = v << 1 | (self.d[self.at >> 3] >> (7 - (self.at & 7))) & 1
            self.at += 1
        return v

    def ue(self):
        """value, and the position of the code's last bit (flipping it gives another value of the same length, unless the code is '1')"""
        zeros = 0
        while self.u(1) == 0:
            zeros += 1
            if zeros > 31:
                raise ValueError("Exp-Golomb code too long")
        v = (1 << zeros) - 1 + self.u(zeros)
        return v, self.where(self.at - 1), zeros

    def se(self):
        v, last, zeros = self.ue()
        return ((v + 1) >> 1) * (1 if v & 1 else -1), last, zeros


def read_sps(nal):
    """nal: the SPS NAL unit with its header byte.  The fields a slice header depends on, and where pic_width_in_mbs_minus1 ends."""
    r = BitReader(nal, 1)
    s = {"profile": r.u(8)}
    r.u(16)
    r.ue()
    s["chroma"] = 1
    if s["profile"] in (100, 110, 122, 244, 44, 83, 86, 118, 128, 138, 139, 134, 135):
        s["chroma"] = r.ue()[0]
        if s["chroma"] == 3 and r.u(1):
            raise ValueError("SPS: separate colour planes")
        r.ue(); r.ue(); r.u(1)
        if r.u(1):
            raise ValueError("SPS: scaling matrices")
    s["frame_num_bits"] = r.ue()[0] + 4
    s["poc_type"] = r.ue()[0]
    if s["poc_type"] == 0:
        s["poc_lsb_bits"] = r.ue()[0] + 4
    elif s["poc_type"] == 1:
        s["delta_always_zero"] = r.u(1)
        r.se(); r.se()
        for _ in range(r.ue()[0]):
            r.se()
    r.ue(); r.u(1)
    _, s["width_last_bit"], s["width_zeros"] = r.ue()
    r.ue()
    if not r.u(1):
        raise ValueError("SPS: field / MBAFF coding")
    return s


def read_pps(nal):
    r = BitReader(nal, 1)
    p = {}
    r.ue(); r.ue()
    p["cabac"] = r.u(1)
    p["bottom_field_poc"] = r.u(1)
    if r.ue()[0]:
        raise ValueError("PPS: slice groups")
    p["refs"] = [r.ue()[0] + 1, r.ue()[0] + 1]
    p["weighted_pred"], p["weighted_bipred"] = r.u(1), r.u(2)
    _, p["init_qp_last_bit"], p["init_qp_zeros"] = r.se()
    r.se(); r.se()
    p["deblocking_control"] = r.u(1)
    r.u(1)
    p["redundant_pic_cnt"] = r.u(1)
    return p


def read_slice_header(nal, sps, pps):
    """nal: the slice NAL unit from its header byte.  Where the three fields the damage aims at end (bit positions in nal)."""
    unit_type, ref_idc = nal[0] & 31, nal[0] >> 5 & 3
    r = BitReader(nal, 1)
    h = {}
    _, h["first_mb_last_bit"], h["first_mb_zeros"] = r.ue()
    t, h["slice_type_last_bit"], h["slice_type_zeros"] = r.ue()
    # the value that the flip of the code's last bit gives: another code of the same length, unless the code is '1'; a type this
    # build's parser takes (P, B, I) is the damage wanted -- the same bins under another syntax
    h["slice_type_flipped"] = ((t + 1) ^ 1) - 1 if h["slice_type_zeros"] else None
    t %= 5                                               # 0 P, 1 B, 2 I
    if t > 2:
        raise ValueError("SP / SI slice")
    r.ue()
    r.u(sps["frame_num_bits"])
    if unit_type == 5:
        r.ue()
    if sps["poc_type"] == 0:
        r.u(sps["poc_lsb_bits"])
        if pps["bottom_field_poc"]:
            r.se()
    elif sps["poc_type"] == 1 and not sps["delta_always_zero"]:
        r.se()
        if pps["bottom_field_poc"]:
            r.se()
    if pps["redundant_pic_cnt"]:
        r.ue()
    if t == 1:
        r.u(1)
    refs = list(pps["refs"])
    if t != 2:
        if r.u(1):
            refs[0] = r.ue()[0] + 1
            if t == 1:
                refs[1] = r.ue()[0] + 1
        for _ in range(2 if t == 1 else 1):              # ref_pic_list_modification
            if r.u(1):
                while True:
                    idc = r.ue()[0]
                    if idc == 3:
                        break
                    r.ue()
    if (pps["weighted_pred"] and t == 0) or (pps["weighted_bipred"] == 1 and t == 1):    # pred_weight_table
        r.ue()
        if sps["chroma"]:
            r.ue()
        for lst in range(2 if t == 1 else 1):
            for _ in range(refs[lst]):
                if r.u(1):
                    r.se(); r.se()
                if sps["chroma"] and r.u(1):
                    r.se(); r.se(); r.se(); r.se()
    if ref_idc:                                          # dec_ref_pic_marking
        if unit_type == 5:
            r.u(2)
        elif r.u(1):
            while True:
                op = r.ue()[0]
                if op == 0:
                    break
                r.ue()
                if op == 3:
                    r.ue()
    if t != 2:
        r.ue()                                           # cabac_init_idc
    _, h["qp_delta_last_bit"], h["qp_delta_zeros"] = r.se()
    return h


def flip_bit(data, bit):
    out = bytearray(data)
    out[bit >> 3] ^= 0x80 >> (bit & 7)
    return bytes(out)


def slice_nal_start(literal, payload_size):
    """The literal in front of a coded block ends with an MP4 length prefix, the NAL header byte and the slice header."""
    for p in range(len(literal) - 6, max(len(literal) - 200, -1), -1):
        if struct.unpack(">I", literal[p:p + 4])[0] == len(literal) - p - 4 + payload_size and (literal[p + 4] & 0x9f) in (1, 5):
            return p + 4
    raise ValueError("no slice NAL unit found in front of the coded block")


def parameter_sets(blocks):
    """(block index, offset of the SPS NAL in its literal, its length, offset of the PPS NAL, its length) from the avcC box."""
    for i, b in enumerate(blocks):
        lit = get(b, F_LITERAL)
        at = lit.find(b"avcC") if lit is not None else -1
        if at >= 0:
            at += 4 + 5
            if lit[at] & 31 < 1:
                raise ValueError("avcC without an SPS")
            sps_len = struct.unpack(">H", lit[at + 1:at + 3])[0]
            sps_at = at + 3
            at = sps_at + sps_len
            if lit[at] < 1:
                raise ValueError("avcC without a PPS")
            pps_len = struct.unpack(">H", lit[at + 1:at + 3])[0]
            return i, sps_at, sps_len, at + 3, pps_len
    raise ValueError("no avcC box in the container's literals")


# ------------------------------------------------------------------------------------------------ the cases
SIZES = [("minus1", lambda s: s - 1), ("plus1", lambda s: s + 1), ("minus2", lambda s: s - 2), ("plus2", lambda s: s + 2),
         ("0", lambda s: 0), ("7", lambda s: 7), ("8", lambda s: 8), ("2p31m1", lambda s: 2**31 - 1), ("2p31", lambda s: 2**31),
         ("2p40", lambda s: 2**40), ("2p63", lambda s: 2**63), ("2p64m1", lambda s: 2**64 - 1)]
UNUSABLE_SIZES = {"2p31": 2**31, "2p40": 2**40, "2p63": 2**63, "2p64m1": 2**64 - 1}    # negative as int64, or above INT_MAX
WHERE = ("first", "mid", "last")
BITS = ("flip_byte0", "flip_mid", "flip_last", "byte", "eight", "random", "zeros", "ones")
LENGTH = ("empty", "one_byte", "half", "short1", "long1", "twice")
CUTS = 10
UNKNOWN_WIRES = (0, 1, 2, 5)
LITERAL = ("slice_type", "first_mb", "qp_delta", "pps", "sps_width")
MP4_VARIANTS = 12


def _names():
    names = ["bits-%s-%s" % (w, k) for w in WHERE for k in BITS]
    names += ["length-%s" % k for k in LENGTH]
    names += ["fields-size_%s" % n for n, _ in SIZES]
    names += ["fields-parity_flipped", "fields-last_byte_absent", "fields-last_byte_empty", "fields-last_byte_two", "fields-last_byte_changed",
              "fields-parity_without_last_byte"]
    names += ["structure-literal_and_cabac", "structure-no_kind", "structure-skip_coded_false", "structure-swapped", "structure-dropped",
              "structure-duplicated", "structure-last_block_dropped"]
    names += ["structure-cut_%d" % k for k in range(CUTS)] + ["structure-cut_mid_varint"]
    names += ["structure-unknown_wire%d" % w for w in UNKNOWN_WIRES]
    names += ["literal-%s" % k for k in LITERAL]
    return names


CONTAINER_CASE_NAMES = _names()
MUST_RESTORE = ["structure-unknown_wire%d" % w for w in UNKNOWN_WIRES]        # unknown fields are skipped: the original comes back
# one case per family: what runs on the long clip
ONE_PER_FAMILY = ["bits-mid-eight", "length-half", "fields-size_plus1", "structure-swapped", "literal-slice_type"]
MP4_CASE_NAMES = ["mp4-%02d" % k for k in range(MP4_VARIANTS)]


def family(name):
    return name.split("-")[0]


def _seed(name):
    return int.from_bytes(name.encode(), "little") % (2**63)


def _with_block(blocks, i, block):
    return blocks[:i] + [block] + blocks[i + 1:]


def _damage_literal_bit(blocks, pick):
    """pick(coded index, literal, nal start, header) -> bit position in the NAL or None; the first coded block that offers one."""
    set_at, sps_at, sps_len, pps_at, pps_len = parameter_sets(blocks)
    lit = get(blocks[set_at], F_LITERAL)
    sps, pps = read_sps(lit[sps_at:sps_at + sps_len]), read_pps(lit[pps_at:pps_at + pps_len])
    fallback = None
    for i in coded_blocks(blocks):
        front = get(blocks[i - 1], F_LITERAL) if i else None
        if front is None:
            continue
        start = slice_nal_start(front, get(blocks[i], F_SIZE))
        bit, same_length = pick(read_slice_header(front[start:], sps, pps))
        damaged = _with_block(blocks, i - 1, replace(blocks[i - 1], F_LITERAL, front[:start] + flip_bit(front[start:], bit)))
        if same_length:
            return damaged
        fallback = fallback or damaged
    return fallback                                      # every code was the one-bit '1': its flip swallows the bits behind it


def container_cases(sound):
    """[(name, bytes)] for every name of CONTAINER_CASE_NAMES, in that order."""
    blocks = parse(sound)
    coded = coded_blocks(blocks)
    if len(coded) < 3:
        raise ValueError("the sound container needs at least three coded blocks")
    at = {"first": coded[0], "mid": coded[len(coded) // 2], "last": coded[-1]}
    mid = at["mid"]
    out = {}

    def cabac_case(name, i, f):
        rng = np.random.default_rng(_seed(name))
        out[name] = serialise(_with_block(blocks, i, replace(blocks[i], F_CABAC, bytes(f(bytearray(get(blocks[i], F_CABAC)), rng)))))

    def flip(pos):
        def f(c, rng):
            c[pos(len(c))] ^= 1 << int(rng.integers(8))
            return c
        return f

    def one_byte(c, rng):
        p = int(rng.integers(len(c)))
        c[p] ^= int(rng.integers(1, 256))
        return c

    def eight(c, rng):
        p = int(rng.integers(max(1, len(c) - 8)))
        c[p:p + 8] = rng.integers(0, 256, 8, dtype=np.uint8).tobytes()[:len(c[p:p + 8])]
        return c

    for w in WHERE:
        i = at[w]
        cabac_case("bits-%s-flip_byte0" % w, i, flip(lambda n: 0))
        cabac_case("bits-%s-flip_mid" % w, i, flip(lambda n: n // 2))
        cabac_case("bits-%s-flip_last" % w, i, flip(lambda n: n - 1))
        cabac_case("bits-%s-byte" % w, i, one_byte)
        cabac_case("bits-%s-eight" % w, i, eight)
        cabac_case("bits-%s-random" % w, i, lambda c, rng: rng.integers(0, 256, len(c), dtype=np.uint8).tobytes())
        cabac_case("bits-%s-zeros" % w, i, lambda c, rng: bytes(len(c)))
        cabac_case("bits-%s-ones" % w, i, lambda c, rng: b"\xff" * len(c))
    cabac_case("length-empty", mid, lambda c, rng: b"")
    cabac_case("length-one_byte", mid, lambda c, rng: c[:1])
    cabac_case("length-half", mid, lambda c, rng: c[:len(c) // 2])
    cabac_case("length-short1", mid, lambda c, rng: c[:-1])
    cabac_case("length-long1", mid, lambda c, rng: c + bytes([int(rng.integers(256))]))
    cabac_case("length-twice", mid, lambda c, rng: c + c)

    def block_case(name, block, i=mid):
        out[name] = serialise(_with_block(blocks, i, block))

    sound_size = get(blocks[mid], F_SIZE)
    for n, f in SIZES:
        block_case("fields-size_" + n, replace(blocks[mid], F_SIZE, f(sound_size)))
    both = [i for i in coded if has(blocks[i], F_PARITY) and has(blocks[i], F_LAST)]
    b = both[len(both) // 2]
    block_case("fields-parity_flipped", replace(blocks[b], F_PARITY, 1 - get(blocks[b], F_PARITY)), b)
    block_case("fields-last_byte_absent", without(without(blocks[b], F_LAST), F_PARITY), b)
    block_case("fields-last_byte_empty", replace(blocks[b], F_LAST, b""), b)
    block_case("fields-last_byte_two", replace(blocks[b], F_LAST, get(blocks[b], F_LAST) + b"\x5a"), b)
    block_case("fields-last_byte_changed", replace(blocks[b], F_LAST, bytes([get(blocks[b], F_LAST)[0] ^ 0x10])), b)
    block_case("fields-parity_without_last_byte", without(blocks[b], F_LAST), b)

    block_case("structure-literal_and_cabac", blocks[mid] + [(F_LITERAL, 2, b"\0\0\1")])
    block_case("structure-no_kind", without(blocks[mid], F_CABAC))
    block_case("structure-skip_coded_false", without(blocks[mid], F_CABAC) + [(F_SKIP, 0, 0)])
    nxt = coded[len(coded) // 2 + 1]
    out["structure-swapped"] = serialise(_with_block(_with_block(blocks, mid, blocks[nxt]), nxt, blocks[mid]))
    out["structure-dropped"] = serialise(blocks[:mid] + blocks[mid + 1:])
    out["structure-duplicated"] = serialise(blocks[:mid + 1] + blocks[mid:])
    out["structure-last_block_dropped"] = serialise(blocks[:-1])
    # the file cut at field boundaries, from the first coded block on: before the block, behind its header, behind each field ...
    bounds, offset = [], len(serialise(blocks[:coded[0]]))
    for blk in blocks[coded[0]:]:
        body = put_fields(blk)
        bounds.append(offset)
        offset += 1 + len(put_varint(len(body)))
        for e in blk:
            bounds.append(offset)
            offset += len(put_fields([e]))
        if len(bounds) >= CUTS:
            break
    for k in range(CUTS):
        out["structure-cut_%d" % k] = sound[:bounds[k]]
    header = put_varint(len(put_fields(blocks[coded[0]])))
    if len(header) < 2:
        raise ValueError("the first coded block's length fits one byte: no varint to cut")
    out["structure-cut_mid_varint"] = sound[:bounds[0] + 2]          # the tag and the first byte of a length that has more
    unknown = {0: (15, 0, 300), 1: (15, 1, b"\1\2\3\4\5\6\7\x08"), 2: (15, 2, b"not a field of Block"), 5: (15, 5, b"\1\2\3\4")}
    for w in UNKNOWN_WIRES:                              # in a coded block, between its fields, and one at the top level too
        damaged = serialise(_with_block(blocks, mid, blocks[mid][:1] + [unknown[w]] + blocks[mid][1:]))
        cut = len(serialise(blocks[:mid]))
        out["structure-unknown_wire%d" % w] = damaged[:cut] + put_fields([(9, unknown[w][1], unknown[w][2])]) + damaged[cut:]

    out["literal-slice_type"] = serialise(_damage_literal_bit(blocks, lambda h: (h["slice_type_last_bit"], h["slice_type_flipped"] is not None and h["slice_type_flipped"] % 5 <= 2)))
    out["literal-first_mb"] = serialise(_damage_literal_bit(blocks, lambda h: (h["first_mb_last_bit"], h["first_mb_zeros"] > 0)))
    out["literal-qp_delta"] = serialise(_damage_literal_bit(blocks, lambda h: (h["qp_delta_last_bit"], h["qp_delta_zeros"] > 0)))
    set_at, sps_at, sps_len, pps_at, pps_len = parameter_sets(blocks)
    lit = get(blocks[set_at], F_LITERAL)
    sps, pps = read_sps(lit[sps_at:sps_at + sps_len]), read_pps(lit[pps_at:pps_at + pps_len])
    for name, nal_at, bit in (("literal-pps", pps_at, pps["init_qp_last_bit"]), ("literal-sps_width", sps_at, sps["width_last_bit"])):
        damaged = lit[:nal_at] + flip_bit(lit[nal_at:], bit)
        out[name] = serialise(_with_block(blocks, set_at, replace(blocks[set_at], F_LITERAL, damaged)))

    assert sorted(out) == sorted(CONTAINER_CASE_NAMES)
    return [(n, out[n]) for n in CONTAINER_CASE_NAMES]


def mp4_cases(mp4):
    """[(name, bytes)]: the sound MP4 with 1, 3 or 20 bytes changed inside mdat, MP4_VARIANTS seeded variants."""
    at = 0
    while at + 8 <= len(mp4):
        size, kind = struct.unpack(">I4s", mp4[at:at + 8])
        if kind == b"mdat":
            lo, hi = at + 8, (at + size if size >= 8 else len(mp4))
            break
        if size < 8:
            raise ValueError("MP4 box of size %d" % size)
        at += size
    else:
        raise ValueError("no mdat box")
    out = []
    for k, name in enumerate(MP4_CASE_NAMES):
        rng = np.random.default_rng(1000 + k)
        data = bytearray(mp4)
        for p in rng.choice(hi - lo, (1, 3, 20)[k % 3], replace=False):
            data[lo + int(p)] ^= int(rng.integers(1, 256))
        out.append((name, bytes(data)))
    return out
