"""The optional digest of a .recode file, stated once for tests/test_digest_recode.py (the CPU stand-in under sanitizers) and
tests/test_gpu_digest_recode.py (the product on the device): the bytes `AVR_DIGEST=1` puts in front of an archive, worked out here
with hashlib and this module's own varints, the corpus cases the project used to restore wrongly without saying so, and damage to
the prefix itself.

The archive with a digest is prefix(original) + the archive without one, so a damaged digest-bearing archive is prefix + a case of
tests/damaged_recode.py's corpus (whose reader takes no top-level field but blocks, and is never handed the prefix).

Pure Python.  Nothing here runs the product."""
import hashlib

import damaged_recode as dmg

MESSAGE = "Verify error: restored file does not match the archive's digest (%d bytes restored, %d recorded)"
EXCEPTION = "Exception (St13runtime_error): "
NOT_PARSED = "Exception (St16invalid_argument): Failed to parse the recoded input"

# Recorded in profiles/damaged_recode.json as exit status 0 with a SHA-256 other than the original's, on realshort.mp4, per setting
# of AVR_MODEL_HOOKS: with the prefix in front, every one of them ends with the digest message.
SILENT = {
    0: ["bits-mid-flip_byte0", "bits-mid-random", "bits-mid-ones", "bits-last-flip_byte0", "bits-last-flip_mid", "bits-last-random", "bits-last-ones",
        "fields-parity_flipped", "fields-last_byte_changed", "literal-qp_delta", "literal-pps", "literal-sps_width"],
    1: ["bits-first-eight", "bits-first-random", "bits-first-ones", "bits-mid-flip_byte0", "bits-mid-flip_mid", "bits-mid-eight", "bits-last-flip_byte0",
        "bits-last-flip_mid", "bits-last-random", "bits-last-ones", "length-one_byte", "fields-parity_flipped", "fields-last_byte_changed",
        "literal-qp_delta", "literal-pps"],
}


def metadata(original):
    """Recoded.metadata's body: sub-field 5 (bytes, 32) = SHA-256 of the original, sub-field 6 (varint) = its length."""
    return b"\x2a\x20" + hashlib.sha256(original).digest() + b"\x30" + dmg.put_varint(len(original))


def prefix(original):
    m = metadata(original)
    return b"\x0a" + dmg.put_varint(len(m)) + m


# What a damaged prefix must end in, in front of an otherwise sound archive:
#   "restores"  the digest (or the size) is merely lost -- its tag names a field no reader knows, which is skipped -- or said twice: exit
#               status 0 and the original
#   "digest"    the archive parses and records something the restored file is not: exit status 1 with the digest message
#   "refused"   the archive does not parse: exit status 1, Failed to parse the recoded input
RESTORES, DIGEST, REFUSED = "restores", "digest", "refused"
PREFIX_CASE_NAMES = ["digest_bit_byte0", "digest_bit_byte15", "digest_bit_byte31", "size_plus1", "size_minus1", "tag_metadata_unknown", "tag_digest_unknown",
                     "tag_size_unknown", "metadata_short1", "metadata_long1", "digest_length_31", "digest_length_33", "prefix_twice"]


def prefix_cases(original):
    """{name: (the bytes that stand in place of prefix(original), how it must end, the size the message names as recorded or None)}.
    A metadata body is below 128 bytes, so its length is one byte at offset 1; the digest's length byte is at 3, the digest at 4 .. 35,
    the size's tag at 36."""
    p, n = prefix(original), len(original)
    assert p[0] == 0x0a and p[1] == len(p) - 2 < 128 and p[2:4] == b"\x2a\x20" and p[36] == 0x30

    def patched(at, value):
        return p[:at] + bytes([value]) + p[at + 1:]

    def resized(size):
        m = p[2:37] + dmg.put_varint(size)
        return b"\x0a" + dmg.put_varint(len(m)) + m
    out = {}
    for k in (0, 15, 31):
        out["digest_bit_byte%d" % k] = (patched(4 + k, p[4 + k] ^ (1 << (k % 8))), DIGEST, n)
    out["size_plus1"] = (resized(n + 1), DIGEST, n + 1)
    out["size_minus1"] = (resized(n - 1), DIGEST, n - 1)
    out["tag_metadata_unknown"] = (patched(0, 15 << 3 | 2), RESTORES, None)         # a top-level field 15: skipped whole
    out["tag_digest_unknown"] = (patched(2, 15 << 3 | 2), RESTORES, None)           # the size is still held to
    out["tag_size_unknown"] = (patched(36, 15 << 3 | 0), RESTORES, None)            # the digest is still held to
    # one too short: the body ends inside the size (behind its tag, or behind a byte that says another follows).  One too long: the
    # body swallows the first block's tag, which reads there as a bytes sub-field whose length, the block's, runs past the body.
    out["metadata_short1"] = (patched(1, p[1] - 1), REFUSED, None)
    out["metadata_long1"] = (patched(1, p[1] + 1), REFUSED, None)
    out["digest_length_31"] = (patched(3, 31), REFUSED, None)                       # sub-field 5 is a digest only at 32 bytes
    out["digest_length_33"] = (patched(3, 33), REFUSED, None)
    out["prefix_twice"] = (p + p, RESTORES, None)                                   # merged, as protobuf does: the later replaces the earlier
    assert sorted(out) == sorted(PREFIX_CASE_NAMES)
    return out
