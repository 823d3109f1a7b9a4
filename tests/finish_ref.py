"""The way back's epilogue in plain Python, for tests/test_finish_emul.py and tests/test_gpu_finish_device.py: what a slice's coded bytes
become under its finish word (include/avrecode_ms_amd.h, AVR_FINISH_WORD) -- the oracle's drop_stop_byte and tail_patch, then escape()
as written here, a byte at a time."""
import itertools

ALPHABET = (0x00, 0x01, 0x03, 0x04, 0x80)
LAST_BYTES = (0x00, 0x03, 0x80)             # a last byte that makes an escape, one that needs one, one that does neither


def escape(p, z=0):
    """H.264 7.4.1's emulation prevention over a payload with z zero bytes directly in front of it: s = z; for every byte b: where
    s == 2 and b <= 3, 0x03 goes in front of it and s = 0; then s = s + 1 if b == 0 else 0.  (In state 0 nothing happens up to the next
    zero byte: those bytes are taken in one piece.)"""
    p = bytes(p)
    s, out, i, n = min(z, 2), bytearray(), 0, len(p)
    while i < n:
        if s == 0:
            j = p.find(0, i)
            j = n if j < 0 else j
            out += p[i:j]
            i = j
            if i == n:
                break
        b = p[i]
        if s == 2 and b <= 3:
            out.append(3)
            s = 0
        out.append(b)
        s = s + 1 if b == 0 else 0
        i += 1
    return bytes(out)


def word(last_byte=0, length_parity=0, patch=False, escaped=False, zeros_before=0):
    """AVR_FINISH_WORD, without the library (zeros_before goes in as it is: 3 is the kernel's to take as 2)."""
    return (last_byte & 0xFF) | (length_parity & 1) << 8 | bool(patch) << 9 | bool(escaped) << 10 | (zeros_before & 3) << 11


def finished(oracle, coded, w):
    """The bytes slice `coded` gives under finish word w."""
    p = oracle.drop_stop_byte(bytes(coded))
    p = oracle.tail_patch(p, (w >> 8) & 1 if (w >> 9) & 1 else -1, w & 0xFF)
    return escape(p, (w >> 11) & 3) if (w >> 10) & 1 else p


def words():
    """No patch, and the patch at either parity with each of LAST_BYTES; plain, and escaped at every z; zeros_before 3."""
    ws = []
    for escaped, z in [(False, 0), (True, 0), (True, 1), (True, 2)]:
        ws.append(word(escaped=escaped, zeros_before=z))
        ws += [word(last, parity, True, escaped, z) for parity in (0, 1) for last in LAST_BYTES]
    return ws + [word(0xFF, 0, True, True, 3)]


def strings(max_len, alphabet=ALPHABET):
    for n in range(max_len + 1):
        for t in itertools.product(alphabet, repeat=n):
            yield bytes(t)
