"""Bin streams for phase B1 as the kernels walk it (B1Walk of csrc/avr_k1p.h), made so that WHERE the coded LPS bins lie is chosen
bin by bin: a stretch opens at a chunk's first coded LPS and closes at the first one at or past the next chunk's start, and the walk
takes another path for each place these two can have in a group of eight bins.

A stream is a row of symbols -- M: a context bin equal to its context's MPS, L: one that is not (a coded LPS), B: a bypass bin, T0:
put_terminate(0), T1: put_terminate(1) as a slice's last bin -- over ten contexts, turned into two-byte records and resolved codes by
walking the contexts' states (cabac_code.h:43-47 on the library's table).  tests/test_k1p_b1walk_emul.py gives the codes to the
host build of B1Walk, tests/test_gpu_k1p_b1walk.py the records to the device."""
import numpy as np

CHUNK = 1024
M, L, B, T0, T1 = range(5)
N_CTX = 10                                                       # contexts 0 .. 4 by turns; 5 .. 9 only where a stream names them
LENGTHS = (3 * CHUNK, 3 * CHUNK - 5, CHUNK + 9, 700)             # 3, 3, 2 and 1 chunks


class Stream:
    def __init__(self, name, syms, ctx=None, states=None, max_stretch=16 * CHUNK):
        self.name, self.syms, self.max_stretch = name, np.asarray(syms, np.uint8), max_stretch
        self.ctx = np.arange(self.syms.size) % 5 if ctx is None else np.asarray(ctx)
        self.states = np.array([10, 37, 62, 91, 120, 2, 9, 14, 5, 20], np.uint8) if states is None else np.asarray(states, np.uint8)
        self.recs = self.codes = None

    def resolve(self, mlps):
        """Records and resolved codes of the symbols: a walk of the ten contexts' states."""
        if self.recs is None:
            st = [int(s) for s in self.states]
            recs, codes = np.zeros(self.syms.size, np.uint16), np.zeros(self.syms.size, np.uint8)
            for i, (sym, k) in enumerate(zip(self.syms.tolist(), self.ctx.tolist())):
                if sym <= L:
                    s = st[k]
                    b = (s & 1) ^ sym
                    recs[i], codes[i] = b | k << 1, s << 1 | b
                    st[k] = mlps[128 + s] if sym == M else mlps[127 - s]
                elif sym == B:
                    recs[i], codes[i] = (i & 1) | 1024 << 1, 252 | (i & 1)
                else:
                    recs[i], codes[i] = (sym == T1) | 1025 << 1, 255 - (sym == T1)
            self.recs, self.codes = recs, codes
        return self.recs, self.codes


def background(rng, n, p_lps=0.0, p_bypass=0.15, p_term0=0.04):
    u = rng.random(n)
    return np.where(u < p_lps, L, np.where(u < p_lps + p_bypass, B, np.where(u < p_lps + p_bypass + p_term0, T0, M))).astype(np.uint8)


def placed(rng, n, opens, closes, inside=0.10):
    """n bins: coded LPS bins at a rate of 3 % in chunk 0, none in chunk 1 before `opens` and at `inside` behind it, none in chunk 2
    before `closes` and 10 % behind it (None: none in that chunk at all)."""
    s = background(rng, n)
    lps = rng.random(n)
    rate = np.zeros(n)
    rate[:CHUNK] = 0.03
    if opens is not None:
        rate[opens + 1:2 * CHUNK] = inside
        s[opens] = L
    if closes is not None:
        rate[closes + 1:] = 0.10
        if closes < n:
            s[closes] = L
    s[(lps < rate) & (s != L)] = L
    return s


def candidates_after(codes, first, upto, lps_range):
    """The four candidate ranges of the stretch that opens at `first`, after bin `upto`."""
    def norm(r):
        while r < 256:
            r <<= 1
        return r
    s = int(codes[first]) >> 1
    R = [norm(int(lps_range[(q << 7) + s])) for q in range(4)]
    for c in codes[first + 1:upto + 1].tolist():
        if c >> 1 == 126:
            continue
        s, sym = c >> 1, ((c >> 1) ^ c) & 1
        for q in range(4):
            rl = int(lps_range[((R[q] >> 6 & 3) << 7) + s])
            R[q] = norm(rl if sym else R[q] - rl)
    return R


def constructed(lps_range, mlps):
    """The streams of three chunks whose middle chunk opens and closes at chosen bins, and the shorter ones."""
    rng = np.random.default_rng(77001)
    out = []
    n = 3 * CHUNK
    # the opening LPS at each place of the chunk's first group and of a later one; the closing LPS at each place of the tail's first
    # group and of a later one
    for later in (0, 1):
        for j in range(8):
            opens, closes = CHUNK + 40 * later + j, 2 * CHUNK + 24 * later + 7 - j
            out.append(Stream(f"open{opens - CHUNK}-close{closes - 2 * CHUNK}", placed(rng, n, opens, closes)))
    out.append(Stream("no-lps-in-chunk", placed(rng, n, None, 2 * CHUNK + 300)))
    s = placed(rng, n, CHUNK + 3, None)
    out.append(Stream("never-closes", s))
    t = s.copy()
    t[-1] = T1
    out.append(Stream("closes-with-the-slice", t))
    for ms in (100, CHUNK - 1, CHUNK, CHUNK + 3, 1500, 2 * CHUNK - 4 - 1):   # too long at the tail's first bin, inside its first group, later, by the slice's last bin
        out.append(Stream(f"too-long-{ms}", s, max_stretch=ms))
    out.append(Stream("closes-before-too-long", placed(rng, n, CHUNK + 3, 2 * CHUNK + 5), max_stretch=CHUNK + 5))
    out.append(Stream("closes-at-too-long", placed(rng, n, CHUNK + 3, 2 * CHUNK + 5), max_stretch=CHUNK + 4))
    # candidates that never meet inside the chunk: bypass bins only from the opening bin to the closing one, which finds four candidates
    s = placed(rng, n, CHUNK + 21, 2 * CHUNK + 11)
    s[CHUNK + 22:2 * CHUNK + 11] = B
    ctx = np.arange(n) % 5
    ctx[CHUNK + 21] = 5                                          # (context 5 is in state 2: four different LPS ranges)
    out.append(Stream("never-meet", s, ctx))
    # ... and that meet in the opening group itself: the group's other bins on contexts 5 .. 9 (low states, ranges far apart), tried
    # until the four ranges are one by the group's last bin
    for opens in (CHUNK + 16, CHUNK + 48 + 2):
        base = placed(rng, n, opens, 2 * CHUNK + 2)
        ctx = np.arange(n) % 5
        group_end = opens | 7
        ctx[opens:group_end + 1] = 5 + np.arange(group_end + 1 - opens) % 5
        for attempt in range(4000):
            window = np.concatenate([[L], np.where(rng.random(group_end - opens) < 0.5, L, M)])
            states = np.concatenate([[10, 37, 62, 91, 120], rng.integers(0, 40, 5)])
            _, codes = Stream("", window, ctx[opens:group_end + 1], states).resolve(mlps)      # (nothing else touches contexts 5 .. 9)
            if len(set(candidates_after(codes, 0, window.size - 1, lps_range))) == 1:
                base[opens:group_end + 1] = window
                out.append(Stream(f"meet-in-group-{opens - CHUNK}", base, ctx, states))
                break
        else:
            raise AssertionError("no stream whose candidates meet in the opening group")
    # an opening and a closing bin between bypass bins and between terminate bins
    for name, other in (("bypass", B), ("terminate", T0)):
        for opens, closes in ((CHUNK + 4, 2 * CHUNK + 3), (CHUNK + 8, 2 * CHUNK + 7), (CHUNK + 15, 2 * CHUNK)):
            s = placed(rng, n, opens, closes)
            s[[opens - 1, opens + 1, closes - 1, closes + 1]] = other
            out.append(Stream(f"between-{name}-{opens - CHUNK}-{closes - 2 * CHUNK}", s))
    # the slice's last bin put_terminate(1), the bin before it the closing LPS; i1 no multiple of eight; shorter slices
    for n in LENGTHS:
        for k in range(2):
            s = background(rng, n, p_lps=(0.03, 0.15)[k])
            s[-1] = T1
            out.append(Stream(f"ends-{n}-{k}", s))
    s = placed(rng, 3 * CHUNK - 5, CHUNK + 1000, 2 * CHUNK + 1016)       # the closing bin in the slice's last, partial group
    out.append(Stream("closes-in-partial-group", s))
    s = placed(rng, 3 * CHUNK - 5, CHUNK + 1023, None)                   # opens at the chunk's last bin, runs to the end
    out.append(Stream("opens-at-last-bin", s))
    s = placed(rng, CHUNK + 9, CHUNK + 2, None)                          # the second chunk nine bins long
    out.append(Stream("short-second-chunk", s))
    out.append(Stream("five-bins", [M, L, B, M, T1]))
    out.append(Stream("one-bin", [T1]))
    return out


def random_streams(seed=77002, per_rate=4, rates=(0.02, 0.12, 0.40)):
    """Streams of the four lengths at three rates of coded LPS bins."""
    rng = np.random.default_rng(seed)
    out = []
    for rate in rates:
        for k in range(per_rate):
            n = LENGTHS[k % 4]
            s = background(rng, n, p_lps=rate)
            s[-1] = T1
            out.append(Stream(f"random-{rate}-{n}", s, ctx=rng.integers(0, N_CTX, n), states=rng.integers(0, 126, N_CTX)))
    return out


def wave_mix(seed=77003):
    """64 slices for one batch: a wave's 64 lanes are 64 consecutive chunks, here of about 25 slices of every rate and length, and
    every eighth slice has no coded LPS in the first 300 bins of a chunk: its lanes are still looking while the others' have merged."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(64):
        n = LENGTHS[i % 4]
        s = background(rng, n, p_lps=(0.02, 0.12, 0.40)[i % 3])
        if i % 8 == 7:
            late = (np.arange(n) % CHUNK < 300) & (s == L)
            late[:CHUNK] = False                                 # (chunk 0 opens at bin 0 whatever its bins are)
            s[late] = M
        s[-1] = T1
        out.append(Stream(f"mix-{i}", s, ctx=rng.integers(0, N_CTX, n), states=rng.integers(0, 126, N_CTX)))
    return out
