"""A second reading of H.264 slice_data() (CABAC, frame macroblocks), independent of avrecode-ms_amd/csrc/host/avr_h264.h.

Written from ITU-T H.264 clauses 7.3.4 - 7.3.5.3.3 (syntax), 9.3.2 (binarisations) and 9.3.3.1.1.1 - 9.3.3.1.3 (ctxIdx derivation);
it neither includes nor imports the parser and is laid out differently on purpose: what a macroblock leaves behind for its
neighbours lives in per-PICTURE arrays indexed by 4x4-block (or 8x8-block, or macroblock) position, and every neighbour is looked up
through one availability function (`Walker.mb_at`), where the parser keeps a `left_` / `up_` pair of macroblock records.

The walker never computes a bin.  At every decision it asks a bin source and writes the pair down as a K1 record of this project,
`(ctxIdx << 1) | bin` with BYPASS / TERMINATE as selectors, over 1024 states:

    replay    the bins come from a recorded stream (tests/host_api.cpp: t_parse_trace); the walker derives its own ctxIdx for each and
              raises `Mismatch` -- position, both selectors, the syntax element it was in -- where the record's differs
    generate  `Generator`, a seeded RNG that picks a VALUE per syntax element (every mb_type / sub_mb_type from a shuffled deck, so that
              each is drawn; ref_idx below the active count; mb_qp_delta in range; escapes within what 9.3.2.3 allows) and binarises it
              with an encoder-side reading of 9.3.2 -- the walker parses with a decoder-side one, and `Generator.begin` checks that the
              two used up the same bins.  `oracle.spec_cabac_encode` (9.3.4.2) turns the log into the slice's payload; `write_*` below add
              SPS, PPS, slice header, rbsp_trailing_bits, emulation prevention and start codes.

WHAT THIS DOES NOT PROVE.  There is no independent copy of Tables 9-12 ... 9-33 (the (m, n) pairs the context states start from) to
be had here, so the generated streams take their 4 x 1024 initial states from the parser's own init_state() (t_init_states).  The
tests built on this module check the DERIVATION of every ctxIdx and that `cabac_init_idc` selects a column at all; the numbers typed
into columns 1 and 2 stay unverified.  And where no real encoder's stream arbitrates, walker and parser
can share one misreading of the standard: replay on the two real clips bounds that for what x264 uses, nothing bounds it elsewhere.
"""
import random

BYPASS, TERMINATE = 1024, 1025
SLICE_P, SLICE_B, SLICE_I = 0, 1, 2


class Mismatch(AssertionError):
    pass


# ---------------------------------------------------------------------------------------------- Table 9-34 and friends
def _by_cat(lt5, c5, cb, c9, cr, c13):
    return [lt5] * 5 + [c5] + [cb] * 3 + [c9] + [cr] * 3 + [c13]


CBF_OFFSET = _by_cat(85, 1012, 460, 1012, 472, 1012)                 # coded_block_flag
CBF_CAT = [0, 4, 8, 12, 16, 0, 0, 4, 8, 4, 0, 4, 8, 8]
SIG_OFFSET = _by_cat(105, 402, 484, 660, 528, 718)                   # significant_coeff_flag, frame coded
LAST_OFFSET = _by_cat(166, 417, 572, 690, 616, 748)                  # last_significant_coeff_flag, frame coded
MAP_CAT = [0, 15, 29, 44, 47, 0, 0, 15, 29, 0, 0, 15, 29, 0]
ABS_OFFSET = _by_cat(227, 426, 952, 708, 982, 766)                   # coeff_abs_level_minus1
ABS_CAT = [0, 10, 20, 30, 39, 0, 0, 10, 20, 0, 0, 10, 20, 0]
# Table 9-43, frame coded 8x8 blocks, by levelListIdx
SIG_8X8 = [0, 1, 2, 3, 4, 5, 5, 4, 4, 3, 3, 4, 4, 4, 5, 5, 4, 4, 4, 4, 3, 3, 6, 7, 7, 7, 8, 9, 10, 9, 8, 7,
           7, 6, 11, 12, 13, 11, 6, 7, 8, 9, 14, 10, 9, 8, 6, 11, 12, 13, 11, 6, 9, 14, 10, 9, 11, 12, 13, 11, 14, 10, 12]
LAST_8X8 = [0] + [1] * 15 + [2] * 16 + [3] * 8 + [4] * 8 + [5] * 4 + [6] * 4 + [7] * 4 + [8] * 3

# Table 7-13 / 7-14: per mb_type, (partition shape, prediction of partition 0, of partition 1); shape 0 16x16, 1 16x8, 2 8x16, 3 8x8;
# prediction bit 0 = list 0, bit 1 = list 1, 0 = direct
L0, L1, BI = 1, 2, 3
B_TYPES = [(0, 0, 0), (0, L0, 0), (0, L1, 0), (0, BI, 0), (1, L0, L0), (2, L0, L0), (1, L1, L1), (2, L1, L1), (1, L0, L1), (2, L0, L1),
           (1, L1, L0), (2, L1, L0), (1, L0, BI), (2, L0, BI), (1, L1, BI), (2, L1, BI), (1, BI, L0), (2, BI, L0), (1, BI, L1), (2, BI, L1),
           (1, BI, BI), (2, BI, BI), (3, 0, 0)]
# Table 7-18: per B sub_mb_type, (prediction, sub-partition shape); shape 0 8x8, 1 8x4, 2 4x8, 3 4x4
B_SUB = [(0, 0), (L0, 0), (L1, 0), (BI, 0), (L0, 1), (L0, 2), (L1, 1), (L1, 2), (BI, 1), (BI, 2), (L0, 3), (L1, 3), (BI, 3)]
SUB_PARTS = {0: [(0, 0, 2, 2)], 1: [(0, 0, 2, 1), (0, 1, 2, 1)], 2: [(0, 0, 1, 2), (1, 0, 1, 2)],
             3: [(0, 0, 1, 1), (1, 0, 1, 1), (0, 1, 1, 1), (1, 1, 1, 1)]}


def count_limit(max_coeff):
    """The nonzero count the reference's count field cannot hold (recode.cpp:865): 2, 4 or 6 bits by block size."""
    return 64 if max_coeff > 16 else 16 if max_coeff > 4 else 4


class Picture:
    """What the macroblocks of one picture leave behind, by position: per macroblock, per luma 4x4 block (4 a side per macroblock),
    per 8x8 block (2 a side), per chroma 4x4 block of a 4:2:0 / 4:2:2 plane (2 wide, 2 or 4 high)."""

    def __init__(self, width, height, chroma):
        self.w, self.h, self.chroma = width, height, chroma
        n = width * height
        self.cw, self.ch = (2, 2) if chroma == 1 else (2, 4) if chroma == 2 else (0, 0)
        self.slice_of = [-1] * n
        self.skip, self.intra, self.nxn, self.direct, self.pcm = ([0] * n for _ in range(5))
        self.t8, self.cpm, self.cbp_l, self.cbp_c = ([0] * n for _ in range(4))
        self.dc = [[0] * n for _ in range(3)]                # coded_block_flag of the DC block of plane 0 / 1 / 2
        self.cbf_l = [[0] * (16 * n) for _ in range(3)]      # luma grid: luma, and Cb / Cr when 4:4:4
        self.cbf_c = [[0] * (self.cw * self.ch * n) for _ in range(2)]
        self.mvd = [[[0] * (16 * n) for _ in range(2)] for _ in range(2)]          # [list][comp], luma grid
        self.ref_gt0 = [[0] * (4 * n) for _ in range(2)]     # [list], 8x8 grid: refIdx > 0 of a partition that is predicted, not direct


class Walker:
    def __init__(self, pic, slice_id, slice_type, first_mb, refs, t8_mode, d8_inference, old_x264_444=False, recs=None, gen=None, keep_se=False):
        self.p, self.sid, self.type, self.first_mb, self.refs = pic, slice_id, slice_type, first_mb, refs
        self.t8_mode, self.d8, self.old444 = t8_mode, d8_inference, old_x264_444
        self.recs, self.pos, self.gen = recs, 0, gen
        self.log = []
        self.se = "start"
        self.addr = first_mb
        self.se_log = [] if keep_se else None
        self.pcm_at = []                                     # generate: log positions right after an I_PCM's terminate bin
        self.full_blocks = 0                                 # blocks whose nonzero count reaches count_limit()
        self.seen_mb_types, self.seen_sub_types = set(), set()

    # ------------------------------------------------------------------------------------------ the bin source
    def _take(self, sel):
        if self.recs is not None:
            if self.pos >= len(self.recs):
                raise Mismatch(f"recorded bins ran out at {self.pos} in {self.se}")
            r = self.recs[self.pos]
            if r >> 1 != sel:
                raise Mismatch(f"bin {self.pos}: the record says selector {r >> 1}, the walker derives {sel}, in {self.se} "
                               f"(macroblock {self.addr}, slice type {self.type})")
            self.pos += 1
            return r & 1
        b = self.gen.bit()
        self.log.append((sel << 1) | b)
        if self.se_log is not None:
            self.se_log.append(self.se)
        return b

    def ctx(self, c):
        return self._take(c)

    def byp(self):
        return self._take(BYPASS)

    def term(self):
        return self._take(TERMINATE)

    def begin(self, se, *info):
        self.se = se
        if self.gen is not None:
            self.gen.begin(se, *info)

    # ------------------------------------------------------------------------------------------ availability (6.4.x)
    def mb_at(self, x, y):
        """Address of the macroblock at (x, y) if it is available to the current one: inside the picture and already decoded in
        THIS slice (the current macroblock itself counts); else -1."""
        p = self.p
        if x < 0 or y < 0 or x >= p.w or y >= p.h:
            return -1
        a = y * p.w + x
        return a if p.slice_of[a] == self.sid else -1

    def block_mb(self, gx, gy, per_w, per_h):
        """The available macroblock that holds block (gx, gy) of a grid with per_w x per_h blocks a macroblock, or -1."""
        if gx < 0 or gy < 0:
            return -1
        return self.mb_at(gx // per_w, gy // per_h)

    # ------------------------------------------------------------------------------------------ slice_data(), 7.3.4
    def run(self, n_mbs=None):
        p = self.p
        addr, count = self.first_mb, 0
        self.prev_qp_nonzero = 0
        while True:
            if addr >= p.w * p.h:
                raise Mismatch("the slice runs past the end of the picture")
            self.start_mb(addr)
            skipped = 0
            if self.type != SLICE_I:
                self.begin("mb_skip_flag")
                inc = sum(1 for n in (self.A, self.B) if n >= 0 and not p.skip[n])
                skipped = self.ctx((11 if self.type == SLICE_P else 24) + inc)
            if skipped:
                p.skip[addr] = 1
                p.direct[addr] = 1 if self.type == SLICE_B else 0
                self.prev_qp_nonzero = 0
            else:
                self.macroblock_layer()
            count += 1
            self.begin("end_of_slice_flag", n_mbs is not None and count == n_mbs)
            if self.term():
                return count
            addr += 1

    def start_mb(self, addr):
        p = self.p
        self.addr, self.mx, self.my = addr, addr % p.w, addr // p.w
        p.slice_of[addr] = self.sid
        for a in (p.skip, p.intra, p.nxn, p.direct, p.pcm, p.t8, p.cpm, p.cbp_l, p.cbp_c, p.dc[0], p.dc[1], p.dc[2]):
            a[addr] = 0
        for by in range(4):
            base = (self.my * 4 + by) * 4 * p.w + self.mx * 4
            for pl in range(3):
                p.cbf_l[pl][base:base + 4] = [0, 0, 0, 0]
            for lst in range(2):
                for c in range(2):
                    p.mvd[lst][c][base:base + 4] = [0, 0, 0, 0]
        for by in range(p.ch):
            base = (self.my * p.ch + by) * 2 * p.w + self.mx * 2
            p.cbf_c[0][base:base + 2] = [0, 0]
            p.cbf_c[1][base:base + 2] = [0, 0]
        for ry in range(2):
            base = (self.my * 2 + ry) * 2 * p.w + self.mx * 2
            p.ref_gt0[0][base:base + 2] = [0, 0]
            p.ref_gt0[1][base:base + 2] = [0, 0]
        self.A, self.B = self.mb_at(self.mx - 1, self.my), self.mb_at(self.mx, self.my - 1)

    # ------------------------------------------------------------------------------------------ macroblock_layer(), 7.3.5
    def macroblock_layer(self):
        p = self.p
        self.begin("mb_type", self.type)
        if self.type == SLICE_I:
            # 9.3.3.1.1.3, ctxIdxOffset 3: condTermFlagN = 0 when N is not available or I_NxN
            inc = sum(1 for n in (self.A, self.B) if n >= 0 and not p.nxn[n])
            t = 0 if not self.ctx(3 + inc) else self.intra16_or_pcm(3 + 3, 3 + 4, (3 + 5, 3 + 6), (3 + 6, 3 + 7), 3 + 7)
            self.seen_mb_types.add(("I", t))
            return self.intra_mb(t)
        if self.type == SLICE_P:
            if self.ctx(14):                                 # prefix 1: an intra type, suffix at ctxIdxOffset 17
                t = 0 if not self.ctx(17) else self.intra16_or_pcm(17 + 1, 17 + 2, (17 + 2, 17 + 3), (17 + 3, 17 + 3), 17 + 3)
                self.seen_mb_types.add(("P", 5 + t))
                return self.intra_mb(t)
            if not self.ctx(15):
                t = 3 if self.ctx(16) else 0                 # 0 0 1 P_8x8, 0 0 0 P_L0_16x16
            else:
                t = 1 if self.ctx(17) else 2                 # 0 1 1 P_L0_L0_16x8, 0 1 0 P_L0_L0_8x16
            self.seen_mb_types.add(("P", t))
            return self.inter_mb(t, (t, L0, L0))
        # B slice, ctxIdxOffset 27 (Table 9-37 (b)); condTermFlagN = 0 when N is not available, B_Skip or B_Direct_16x16
        inc = sum(1 for n in (self.A, self.B) if n >= 0 and not p.direct[n])
        if not self.ctx(27 + inc):
            t = 0
        elif not self.ctx(27 + 3):
            t = 1 + self.ctx(27 + 5)
        else:
            v = self.ctx(27 + 4)
            for _ in range(3):
                v = 2 * v + self.ctx(27 + 5)
            if v < 8:                                        # 1 1 0 x x x
                t = 3 + v
            elif v == 13:                                    # 1 1 1 1 0 1: intra, suffix at ctxIdxOffset 32
                t = 0 if not self.ctx(32) else self.intra16_or_pcm(32 + 1, 32 + 2, (32 + 2, 32 + 3), (32 + 3, 32 + 3), 32 + 3)
                self.seen_mb_types.add(("B", 23 + t))
                return self.intra_mb(t)
            elif v == 14:
                t = 11
            elif v == 15:
                t = 22
            else:                                            # 1 1 1 0 x x x / 1 1 1 1 0 0 x: seven bins
                t = 2 * v + self.ctx(27 + 5) - 4
        self.seen_mb_types.add(("B", t))
        return self.inter_mb(t, B_TYPES[t])

    def intra16_or_pcm(self, c_luma, c_chroma, c4, c5, c6):
        """The bins of an intra mb_type after its first (Table 9-36): terminate bin (I_PCM), then I_16x16's luma cbp flag, chroma
        cbp (one or two bins) and prediction mode (two bins); the contexts of bins 4 and 5 depend on bin 3."""
        if self.term():
            return 25
        luma = self.ctx(c_luma)
        b3 = self.ctx(c_chroma)
        if b3:
            chroma = 1 + self.ctx(c4[0])
            mode = 2 * self.ctx(c5[0])
            mode += self.ctx(c6)
        else:
            chroma = 0
            mode = 2 * self.ctx(c4[1])
            mode += self.ctx(c5[1])
        return 1 + mode + 4 * chroma + 12 * luma

    # ------------------------------------------------------------------------------------------ intra macroblocks
    def intra_mb(self, t):
        p, addr = self.p, self.addr
        p.intra[addr] = 1
        if t == 25:                                          # I_PCM: its neighbours see it through the rules for I_PCM in 9.3.3.1.1.x
            p.pcm[addr] = 1
            p.cbp_l[addr], p.cbp_c[addr] = 15, 2
            self.prev_qp_nonzero = 0
            self.pcm_at.append(len(self.log))
            return
        if t == 0:
            p.nxn[addr] = 1
            if self.t8_mode:
                p.t8[addr] = self.transform_size_8x8_flag()
            for _ in range(4 if p.t8[addr] else 16):
                self.begin("prev_intra_pred_mode_flag")
                if not self.ctx(68):
                    self.begin("rem_intra_pred_mode")
                    self.ctx(69)
                    self.ctx(69)
                    self.ctx(69)
        if p.chroma in (1, 2):
            self.begin("intra_chroma_pred_mode")             # 9.3.3.1.1.8: N counts when it is intra, not I_PCM, with a mode other than 0
            inc = sum(1 for n in (self.A, self.B) if n >= 0 and p.intra[n] and not p.pcm[n] and p.cpm[n] != 0)
            m = 0
            if self.ctx(64 + inc):
                m = 1
                while m < 3 and self.ctx(64 + 3):
                    m += 1
            p.cpm[addr] = m
        if t == 0:
            self.coded_block_pattern()
        else:
            p.cbp_l[addr] = 15 if t >= 13 else 0
            p.cbp_c[addr] = ((t - 1) // 4) % 3
        if p.cbp_l[addr] or p.cbp_c[addr] or t != 0:
            self.mb_qp_delta()
            self.residual(t != 0)
        else:
            self.prev_qp_nonzero = 0

    def transform_size_8x8_flag(self):
        self.begin("transform_size_8x8_flag")
        return self.ctx(399 + sum(1 for n in (self.A, self.B) if n >= 0 and self.p.t8[n]))

    def coded_block_pattern(self):
        """9.3.3.1.1.4.  Prefix: one bin per 8x8 luma block; the neighbouring 8x8 block is looked up on the 8x8 grid."""
        p, addr = self.p, self.addr
        self.begin("coded_block_pattern", p.chroma in (1, 2))
        cbp = 0
        for b8 in range(4):
            inc = 0
            for k, (dx, dy) in enumerate(((-1, 0), (0, -1))):
                rx, ry = self.mx * 2 + (b8 & 1) + dx, self.my * 2 + (b8 >> 1) + dy
                n = self.block_mb(rx, ry, 2, 2)
                if n < 0 or p.pcm[n]:
                    cond = 0
                elif n == addr:
                    cond = 0 if (cbp >> ((ry & 1) * 2 + (rx & 1))) & 1 else 1
                elif p.skip[n]:
                    cond = 1
                else:
                    cond = 0 if (p.cbp_l[n] >> ((ry & 1) * 2 + (rx & 1))) & 1 else 1
                inc += cond << k
            cbp |= self.ctx(73 + inc) << b8
        p.cbp_l[addr] = cbp
        if p.chroma in (1, 2):
            def cond(n, bin_idx):
                if n < 0:
                    return 0
                if p.pcm[n]:
                    return 1
                if p.skip[n]:
                    return 0
                return int(p.cbp_c[n] != 0) if bin_idx == 0 else int(p.cbp_c[n] == 2)
            c = 0
            if self.ctx(77 + cond(self.A, 0) + 2 * cond(self.B, 0)):
                c = 1 + self.ctx(77 + 4 + cond(self.A, 1) + 2 * cond(self.B, 1))
            p.cbp_c[addr] = c

    def mb_qp_delta(self):
        self.begin("mb_qp_delta")                            # 9.3.3.1.1.5; unary, bins 0 / 1 / 2+ at ctxIdxInc (0 or 1) / 2 / 3
        n = 0
        if self.ctx(60 + self.prev_qp_nonzero):
            n = 1
            while self.ctx(60 + (2 if n == 1 else 3)):
                n += 1
                if n > 4096:
                    raise Mismatch("mb_qp_delta without end")
        self.prev_qp_nonzero = int(n != 0)

    # ------------------------------------------------------------------------------------------ inter macroblocks
    def inter_mb(self, t, shape_pred):
        p, addr = self.p, self.addr
        shape, pred0, pred1 = shape_pred
        is_b = self.type == SLICE_B
        # parts: (x, y, w, h) in 4x4 blocks inside the macroblock, prediction, in syntax order; a direct one has prediction 0
        parts, no_sub_below_8x8 = [], True
        if shape == 0:
            parts = [(0, 0, 4, 4, pred0)]
            if is_b and t == 0:
                p.direct[addr] = 1
        elif shape == 1:
            parts = [(0, 0, 4, 2, pred0), (0, 2, 4, 2, pred1)]
        elif shape == 2:
            parts = [(0, 0, 2, 4, pred0), (2, 0, 2, 4, pred1)]
        else:
            for q in range(4):
                self.begin("sub_mb_type", self.type)
                if not is_b:                                 # Table 9-37 (a): 1 8x8, 0 0 8x4, 0 1 1 4x8, 0 1 0 4x4; ctxIdx 21, 22, 23
                    s = 0 if self.ctx(21) else 1 if not self.ctx(22) else 2 if self.ctx(23) else 3
                    pr, sub = L0, s
                else:                                        # ctxIdxOffset 36: bins 0, 1 at 36, 37; bin 2 at 38 when bin 1 is set, else 39; then 39
                    if not self.ctx(36):
                        s = 0
                    elif not self.ctx(37):
                        s = 1 + self.ctx(39)
                    elif not self.ctx(38):
                        s = 3 + 2 * self.ctx(39)
                        s += self.ctx(39)
                    elif not self.ctx(39):
                        s = 7 + 2 * self.ctx(39)
                        s += self.ctx(39)
                    else:
                        s = 11 + self.ctx(39)
                    pr, sub = B_SUB[s]
                self.seen_sub_types.add(("B" if is_b else "P", s))
                x0, y0 = (q & 1) * 2, (q >> 1) * 2
                if is_b and s == 0:
                    if not self.d8:
                        no_sub_below_8x8 = False
                elif sub:
                    no_sub_below_8x8 = False
                parts.append((x0, y0, 2, 2, pr, [(x0 + a, y0 + b, c, d) for a, b, c, d in SUB_PARTS[sub]]))
        direct16 = is_b and t == 0
        if not direct16:
            for lst in range(2 if is_b else 1):              # all ref_idx_l0, then all ref_idx_l1 (7.3.5.1, 7.3.5.2)
                for part in parts:
                    if (part[4] >> lst) & 1 and self.refs[lst] > 1:
                        self.ref_idx(lst, part)
            for lst in range(2 if is_b else 1):
                for part in parts:
                    if (part[4] >> lst) & 1:
                        for x, y, w, h in (part[5] if len(part) > 5 else [part[:4]]):
                            self.mvd(lst, x, y, w, h)
        self.coded_block_pattern()
        if direct16 and not self.d8:
            no_sub_below_8x8 = False
        if p.cbp_l[addr] and self.t8_mode and no_sub_below_8x8:
            p.t8[addr] = self.transform_size_8x8_flag()
        if p.cbp_l[addr] or p.cbp_c[addr]:
            self.mb_qp_delta()
            self.residual(False)
        else:
            self.prev_qp_nonzero = 0

    def ref_idx(self, lst, part):
        """9.3.3.1.1.6: the 8x8 blocks left of and above the partition's corner count when they hold refIdx > 0 of a partition that is
        predicted from this list and not direct, in an available macroblock."""
        p = self.p
        self.begin("ref_idx", self.refs[lst] - 1)
        rx, ry = self.mx * 2 + part[0] // 2, self.my * 2 + part[1] // 2
        inc = 0
        for k, (x, y) in enumerate(((rx - 1, ry), (rx, ry - 1))):
            if self.block_mb(x, y, 2, 2) >= 0 and p.ref_gt0[lst][y * 2 * p.w + x]:
                inc += 1 << k
        v = 0
        if self.ctx(54 + inc):
            v = 1
            while self.ctx(54 + (4 if v == 1 else 5)):
                v += 1
                if v > 64:
                    raise Mismatch("ref_idx without end")
        for y in range(ry, ry + part[3] // 2):
            for x in range(rx, rx + part[2] // 2):
                p.ref_gt0[lst][y * 2 * p.w + x] = int(v > 0)

    def mvd(self, lst, x, y, w, h):
        """9.3.3.1.1.7 and UEG3 (9.3.2.3: signedValFlag 1, uCoff 9): per component, the sum of the absolute differences of the 4x4
        blocks left of and above the partition's corner selects the first bin's context."""
        p = self.p
        gx, gy = self.mx * 4 + x, self.my * 4 + y
        for comp in range(2):
            self.begin("mvd_x" if comp == 0 else "mvd_y")
            store = p.mvd[lst][comp]
            total = 0
            for nx, ny in ((gx - 1, gy), (gx, gy - 1)):
                if self.block_mb(nx, ny, 4, 4) >= 0:
                    total += store[ny * 4 * p.w + nx]
            base = 40 if comp == 0 else 47
            v = 0
            if self.ctx(base + (0 if total < 3 else 1 if total <= 32 else 2)):
                v = 1
                while v < 9 and self.ctx(base + min(2 + v, 6)):
                    v += 1
                if v == 9:
                    k = 3
                    while self.byp():
                        v += 1 << k
                        k += 1
                        if k > 40:
                            raise Mismatch("mvd escape without end")
                    for i in range(k - 1, -1, -1):
                        v += self.byp() << i
                self.byp()                                   # sign
            for j in range(gy, gy + h):
                row = j * 4 * p.w
                for i in range(gx, gx + w):
                    store[row + i] = v

    # ------------------------------------------------------------------------------------------ residual(), 7.3.5.3
    def residual(self, i16):
        p, addr = self.p, self.addr
        self.residual_luma(0, i16)
        if p.chroma in (1, 2):
            n_dc = 4 * (p.ch // 2)
            if p.cbp_c[addr]:
                for c in range(2):                           # chroma DC, ctxBlockCat 3
                    inc = self.dc_inc(1 + c, lambda n: p.cbp_c[n] != 0)
                    p.dc[1 + c][addr] = self.block(3, n_dc, inc)
            if p.cbp_c[addr] == 2:
                for c in range(2):                           # chroma AC, ctxBlockCat 4: blocks in raster order of a 2-wide plane
                    for blk in range(n_dc):
                        gx, gy = self.mx * 2 + (blk & 1), self.my * p.ch + (blk >> 1)
                        inc = 0
                        for k, (nx, ny) in enumerate(((gx - 1, gy), (gx, gy - 1))):
                            inc += self.cbf_cond(self.block_mb(nx, ny, 2, p.ch), p.cbf_c[c], ny * 2 * p.w + nx, False) << k
                        p.cbf_c[c][gy * 2 * p.w + gx] = self.block(4, 15, inc)
        elif p.chroma == 3:
            self.residual_luma(1, i16)
            self.residual_luma(2, i16)

    def dc_inc(self, plane, has_block):
        """ctxIdxInc of a DC block's coded_block_flag: the DC block of the same plane in A and B, where that macroblock has one."""
        p = self.p
        inc = 0
        for k, n in enumerate((self.A, self.B)):
            if n < 0:
                cond = p.intra[self.addr]
            elif p.pcm[n]:
                cond = 1
            elif p.skip[n] or not has_block(n):
                cond = 0
            else:
                cond = p.dc[plane][n]
            inc += cond << k
        return inc

    def cbf_cond(self, n, store, index, need_8x8):
        """condTermFlagN of 9.3.3.1.1.9 for a block of macroblock n (or -1) whose coded_block_flag sits at store[index]."""
        p = self.p
        if n < 0:
            return p.intra[self.addr]
        if p.pcm[n]:
            return 1
        if need_8x8 and not p.t8[n]:                         # an 8x8 block's neighbour is an 8x8 block or nothing
            return p.intra[self.addr] if self.old444 else 0  # (x264 before build 151 treated it as an unavailable macroblock)
        if p.skip[n]:
            return 0
        return store[index]                                  # 0 where the block was not coded (its cbp bit clear)

    def residual_luma(self, plane, i16):
        p, addr = self.p, self.addr
        cat_dc, cat_ac, cat_4x4, cat_8x8 = ((0, 1, 2, 5), (6, 7, 8, 9), (10, 11, 12, 13))[plane]
        store = p.cbf_l[plane]
        gw = 4 * p.w
        if i16:
            inc = self.dc_inc(plane, lambda n: p.intra[n] and not p.nxn[n])
            p.dc[plane][addr] = self.block(cat_dc, 16, inc)
        for b8 in range(4):
            if not (p.cbp_l[addr] >> b8) & 1:
                continue
            bx, by = self.mx * 4 + (b8 & 1) * 2, self.my * 4 + (b8 >> 1) * 2
            if p.t8[addr]:
                if p.chroma == 3:                            # 7.3.5.3.3: an 8x8 block's coded_block_flag is sent only with 4:4:4
                    inc = 0
                    for k, (nx, ny) in enumerate(((bx - 1, by), (bx, by - 1))):
                        inc += self.cbf_cond(self.block_mb(nx, ny, 4, 4), store, ny * gw + nx, True) << k
                    flag = self.block(cat_8x8, 64, inc)
                else:
                    flag = self.block(cat_8x8, 64, None)     # ... otherwise inferred 1
                for j in range(2):
                    for i in range(2):
                        store[(by + j) * gw + bx + i] = flag
            else:
                for b4 in range(4):
                    gx, gy = bx + (b4 & 1), by + (b4 >> 1)
                    inc = 0
                    for k, (nx, ny) in enumerate(((gx - 1, gy), (gx, gy - 1))):
                        inc += self.cbf_cond(self.block_mb(nx, ny, 4, 4), store, ny * gw + nx, False) << k
                    store[gy * gw + gx] = self.block(cat_ac if i16 else cat_4x4, 15 if i16 else 16, inc)

    def block(self, cat, max_coeff, cbf_inc):
        """residual_block_cabac(), 7.3.5.3.3 / 9.3.3.1.3.  Returns the coded_block_flag."""
        if cbf_inc is not None:
            self.begin("coded_block_flag")
            if not self.ctx(CBF_OFFSET[cat] + CBF_CAT[cat] + cbf_inc):
                return 0
        sig, last = SIG_OFFSET[cat] + MAP_CAT[cat], LAST_OFFSET[cat] + MAP_CAT[cat]
        is8 = cat in (5, 9, 13)
        c8 = (2 if self.p.chroma == 2 else 1) if cat == 3 else 1           # NumC8x8 = 4 / (SubWidthC * SubHeightC)
        count, i = 0, 0
        while i < max_coeff - 1:
            if is8:
                a, b = SIG_8X8[i], LAST_8X8[i]
            elif cat == 3:
                a = b = min(i // c8, 2)
            else:
                a = b = i
            self.begin("significant_coeff_flag", i, count, max_coeff)
            if self.ctx(sig + a):
                count += 1
                self.begin("last_significant_coeff_flag", i, count, max_coeff)
                if self.ctx(last + b):
                    break
            i += 1
        else:
            count += 1                                       # no last flag: the final coefficient is significant by inference
        if count >= count_limit(max_coeff):
            self.full_blocks += 1
        base = ABS_OFFSET[cat] + ABS_CAT[cat]
        gt1 = eq1 = 0
        for _ in range(count):                               # in reverse scan order
            self.begin("coeff_abs_level_minus1")
            if not self.ctx(base + (0 if gt1 else min(4, 1 + eq1))):
                eq1 += 1
            else:
                c = base + 5 + min(4 - (1 if cat == 3 else 0), gt1)
                n = 1
                while n < 14 and self.ctx(c):
                    n += 1
                if n == 14:                                  # UEG0 suffix
                    k = 0
                    while self.byp():
                        k += 1
                        if k > 40:
                            raise Mismatch("coeff_abs_level_minus1 escape without end")
                    for _ in range(k):
                        self.byp()
                gt1 += 1
            self.begin("coeff_sign_flag")
            self.byp()
        return 1


# ---------------------------------------------------------------------------------------------- the generating bin source
def _tu(v, cmax):
    return [1] * min(v, cmax) + ([0] if v < cmax else [])


def _egk(v, k):
    out = []
    while v >= (1 << k):
        out.append(1)
        v -= 1 << k
        k += 1
    out.append(0)
    return out + [(v >> i) & 1 for i in range(k - 1, -1, -1)]


def _i_type_bins(t):                                         # Table 9-36 without the first bin's context question
    if t == 0:
        return [0]
    if t == 25:
        return [1, 1]
    mode, chroma, luma = (t - 1) % 4, ((t - 1) // 4) % 3, (t - 1) // 12
    return [1, 0, luma] + ([0] if chroma == 0 else [1, chroma - 1]) + [mode >> 1, mode & 1]


P_TYPE_BINS = {0: [0, 0, 0], 1: [0, 1, 1], 2: [0, 1, 0], 3: [0, 0, 1]}
B_TYPE_BINS = ["0", "100", "101", "110000", "110001", "110010", "110011", "110100", "110101", "110110", "110111", "111110",
               "1110000", "1110001", "1110010", "1110011", "1110100", "1110101", "1110110", "1110111", "1111000", "1111001", "111111"]
P_SUB_BINS = {0: [1], 1: [0, 0], 2: [0, 1, 1], 3: [0, 1, 0]}
B_SUB_BINS = ["0", "100", "101", "11000", "11001", "11010", "11011", "111000", "111001", "111010", "111011", "11110", "11111"]


class Generator:
    """Chooses a value per syntax element and hands out its bins.  `profile` keys (all optional): p_skip, p_intra (in P / B slices),
    p_cbp (per luma bit), p_cbf, p_sig, p_last, p_t8, refs_high (draw large ref_idx), mvd (list of |mvd| to draw from), levels (list of
    coeff_abs_level_minus1 to draw from), qp (list of mapped mb_qp_delta), pcm (allow I_PCM; pcm_once: one only), no_full_blocks (keep
    every block's nonzero count below count_limit()), i16_only.  `decks`: a dict shared by the generators of one file, so that the
    shuffled decks of mb_type / sub_mb_type values run on from slice to slice."""

    def __init__(self, seed, profile=None, decks=None):
        self.r = random.Random(seed)
        self.o = dict(p_skip=0.15, p_intra=0.2, p_cbp=0.6, p_cbf=0.7, p_sig=0.5, p_last=0.25, p_t8=0.5, refs_high=False,
                      mvd=[0, 0, 0, 1, 1, 2, 3, 5, 8, 9, 12, 16, 17, 31, 33, 40, 70, 300, 5000],
                      levels=[0] * 8 + list(range(1, 16)) + [20, 200, 30000],
                      qp=[0] * 6 + [1, 2, 3, 4, 7, 20, 52], pcm=False, no_full_blocks=False, i16_only=False, pcm_once=False)
        self.o.update(profile or {})
        self.q = []
        self.decks = {} if decks is None else decks
        self.se = None
        self.pcm_done = False

    def deck(self, name, values):
        d = self.decks.get(name)
        if not d:
            d = self.decks[name] = list(values)
            self.r.shuffle(d)
        return d.pop()

    def bit(self):
        if not self.q:
            raise Mismatch(f"the walker asks for a bin that the binarisation of {self.se} does not have")
        return self.q.pop(0)

    def flag(self, p):
        return [int(self.r.random() < p)]

    def begin(self, se, *info):
        if self.q:
            raise Mismatch(f"{len(self.q)} bins of {self.se} were not parsed")
        self.se = se
        o, r = self.o, self.r
        if se == "mb_skip_flag":
            self.q = self.flag(o["p_skip"])
        elif se == "end_of_slice_flag":
            self.q = [int(info[0])]
        elif se == "mb_type":
            self.q = self.mb_type_bins(info[0])
        elif se == "sub_mb_type":
            self.q = (list(P_SUB_BINS[self.deck("ps", range(4))]) if info[0] == SLICE_P
                      else [int(c) for c in B_SUB_BINS[self.deck("bs", range(13))]])
        elif se == "ref_idx":
            v = r.choice([0, 0, 1, info[0], r.randint(0, info[0])]) if o["refs_high"] else r.choice([0, 0, r.randint(0, info[0])])
            self.q = [1] * min(v, info[0]) + [0]
        elif se in ("mvd_x", "mvd_y"):
            v = r.choice(o["mvd"])
            self.q = _tu(v, 9) + (_egk(v - 9, 3) if v >= 9 else []) + ([r.getrandbits(1)] if v else [])
        elif se == "mb_qp_delta":
            self.q = [1] * r.choice(o["qp"]) + [0]
        elif se == "transform_size_8x8_flag":
            self.q = self.flag(o["p_t8"])
        elif se == "prev_intra_pred_mode_flag":
            self.q = self.flag(0.5)
        elif se == "rem_intra_pred_mode":
            self.q = [r.getrandbits(1) for _ in range(3)]
        elif se == "intra_chroma_pred_mode":
            self.q = _tu(r.randint(0, 3), 3)
        elif se == "coded_block_pattern":
            self.q = [int(r.random() < o["p_cbp"]) for _ in range(4)]
            if info[0]:
                c = r.randint(0, 2)
                self.q += [0] if c == 0 else [1, c - 1]
        elif se == "coded_block_flag":
            self.q = self.flag(o["p_cbf"])
        elif se == "significant_coeff_flag":
            i, count, max_coeff = info
            if o["no_full_blocks"] and max_coeff in (4, 16, 64) and i == max_coeff - 2 and count == i:
                self.q = [0]                                 # every coefficient so far is nonzero and the last would be by inference
            else:
                self.q = self.flag(o["p_sig"])
        elif se == "last_significant_coeff_flag":
            self.q = self.flag(o["p_last"])
        elif se == "coeff_abs_level_minus1":
            v = r.choice(o["levels"])
            self.q = _tu(v, 14) + (_egk(v - 14, 0) if v >= 14 else [])
        elif se == "coeff_sign_flag":
            self.q = [r.getrandbits(1)]
        else:
            raise Mismatch(f"the generator does not know {se}")

    def mb_type_bins(self, slice_type):
        o, r = self.o, self.r
        pcm = o["pcm"] and not (o["pcm_once"] and self.pcm_done)

        def intra():
            if o["i16_only"]:
                t = self.deck("i16", range(1, 25))
            elif pcm:
                t = self.deck("ipcm", [25, 0, 3, 14])
            else:
                t = self.deck("i", list(range(25)) + [0] * 6)
            if t == 25:
                self.pcm_done = True
            return _i_type_bins(t)
        if slice_type == SLICE_I:
            return intra()
        if r.random() < o["p_intra"]:
            return ([1] if slice_type == SLICE_P else [1, 1, 1, 1, 0, 1]) + intra()
        if slice_type == SLICE_P:
            return list(P_TYPE_BINS[self.deck("p", [0, 1, 2, 3, 3, 3])])
        return [int(c) for c in B_TYPE_BINS[self.deck("b", list(range(23)) + [22] * 6)]]


# ---------------------------------------------------------------------------------------------- bits, NAL units, headers
class Bits:
    def __init__(self):
        self.b = []

    def u(self, n, v):
        self.b += [(v >> i) & 1 for i in range(n - 1, -1, -1)]
        return self

    def ue(self, v):
        n = (v + 1).bit_length()
        return self.u(n - 1, 0).u(n, v + 1)

    def se(self, v):
        return self.ue(2 * v - 1 if v > 0 else -2 * v)

    def trailing(self):
        self.b.append(1)
        self.b += [0] * (-len(self.b) % 8)
        return self

    def align(self, bit):
        self.b += [bit] * (-len(self.b) % 8)
        return self

    def bytes(self):
        assert len(self.b) % 8 == 0
        return bytes(int("".join(map(str, self.b[i:i + 8])), 2) for i in range(0, len(self.b), 8))


def escape(rbsp):
    """7.4.1: emulation_prevention_three_byte before a byte <= 3 that follows two zeros, and after a final zero."""
    out, zeros = bytearray(), 0
    for v in rbsp:
        if zeros >= 2 and v <= 3:
            out.append(3)
            zeros = 0
        out.append(v)
        zeros = zeros + 1 if v == 0 else 0
    if rbsp and rbsp[-1] == 0:
        out.append(3)
    return bytes(out)


def nal(ref_idc, unit_type, rbsp, long_start=False):
    return (b"\0\0\0\1" if long_start else b"\0\0\1") + bytes([(ref_idc << 5) | unit_type]) + escape(rbsp)


def scaling_list(b, size, mode, rng):
    """7.3.2.1.1.1.  mode: 'full' every delta_scale, 'short' nextScale = 0 part of the way, 'default' nextScale = 0 at once."""
    last = 8
    for j in range(size):
        if mode == "default" or (mode == "short" and j == size // 3):
            d = -last
            b.se(d + 256 if d < -128 else d)
            return
        nxt = rng.randint(1, 255)
        d = nxt - last
        b.se(d - 256 if d > 127 else d + 256 if d < -128 else d)
        last = nxt


def write_sps(s, rng):
    """7.3.2.1.1.  s: dict with chroma, width, height, and optional poc_type, frame_mbs_only, direct_8x8, scaling, id, log2_frame_num,
    log2_poc_lsb, delta_always_zero, profile."""
    b = Bits()
    chroma = s["chroma"]
    profile = s.get("profile", {0: 100, 1: 100, 2: 122, 3: 244}[chroma])
    b.u(8, profile).u(8, 0).u(8, 40).ue(s.get("id", 0))
    if profile in (100, 110, 122, 244, 44, 83, 86, 118, 128, 138, 139, 134, 135):
        b.ue(chroma)
        if chroma == 3:
            b.u(1, 0)
        b.ue(0).ue(0).u(1, 0)
        modes = s.get("scaling")
        b.u(1, 1 if modes else 0)
        if modes:
            for i in range(8 if chroma != 3 else 12):
                m = modes[i % len(modes)]
                b.u(1, 0 if m is None else 1)
                if m is not None:
                    scaling_list(b, 16 if i < 6 else 64, m, rng)
    else:
        assert chroma == 1 and not s.get("scaling")
    b.ue(s.get("log2_frame_num", 4) - 4)
    poc = s.get("poc_type", 0)
    b.ue(poc)
    if poc == 0:
        b.ue(s.get("log2_poc_lsb", 6) - 4)
    elif poc == 1:
        b.u(1, s.get("delta_always_zero", 0)).se(-3).se(5).ue(3).se(2).se(-1).se(7)
    b.ue(4).u(1, 0).ue(s["width"] - 1)
    fmo = s.get("frame_mbs_only", 1)
    b.ue((s["height"] if fmo else s["height"] // 2) - 1).u(1, fmo)
    if not fmo:
        b.u(1, 0)
    b.u(1, s.get("direct_8x8", 1)).u(1, 0).u(1, 0)
    return b.trailing().bytes()


def write_pps(p, sps, rng):
    """7.3.2.2.  p: dict with id and optional cabac, bottom_poc, slice_groups, refs, weighted, bipred, init_qp, deblock, redundant, t8,
    scaling."""
    b = Bits()
    b.ue(p.get("id", 0)).ue(sps.get("id", 0)).u(1, p.get("cabac", 1)).u(1, p.get("bottom_poc", 0))
    groups = p.get("slice_groups", 1)
    b.ue(groups - 1)
    if groups > 1:
        b.ue(0)                                              # slice_group_map_type 0: interleaved, a run length per group
        for _ in range(groups):
            b.ue(2)
    refs = p.get("refs", (1, 1))
    b.ue(refs[0] - 1).ue(refs[1] - 1).u(1, p.get("weighted", 0)).u(2, p.get("bipred", 0))
    b.se(p.get("init_qp", 26) - 26).se(0).se(p.get("chroma_qp_offset", 0))
    b.u(1, p.get("deblock", 0)).u(1, 0).u(1, p.get("redundant", 0))
    if p.get("t8", 0) or p.get("scaling"):
        b.u(1, p.get("t8", 0))
        modes = p.get("scaling")
        b.u(1, 1 if modes else 0)
        if modes:
            for i in range(6 + (2 if sps["chroma"] != 3 else 6) * p.get("t8", 0)):
                m = modes[i % len(modes)]
                b.u(1, 0 if m is None else 1)
                if m is not None:
                    scaling_list(b, 16 if i < 6 else 64, m, rng)
        b.se(p.get("chroma_qp_offset", 0))
    return b.trailing().bytes()


def write_slice_header(h, sps, pps, rng):
    """7.3.3, every branch the parser reads.  h: dict with first_mb, type, qp, idr, ref_idc and optional cabac_init_idc, refs (override),
    rplm, mmco, deblock_idc, frame_num, redundant_cnt.  Returns (the header's bits -- aligned with cabac_alignment_one_bit when the picture
    parameter set says CABAC --, the active reference counts)."""
    b = Bits()
    t = h["type"]
    b.ue(h["first_mb"]).ue(t + 5 * h.get("type_plus5", 0)).ue(pps.get("id", 0))
    b.u(sps.get("log2_frame_num", 4), h.get("frame_num", 0))
    if not sps.get("frame_mbs_only", 1):
        b.u(1, 0)                                            # field_pic_flag
    if h["idr"]:
        b.ue(h.get("idr_pic_id", 0))
    poc = sps.get("poc_type", 0)
    if poc == 0:
        b.u(sps.get("log2_poc_lsb", 6), h.get("poc_lsb", 0))
        if pps.get("bottom_poc", 0):
            b.se(h.get("delta_poc_bottom", -2))
    elif poc == 1 and not sps.get("delta_always_zero", 0):
        b.se(h.get("delta_poc0", 3))
        if pps.get("bottom_poc", 0):
            b.se(h.get("delta_poc1", -1))
    if pps.get("redundant", 0):
        b.ue(h.get("redundant_cnt", 0))
    if t == SLICE_B:
        b.u(1, h.get("direct_spatial", 1))
    refs = list(pps.get("refs", (1, 1)))
    if t != SLICE_I:
        over = h.get("refs")
        b.u(1, 1 if over else 0)
        if over:
            b.ue(over[0] - 1)
            refs[0] = over[0]
            if t == SLICE_B:
                b.ue(over[1] - 1)
                refs[1] = over[1]
        for lst in range(2 if t == SLICE_B else 1):          # ref_pic_list_modification()
            ops = h.get("rplm", ((), ()))[lst]
            b.u(1, 1 if ops else 0)
            if ops:
                for idc, v in ops:
                    b.ue(idc).ue(v)
                b.ue(3)
        if (pps.get("weighted", 0) and t == SLICE_P) or (pps.get("bipred", 0) == 1 and t == SLICE_B):
            b.ue(rng.randint(0, 7))                          # pred_weight_table()
            if sps["chroma"] != 0:
                b.ue(rng.randint(0, 7))
            for lst in range(2 if t == SLICE_B else 1):
                for _ in range(refs[lst]):
                    f = rng.getrandbits(1)
                    b.u(1, f)
                    if f:
                        b.se(rng.randint(-128, 127)).se(rng.randint(-128, 127))
                    if sps["chroma"] != 0:
                        f = rng.getrandbits(1)
                        b.u(1, f)
                        if f:
                            for _ in range(4):
                                b.se(rng.randint(-128, 127))
    if h["ref_idc"]:                                         # dec_ref_pic_marking()
        if h["idr"]:
            b.u(1, 0).u(1, h.get("long_term_reference", 0))
        else:
            ops = h.get("mmco")
            b.u(1, 1 if ops else 0)
            if ops:
                for op in ops:
                    b.ue(op)
                    if op in (1, 3):
                        b.ue(rng.randint(0, 9))
                    if op == 2:
                        b.ue(rng.randint(0, 9))
                    if op in (3, 6):
                        b.ue(rng.randint(0, 3))
                    if op == 4:
                        b.ue(rng.randint(0, 5))
                b.ue(0)
    if pps.get("cabac", 1) and t != SLICE_I:
        b.ue(h.get("cabac_init_idc", 0))
    b.se(h["qp"] - pps.get("init_qp", 26))
    if pps.get("deblock", 0):
        idc = h.get("deblock_idc", 0)
        b.ue(idc)
        if idc != 1:
            b.se(rng.randint(-6, 6)).se(rng.randint(-6, 6))
    if pps.get("cabac", 1):
        b.align(1)
    return b, refs
