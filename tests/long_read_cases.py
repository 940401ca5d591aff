"""Seeded windows for the alignment path (plat_align_window_batch and its asynchronous twin) with reads of 251 to 2000 bases, the lengths at
which plat_align.hip takes code the committed goldens and the other seeded batches never enter: k_pairs sends every read above 256 bases to
the exact vote of k_seed_slow, k_prep_reads stages a window through LDS only while its longest read has at most 448 bases, and the scratch
sizes (LDS image, diagonal counters, traceback rows) follow the longest read of the batch.  Plain Python and numpy, no device and no oracle:
tests/test_long_read_cases_cpu.py checks on the oracle alone that the batches do what they are here for, tests/test_gpu_long_reads.py
compares the device with the oracle on them."""
import numpy as np

from platypus_amd import hostapi as H

# both thresholds at +-1, the 64-base chunk boundaries of the fifth to ninth plane word, two lengths far out
LADDER = (251, 256, 257, 319, 320, 321, 447, 448, 449, 511, 512, 513, 640, 1000, 2000)
QUAL_MEANS = (20, 36, 60, 90)
WS = 5000                                                                  # first base of every window
B = b"ACGT"
# the windows of ladder_batch, in order: (name, reads).  few / many: the two pair packings of k_pairs (fewer than 13 reads: whole haplotypes
# to a wave; otherwise 64 pairs) and a second, partial group of 64 reads in k_prep_reads; tandem: a repeat across the site, several
# arg-max diagonals in the vote; hapn: N's in the haplotypes; edge: a flank shorter than the reads, which overhang both haplotype ends
LADDER_WINDOWS = (("plain", 20), ("few", 9), ("many", 70), ("tandem", 16), ("hapn", 16), ("edge", 16), ("plain", 14), ("tandem", 13))
# flank mode: a read's last bases right of the site; see _window
FLANK_SAFE_TAIL = 100


def _rnd(rng, n):
    return bytes(rng.choice(list(B), n).astype(np.uint8))


def _sub(rng, c):
    return B[((B.index(c) if c in B else 0) + 1 + int(rng.integers(0, 3))) % 4]


def _quals(rng, L, mean, tail):
    q = np.clip(rng.normal(mean, 6, L), 2, 93).astype(np.uint8)
    if tail:                                                               # a low-quality tail, as a sequencer leaves it
        n = int(rng.integers(10, 41))
        q[L - n:] = rng.integers(2, 11, n).astype(np.uint8)
    return bytes(q.tolist())


def _haplotypes(rng, L, W, buf, name, indels):
    """The reference, a SNP, a 5-base deletion and a 12-base insertion, the last two at one site inside the window (indels=False: SNPs only).
    Returns (haplotypes, shift of each right of the site, site)."""
    ref = bytearray(_rnd(rng, W + 2 * buf))
    site = buf + int(rng.integers(2, W - 2))
    unit = b""
    if name == "tandem":                                                   # a homopolymer or a repeat of unit 2..6 across the site
        unit = _rnd(rng, int(rng.choice([1, 2, 3, 4, 6])))
        k = int(rng.integers(30, 60))
        a = site - k // 2
        ref[a:a + k] = (unit * k)[:k]
    if name == "hapn":
        for _ in range(3):
            p = int(rng.integers(max(0, buf - L // 2), min(len(ref) - 4, buf + W + L // 2)))
            n = int(rng.integers(1, 4))
            ref[p:p + n] = b"N" * n
    ref = bytes(ref[:W + 2 * buf])
    snp = bytearray(ref)
    p = buf + int(rng.integers(0, W))
    snp[p] = _sub(rng, snp[p:p + 1])
    haps, shifts = [ref, bytes(snp)], [0, 0]
    if indels:
        haps.append(ref[:site] + ref[site + 5:]); shifts.append(-5)
        haps.append(ref[:site] + ((unit * 12)[:12] if unit else _rnd(rng, 12)) + ref[site:]); shifts.append(12)
    else:
        snp2 = bytearray(ref)
        p2 = buf + (p - buf + 1 + int(rng.integers(0, W - 1))) % W
        snp2[p2] = _sub(rng, snp2[p2:p2 + 1])
        haps.append(bytes(snp2)); shifts.append(0)
    return haps, shifts, site


def _edited(rng, src, off, L, i, clean):
    """L bases of `src` from `off` (random bases where that lies outside it) with 0..3 substitutions; every third read carries an indel of 1..8
    bases, some an N."""
    seq = bytearray(src[p] if 0 <= p < len(src) else B[int(rng.integers(0, 4))] for p in range(off, off + L))
    if clean:
        return bytes(seq)
    for _ in range(int(rng.integers(0, 4))):
        p = int(rng.choice([0, L - 1, int(rng.integers(0, L)), int(rng.integers(0, L))]))
        seq[p] = _sub(rng, seq[p:p + 1])
    if i % 3 == 0:
        n = int(rng.integers(1, 9))
        p = int(rng.choice([int(rng.integers(1, 20)), L - int(rng.integers(2, 20)), int(rng.integers(1, L - 1))]))
        if rng.random() < 0.5:                                             # bases inserted into the read, its tail drops off
            seq[p:p] = _rnd(rng, n)
            del seq[L:]
        else:                                                              # bases deleted from the read, the source fills the tail
            del seq[p:p + n]
            need = L - len(seq)
            tail = src[off + L:off + L + need]
            seq += tail + _rnd(rng, need - len(tail))
    if i % 7 == 3:
        seq[int(rng.integers(0, L))] = ord("N")
    return bytes(seq)


def _window(rng, lengths, name, flank_safe=False, clean=False, qmeans=QUAL_MEANS, extras=True, long_kind=None, pin_left=None):
    """One window spec for hostapi._pack_windows.  lengths: the length of every read that overlaps the window, in the order of their making;
    the flank follows the longest, min(2 L, 2500), except in an edge window (L // 3 + 8: reads start at haplotype offsets below 16, end within
    L + 15 of the haplotype's end or hang over either end).
    flank_safe: for --calculateFlankScore.  The reference's traceback is undefined for a DP in which no final cell stays below 0x7800 (plain
    score 15 872), so no DP of any pair may get there: a read lies left of the indel site but for its last FLANK_SAFE_TAIL bases at the most
    (those bases are all a DP at the mapping position can lose against a haplotype shifted right of the site: 100 x 93 < 15 872), mapping
    positions are within 2 bases of the truth, no mate is placed elsewhere, an edge window's haplotypes differ by SNPs only and its reads
    neither hang over a haplotype end nor end within 10 bases of it (the DP at the clamped mapping position would lose the whole read).
    long_kind: (length, "bad") puts the reads of that length among the bad reads, which follow the good ones in the window's read list.
    pin_left: reads of that length start left of every read of at most 250 bases."""
    Lmax = max(lengths)
    edge = name == "edge"
    buf = Lmax // 3 + 8 if edge else min(2 * Lmax, 2500)
    W = int(rng.integers(Lmax // 3 + 60, Lmax // 3 + 100)) if edge else int(rng.integers(20, 80))
    haps, shifts, site = _haplotypes(rng, Lmax, W, buf, name, indels=not (edge and flank_safe))
    good, bad, broken = [], [], []
    for i, L in enumerate(lengths):
        j = i % len(haps)                                                  # reads come from every haplotype
        src = haps[j]
        lo, hi = max(0, buf - L + 8), min(len(src) - L, buf + W - 8)
        if flank_safe and not edge:
            hi = min(hi, site + FLANK_SAFE_TAIL - L)
        if edge:
            m = i % 4
            over = L > buf + 24 and not flank_safe                         # (a read that hangs over an end by more than the band fits no DP)
            off = (int(rng.integers(0, 16)) if m == 0 else len(src) - L - int(rng.integers(10 if flank_safe else 0, 19)) if m == 1
                   else -int(rng.integers(1, 12)) if m == 2 and over else len(src) - L + int(rng.integers(1, 12)) if m == 3 and over
                   else int(rng.integers(lo, max(hi, lo) + 1)))
        elif L == pin_left:
            off = lo + int(rng.integers(0, 20))
        else:
            off = int(rng.integers(lo, max(hi, lo) + 1))
        refoff = off if off <= site else max(off - shifts[j], site)        # where a mapper puts the read's first base
        seq = _edited(rng, src, off, L, i, clean)
        qual = _quals(rng, L, int(qmeans[i % len(qmeans)]), tail=(not clean and i % 5 == 2))
        jitter = int(rng.integers(-2, 2)) if (not clean and i % 4 == 1) else 0
        r = H.AlignedRead(seq, qual, WS - buf + refoff + jitter, int(rng.choice([60, 60, 60, 29])), 3)
        (bad if long_kind is not None and L == long_kind[0] else good).append(r)
    if extras and not edge:
        L = lengths[0]
        if buf + 3 - L >= 0:                                               # overlap with the window 3 < 7: skipped
            good.append(H.AlignedRead(haps[0][buf + 3 - L:buf + 3], _quals(rng, L, 36, False), WS + 3 - L, 60, 3))
        bad.append(H.AlignedRead(haps[0][buf - L // 2:buf - L // 2 + L], _quals(rng, L, 36, False), WS - L // 2, 60, 3 | 512))    # QCFail: skipped
        if not flank_safe:                                                 # a mate mapped elsewhere: its DP at the mapping position fits nowhere
            off = int(rng.integers(lo, max(hi, lo) + 1))
            broken.append(H.AlignedRead(_edited(rng, haps[1], off, L, 1, clean), _quals(rng, L, 60, False),
                                        WS - buf + off + int(rng.choice([-3000, 3000])), 60, 1, matePos=WS + 1))
    bufs = [H.bamReadBuffer(good, bad, broken)]
    bufs[0].setWindowPointers(WS, WS + W)
    return (haps, WS, WS + W, buf, bufs)


def ladder_batch(L, flank_safe=False, clean=False):
    """The windows of LADDER_WINDOWS with reads of L bases only.  Haplotypes reach about 5 kb at L = 2000 (past 4096: k_sweep and k_seed_slow
    index them in direct mode)."""
    rng = np.random.default_rng(1000 + L + (50000 if flank_safe else 0))
    specs = []
    for k, (name, n) in enumerate(LADDER_WINDOWS):
        qm = (90, 60) if k == 6 else QUAL_MEANS                           # the second plain window: quality sums far above DP_SWAR_MAX_QSUM
        specs.append(_window(rng, [L] * n, name, flank_safe=flank_safe, clean=clean, qmeans=qm))
    return H._pack_windows(specs)


def _short(rng, n):
    return [int(x) for x in rng.integers(36, 251, n)]


def mixed_batches():
    """name -> HostBatch.
    one_long   windows of 36..250-base reads with exactly one read of 449, 600 or 2000 bases each, which is the window's first read (it starts
               left of all others), its last (the only bad read) or the middle of the second group of 64 (96 good reads ahead of it, bad reads
               behind it).  The window is not staged; the short reads take k_pairs' shortcuts on what the byte loop computed.
    seam       a window whose longest read has 448 bases next to one whose longest has 449.
    far_long   windows of 100-base reads only, in a batch whose longest read elsewhere has 2000 bases (LDS image and scratch sized by 2000).
    steps      one window whose reads run from 251 to 513 bases in steps of 1.
    low_quals  a window whose longest read has 448 bases and one whose longest has 449, each with eight reads of low_quality_trap."""
    rng = np.random.default_rng(77001)
    out = {}
    specs = []
    for Llong, where in ((449, "first"), (600, "last"), (2000, "middle"), (2000, "first"), (449, "middle"), (600, "first"), (2000, "last")):
        if where == "first":
            specs.append(_window(rng, [Llong] + _short(rng, 19), "plain", extras=False, pin_left=Llong))
        elif where == "last":
            specs.append(_window(rng, _short(rng, 19) + [Llong], "plain", extras=False, long_kind=(Llong, "bad")))
        else:
            haps, ws, we, buf, bufs = _window(rng, _short(rng, 96) + [Llong], "plain", extras=False, long_kind=(Llong, "bad"), pin_left=Llong)
            more = [H.AlignedRead(haps[0][buf - 20 + k:buf + 80 + k], _quals(rng, 100, 36, False), WS - 20 + k, 60, 3) for k in range(20)]
            b = H.bamReadBuffer(bufs[0].reads.array, bufs[0].badReads.array + more, [])      # (the long read starts left of them: index 96)
            b.setWindowPointers(ws, we)
            specs.append((haps, ws, we, buf, [b]))
    out["one_long"] = H._pack_windows(specs)
    out["seam"] = H._pack_windows([_window(rng, _short(rng, 15) + [448], "plain"), _window(rng, _short(rng, 15) + [449], "plain"),
                                   _window(rng, [448] * 14, "tandem"), _window(rng, [449] * 14, "tandem")])
    out["far_long"] = H._pack_windows([_window(rng, [100] * 20, "plain"), _window(rng, [100] * 70, "tandem"), _window(rng, [2000] * 9, "plain"),
                                       _window(rng, [100] * 9, "hapn")])
    out["steps"] = H._pack_windows([_window(rng, list(range(251, 514)), "plain", extras=False)])
    specs = []
    for Llong in (448, 449):                                               # staged / not staged: nlow from the LDS image / from the byte loop
        haps, ws, we, buf, bufs = _window(rng, _short(rng, 12) + [Llong], "plain", extras=False)
        traps = [low_quality_trap(haps[0], buf - 120 + 3 * k, WS - 120 + 3 * k) for k in range(8)]
        b = H.bamReadBuffer(bufs[0].reads.array + traps, [], [])
        b.setWindowPointers(ws, we)
        specs.append((haps, ws, we, buf, [b]))
    out["low_quals"] = H._pack_windows(specs)
    return out


TRAP_LEN, TRAP_AT, TRAP_Q = 250, (65, 105, 145, 185), 60


def low_quality_trap(hap, off, pos):
    """A read for which k_pairs' ungapped proof needs the count of low qualities (nlow): 250 bases of `hap` from `off` at quality 1, but for
    four bases of quality 60, 40 apart, that hold the haplotype's NEXT base.  On its mapping diagonal the read has those four mismatches
    (240) and the bound passes every test when it takes all other bases for quality 20 or more; one diagonal further the four match and
    the rest costs 1 per mismatch, about 185.  The DP finds that, and so must the proof."""
    seq, q = bytearray(hap[off:off + TRAP_LEN]), bytearray([1]) * TRAP_LEN
    for p in TRAP_AT:
        while hap[off + p] == hap[off + p + 1]:
            p += 1
        seq[p], q[p] = hap[off + p + 1], TRAP_Q
    return H.AlignedRead(bytes(seq), bytes(q), pos, 60, 3)


def nowhere_batch():
    """Reads of random bases, 300, 700 and 2000 of them, qualities 60..93, passed as mates (read_kind 2: none is skipped): no read belongs
    anywhere on its haplotypes.  Plain mode only."""
    rng = np.random.default_rng(77002)
    specs = []
    for L in (300, 700, 2000):
        buf, W = min(2 * L, 2500), 40
        ref = _rnd(rng, W + 2 * buf)
        haps = [ref, ref[:buf + 9] + ref[buf + 14:], ref[:buf + 20] + _rnd(rng, 12) + ref[buf + 20:]]
        mates = [H.AlignedRead(_rnd(rng, L), bytes(rng.integers(60, 94, L).astype(np.uint8).tolist()), WS - L // 2 + 3 * k, 60, 1, matePos=WS + 1 + k)
                 for k in range(8)]
        b = H.bamReadBuffer([], [], mates)
        b.setWindowPointers(WS, WS + W)
        specs.append((haps, WS, WS + W, buf, [b]))
    return H._pack_windows(specs)


def flank_batches(only=None):
    """length -> HostBatch for --calculateFlankScore: the ladder up to 1000 bases and 2000 with clean reads, built flank_safe (see _window).
    only: that length alone."""
    return {L: ladder_batch(L, flank_safe=True, clean=(L == 2000)) for L in LADDER if (L <= 1000 or L == 2000) and only in (None, L)}


# ---- the two reference fixtures (tests/golden/gen_golden.py: gen_mapalign_wide, gen_dp_wide) ------------------------------------------
SATURATED = 15872          # the plain score of a DP in which no final cell is below 0x7800: (0x7800 + 0x8000) >> 2


def wide_mapalign_cases(golden_dir):
    """mapalign_wide_cases.json.gz in the case format of mapalign_cases.json.gz (the qualities, a hex string there, as a list)."""
    import gzip
    import json
    import os
    cases = json.load(gzip.open(os.path.join(golden_dir, "mapalign_wide_cases.json.gz"), "rt"))
    for c in cases:
        c["qual"] = list(bytes.fromhex(c["qual"]))
    return cases


def strings_of(ops, firstpos, hap, read):
    """The two alignment strings of fastAlignmentRoutine from dp_wide_cases.npz's run-length columns (gen_golden.ops_of)."""
    import re
    a1, a2, x, y = bytearray(), bytearray(), firstpos, 0
    for n, c in re.findall(r"(\d+)([MID])", ops):
        n = int(n)
        a1 += hap[x:x + n] if c != "I" else b"-" * n
        a2 += read[y:y + n] if c != "D" else b"-" * n
        x += n if c != "I" else 0
        y += n if c != "D" else 0
    return bytes(a1), bytes(a2)
