"""Seeded inputs for plat_stage_b_batch past the committed goldens (a plain module: it calls nothing under test).  It returns
stage_b_reference.region() dicts with the options and capacities of each call; tests/test_stage_b_cases_cpu.py proves on the mirror alone
that they reach what they are meant to reach, tests/test_gpu_stage_b_fuzz.py hands them to the device.

References are random A/C/G/T with planted homopolymers and tandem repeats (unit 1..6, 4..200 bases, a few longer ones for the 384-byte
stage), some with an N; every reference window starts inside its contig and ends before the contig does.  Candidates come in shuffled
first-record order: SNPs, MNPs of 2..20 bases, insertions and deletions of 1..40 bases at the right end, the middle and the left end of
repeats (several placements of ONE indel in one repeat normalise to one variant and merge), partial-unit insertions, replacements, indels at
refPos 99 / 100 and at both ends of the reference window.  The three read tables of a region are drawn independently.

Where a region is meant to stay on the device its candidates get distinct sort keys (refPos, type, nRemoved): two kept variants of one key
are the dictionary's to order (reason 2), which a dense random region rightly comes back with."""
import functools

import numpy as np

import stage_b_reference as R

B = b"ACGT"
RLENS = (36, 100, 150, 250, 400)
BIG = dict(cap_vars=256, cap_windows=128, cap_added=4096, cap_batch_windows=4096, cap_batch_haps=1 << 15, cap_batch_reads=1 << 17, cap_hap_bytes=1 << 24)


def rnd(rng, n):
    return bytes(B[i] for i in rng.integers(0, 4, n))


def other(rng, base, avoid=b""):
    """A base that differs from `base` (and from those in `avoid`)."""
    base = base[0] if isinstance(base, (bytes, bytearray)) else base
    ok = [c for c in B if c != base and c not in avoid]
    return bytes([ok[int(rng.integers(0, len(ok)))]])


def contig(rng, n, repeats=(), n_at=()):
    """Random bases with `repeats` = (at, unit, length) planted; the bases on either side of a repeat end it.  n_at: positions of an N."""
    c = bytearray(rnd(rng, n))
    for at, unit, length in repeats:
        c[at:at + length] = (unit * (length // len(unit) + 1))[:length]
        c[at - 1] = other(rng, unit[-1])[0]
        c[at + length] = other(rng, unit[length % len(unit)])[0]
    for p in n_at:
        c[p] = ord("N")
    return bytes(c)


# ---- candidates: (pos, nrem, added, support) in the reference's coordinates (a deletion is labelled with the base before it) -------------------

def snp(rng, c, p, s=2):
    return (p, 1, other(rng, c[p]), s)


def mnp(rng, c, p, k, d, s=2):
    """k bases at p of which d differ (the first and, for d >= 2, the last among them)."""
    at = {0} | ({k - 1} if d >= 2 else set())
    rest = [i for i in range(1, k - 1)]
    at |= set(rng.permutation(rest)[:d - len(at)].tolist()) if d > len(at) else set()
    return (p, k, bytes(other(rng, c[p + i])[0] if i in at else c[p + i] for i in range(k)), s)


def dele(c, p, k, s=2):
    return (p, k, b"", s)


def ins(added, p, s=2):
    return (p, 0, bytes(added), s)


def ins_unit(c, p, a, unit, k, s=2):
    """k bases of the repeat (unit from a) inserted behind p, in the repeat's phase: every placement inside the repeat is one variant."""
    return (p, 0, bytes(unit[(p + 1 - a + i) % len(unit)] for i in range(k)), s)


def rep(rng, c, p, nrem, nadd, s=2):
    return (p, nrem, other(rng, c[p]) + rnd(rng, nadd - 1), s)


def vtype(cand):
    nrem, nadd = cand[1], len(cand[2])
    return (0 if nadd == 1 else 1) if nrem == nadd else 2 if nrem == 0 else 3 if nadd == 0 else 4


def key(cand):
    return (max(cand[0], 0), vtype(cand), cand[1])


def pure_indel(cand):
    return vtype(cand) in (2, 3)


def distinct_keys(cands):
    """The candidates with the later ones of an equal sort key dropped."""
    seen, out = set(), []
    for c in cands:
        if key(c) not in seen:
            seen.add(key(c))
            out.append(c)
    return out


def shuffled(rng, cands):
    return [cands[i] for i in rng.permutation(len(cands))]


# ---- read tables -----------------------------------------------------------------------------------------------------------------------------

def good_reads(rng, lo, hi, rlen, step=None):
    """Reads (pos, end, length) every `step` bases over [lo, hi): ends a few bases off pos + length (deletions, clipping)."""
    out, p = [], max(1, lo)
    step = step or int(rng.integers(7, 41))
    while p < hi:
        ln = int(rng.integers(max(20, rlen - 30), rlen + 1))
        out.append((p, p + ln + int(rng.integers(-3, 6)), ln))
        p += int(rng.integers(0, 2 * step))
    return out


def broken_reads(rng, lo, hi, rlen, n):
    """Reads (pos, end, length, mate position) sorted by the mate's position, the mates spread around [lo, hi)."""
    out = []
    for _ in range(n):
        p = int(rng.integers(1, hi + 400))
        out.append((p, p + rlen, rlen, int(rng.integers(max(1, lo - 2 * rlen), hi + 2 * rlen))))
    return sorted(out, key=lambda r: r[3])


def tables(rng, lo, hi, rlen, mode):
    """The three tables of a region, each drawn on its own.  mode: 'plain', 'none' (no good reads), 'one', 'deep' (more than 256 good reads
    over the first windows), 'ends' (good reads that end exactly where the first window starts, and on the bases around it), 'raise' (a bad-reads table whose pointers come out s > e: the
    reference raises), 'long' (a longest read larger than any in the table)."""
    good = good_reads(rng, lo - rlen, hi, rlen)
    bad = good_reads(rng, lo - rlen, hi, rlen, step=int(rng.integers(20, 90))) if rng.random() < 0.7 else []
    broken = broken_reads(rng, lo, hi, rlen, int(rng.choice([0, 1, 12, 70])))
    longest = None
    if mode == "none":
        good = []
    elif mode == "one":
        good = [(max(1, (lo + hi) // 2 - rlen // 2), (lo + hi) // 2 + rlen // 2, rlen)]
        bad = bad[:1]
    elif mode == "deep":
        good = sorted(good + [(p, p + rlen, rlen) for p in rng.integers(max(1, lo - rlen // 2), lo + 40, 300).tolist()])
        bad = sorted(bad + [(p, p + rlen, rlen) for p in rng.integers(max(1, lo - rlen // 2), lo + 40, 70).tolist()])
    elif mode == "ends":                                                          # reads that end on every base of the 21 before the first variant: one of
        good = sorted(good + [(e - rlen // 2, e, rlen // 2) for e in range(max(2 + rlen // 2, lo - 21), lo + 1) for _ in range(2)])   # them is the window's start
    elif mode == "raise":
        bad = [(p, 1, rlen) for p in range(max(1, lo - rlen), hi + 2 * rlen, 9)]          # every read "ends" at 1: the start pointer runs past the end pointer
    elif mode == "long":
        longest = [5000, max([r[1] - r[0] for r in bad], default=0), 700]
    return dict(reads=good, bad=bad, broken=broken, longest=longest)


# ---- regions -------------------------------------------------------------------------------------------------------------------------------------

def make(rng, c, cands, rlen, rss=None, rend=None, start=None, end=None, mode="plain", inside=False, **kw):
    """A region over contig c.  The reference window [rss, rend) holds every candidate with the room the kernels ask for unless the
    caller sets it; start / end default to the window; inside: they lie strictly inside the candidates' span."""
    ps = [x[0] for x in cands] or [len(c) // 2]
    room = 2 * min(2 * rlen, 500) + 160
    rss = max(1, min(ps) - room - int(rng.integers(0, 50))) if rss is None else rss
    rend = min(len(c) - 1, max(ps) + room + int(rng.integers(0, 50))) if rend is None else rend
    start, end = rss if start is None else start, rend if end is None else end
    if inside and len(ps) >= 4:
        q = sorted(ps)
        start, end = q[1] - int(rng.integers(0, 3)), q[-2] + int(rng.integers(0, 3))
    t = tables(rng, min(ps), max(ps) + 1, rlen, mode)
    t.update(kw)
    return R.region(c[rss:rend], cands, start=start, end=end, rlen=rlen, ref_seq_start=rss, contig_len=len(c), **t)


def spaced(rng, n, n_indel=0, gap=(3, 9), at=700, rlen=100, types="snp", **kw):
    """n candidates of distinct positions `gap` apart from `at`, n_indel of them pure insertions / deletions at refPos >= 100; indels sit
    between two different bases that also differ from the indel's own ends, so they stay where they are and keep their keys apart."""
    ps = (at + np.cumsum(rng.integers(gap[0], gap[1] + 1, n))).tolist() if n else []
    c = bytearray(contig(rng, (ps[-1] if ps else at) + 1600))
    which = set(rng.permutation(n)[:n_indel].tolist())
    cands = []
    for i, p in enumerate(ps):
        s = int(rng.integers(2, 7))
        if i in which:
            k = int(rng.integers(1, 4)) if gap[0] >= 6 else 1
            if rng.random() < 0.5 or gap[0] < 6:
                a = rnd(rng, k)
                c[p] = other(rng, a[-1])[0]                                       # the base before differs from the last added one: it cannot move
                cands.append(ins(a, p, s))
            else:
                c[p] = other(rng, c[p + k])[0]
                cands.append(dele(c, p, k, s))
        elif types == "mixed" and rng.random() < 0.25 and gap[0] >= 6:
            cands.append(mnp(rng, c, p, 2, 2, s))
        else:
            cands.append(snp(rng, c, p, s))
    return make(rng, bytes(c), shuffled(rng, cands), rlen, **kw)


def clustered(rng, n, rlen, edge=False, n_base=False, dense=False, **kw):
    """1..n candidates in clusters over a reference with planted repeats: all five types, indels inside the repeats at several placements."""
    M = 1400                                                                      # room for the longest haplotype flank on either side
    L = 2 * M + 600 + 14 * n
    reps, p = [], M + 40
    while p < L - M:
        unit = rnd(rng, int(rng.integers(1, 7)))
        if len(set(unit)) == 1:
            unit = unit[:1]
        length = int(rng.choice([4, 7, 12, 25, 60, 63, 64, 65, 130, 200]))
        reps.append((p, unit, length))
        p += length + int(rng.integers(40, 400))
    c = contig(rng, L, reps, n_at=[int(rng.integers(300, L - 300))] if n_base else ())
    cands, p = [], M - 40 + int(rng.integers(0, 60))
    while len(cands) < n and p < L - M + 20:
        t, s = rng.random(), int(rng.integers(1, 7))
        if t < 0.45:
            cands.append(snp(rng, c, p, s))
        elif t < 0.6:
            k = int(rng.integers(2, 21))
            cands.append(mnp(rng, c, p, k, int(rng.integers(1, min(k, 17) + 1)), s))
        elif t < 0.75:
            k = int(rng.integers(1, 41))
            cands.append(ins(c[p + 1:p + 1 + k] if rng.random() < 0.6 else rnd(rng, k), p, s))
        elif t < 0.9:
            cands.append(dele(c, p, int(rng.integers(1, 41)), s))
        else:
            cands.append(rep(rng, c, p, int(rng.integers(2, 6)), 1, s) if rng.random() < 0.5 else rep(rng, c, p, 1, int(rng.integers(2, 6)), s))
        p += int(rng.choice([1, 2, 3, 5, 8, 9, 12, 15, 20, 60, 200] if not dense else [0, 0, 1, 1, 2]))
    for at, unit, length in reps:                                                  # one indel of the repeat at its right end, its middle and its left end
        if rng.random() < 0.7 and len(cands) < n + 12:
            m, k = len(unit), len(unit) * int(rng.integers(1, max(2, min(40, length) // len(unit))))
            k = min(k, 40 - 40 % m) or m
            if k > length:
                continue
            deletion = rng.random() < 0.5
            hi = at + length - k - 1 if deletion else at + length - 1
            for q in sorted({hi, (at + hi) // 2, at - 1} if rng.random() < 0.7 else {hi}):
                cands.append(dele(c, q, k, int(rng.integers(1, 4))) if deletion else ins_unit(c, q, at, unit, k, int(rng.integers(1, 4))))
            if m > 1 and rng.random() < 0.5:                                       # a partial unit: it moves only as far as its own bases repeat
                cands.append(ins_unit(c, at + length - 1, at, unit, m + 1 if m + 1 <= 40 else 1))
    cands = cands if dense else distinct_keys(cands)
    if edge:                                                                      # an indel whose normalisation window leaves the reference window
        ps = [x[0] for x in cands]
        rss = min(ps) - int(rng.integers(5, rlen))
        return make(rng, c, shuffled(rng, cands + [dele(c, min(ps) - 1, 1, 3)]), rlen, rss=rss, **kw)
    return make(rng, c, shuffled(rng, cands), rlen, **kw)


def key_run(rng, m, extra=0, rlen=150):
    """m placements of one single-base deletion in a homopolymer: after normalisation a run of m candidates of one key, all one variant
    (more than 48 count as the dictionary's).  extra: SNPs around it."""
    at, length = 800, max(m + 2, 8)
    c = contig(rng, 2600, [(at, b"T", length)])
    cands = [dele(c, at - 1 + i, 1, 2 + i % 3) for i in range(m)]
    cands += [snp(rng, c, at - 60 - 11 * i, 3) for i in range(extra)] + [snp(rng, c, at + length + 30 + 13 * i, 3) for i in range(extra)]
    return make(rng, c, shuffled(rng, cands), rlen)


def long_walks(rng):
    """Indels of one repeat unit given at the right end of repeats of unit 1..6 and 63..200 bases, under read lengths that let the walk
    reach the left end or stop at its window's end; one placement at the left end with them (a moved and an unmoved one, merged)."""
    out = []
    for length in (63, 64, 65, 127, 128, 130, 200):
        for m in (1, 2, 3, 6):
            unit = rnd(rng, 1) if m == 1 else b"ACGTCA"[:m] if m < 6 else b"ACGGTT"
            at = 900
            c = contig(rng, 2600, [(at, unit, length)])
            rlen = int(rng.choice([100, 250, 400]))
            k = m * int(rng.integers(1, 3))
            cands = [dele(c, at + length - k - 1, k, 2), dele(c, at - 1, k, 3), ins_unit(c, at + length - 1, at, unit, k, 2), ins_unit(c, at - 1, at, unit, k, 1),
                     snp(rng, c, at - 40), snp(rng, c, at + length + 30)]
            out.append(make(rng, c, shuffled(rng, cands), rlen))
    return out


def edges(rng):
    """Indels at refPos 99 and 100, at both ends of the reference window (one byte inside, one byte outside what the rule needs) and next to
    the contig's end; a size above maxSize last and not last in sorted order."""
    out = []
    c = contig(rng, 2400, [(90, b"A", 30)])
    out.append(make(rng, c, [dele(c, 99, 1, 3), snp(rng, c, 300)], 100, rss=0, rend=1500))
    out.append(make(rng, c, [dele(c, 100, 1, 3), snp(rng, c, 300)], 100, rss=0, rend=1500))
    out.append(make(rng, c, [ins(b"A", 99, 3), ins(b"A", 104, 3), snp(rng, c, 300)], 100, rss=0, rend=1500))
    c = contig(rng, 4000, [(1500, b"G", 12)])
    for rlen in (100, 150):
        w = 1 + rlen
        for rss in (1505 - w, 1505 - w + 1):                                     # the window starts at wmin; one base behind it (reason 1)
            out.append(make(rng, c, [dele(c, 1505, 1, 3), snp(rng, c, 1700)], rlen, rss=rss, rend=3000))
        for rend in (1505 + w, 1505 + w - 1):                                    # ... ends at wmax; one base before it (reason 1)
            out.append(make(rng, c, [dele(c, 1505, 1, 3), snp(rng, c, 1400)], rlen, rss=600, rend=rend))
    for tail in (2, 3):                                                           # the deletion's tail is empty at the contig's end (reason 1) / one base
        c = contig(rng, 2000)
        out.append(make(rng, c, [dele(c, len(c) - 2 - tail, 2, 3), snp(rng, c, 1500)], 150, rss=700, rend=len(c)))
    c = contig(rng, 6000)
    big = [dele(c, 1200, 70, 5), dele(c, 2000, 59, 5), dele(c, 2600, 61, 5), snp(rng, c, 3000, 4)]
    out.append(make(rng, c, big, 100))                                            # above maxSize 60 and not last
    out.append(make(rng, c, big[:3] + [dele(c, 3000, 70, 5)], 100))               # ... and as the last run (no size test there)
    out.append(make(rng, c, big[:3] + [dele(c, 3000, 70, 1)], 100))               # ... the last run, too weak
    return out


def hap_windows(rng, rlen, n_windows=8):
    """Windows of 1..5 variants, 120+ bases apart: all five types, abutting and overlapping pairs, and variant sets that spell ONE sequence."""
    L = 1800 + 260 * n_windows
    c = bytearray(contig(rng, L))
    cands, p = [], 900
    for w in range(n_windows):
        kind = int(rng.integers(0, 12))
        if kind == 0:                                                             # two SNPs against the MNP of both: merged by the priors
            a, b = snp(rng, c, p), snp(rng, c, p + 1)
            cands += [a, b, (p, 2, a[2] + b[2], 2)]
        elif kind == 1:                                                           # an MNP of one difference against the SNP: the LATER one stays
            a = snp(rng, c, p + 1)
            cands += [(p, 2, bytes(c[p:p + 1]) + a[2], 2), a]
        elif kind == 2:                                                           # two MNPs of one difference and one sequence: the first stays
            a = snp(rng, c, p + 1)
            cands += [(p, 2, bytes(c[p:p + 1]) + a[2], 2), (p + 1, 2, a[2] + bytes(c[p + 2:p + 3]), 2)]
        elif kind == 3:                                                           # a replacement that spells a deletion: one sequence with an indel
            c[p:p + 4] = b"GAAC"
            c[p - 1] = ord("T")
            cands += [(p + 1, 2, b"A", 2), dele(c, p, 1)] if p >= 100 else []
        elif kind == 4:                                                           # MNPs of 17 differences (one sequence) / of none (the reference's)
            k = 18
            alt = bytes(other(rng, x)[0] for x in c[p + 1:p + k])
            cands += [(p, k, bytes(c[p:p + 1]) + alt, 2), (p + 1, k - 1, alt, 2)] if rng.random() < 0.6 else [(p, 3, bytes(c[p:p + 3]), 2), snp(rng, c, p + 7)]
        elif kind == 5:                                                           # a SNP that ends where an indel starts (valid), and one inside a deletion (not)
            c[p + 1] = other(rng, c[p + 4])[0]
            cands += [snp(rng, c, p), dele(c, p, 3), snp(rng, c, p + 2), snp(rng, c, p + 9)]
        elif kind == 6:                                                           # a deletion that reaches over the next variants
            k = int(rng.integers(8, 30))
            c[p] = other(rng, c[p + k])[0]
            cands += [dele(c, p, k), snp(rng, c, p + k // 2), ins(other(rng, c[p + k + 3]), p + k + 3), snp(rng, c, p + k + 1)]
        else:                                                                     # 1..5 variants that do not touch: every combination is valid
            n, q = int(rng.integers(1, 6)), p
            for _ in range(n):
                t = rng.random()
                if t < 0.5:
                    cands.append(snp(rng, c, q))
                elif t < 0.65:
                    cands.append(mnp(rng, c, q, 3, 2))
                elif t < 0.8:
                    a = rnd(rng, int(rng.integers(1, 6)))
                    c[q] = other(rng, a[-1])[0]
                    cands.append(ins(a, q))
                elif t < 0.92:
                    c[q] = other(rng, c[q + 2])[0]
                    cands.append(dele(c, q, 2))
                else:
                    cands.append(rep(rng, c, q, 2, 1))
                q += int(rng.integers(4, 8))
        p += 260
    # the bases changed above may have turned a SNP into the reference's base: made again over the final contig
    c = bytes(c)
    fixed = [(x[0], 1, other(rng, c[x[0]]), x[3]) if vtype(x) == 0 and x[2] == c[x[0]:x[0] + 1] else x for x in cands]
    return make(rng, c, shuffled(rng, distinct_keys(fixed)), rlen)


def refused(rng):
    """Regions the merge already refused, or with more candidates than the call holds (reason 5)."""
    c = contig(rng, 3000)
    cands = [snp(rng, c, 1400 + 20 * i) for i in range(6)]
    return [make(rng, c, cands, 100, merge_status=R.ERR_OVERFLOW), make(rng, c, cands, 100, merge_status=R.ERR_BAD_INPUT), make(rng, c, cands, 100, n_cands=5000)]


def stage_regions(rng):
    """Haplotypes that agree on the whole 384-byte stage behind the common prefix and go on: a deletion inside a tandem repeat of 450 bases
    (the haplotype equals the reference to the repeat's end), and a deletion of 400 bases with a SNP near its far end."""
    out = []
    for unit in (b"A", b"CAG", b"ACGGTT"):
        c = contig(rng, 3600, [(1200, unit, 450)])
        out.append(make(rng, c, [dele(c, 1199, len(unit) * 2, 3), snp(rng, c, 1190)], 250))
    c = contig(rng, 3600)
    out.append(make(rng, c, [dele(c, 1200, 400, 3), snp(rng, c, 1590), snp(rng, c, 1195)], 250))
    return out


# ---- options ---------------------------------------------------------------------------------------------------------------------------------------

def option_sets():
    """Option sets over the listed ranges: four fixed ones that keep most windows on the device, eight drawn."""
    rng = np.random.default_rng(4201)
    out = [R.options(), R.options(mergeClusteredVariants=0, minReads=1), R.options(largeWindows=1, maxVarDist=50, minVarDist=20, maxSize=600),
           R.options(maxVariants=5, maxHaplotypes=33, filterVarsByCoverage=0, minVarDist=5, maxVarDist=12, minReads=3)]
    for k in range(8):
        out.append(R.options(mergeClusteredVariants=int(rng.random() < 0.8), maxVarDist=int(rng.integers(5, 51)), minVarDist=int(rng.integers(1, 21)),
                             largeWindows=int(rng.random() < 0.3), maxVariants=int(rng.integers(1, 9)), maxHaplotypes=int(rng.integers(3, 51)),
                             filterVarsByCoverage=int(rng.random() < 0.5), skipDifficultWindows=int(rng.random() < 0.5), maxSize=int(rng.choice([60, 200, 600, 1500])),
                             minReads=int(rng.integers(1, 6)), maxReads=float(rng.choice([5000000.0, 5000000.0, 200.0, 40.0]))))
    return out


def call(name, regions, o, **over):
    return dict(name=name, regions=regions, o=o, cp=R.caps(**dict(BIG, **over)))


@functools.lru_cache(maxsize=None)
def corpus():
    """The calls of the corpus, option set by option set: [dict(name, regions, o, cp)]."""
    calls = []
    modes = ["plain", "plain", "ends", "deep", "none", "one", "raise", "long", "plain", "plain"]
    for k, o in enumerate(option_sets()):
        rng = np.random.default_rng(7000 + k)
        regs = []
        for j in range(10):
            rlen = int(rng.choice(RLENS))
            n = int(rng.choice([1, 2, 5, 12, 25, 40, 60]))
            regs.append(clustered(rng, n, rlen, edge=(j == 8 and k % 2 == 0), n_base=(j % 4 == 1), dense=(j == 9 and k % 4 == 0), mode=modes[(j + k) % 10],
                                  inside=(j % 3 == 0)))
        regs += [hap_windows(rng, int(rng.choice(RLENS))) for _ in range(4)]
        regs.insert(3, make(rng, contig(rng, 3000), [], 100))                     # an empty region between loaded ones
        if k == 0:
            regs += long_walks(rng)
        if k == 1:
            regs += edges(rng) + refused(rng)
        if k == 2:
            regs += stage_regions(rng) + [key_run(rng, m, extra=2) for m in (1, 2, 3)]
        if k == 3:
            regs += [hap_windows(rng, r, 10) for r in RLENS]
        calls.append(call("options %d" % k, regs, dict(o, maxSize=60) if k == 1 else o))
    # the first option set's regions again under capacities that some of them overflow (reason 6)
    calls.append(call("options 0, tight capacities", calls[0]["regions"][:15], calls[0]["o"], cap_vars=12, cap_windows=6, cap_added=24))
    return calls


@functools.lru_cache(maxsize=None)
def ladder():
    """The size ladder: one call per seam.  -> {name: call}"""
    rng = np.random.default_rng(9100)
    o = R.options(maxVarDist=9, minVarDist=4, minReads=2)
    wide = dict(cap_vars=1024, cap_windows=512, cap_added=2048)
    cands = [spaced(rng, n, n_indel=min(n, 3)) for n in (0, 1, 2, 63, 64, 65, 200)] + [spaced(rng, 1000 + int(rng.integers(0, 25)), n_indel=5)]
    indels = [spaced(rng, 40, n_indel=k, gap=(6, 12), types="mixed") for k in (0, 1, 15, 16, 17, 33)]
    runs = [key_run(rng, m) for m in (1, 2, 3, 48, 49)]
    windows = [spaced(rng, n, gap=(24, 30), mode="plain") for n in (255, 256, 257, 370)] + [spaced(rng, 1, gap=(24, 30)), make(rng, contig(rng, 3000), [], 100)]
    return dict(candidates=call("ladder, candidates", cands, o, **wide), indels=call("ladder, indels", indels, o, **wide), runs=call("ladder, key runs", runs, o, **wide),
                windows=call("ladder, windows", windows, o, **wide))


def all_regions():
    return [reg for c in corpus() for reg in c["regions"]]


def draw(n, seed):
    """n regions drawn from the corpus (flagged and unflagged, loaded and empty as they come)."""
    regs = all_regions()
    rng = np.random.default_rng(seed)
    return [regs[i] for i in rng.integers(0, len(regs), n)]


# ---- the dictionary replay from real scans -------------------------------------------------------------------------------------------------------

REPLAY_TARGETS = (5, 6, 21, 22, 85, 86, 341, 342, 1365, 1366, 2000)
REPLAY_SITES = (1200, 1800)


def replay_scan(seed, n_records, length=3000, step=5):
    """150-base reads every `step` bases over a region of `length` bases: two alleles in turn at each of REPLAY_SITES (both pass the support
    filter: their order is the dictionaries') and n_records - 4 single mismatches where thirty reads overlap, no two of one read next to
    each other and no (position, base) seen twice, so that the scan holds n_records distinct records of which all but four fail the
    filter.  -> the scan dict of Engine.candidates"""
    rng = np.random.default_rng(seed)
    ref = contig(rng, length)
    starts = list(range(60, length - 210, step))
    inner = [k for k, pos in enumerate(starts) if pos >= 250 and pos + 150 <= length - 250]
    noise = n_records - 2 * len(REPLAY_SITES)
    per = np.zeros(len(starts), dtype=int)
    per[inner] = noise // len(inner)                                              # (at most six a read: they have to stay apart, see below)
    per[rng.permutation(inner)[:noise % len(inner)]] += 1
    used, reads = set(), []
    for k, pos in enumerate(starts):
        seq = bytearray(ref[pos:pos + 150])
        for j, p in enumerate(REPLAY_SITES):
            if pos + 12 <= p < pos + 138:
                seq[p - pos] = [b for b in B if b != ref[p]][(k + j) % 2]
        mine, tries = set(), 0
        while len(mine) < per[k]:
            p = pos + int(rng.integers(15, 135))
            alt = other(rng, ref[p])
            if (p, alt) in used or any(abs(p - q) < 12 for q in mine | set(REPLAY_SITES)):   # (mismatches within minFlank of each other are ONE record)
                tries += 1
                if tries % 200 == 0:
                    used -= {(q, bytes(seq[q - pos:q - pos + 1])) for q in mine}
                    for q in mine:
                        seq[q - pos] = ref[q]
                    mine = set()
                continue
            mine.add(p)
            used.add((p, alt))
            seq[p - pos] = alt[0]
        reads.append(dict(seq=bytes(seq), qual=b"\x28" * 150, pos=pos, flag=3, cigar=[(0, 150)], end=pos + 150))
    return dict(ref=ref, ref_seq_start=0, contig_len=length, reads=reads)


def scan_records(rec, count, blob, scan, first_read, max_per_read, cand_rows):
    """The distinct records of one scan in first-record order, and its candidates as stage_b_reference takes them.  rec / count / blob: the
    records of the call (Engine.last_candidates); scan: the scan dict; first_read: the index of its first read in the call; cand_rows: the
    rows of the merge for this scan.
    -> (cands [(pos, nrem, added, support, first-record id)], distinct [(pos, removed, added, index into cands or None)])"""
    rows = sorted(list(map(int, r)) for r in cand_rows)
    cands = [(r[3], r[4], blob[r[7]:r[7] + r[5]], r[1], r[0]) for r in rows]
    by_id = {c[4]: i for i, c in enumerate(cands)}
    ref, rss = scan["ref"], scan["ref_seq_start"]
    distinct, seen = [], set()
    for r in range(first_read, first_read + len(scan["reads"])):
        for k in range(int(count[r])):
            pos, nrem, nadd, ro, ao = (int(x) for x in rec[r, k])
            at = (pos + 1 if (nrem and not nadd) else pos) - rss
            rkey = (pos, ref[at:at + nrem] if nrem else b"", blob[ao:ao + nadd] if nadd else b"")
            if rkey not in seen:
                seen.add(rkey)
                distinct.append(rkey + (by_id.get(r * max_per_read + k),))
    return cands, distinct
