"""Seeded inputs for the kernels that walk a read along its CIGAR -- the candidate scan (k_candidates, k_candidates_codes, k_candidates_packed)
and the read statistics of the INFO field (k_variant_read_stats, k_variant_read_stats_packed) -- at the shapes the committed goldens do not
reach: reads of 1..641 bases around every word and trip seam of the two scans, every CIGAR operation, read lists of more than two trips of
64.  Plain Python and numpy: tests/test_read_walk_cases_cpu.py checks on the oracle alone that the inputs do what they are here for, and
tests/test_gpu_read_walk_fuzz.py compares the device with the oracle on them."""
import numpy as np

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
N = ord("N")
M_, I_, D_, SKIP_, S_, H_, P_, EQ_, X_ = range(9)                     # CIGAR operations as BAM numbers them

REF_LEN = 2000
# the byte scan takes 32 bases per trip, the scan on codes 32 per word and 160 per trip
LENGTHS = (1, 2, 7, 9, 10, 11, 19, 20, 21, 31, 32, 33, 63, 64, 65, 127, 128, 129, 159, 160, 161, 191, 192, 193, 250, 319, 320, 321, 400, 641)
MIN_FLANKS = (0, 3, 10)
MIN_BASE_QUALS = (5, 20)
SCAN_SETTINGS = tuple((f, q, 1, 1) for q in MIN_BASE_QUALS for f in MIN_FLANKS) + ((10, 20, 1, 0), (10, 20, 0, 1), (10, 20, 0, 0))
FLANKS = (2, 3, 4, 9, 10, 11)                                          # shorter than, equal to and longer than minFlank 3 and 10
# qualities of mismatching bases: around both thresholds, and above 63 (exceptions of the packed table); the reference asserts 0..93
MISMATCH_QUALS = np.array([4, 5, 6, 19, 20, 21, 30, 64, 93], dtype=np.uint8)
MISMATCH_QUAL_P = np.array([.05, .05, .05, .08, .10, .10, .30, .15, .12])
BASE_QUALS = np.array([21, 22, 25, 30, 40, 64, 70, 93], dtype=np.uint8)


def ref_span(cigar):
    """Reference bases from a read's `pos` to its end as the two walks count them (a leading soft clip moves the position on)."""
    return sum(ln for k, (op, ln) in enumerate(cigar) if op in (M_, D_, SKIP_, EQ_, X_) or (op == S_ and k == 0))


def read_len(cigar):
    return sum(ln for op, ln in cigar if op in (M_, I_, S_, EQ_, X_))


def segments(read):
    """(op, read offset, reference position, length) of every M, = and X segment, as getVariantCandidatesFromSingleRead walks the CIGAR."""
    out, ro, fo = [], 0, 0
    for k, (op, ln) in enumerate(read["cigar"]):
        if op in (M_, EQ_, X_):
            out.append((op, ro, read["pos"] + fo, ln)); ro += ln; fo += ln
        elif op == I_:
            ro += ln
        elif op in (D_, SKIP_):
            fo += ln
        elif op == S_:
            ro += ln
            if k == 0:
                fo += ln
    return out


def read_index_of(read, ref_pos):
    """Index in the read of the base aligned to ref_pos in an M or X segment, or None."""
    for op, ro, fp, ln in segments(read):
        if op != EQ_ and fp <= ref_pos < fp + ln:
            return ro + ref_pos - fp
    return None


class Region:
    """One reference window and the reads built along it."""

    def __init__(self, rng, ref_seq_start, contig_len, n_positions=()):
        self.rng = rng
        self.ref = ACGT[rng.integers(0, 4, REF_LEN)].copy()
        self.ref[list(n_positions)] = N
        self.n_positions = tuple(n_positions)
        self.src = self.ref.copy()                                      # what the reads are copied from: A, C, G, T, N whatever becomes of `ref`
        self.ref_seq_start, self.contig_len = ref_seq_start, contig_len
        self.reads, self.notes = [], []

    def other(self, b):
        k = np.nonzero(ACGT == b)[0]
        return ACGT[(int(k[0]) + 1 + int(self.rng.integers(0, 3))) % 4] if len(k) else ord("A")

    def read(self, at, cigar, mism=(), quals=None, edit=None, flag=0, mapq=60, note=None, past_end=False):
        """A read whose bases follow the reference through `cigar` from window index `at`: random bases where the read has its own (I, S),
        every base of an X segment changed, then `mism` (read indices) changed, `edit` {index: byte} and `quals` {index: quality} applied."""
        rng = self.rng
        assert 0 <= at and (past_end or at + ref_span(cigar) <= REF_LEN), "reads stay inside their reference window"
        s, fp = [], at
        for k, (op, ln) in enumerate(cigar):
            if op in (M_, EQ_):
                s.append(self.src[fp:fp + ln].copy()); fp += ln
            elif op == X_:
                s.append(np.array([self.other(b) for b in self.src[fp:fp + ln]], dtype=np.uint8)); fp += ln
            elif op in (I_, S_):
                s.append(ACGT[rng.integers(0, 4, ln)])
                if op == S_ and k == 0:
                    fp += ln
            elif op in (D_, SKIP_):
                fp += ln
        s = np.concatenate(s).astype(np.uint8) if s else np.zeros(0, dtype=np.uint8)
        n = len(s)
        q = BASE_QUALS[rng.integers(0, len(BASE_QUALS), n)].copy()
        for i in mism:
            if 0 <= i < n:
                s[i] = self.other(s[i])
                q[i] = rng.choice(MISMATCH_QUALS, p=MISMATCH_QUAL_P)
        for i, v in (quals or {}).items():
            if 0 <= i < n:
                q[i] = v
        for i, v in (edit or {}).items():
            if 0 <= i < n:
                s[i] = v
        p = self.ref_seq_start + at
        self.reads.append(dict(seq=s.tobytes(), qual=q.tobytes(), pos=p, end=p + ref_span(cigar), mapq=mapq, flag=flag, cigar=[tuple(c) for c in cigar]))
        self.notes.append(note)
        return len(self.reads) - 1

    def place(self, cigar):
        return int(self.rng.integers(0, REF_LEN - ref_span(cigar) + 1))

    def as_dict(self):
        return dict(ref=self.ref.tobytes(), ref_seq_start=self.ref_seq_start, contig_len=self.contig_len, reads=self.reads)


def _pair_groups(n):
    """Mismatch pairs exactly minFlank and minFlank + 1 apart for the three minFlank values, with a mismatch the loop ignores between them
    (quality 0, or an N) where there is room for one: (indices, {index: quality}, {index: byte})."""
    mism, quals, edit = [], {}, {}
    for shift in (0, 140, 300):
        for k, (a, d) in enumerate(((12, 1), (30, 3), (50, 4), (75, 10), (110, 11))):
            a += shift
            if a + d >= n:
                continue
            mism += [a, a + d]
            quals[a], quals[a + d] = 30, 64
            if d >= 2:
                mism.append(a + 1)
                if k % 2:
                    quals[a + 1] = 0
                else:
                    edit[a + 1] = N
    return mism, quals, edit


def _flavours(n, rng):
    """(name, cigar, keywords of Region.read, placement) for reads of n bases; placement None = anywhere, or ("n", reference offset of a
    deletion inside the read) = that deletion over a reference N, or ("clamp", d) = the read's last M base d bases before the window's end."""
    def rand_mism(lo=0, hi=None, k=None):
        hi = n if hi is None else hi
        k = 1 + (hi - lo) // 25 if k is None else k
        return sorted(set(rng.integers(lo, hi, k).tolist())) if hi > lo else []
    out = []
    plain = [(M_, n)]
    seam = lambda idx: dict(mism=idx, quals={i: 21 + 30 * (i % 3) for i in idx})
    out.append(("plain_a", plain, seam([0, n - 1, 159, 320]), None))                # lo and hi - 1 of minFlank 0, and the seams of the scan on codes
    out.append(("plain_b", plain, seam([3, n - 4, 160]), None))                     # ... of minFlank 3
    out.append(("plain_c", plain, seam([10, n - 11, 161, 319]), None))              # ... of minFlank 10
    for _ in range(3):
        out.append(("plain_random", plain, dict(mism=rand_mism()), None))
    if n > 160:                                                                     # the second and later trips of the scan on codes
        for _ in range(4):
            out.append(("plain_late", plain, dict(mism=rand_mism(150, n, n // 12)), None))
    out.append(("n_ends", plain, dict(mism=rand_mism(), edit={0: N, n - 1: N}), None))
    out.append(("qcfail", plain, dict(mism=rand_mism(), flag=512 | (16 if n % 2 else 0)), None))
    mism, quals, edit = _pair_groups(n)
    if mism:
        out.append(("pairs", plain, dict(mism=mism, quals=quals, edit=edit), None))
    if n >= 3:
        a = min(5, (n - 1) // 2)
        out.append(("clip", [(S_, a), (M_, n - 2 * a), (S_, a)], dict(mism=rand_mism(a, n - a)), None))
        x, e = max(1, n // 3), max(1, n // 3)
        out.append(("h_x_n_eq_p", [(H_, 3), (X_, x), (SKIP_, 50), (EQ_, e), (P_, 2), (M_, n - x - e), (H_, 2)],
                    dict(mism=rand_mism(x, n)), None))                              # (mismatches inside the = segment too: never looked at)
    for f in FLANKS:                                                                 # both flanking M segments of f bases
        for op in (I_, D_):
            k = 1 + (f + n) % 3
            rest = n - 2 * f - (k if op == I_ else 0)
            if rest < 0:
                continue
            cig = ([(S_, rest)] if rest else []) + [(M_, f), (op, k), (M_, f)]
            out.append(("flank_%d_%s" % (f, "ID"[op - 1]), cig, dict(mism=rand_mism(rest, n, 1)), None))
    if n >= 3:
        a, k = n // 2, 1 + n % 3
        k = min(k, n - a - 1) if n - a - 1 >= 1 else 0
        if k:
            out.append(("m_i_m", [(M_, a), (I_, k), (M_, n - a - k)], dict(mism=rand_mism()), None))
            out.append(("i_first", [(I_, k), (M_, n - k)], dict(mism=rand_mism()), None))
            out.append(("i_last", [(M_, n - k), (I_, k)], dict(mism=rand_mism()), None))
            out.append(("i_d", [(M_, a), (I_, k), (D_, 2), (M_, n - a - k)], dict(mism=rand_mism()), None))
            out.append(("d_i", [(M_, a), (D_, 3), (I_, k), (M_, n - a - k)], dict(mism=rand_mism()), None))
        if n >= 7:
            out.append(("i_with_n", [(M_, a), (I_, 3), (M_, n - a - 3)], dict(edit={a + 1: N}), None))
    if n >= 2:
        a = n // 2
        out.append(("m_d_m", [(M_, a), (D_, 1 + n % 4), (M_, n - a)], dict(mism=rand_mism()), None))
        out.append(("d_over_n", [(M_, a), (D_, 6), (M_, n - a)], dict(mism=rand_mism()), ("n", a)))
    out.append(("d_first", [(D_, 2), (M_, n)], dict(mism=rand_mism()), None))
    out.append(("d_last", [(M_, n), (D_, 2)], dict(mism=rand_mism()), None))
    out.append(("d_clamped", [(M_, n), (D_, 10)], dict(past_end=True), ("clamp", 5)))                # the deletion reaches past contig_len - 1: cut there
    out.append(("d_clamped_away", [(M_, n), (D_, 10)], dict(past_end=True), ("clamp", 0)))           # ... and starts there: nothing is left of it
    return out


def scan_regions(seed=20261):
    """Four regions for the candidate scan: [dict(ref, ref_seq_start, contig_len, reads)], and per region the flavour name of every read.
    Region 0 starts at the contig's first base (a leading insertion there is reported at max(0, -1)); region 1 ends at its contig's last base
    (the deletion clamp); region 3 has lowercase and IUPAC reference bytes (the scan on codes takes the byte scan there)."""
    rng = np.random.default_rng(seed)
    n_pos = [sorted((660 + 56 * np.arange(12) + rng.integers(0, 40, 12)).tolist()) for _ in range(4)]
    regs = [Region(rng, 0, 5000, n_pos[0]), Region(rng, 1000, 1000 + REF_LEN, n_pos[1]), Region(rng, 123457, 1000000, n_pos[2]),
            Region(rng, 500, 1000000, n_pos[3])]
    odd = regs[3].ref
    for i in rng.integers(0, REF_LEN, 40).tolist():
        if odd[i] != N:
            odd[i] = odd[i] + 32                                                     # lowercase
    for i, b in zip(rng.integers(0, REF_LEN, 8).tolist(), b"RYKMSWBD"):
        if odd[i] != N:
            odd[i] = b
    k = 0
    regs[0].read(0, [(I_, 3), (M_, 40)], note="i_first_at_0")
    for n in LENGTHS:
        for name, cigar, kw, where in _flavours(n, rng):
            assert read_len(cigar) == n
            reg = regs[k % 4]
            k += 1
            if where is None:
                at = reg.place(cigar)
            elif where[0] == "n":
                reg = regs[k % 3]                                                    # (a region whose N positions were not overwritten)
                p = reg.n_positions[k % 12]
                at = p - where[1] - 2
            else:
                reg = regs[1]
                at = REF_LEN - where[1] - n
            reg.read(at, cigar, note=name, **kw)
    return [r.as_dict() for r in regs], [r.notes for r in regs]


def overflow_region(seed=20262):
    """One region whose second read emits far more records than a slice of 8 holds."""
    rng = np.random.default_rng(seed)
    reg = Region(rng, 77, 100000)
    reg.read(100, [(M_, 150)], mism=[40, 90], quals={40: 30, 90: 21})
    reg.read(300, [(M_, 641)], mism=list(range(15, 620, 13)), quals={i: 30 for i in range(15, 620, 13)}, note="many")
    reg.read(1200, [(M_, 33), (I_, 2), (M_, 40)], mism=[20], quals={20: 64})
    return [reg.as_dict()]


def scan_alignments(regions, min_flank):
    """Base index modulo 32, in the read blob and in the reference blob as Engine.candidates lays them out, of the first base the scan on codes
    asks codes_at() for in every M / X segment it scans: (set of read alignments, set of reference alignments)."""
    ra, fa = set(), set()
    soff = roff = 0
    for g in regions:
        for r in g["reads"]:
            rlen = len(r["seq"])
            if not r["flag"] & 512:
                for op, ro, fp, ln in segments(r):
                    if op == EQ_ or (op == M_ and ln < min_flank):
                        continue
                    lo = min(min_flank, ln) if ro == 0 else 0
                    hi = min(ln, rlen - min_flank - ro)
                    if lo < hi:
                        ra.add((soff + ro + lo) % 32)
                        fa.add((roff + fp - g["ref_seq_start"] + lo) % 32)
            soff += rlen
        roff += len(g["ref"])
    return ra, fa


def source_gaps(n_reads):
    """Free bytes in front of every read's packed bytes: never zero, so that the sources lie at every alignment."""
    return [1 + (7 * k) % 15 for k in range(n_reads)]


# ---- read statistics ------------------------------------------------------------------------------------------------------------------------
GOOD_COUNTS = (0, 1, 63, 64, 65, 129, 200)
BAD_COUNTS = (0, 1, 70, 130)
STATS_SETTINGS = ((1, 0), (7, 1), (11, 0), (11, 1))                    # (bad_reads_window, exact)
STATS_QUALS = np.array([5, 6, 19, 20, 21, 30, 40, 64, 93], dtype=np.uint8)
# (good, bad) reads per sample of every window; all windows of a group have the same number of samples
STATS_LAYOUT = {1: [[(0, 0)], [(1, 1)], [(63, 70)], [(64, 0)], [(65, 130)], [(129, 1)], [(200, 70)]],
                2: [[(200, 130), (0, 1)], [(129, 0), (65, 70)], [(1, 0), (64, 1)], [(63, 130), (200, 0)]],
                3: [[(129, 70), (0, 0), (200, 1)], [(65, 1), (64, 130), (63, 0)], [(1, 70), (200, 130), (129, 0)]]}
CENTRE = 1000
FORCED = (62, 63, 64, 65, 126, 127, 128, 129, 190, 191, 192, 193)     # supporting reads on both sides of lanes 63 | 64 of every trip


def _window_variants(reg, rng, k_ins, k_del):
    ref = reg.ref
    b = lambda a, e: ref[a:e].tobytes()
    alt = lambda a, e: bytes(reg.other(x) for x in ref[a:e])
    ins = ACGT[rng.integers(0, 4, k_ins)].tobytes()
    v = [dict(pos=CENTRE, removed=b(CENTRE, CENTRE + 1), added=alt(CENTRE, CENTRE + 1)),                       # SNP: the forced supporters carry it
         dict(pos=CENTRE + 10, removed=b(CENTRE + 10, CENTRE + 13), added=alt(CENTRE + 10, CENTRE + 13)),      # MNP
         dict(pos=CENTRE + 20, removed=b"", added=ins),                                                        # insertion of 1..20 bases
         dict(pos=CENTRE + 30, removed=b(CENTRE + 31, CENTRE + 31 + k_del), added=b""),                        # deletion of 1..20 bases
         dict(pos=CENTRE + 40, removed=b(CENTRE + 40, CENTRE + 41), added=alt(CENTRE + 40, CENTRE + 41)),      # SNP at reads' first / last base, one off either end
         dict(pos=CENTRE + 50, removed=b(CENTRE + 50, CENTRE + 51), added=alt(CENTRE + 50, CENTRE + 51)),      # SNP under soft clips, insertions, N skips
         dict(pos=CENTRE + 5, removed=b(CENTRE + 5, CENTRE + 7), added=alt(CENTRE + 5, CENTRE + 7)),           # MNP
         dict(pos=CENTRE + 60, removed=b"", added=ACGT[rng.integers(0, 4, 1)].tobytes())]
    n = int(rng.integers(4, 9))
    v = v[:n]
    for k, x in enumerate(v):
        wide = (0, 1, 5, 500)[(k + n) % 4]                              # 0: bam_min = bam_max = pos; 500: vmin - readPos clamps at 0 and at rlen
        x["bam_min"] = reg.ref_seq_start + x["pos"] - wide
        x["bam_max"] = reg.ref_seq_start + x["pos"] + (max(len(x["removed"]), len(x["added"])) + wide if wide else 0)
        x["pos"] += reg.ref_seq_start
    return v


def _stats_read(reg, rng, variants, k_ins, k_del, forced=None):
    """One read near the window's variants; `forced`: a plain read over the first SNP that carries it, with its own window minimum."""
    rss = reg.ref_seq_start
    flag = 16 if rng.random() < 0.5 else 0
    mapq = int(rng.integers(0, 61))
    if forced is not None:
        i = reg.read(CENTRE - 50 + forced % 7, [(M_, 100)], flag=flag, mapq=mapq)
        r = reg.reads[i]
        s, q = bytearray(r["seq"]), bytearray(r["qual"])
        at = variants[0]["pos"] - r["pos"]
        s[at] = variants[0]["added"][0]
        q[at] = 6 + forced % 15
        r["seq"], r["qual"] = bytes(s), bytes(q)
        return r
    P4, P5 = CENTRE + 40, CENTRE + 50
    special = [(P4, [(M_, 30)]), (P4 - 29, [(M_, 30)]), (P4 + 1, [(M_, 30)]), (P4 - 30, [(M_, 30)]),       # first base, last base, one before the start, one past the end
               (P5 - 5, [(S_, 10), (M_, 50)]), (P5 - 25, [(M_, 20), (SKIP_, 30), (M_, 20)]), (P5 - 24, [(M_, 25), (I_, 5), (M_, 25)]),
               (P5 - 40, [(M_, 38), (S_, 12)]), (P4, [(M_, 1)]), (CENTRE, [(X_, 1)])]
    u = rng.random()
    if u < 0.15:
        at, cigar = special[int(rng.integers(0, len(special)))]
    else:
        n = int(rng.choice([1, 2, 7, 20, 33, 64, 100, 129, 160, 161, 250, 400])) if u < 0.4 else int(rng.integers(1, 401))
        kind = int(rng.integers(0, 8))
        a = max(1, n // 2)
        ki = k_ins if rng.random() < 0.5 else int(rng.integers(1, 21))
        kd = k_del if rng.random() < 0.5 else int(rng.integers(1, 21))
        if kind == 1 and n >= 3:
            c = min(8, (n - 1) // 2)
            cigar = [(S_, c), (M_, n - 2 * c), (S_, c)]
        elif kind == 2 and n - a - ki >= 1:
            cigar = [(M_, a), (I_, ki), (M_, n - a - ki)]
        elif kind == 3 and n >= 2:
            cigar = [(M_, a), (D_, kd), (M_, n - a)]
        elif kind == 4 and n >= 2:
            cigar = [(M_, a), (SKIP_, int(rng.integers(1, 40))), (M_, n - a)]
        elif kind == 5 and n >= 3:
            x = n // 3
            cigar = [(H_, 2), (EQ_, x), (P_, 1), (X_, x), (M_, n - 2 * x), (H_, 1)]
        elif kind == 6 and n - ki >= 1:
            cigar = [(I_, ki), (M_, n - ki)] if rng.random() < 0.5 else [(M_, n - ki), (D_, kd), (I_, ki)]
        else:
            cigar = [(M_, n)]
        span = ref_span(cigar)
        if rng.random() < 0.1:
            at = reg.place(cigar)                                      # anywhere: most of these do not overlap a variant
        else:
            at = int(rng.integers(CENTRE - span - 5, CENTRE + 70))
        at = max(0, min(REF_LEN - span, at))
    i = reg.read(at, cigar, flag=flag, mapq=mapq)
    r = reg.reads[i]
    s, q = bytearray(r["seq"]), bytearray(STATS_QUALS[rng.integers(0, len(STATS_QUALS), len(r["seq"]))].tobytes())
    ro = 0
    for op, ln in r["cigar"]:                                           # an insertion of the variant's length carries its bases half the time
        if op == I_ and ln == k_ins and rng.random() < 0.5:
            s[ro:ro + ln] = variants[2]["added"] if len(variants) > 2 else s[ro:ro + ln]
        if op in (M_, I_, S_, EQ_, X_):
            ro += ln
    for v in variants:                                                  # SNPs and MNPs: carried by half the reads that cover them
        if len(v["removed"]) == len(v["added"]) and rng.random() < 0.5:
            at = read_index_of(r, v["pos"])
            if at is not None and at + len(v["added"]) <= len(s):
                s[at:at + len(v["added"])] = v["added"]
    if len(s) and rng.random() < 0.2:
        q[int(rng.integers(0, len(s)))] = int(rng.choice([0, 3, 4]))   # below the threshold of 5: drops the read where the variant's span holds it
    if len(s) and rng.random() < 0.05:
        s[int(rng.integers(0, len(s)))] = N
    r["seq"], r["qual"] = bytes(s), bytes(q)
    return r


def stats_windows(seed=20263):
    """{number of samples: [window]} for Engine.variant_read_stats / Oracle.variant_read_stats; a window = dict(variants, samples,
    var_in_genotype) as both take it."""
    rng = np.random.default_rng(seed)
    out = {}
    for n_ind, layout in STATS_LAYOUT.items():
        wins = []
        for w, counts in enumerate(layout):
            reg = Region(rng, 1000 * w + 17 * n_ind, 10 ** 7)
            k_ins, k_del = int(rng.integers(1, 21)), int(rng.integers(1, 21))
            variants = _window_variants(reg, rng, k_ins, k_del)
            samples = []
            for ng, nb in counts:
                good = [_stats_read(reg, rng, variants, k_ins, k_del, forced=j if j in FORCED else None) for j in range(ng)]
                bad = [_stats_read(reg, rng, variants, k_ins, k_del) for _ in range(nb)]
                samples.append(dict(good=good, bad=bad))
            vig = rng.integers(0, 2, (len(variants), n_ind)).astype(np.uint8)
            vig[0, :] = [1 if ng > 65 else int(x) for (ng, nb), x in zip(counts, vig[0])]
            wins.append(dict(variants=variants, samples=samples, var_in_genotype=vig.tolist()))
        out[n_ind] = wins
    return out


def oracle_stats(oracle, window, bad_reads_window, exact):
    return oracle.variant_read_stats(window["variants"], window["samples"], window["var_in_genotype"], 20, bad_reads_window, exact)
