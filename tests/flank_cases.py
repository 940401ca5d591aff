"""Batches for --calculateFlankScore=1 (dp_traceback.hpp, k_dp_tb_jobs, the slab loop of align_impl, select_best on flank-reduced scores) and a
classifier of what the oracle's tracebacks on them contain.  No device: tests/test_flank_cases_cpu.py holds the batches to what they are for,
tests/test_gpu_flank_stress.py runs them on the device.

The four stress batches are the builders of the plain path's tests, unchanged and with their seeds.  The seam batch puts one event per read at
every offset around a flank boundary (haplotype offsets F and hapLen - F), where calculateFlankScore charges a gap's columns to the flank one by
one and the tie-breaks of the labelled DP decide on which side a gap lands."""
import functools
import itertools

import numpy as np

LENGTHS = (36, 100, 250)
FLANKS = (1, 7, 8, 9, 40, None)                                          # None: min(2 L, 500)
CONTEXTS = ("random", "homopolymer", "tandem")
QMAX = 60                                                                # 250 bases x 60 = 15 000 < 15 872: no traceback-mode DP saturates
WS = 5000
B = b"ACGT"


def stress_batches():
    """name -> builder of the four stress batches that the plain path is pinned by."""
    from test_gpu_parity import _adversarial_batch
    from test_gpu_seed_indels import _indel_batch
    return {"adversarial": lambda: _adversarial_batch(1), "adversarial_gapped": lambda: _adversarial_batch(3, gapped=True),
            "indel_random": lambda: _indel_batch(31, 100, False), "indel_repeat": lambda: _indel_batch(32, 100, True)}


def seam_batch(seed=41):
    """(HostBatch, meta): one window per (read length, flank, context), 54 in all, of two to four haplotypes: the base, and of an N variant
    (N on F - 1, F, hapLen - F - 1, hapLen - F), a SNP variant, a 3-base deletion and a 2-base insertion in the window's middle what the count
    allows.  The context (random sequence, a homopolymer of 12..50 bases, a tandem repeat of unit 2..4) spans both boundaries of the base.

    Reads, L bases cut from a haplotype `src` of the window (all of them in turn) at offset o, mapped at o:
      events     bases inserted into the read or deleted from it, k = 1..6, at src offset boundary + d for every d in -k-1 .. 1, for both
                 boundaries of src; the boundary lies k + 3 bases into the read, at its middle or k + 5 before its end (in turn).  An inserted piece
                 is the k bases that follow (a repeat grows by a piece of itself) or random.  Every sixth again with a quality-0 base next to it.
      subst      one substitution, and one read N, exactly on F - 1, F, hapLen - F - 1, hapLen - F
      start      o = 0..7 (the slice starts at the haplotype's first base, st = 0) with an event in the first 10 bases
      clamped    o = hapLen - L - 14, - 11, - 8: the mapping position is clamped to hapLen - L - 15
    A slice ends at hapLen - 8 (calign.pyx:229,253-256), so no read is cut past that and a right flank of up to 8 bases is never aligned to: events
    there fall away, as do offsets left of the haplotype's second base (F = 1).  A read with fewer than 7 bases in the window goes in as a
    broken mate (never skipped, chaplotype.pyx:365-373).  meta: per window (L, F, context, events kept)."""
    from platypus_amd import hostapi as H
    rng = np.random.default_rng(seed)
    rnd = lambda n: bytes(rng.choice(list(B), n).astype(np.uint8))
    other = lambda c: B[((B.index(c) if c in B else 0) + 1 + int(rng.integers(0, 3))) % 4]
    specs, meta = [], []
    for wi, (L, F_, ctx) in enumerate(itertools.product(LENGTHS, FLANKS, CONTEXTS)):
        F = min(2 * L, 500) if F_ is None else F_
        W = max(L + 24 - 2 * F, 30) + int(rng.integers(0, 9))           # every haplotype keeps L + 15 bases and is longer than 2 F
        ref = bytearray(rnd(W + 2 * F))
        if ctx != "random":
            for right in (0, 1):
                n = int(rng.integers(12, 51))
                out = min(n // 2, F)                                     # bases of the context in the flank, the rest in the window
                inn = min(n - out, W // 2 - 3)
                a = F + W - inn if right else F - out
                unit = rnd(1)
                while ctx == "tandem" and len(set(unit)) < 2:
                    unit = rnd(int(rng.integers(2, 5)))
                assert 12 <= out + inn <= 50
                ref[a:a + out + inn] = (unit * 50)[:out + inn]
        base = bytes(ref)
        mid = F + W // 2
        hN = bytearray(base)
        for p in (F - 1, F, len(base) - F - 1, len(base) - F):
            hN[p] = ord("N")
        hS = bytearray(base); hS[mid] = other(hS[mid])
        hD = bytearray(base[:mid] + base[mid + 3:]); hD[mid - 2] = other(hD[mid - 2])
        nH = (2, 3, 2, 4)[wi % 4]
        haps = {2: [base, bytes(hN)], 3: [base, bytes(hD), bytes(hN)], 4: [base, bytes(hS), base[:mid] + rnd(2) + base[mid:], bytes(hN)]}[nH]
        assert len(set(haps)) == nH and all(len(h) >= L + 18 and len(h) > 2 * F for h in haps)
        good, broken = [], []

        def quals(n_read):
            q = np.clip(rng.normal(50, 8, L), 2, QMAX) if n_read % 5 == 4 else np.clip(rng.normal(34, 6, L), 2, 41)
            return q.astype(np.uint8)

        def add(seq, q, o):
            assert len(seq) == L and len(q) == L and int(q.max()) <= QMAX
            pos = WS - F + o
            r = H.AlignedRead(bytes(seq), bytes(q.tolist()), pos, 60, 3, matePos=WS)
            (good if min(WS + W, pos + L) - max(WS, pos) >= 7 else broken).append(r)

        def cut(src, o, p, ins, k, piece=None):
            """L bases of src from o with k bases inserted before (ins) or deleted from src offset p; what src lacks at its end is random."""
            s = src[o:p] + (piece + src[p:p + L] if ins else src[p + k:p + k + L])
            return bytearray((s + rnd(L))[:L])

        n_ev = 0
        for right, ins, k in itertools.product((0, 1), (1, 0), range(1, 7)):
            for d in range(-k - 1, 2):
                src = haps[n_ev % nH]
                b = len(src) - F if right else F
                p = b + d
                o = min(max(b - (k + 3, L // 2, L - 5 - k)[n_ev % 3], 0), len(src) - L - 8)
                i = p - o                                                # the event's place in the read
                if not (1 <= i <= L - 2 and p >= 1):
                    continue
                piece = None
                if ins:
                    piece = src[p:p + k] if (ctx != "random" and n_ev % 2 == 0 and p + k <= len(src)) else rnd(k)
                seq, q = cut(src, o, p, ins, k, piece), quals(n_ev)
                add(seq, q, o)
                if n_ev % 6 == 0:                                        # the same read with a free base next to the event: paths tie, labels decide
                    q0 = q.copy()
                    q0[min((i - 1, i + k if ins else i)[(n_ev // 6) % 2], L - 1)] = 0
                    add(seq, q0, o)
                n_ev += 1
        for j, p in enumerate((F - 1, F, len(base) - F - 1, len(base) - F)):
            o = min(max(p - L // 2, 0), len(base) - L - 8)
            if not 0 <= p - o < L:
                continue
            for ch in (other(base[p]), ord("N")):
                seq = bytearray(base[o:o + L]); seq[p - o] = ch
                add(seq, quals(j), o)
        for o in range(8):
            k, i = 1 + o % 3, 1 + (o * 4) % 9
            add(cut(base, o, o + i, o % 2, k, rnd(k)), quals(o), o)
        for o in (len(base) - L - 14, len(base) - L - 11, len(base) - L - 8):
            p = len(base) - F - 1
            seq = cut(base, o, p, 0, 2) if 1 <= p - o <= L - 2 else bytearray(base[o:o + L])
            add(seq, quals(o), o)
        buf = H.bamReadBuffer(good, brokenMates=broken)
        buf.setWindowPointers(WS, WS + W)
        assert len(buf.windowReads()) == len(good) + len(broken)
        specs.append((haps, WS, WS + W, F, [buf]))
        meta.append((L, F, ctx, n_ev))
    return H._pack_windows(specs), meta


@functools.lru_cache(maxsize=None)
def batch(name):
    """The batch of that name, built once per process: the four of stress_batches() and "seam"."""
    return seam_batch()[0] if name == "seam" else stress_batches()[name]()


NAMES = ("adversarial", "adversarial_gapped", "indel_random", "indel_repeat", "seam")
COUNT_KEYS = ("classified", "with_gap", "ins_cols_in_flank", "del_cols_in_flank", "del_runs_crossing_left", "del_runs_crossing_right",
              "first_column_gap", "n_mismatch_cols_in_flank")


def classify(aln1, aln2, x, hapLen, F):
    """What one alignment (the haplotype's string, the read's, the haplotype offset of its first column) holds, column by column as
    calculateFlankScore walks it (align.c:593-644): COUNT_KEYS[1:] in order."""
    gap = ins_in = del_in = cross_l = cross_r = first = nmm = 0
    prev_del = False
    for i, (c1, c2) in enumerate(zip(aln1, aln2)):
        infl = x < F or x >= hapLen - F
        if c2 == 45:                                                     # '-' in the read: a deletion column
            gap = 1; del_in += infl; first |= i == 0
            if prev_del:
                cross_l += x == F; cross_r += x == hapLen - F
            prev_del = True
            x += 1
            continue
        prev_del = False
        if c1 == 45:                                                     # '-' in the haplotype: an insertion column
            gap = 1; ins_in += infl; first |= i == 0
        else:
            nmm += infl and c1 == 78 and c1 != c2
            x += 1
    return gap, ins_in, del_in, cross_l, cross_r, int(first), nmm


def traceback_counts(oracle, hb, limit=None, ref=None, per_window=False):
    """The oracle on a batch in both modes, and its traceback of the DP at the mapping position (calign.pyx:252-267: idx0 clamped to
    hapLen - L - 15, st = max(0, idx0 - 8), firstpos + st as calculateFlankScore gets it) over the first `limit` such DPs that score above 0.
    A dict: pairs, windows, score_differs / score_becomes_0 (pairs the two modes score differently / that flank mode brings to 0),
    windows_dp_differs, saturated, and COUNT_KEYS.  ref (a RefAlign): score, strings, firstpos and flank score of every classified DP are
    asserted equal to the unmodified align.c's.  per_window: a list of such dicts, one per window, instead of their sum."""
    out, left = [], (1 << 62) if limit is None else limit
    for w in range(hb.n_windows):
        haps, rd = hb.window_haps(w), hb.window_reads(w)
        ws, we, F = int(hb.win_start[w]), int(hb.win_end[w]), int(hb.win_flank[w])
        _, sc0, n0 = oracle.align_window(haps, ws, we, F, rd)
        oracle.tb_saturated()
        _, sc1, n1 = oracle.align_window(haps, ws, we, F, rd, do_flank=1)
        c = dict.fromkeys(COUNT_KEYS, 0)
        c.update(pairs=sc0.size, windows=1, score_differs=int((sc0 != sc1).sum()), score_becomes_0=int(((sc1 == 0) & (sc0 != 0)).sum()),
                 windows_dp_differs=int(n0 != n1), saturated=oracle.tb_saturated())
        for h, hap in enumerate(haps):
            go = oracle.gap_open(hap)
            for r, (seq, q) in enumerate(zip(rd["seq"], rd["qual"])):
                if left <= 0 or sc0[h, r] < 0 or len(seq) < 7:          # (skipped by the overlap rule; shorter than a k-mer: no DP)
                    continue
                L = len(seq)
                st = max(0, min(int(rd["pos"][r]) - (ws - F), len(hap) - L - 15) - 8)
                got = oracle.dp_align(hap[st:], seq, q, go[st:])
                if got[0] <= 0:
                    continue
                left -= 1
                if ref is not None:
                    assert ref.dp_align(hap[st:], seq, q, go[st:]) == got, (w, h, r)
                    args = (len(hap), F, q, go, got[3] + st, got[1], got[2])
                    assert ref.flank_score(*args) == oracle.flank_score(*args), (w, h, r)
                c["classified"] += 1
                for key, v in zip(COUNT_KEYS[1:], classify(got[1], got[2], got[3] + st, len(hap), F)):
                    c[key] += int(v)
        out.append(c)
    return out if per_window else {k: sum(c[k] for c in out) for k in out[0]}
