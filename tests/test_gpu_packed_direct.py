"""Packed bases read where they lie: the entry points that take a chunk's reads as PLAT_READS_PACKED bytes at their source, each against its
counterpart on the expanded (ASCII) table -- plat_pack_codes_pieces / plat_unpack_reads_pieces_codes, plat_gather_reads_packed / plat_gather_reads,
plat_candidates_batch_packed / plat_candidates_batch_codes, plat_variant_read_stats_packed_batch / plat_variant_read_stats_batch -- and the
native region loop on its three read paths: the default, PLAT_CALLER_EXPAND=1 (the full expansion) and PLAT_CALLER_NO_CODES=1 (the byte scan).
Integer / byte work: everything is compared exactly."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PAD = 32
ACTG = np.frombuffer(b"ACTG", dtype=np.uint8)


@pytest.fixture(scope="module")
def eng():
    from platypus_amd.engine import Engine
    return Engine(0)


def _dev(eng, a, dt):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(eng.device)


# ---- the codes-only first pass ------------------------------------------------------------------------------------------------------------------
def test_codes_only_pass_equals_the_full_unpack_word_for_word(eng):
    """Pieces of 0, 1, 15, 16, 17, 31, 33, 150 and 4099 bytes, each at every source misalignment x every destination misalignment (0-15), laid back to
    back as a chunk's tables are (short filler pieces set the next destination's alignment: neighbours share a dword all along); exceptions on a
    piece's first and last byte and on both sides of a dword boundary.  The output buffer starts as a pattern, not as zeros: every word up to the
    eight tail words must come out as plat_unpack_reads_pieces_codes writes it (and as numpy packs the expanded bytes), the tail zero, the words
    behind it untouched."""
    import torch
    from platypus_amd import _lib
    from platypus_amd.engine import Engine
    rng = np.random.default_rng(2101)
    lengths = [0, 1, 15, 16, 17, 31, 33, 150, 4099]
    plan = []                                                               # (length, source misalignment), destination fixed below
    dst = 0
    for n in lengths:
        for sm in range(16):
            for dm in range(16):
                fill = (dm - dst) % 16
                if fill:
                    plan.append((fill, int(rng.integers(0, 16)), dst)); dst += fill
                assert dst % 16 == dm
                plan.append((n, sm, dst)); dst += n
    total = dst
    src_at, at = [], 0
    for n, sm, _ in plan:
        at += (sm - at) % 16
        src_at.append(at); at += n
    blob = rng.integers(0, 256, at + 64).astype(np.uint8)
    dblob = _dev(eng, blob, np.uint8)
    assert dblob.data_ptr() % 16 == 0
    pieces = np.array([[dblob.data_ptr() + a, d, n] for (n, _, d), a in zip(plan, src_at)], dtype=np.int64)
    pc = _dev(eng, pieces.reshape(-1), np.int64)
    big = [k for k, (n, _, _) in enumerate(plan) if n >= 33]
    exc = set()
    for k in (big[0], big[7], big[100], big[-1], big[-300]):
        n, _, d = plan[k]
        first_line = (d + 15) // 16 * 16                                   # a dword boundary inside the piece
        exc.update([d, d + n - 1, first_line - 1, first_line, first_line + 16 - 1, first_line + 16])
    exc_i = np.array(sorted(e for e in exc if 0 <= e < total), dtype=np.int64)
    exc_b = rng.choice(np.frombuffer(b"NACGT", dtype=np.uint8), len(exc_i))
    exc_b[::2] = ord("N")
    exc_q = rng.integers(0, 94, len(exc_i)).astype(np.uint8)
    di, db, dq = _dev(eng, exc_i, np.int64), _dev(eng, exc_b, np.uint8), _dev(eng, exc_q, np.uint8)
    nw = (total + 15) // 16
    most = max(n for n, _, _ in plan)
    oseq = torch.zeros(total + PAD, dtype=torch.uint8, device=eng.device)
    oqual = torch.zeros(total + PAD, dtype=torch.uint8, device=eng.device)
    old = torch.full((nw + 8,), -1, dtype=torch.int32, device=eng.device)
    _lib.check(eng.lib.plat_unpack_reads_pieces_codes(eng.ctx, len(plan), most, pc.data_ptr(), oseq.data_ptr(), oqual.data_ptr(), old.data_ptr(), total,
                                                      len(exc_i), di.data_ptr(), db.data_ptr(), dq.data_ptr(), eng._stream()), "plat_unpack_reads_pieces_codes")
    SENT = 0x5EA1AB1E
    new = torch.from_numpy(np.full(nw + 8 + 16, SENT, dtype=np.uint32).view(np.int32)).to(eng.device)
    eng.pack_codes_pieces(pc, len(plan), most, new, total, di, db)
    got, want = new.cpu().numpy().view(np.uint32), old.cpu().numpy().view(np.uint32)
    assert np.array_equal(got[:nw + 8], want)
    assert (got[nw:nw + 8] == 0).all() and (got[nw + 8:] == SENT).all()
    assert np.array_equal(want, Engine.base_codes(oseq.cpu().numpy()[:total].tobytes()))


# ---- the gather --------------------------------------------------------------------------------------------------------------------------------
def _gather_case():
    rng = np.random.default_rng(2102)
    lens = [n for n in (0, 1, 15, 16, 17, 150, 251) for _ in range(16)]
    seqs, quals = [], []
    for k, n in enumerate(lens):
        s, q = ACTG[rng.integers(0, 4, n)].copy(), rng.integers(0, 64, n).astype(np.uint8)
        if n and k % 3 == 0:
            s[0] = ord("N"); s[-1] = ord("N")                              # exceptions on the read's first and last base
        if n and k % 5 == 0:
            q[n // 2] = 64 + k % 30                                         # a quality above 63
        seqs.append(s.tobytes()); quals.append(q.tobytes())
    gaps, at = [], 0
    for k, n in enumerate(lens):                                            # read k's packed bytes start at alignment k % 16
        g = (k % 16 - at) % 16
        gaps.append(g); at += g + n
    return lens, seqs, quals, gaps


def test_packed_gather_equals_the_gather_of_the_expanded_table(eng):
    """Reads of 0, 1, 15, 16, 17, 150 and 251 bases, each with its packed bytes at every alignment 0-15; N on a read's first and last base and
    qualities above 63 (exceptions); every read gathered at least twice, destinations at every alignment with three sentinel bytes behind each."""
    import torch
    from platypus_amd import _lib
    lens, seqs, quals, gaps = _gather_case()
    n = len(lens)
    rng = np.random.default_rng(2103)
    pk = eng.pack_reads(seqs, quals, gaps)
    assert sorted(set((pk["src"].cpu().numpy() % 16).tolist())) == list(range(16)) and pk["reads"].n_exc > 20
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    seq = np.frombuffer(b"".join(seqs), dtype=np.uint8)
    qual = np.frombuffer(b"".join(quals), dtype=np.uint8)
    pos, end = rng.integers(0, 1 << 30, n), rng.integers(0, 1 << 30, n)
    mapq, flags = rng.integers(0, 256, n), rng.integers(0, 1 << 12, n)
    src = np.concatenate([np.arange(n), np.arange(n)[::-1], rng.integers(0, n, 300), [5] * 20])
    slen = np.asarray(lens)[src]
    doff = np.concatenate([[0], np.cumsum(slen + 3)]).astype(np.int64)     # (three bytes between destination reads: nobody's)
    nd = len(src)
    d = dict(src=_dev(eng, src, np.int32), doff=_dev(eng, doff, np.int64), seq=_dev(eng, np.concatenate([seq, np.zeros(PAD, np.uint8)]), np.uint8),
             qual=_dev(eng, np.concatenate([qual, np.zeros(PAD, np.uint8)]), np.uint8), off=_dev(eng, off, np.int64), pos=_dev(eng, pos, np.int32),
             end=_dev(eng, end, np.int32), mapq=_dev(eng, mapq, np.uint8), flags=_dev(eng, flags, np.int32))

    def outputs():
        return dict(seq=torch.full((int(doff[-1]) + PAD,), 0xEE, dtype=torch.uint8, device=eng.device),
                    qual=torch.full((int(doff[-1]) + PAD,), 0xEE, dtype=torch.uint8, device=eng.device),
                    pos=torch.zeros(nd, dtype=torch.int32, device=eng.device), end=torch.zeros(nd, dtype=torch.int32, device=eng.device),
                    mapq=torch.zeros(nd, dtype=torch.uint8, device=eng.device), flags=torch.zeros(nd, dtype=torch.int32, device=eng.device))
    a, b = outputs(), outputs()
    _lib.check(eng.lib.plat_gather_reads(eng.ctx, nd, d["src"].data_ptr(), d["doff"].data_ptr(), d["seq"].data_ptr(), d["qual"].data_ptr(), d["off"].data_ptr(),
                                         d["pos"].data_ptr(), d["end"].data_ptr(), d["mapq"].data_ptr(), d["flags"].data_ptr(), a["seq"].data_ptr(), a["qual"].data_ptr(),
                                         a["pos"].data_ptr(), a["end"].data_ptr(), a["mapq"].data_ptr(), a["flags"].data_ptr(), eng._stream()), "plat_gather_reads")
    eng.gather_reads_packed(nd, d["src"], d["doff"], pk["reads"], d["off"], d["pos"], d["end"], d["mapq"], d["flags"], b["seq"], b["qual"], b["pos"], b["end"],
                            b["mapq"], b["flags"])
    for k in a:
        assert np.array_equal(a[k].cpu().numpy(), b[k].cpu().numpy()), k
    got = b["seq"].cpu().numpy()
    assert all((got[doff[k] + slen[k]:doff[k + 1]] == 0xEE).all() for k in range(nd)) and (got[doff[-1]:] == 0xEE).all()
    want = np.concatenate([np.concatenate([seq[off[s]:off[s + 1]], [0xEE] * 3]) for s in src]).astype(np.uint8)
    assert np.array_equal(got[:doff[-1]], want)                              # (and both are what numpy gathers)


# ---- the scan and the read statistics -------------------------------------------------------------------------------------------------------
MIN_FLANK, MIN_BQ = 10, 20


def _scan_regions():
    """Two regions, ~100 reads each: random reads with a sprinkling of mismatches, and the reads the scan's edges ask for (see the test)."""
    rng = np.random.default_rng(2104)
    regions, notes = [], {}
    for g in range(2):
        ref = ACTG[rng.integers(0, 4, 700)].copy()
        if g == 1:
            ref[300] = ord("R")                                             # an irregular reference region: scanned byte by byte
        reads = []

        def other(b):
            return ACTG[(int(np.nonzero(ACTG == b)[0][0]) + 1) % 4] if b in ACTG else ord("A")

        def read(pos, n=100, cigar=None, mism=(), qual=30, flag=0, edit=None, quals=None):
            cigar = cigar or [(0, n)]
            s, rp, fp = [], 0, pos
            for op, ln in cigar:                                            # the read's bases follow the reference through its CIGAR
                if op == 0:
                    s.append(ref[fp:fp + ln]); fp += ln
                elif op in (1, 4):
                    s.append(ACTG[rng.integers(0, 4, ln)])
                    if op == 4 and not s[:-1]:
                        fp += ln                                            # (a leading soft clip: `pos` is where the clipped bases would start)
                elif op == 2:
                    fp += ln
            s = np.concatenate(s).copy()
            for i in mism:
                s[i] = other(s[i])
            q = np.full(len(s), qual, dtype=np.uint8)
            for i, v in (quals or {}).items():
                q[i] = v
            for i, v in (edit or {}).items():
                s[i] = v
            reads.append(dict(seq=s.tobytes(), qual=q.tobytes(), pos=pos, end=fp, mapq=60, flag=flag, cigar=cigar))
            return len(reads) - 1
        for _ in range(85):
            n = int(rng.integers(60, 140))
            p = int(rng.integers(0, 700 - n - 1))
            k = int(rng.integers(0, 4))
            read(p, n, mism=sorted(set(rng.integers(0, n, k).tolist())), quals={int(rng.integers(0, n)): int(rng.integers(0, 40))})
        N = ord("N")
        notes[g] = dict(
            flank=read(40, mism=(9, 10, 89, 90)),                            # SNPs exactly at minFlank from either end (10, 89) and one base outside (9, 90)
            mnp_n=read(60, mism=(30, 32, 35), edit={31: N}),                # an MNP whose span holds an N
            ins_n=read(80, cigar=[(0, 40), (1, 3), (0, 57)], edit={41: N}),  # an insertion containing N: dropped
            ins=read(90, cigar=[(0, 40), (1, 3), (0, 57)]),
            ins_first=read(100, cigar=[(1, 4), (0, 96)]),                   # an insertion as the first operation
            clip=read(120, cigar=[(4, 5), (0, 95)], mism=(30, 50)),         # a soft clip
            dele=read(140, cigar=[(0, 50), (2, 2), (0, 50)], mism=(20,)),
            q_hi=read(160, mism=(40, 70), quals={40: 70, 70: 200}),         # mismatches whose qualities are exceptions (> 63)
            q_lo=read(180, mism=(40, 60), quals={40: MIN_BQ - 1, 60: MIN_BQ}),   # one below minBaseQual, one at it
            qcfail=read(200, mism=(30, 40, 50), flag=512),                  # Read_IsQCFail: skipped
            many=read(220, n=251, mism=tuple(range(15, 236, 13))),          # 17 runs: overflows a slice of one record (and of eight)
            n_run=read(250, mism=(50,), edit={i: N for i in range(20, 45)}),
        )
        off = sum(len(r["seq"]) for r in reads)
        read(300, n=60 + (31 - off - 60) % 32)                              # the next read starts at base 31 of a code word (of the region's blob so far)
        notes[g]["word31"] = read(320, mism=(11, 12, 43, 75))
        regions.append(dict(ref=ref.tobytes(), ref_seq_start=0, contig_len=len(ref) + 1, reads=reads))
    return regions, notes


def _source_gaps(regions):
    """Bytes in front of every read's packed bytes: the sources then lie at every alignment, whatever the reads' lengths."""
    gaps, at, k = [], 0, 0
    for g in regions:
        for r in g["reads"]:
            gp = (k % 16 - at) % 16
            gaps.append(gp); at += gp + len(r["seq"]); k += 1
    return gaps


@pytest.fixture(scope="module")
def scan_regions():
    return _scan_regions()


def test_packed_scan_equals_the_scan_of_the_expanded_table(eng, scan_regions):
    """rec, count and status of plat_candidates_batch_packed equal plat_candidates_batch_codes' on the expanded bytes, with a slice of ONE record per
    read (most reads overflow: the retry's first half) and with room for every record; and read_seq[x[4] .. x[4] + x[2]) of every record -- those
    that did not fit their slice included -- holds the expanded bytes, every other byte of read_seq what it was."""
    regions, notes = scan_regions
    reads = [r for g in regions for r in g["reads"]]
    blob = np.frombuffer(b"".join(r["seq"] for r in reads), dtype=np.uint8)
    off = np.concatenate([[0], np.cumsum([len(r["seq"]) for r in reads])])
    first = [0, len(regions[0]["reads"])]
    w31 = first[1] + notes[1]["word31"]
    assert off[first[0] + notes[0]["word31"]] % 32 == 31 or off[w31] % 32 == 31
    gaps = _source_gaps(regions)
    kw = dict(min_flank=MIN_FLANK, min_base_qual=MIN_BQ, retry=False)
    eng.candidates(regions, codes=True, max_per_read=1, **kw)
    a1 = eng.last_candidates
    eng.candidates(regions, packed=True, gaps=gaps, max_per_read=1, **kw)
    b1 = eng.last_candidates
    need = int(a1["count"].max())
    eng.candidates(regions, codes=True, max_per_read=need, **kw)
    a2 = eng.last_candidates
    eng.candidates(regions, packed=True, gaps=gaps, max_per_read=need, **kw)
    b2 = eng.last_candidates
    for a, b in ((a1, b1), (a2, b2)):
        assert np.array_equal(a["rec"], b["rec"]) and np.array_equal(a["count"], b["count"]) and np.array_equal(a["status"], b["status"])
    assert need >= 17 and (a1["status"] == -8).sum() > 40 and (a2["status"] == 0).all()
    touched = np.zeros(len(blob), dtype=bool)
    n_read_side = 0
    for r in np.nonzero(a2["count"])[0]:
        for p_, nrem, nadd, ro, ao in a2["rec"][r, :a2["count"][r]].tolist():
            if nadd:
                assert off[r] <= ao and ao + nadd <= off[r + 1]
                touched[ao:ao + nadd] = True; n_read_side += 1
    for b in (b1, b2):                                                      # (the slice of one record: the bytes of the records that did not fit are there too)
        assert np.array_equal(b["read_seq"][touched], blob[touched]) and (b["read_seq"][~touched] == 0xEE).all()
    assert n_read_side > 150
    # the reads the edges ask for did what they are there for
    def recs(g, key):
        r = first[g] + notes[g][key]
        return [tuple(x[:3]) for x in a2["rec"][r, :a2["count"][r]].tolist()]
    for g in (0, 1):
        assert recs(g, "flank") == [(40 + 10, 1, 1), (40 + 89, 1, 1)]
        assert recs(g, "mnp_n") == [(60 + 30, 6, 6)]
        r = first[g] + notes[g]["mnp_n"]
        ao, nadd = a2["rec"][r, 0, 4], a2["rec"][r, 0, 2]
        assert ord("N") in blob[ao:ao + nadd] and ord("N") in b2["read_seq"][ao:ao + nadd]
        assert recs(g, "ins_n") == [] and [x[1:] for x in recs(g, "ins")] == [(0, 3)] and recs(g, "ins_first")[0][1:] == (0, 4)
        assert a2["rec"][first[g] + notes[g]["ins_first"], 0, 4] == off[first[g] + notes[g]["ins_first"]]
        assert len(recs(g, "clip")) == 2 and (0 + 140 + 49, 2, 0) in recs(g, "dele")
        assert len(recs(g, "q_hi")) == 2 and len(recs(g, "q_lo")) == 1 and recs(g, "qcfail") == [] and len(recs(g, "many")) == 17
        assert len(recs(g, "word31")) == 3


def test_packed_read_statistics_equal_the_expanded_table_s(eng, scan_regions):
    """plat_variant_read_stats_packed_batch on the scan's reads (good and bad lists, a quality of 200 -- negative as the reference's signed char --
    inside a variant's window, N bases, insertions and deletions to match exactly or not): every output equal."""
    regions, notes = scan_regions
    found = eng.candidates(regions, codes=True, min_flank=MIN_FLANK, min_base_qual=MIN_BQ, max_per_read=32)
    windows = []
    for g, reg in enumerate(regions):
        seen, variants = set(), []
        for p_, rem, add, r in found[g]:
            if (p_, rem, add) in seen or len(variants) >= 40:
                continue
            seen.add((p_, rem, add))
            variants.append(dict(pos=p_, removed=rem, added=add, bam_min=p_ - 1, bam_max=p_ + max(len(rem), len(add)) + 1))
        q_hi = reg["reads"][notes[g]["q_hi"]]
        variants.append(dict(pos=q_hi["pos"] + 68, removed=b"A", added=b"C", bam_min=q_hi["pos"] + 66, bam_max=q_hi["pos"] + 74))   # (the quality of 200 lies inside)
        reads = sorted(reg["reads"], key=lambda x: x["pos"])
        windows.append(dict(variants=variants, samples=[dict(good=reads[::2] + reads[1::4], bad=reads[3::4])],
                            var_in_genotype=[[k % 3 != 0] for k in range(len(variants))]))
    n_reads = sum(len(s["good"]) + len(s["bad"]) for w in windows for s in w["samples"])
    gaps = [(k * 7) % 16 for k in range(n_reads)]
    for exact in (0, 1):
        a = eng.variant_read_stats(windows, bad_reads_window=11, exact=exact)
        b = eng.variant_read_stats(windows, bad_reads_window=11, exact=exact, packed=True, gaps=gaps)
        assert a == b
        assert sum(v[0][2] for w in a for v in w) > 60 and sum(len(v[3]) for w in a for v in w) > 30       # supporting reads, MMLQ entries


# ---- the region loop -----------------------------------------------------------------------------------------------------------------------
SWITCHES = ("PLAT_CALLER_EXPAND", "PLAT_CALLER_NO_CODES")


def _region_cases(inputs, switch=None):
    """The four region-loop cases: {name: [record text, region text lengths, counters]} -- and, from a counting pass over the first, the
    algorithmic bytes of the first pass (1 1/4 per base when the bases are read where they lie, 3 1/4 when the table is expanded, 3 without
    the codes) -- with `switch` (one of SWITCHES, or None) set to 1 in the environment and the other unset, as tests/test_gpu_stage_b.py sets its own."""
    old = {k: os.environ.pop(k, None) for k in SWITCHES}
    if switch:
        os.environ[switch] = "1"
    try:
        return _region_cases_here(*inputs)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _region_inputs():
    """(fasta, [(chrom, start, end, [bamReadBuffer])]) of the region-loop cases."""
    from platypus_amd import hostapi as H, synth
    rng = np.random.default_rng(2105)
    regs = [synth.config4_region(2100 + i, n_samples=1, region_len=2500, snp_rate=8e-3, indel_rate=3e-3, read_len=100, depth=24) for i in range(3)]
    fasta = H.FastaFile({r["chrom"]: r["ref"] for r in regs})
    work = []
    for r in regs:
        good, bad, broken = [], [], []
        for x in r["samples"][0]:
            seq, qual = bytearray(x["seq"]), bytearray(x["qual"])
            u = rng.random()
            if u < 0.05:
                seq[int(rng.integers(0, len(seq)))] = ord("N")              # exceptions: N bases and qualities above 63
            elif u < 0.1:
                qual[int(rng.integers(0, len(qual)))] = 64 + int(rng.integers(0, 30))
            a = H.AlignedRead(bytes(seq), bytes(qual), x["pos"], x["mapq"], x["flag"], end=x["end"], cigarOps=x["cigar"])
            u = rng.random()
            if u < 0.06:
                a.mapq = 5; a.bitFlag |= 512; bad.append(a)
            elif u < 0.1:
                a.matePos = a.pos + int(rng.integers(-300, 300)); broken.append(a)
            else:
                good.append(a)
        broken.sort(key=lambda q: q.matePos)
        work.append((r["chrom"], r["start"], r["end"], [H.bamReadBuffer(good, bad, broken, sample="S1")]))
    return fasta, work


def _region_cases_here(fasta, work):
    import torch
    from platypus_amd import fastcaller as F, hostapi as H
    from platypus_amd.options import default_options

    def regions(resident=False, drop=None):
        out, keep = [], []
        for k, (c, s, e, b) in enumerate(work):
            if drop == k:
                b = [H.bamReadBuffer([], [], [], sample="S1")]
            rr = F.RegionReads.from_buffers(c, s, e, fasta, b, packed=True)
            if resident:                                                    # the packed bytes in HBM already (dev_seq): nothing of them crosses the link
                for tabs in rr.samples:
                    for t in tabs:
                        if t.n:
                            d = torch.from_numpy(t.seq).to("cuda:0")
                            keep.append(d)
                            t.struct().dev_seq = d.data_ptr()
            out.append(rr)
        return out, keep

    def run(rs, counting=False, **opt):
        o = default_options()
        for k, v in opt.items():
            setattr(o, k, v)
        nc = F.NativeCaller(0, 1, 4)                                        # (one chunk of all three regions)
        try:
            if counting:
                nc.count_cells(True)
            txt = nc.call_regions(rs, ["S1"], o)
            st = nc.stats
            return [txt, nc.region_text_lengths(len(rs)).tolist(),
                    [st[k] for k in ("n_reads", "n_candidate_records", "n_variants", "n_windows", "n_records", "n_assembler_variants", "input_bytes")]], st
        finally:
            nc.close()
    out = {}
    rs, keep = regions(resident=True)
    out["resident"], _ = run(rs)
    up, _ = regions()
    out["uploaded"], _ = run(up)
    rs2, keep2 = regions(resident=True, drop=1)
    out["empty_table"], _ = run(rs2)
    out["assemble"], _ = run(up, assemble=1)
    _, st = run(up, counting=True)
    n_bases = sum(int(t.off[t.n]) for rr in up for tabs in rr.samples for t in tabs)
    out["first_pass_bytes"] = [int(st["unpack_bytes"]), n_bases]
    return out


def test_region_loop_gives_the_text_of_the_full_expansion():
    """Three small regions in one chunk -- reads, badReads and brokenMates tables, N and Q > 63 exceptions -- resident (dev_seq) and uploaded, a
    chunk with an empty table, and assemble=1: record text, region text lengths and counters of the default path are those of PLAT_CALLER_EXPAND=1
    and of PLAT_CALLER_NO_CODES=1, all in this process (the switches are read at every call).  The counting pass says which path each run took;
    the default path run again last gives what it gave first (a switch frozen at the process's first chunk, or at the first one set, would not)."""
    inputs = _region_inputs()
    here = _region_cases(inputs)
    expanded = _region_cases(inputs, "PLAT_CALLER_EXPAND")
    bytescan = _region_cases(inputs, "PLAT_CALLER_NO_CODES")
    again = _region_cases(inputs)
    for there in (expanded, bytescan):
        for case in ("resident", "uploaded", "empty_table", "assemble"):
            assert here[case][:2] == there[case][:2], case
            assert here[case][2][:6] == there[case][2][:6], case
            assert here[case][0].count("\n") > 20, case
    for run in (here, expanded, bytescan):
        assert run["resident"][0] == run["uploaded"][0] and run["resident"][2][6] < run["uploaded"][2][6]
        assert run["assemble"][2][5] > 0
    b_here, n = here["first_pass_bytes"]
    assert [n, n] == [expanded["first_pass_bytes"][1], bytescan["first_pass_bytes"][1]]
    assert b_here == n + n // 4 and expanded["first_pass_bytes"][0] == 3 * n + n // 4 and bytescan["first_pass_bytes"][0] == 3 * n
    assert again == here
