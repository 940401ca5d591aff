"""Whole BAM files written in memory for the tests of include/platypus_caller_bamfile.h: header text + references, records in the order
given (coordinate order for the hand-made files), the record stream cut into BGZF blocks of about 120 payload bytes -- records and
chunks cross blocks -- with the 28-byte EOF block behind them, and a .bai built the way index_query_cases.synthetic_bai builds one: ONE
CHUNK PER RECORD, bin = reg2bin(beg, end), the linear index holding the lowest record offset per 16 kb window.

Also here: the Python restatements the tests compare the library with -- the window of a region, the fetch of a region from a file
(tabixindex.BamIndex's query and tabixindex.cut_chunks, the BAI rule and the cut by BSIZE)."""
import gzip
import json
import os
import struct

import numpy as np

from platypus_amd import synth, tabixindex
from tests import bgzf_cases as K
from tests import index_query_cases as Q

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "bam_header_cases.json.gz")
BLOCK_PAYLOAD = 120


def golden():
    with gzip.open(GOLDEN, "rt") as f:
        return json.load(f)


def bam_header(text, refs):
    """BAM\\1, l_text, text, n_ref, (l_name, name NUL-ended, l_ref) per reference."""
    text = text if isinstance(text, bytes) else text.encode()
    out = b"BAM\x01" + struct.pack("<i", len(text)) + text + struct.pack("<i", len(refs))
    for name, length in refs:
        name = (name if isinstance(name, bytes) else name.encode()) + b"\0"
        out += struct.pack("<i", len(name)) + name + struct.pack("<i", length)
    return out


def record_span(rec):
    """(tid, beg, end) of one record (block_size word in front) as the record walk sees it: end = pos + the CIGAR's reference length, pos + 1 without one."""
    tid, pos = struct.unpack_from("<ii", rec, 4)
    l_name, n_cig = rec[12], struct.unpack_from("<H", rec, 16)[0]
    words = struct.unpack_from("<%dI" % n_cig, rec, 36 + l_name)
    return tid, pos, pos + (sum(w >> 4 for w in words if (w & 15) in (0, 2, 3, 7, 8)) if n_cig else 1)


def write_bam(text, refs, records, block_payload=BLOCK_PAYLOAD, header_payload=None):
    """(the .bam's bytes, the .bai's bytes, where every record lies: [(tid, beg, end, u, v)]).  The header goes into blocks of its own
    (header_payload bytes each, by default block_payload), the records into blocks of block_payload bytes."""
    head = bam_header(text, refs)
    hs, _ = synth.bgzf_stream(head, block_payload=header_payload or block_payload, eof=False)
    body = b"".join(records)
    bs, off = synth.bgzf_stream(body, block_payload=block_payload, eof=True)
    off = [int(o) + len(hs) for o in off]
    vo = lambda at: (off[at // block_payload] << 16) | (at % block_payload)
    placed, at = [], 0
    for rec in records:
        tid, beg, end = record_span(rec)
        placed.append((tid, beg, end, vo(at), vo(at + len(rec))))
        at += len(rec)
    bins, lin = [dict() for _ in refs], [[0] * ((length >> 14) + 1) for _, length in refs]
    for tid, beg, end, u, v in placed:
        if tid < 0 or end <= beg:
            continue
        bins[tid].setdefault(Q.reg2bin(beg, end), []).append((u, v))
        for w in range(beg >> 14, ((end - 1) >> 14) + 1):
            if lin[tid][w] == 0 or u < lin[tid][w]:
                lin[tid][w] = u
    for ln in lin:                                                          # (as an indexer leaves it: an empty window takes the offset of the one in front)
        for w in range(1, len(ln)):
            if ln[w] == 0:
                ln[w] = ln[w - 1]
    bai = Q.Hand(bins, lin, pseudo=(0,), n_no_coor=0).bai()
    return hs + bs, bai, placed


def sq_lines(refs):
    return "".join("@SQ\tSN:%s\tLN:%d\n" % (n, l) for n, l in refs)


# ---- the hand-made files --------------------------------------------------------------------------------------------------------------
def _spread(rng, tid, n, lo, hi, aux=None):
    pos = sorted(rng.randrange(lo, hi) for _ in range(n))
    return [K.record(tid, p, [(0, ln)], n_bases=ln, name=b"q%d\0" % i, aux=aux(i) if aux else b"")
            for i, p in enumerate(pos) for ln in [rng.randrange(20, 51)]]


def two_contigs():
    """2 references, 60 records of 20-50 bases and three spliced ones that span 16 kb windows (they lie in bins of a higher level, so a
    fetch comes back as several chunks), one @RG."""
    import random
    rng = random.Random(11)
    refs = [("chrA", 40000), ("chrB", 30000)]
    text = "@HD\tVN:1.4\tSO:coordinate\n" + sq_lines(refs) + "@RG\tID:g1\tSM:NA1\tPL:X\n@PG\tID:w\tPN:w\n@CO\tany text: here\n"
    recs = _spread(rng, 0, 40, 100, 39000) + _spread(rng, 1, 20, 50, 29000)
    for p in (3000, 12000, 21000):
        recs.append(K.record(0, p, [(0, 20), (3, 17000), (0, 20)], n_bases=40, name=b"spliced\0"))
    recs.sort(key=lambda r: record_span(r)[:2])
    return dict(name="two_contigs.bam", text=text, refs=refs, records=recs, groups=[(b"g1", b"NA1")], samples=[b"NA1"])


def two_samples_merged():
    """2 @RG with different SM, the records alternating between them."""
    import random
    rng = random.Random(12)
    refs = [("chrA", 40000), ("chrB", 30000)]
    text = "@HD\tVN:1.4\n" + sq_lines(refs) + "@RG\tID:ga\tSM:T2\n@RG\tID:gb\tSM:T1\n"
    recs = _spread(rng, 0, 40, 100, 39000, aux=lambda i: b"RGZ" + (b"ga", b"gb")[i % 2] + b"\0")
    return dict(name="two_samples_merged.bam", text=text, refs=refs, records=recs, groups=[(b"ga", b"T2"), (b"gb", b"T1")], samples=[b"T2", b"T1"])


def split_pair():
    """One sample over two files."""
    import random
    rng = random.Random(13)
    refs = [("chrA", 40000), ("chrB", 30000)]
    out = []
    for k, g in enumerate(("ra", "rb")):
        text = sq_lines(refs) + "@RG\tID:%s\tSM:ONE\n" % g
        recs = _spread(rng, 0, 25, 100 + 15000 * k, 15000 * (k + 1), aux=lambda i, g=g: b"RGZ" + g.encode() + b"\0")
        out.append(dict(name="split_%s.bam" % "ab"[k], text=text, refs=refs, records=recs, groups=[(g.encode(), b"ONE")], samples=[b"ONE"]))
    return out


def no_rg():
    """No @RG line: the sample is the file name's."""
    import random
    rng = random.Random(14)
    refs = [("chrA", 40000)]
    return dict(name="some/dir/no_rg.sample.bam", text="@HD\tVN:1.0\n" + sq_lines(refs), refs=refs, records=_spread(rng, 0, 12, 10, 30000), groups=[],
                samples=[b"no_rg.sample"])


def hand_files():
    a, b = split_pair()
    return [two_contigs(), two_samples_merged(), a, b, no_rg()]


def built(f, **kw):
    """f with its bytes: bam, bai, placed."""
    bam, bai, placed = write_bam(f["text"], f["refs"], f["records"], **kw)
    return dict(f, bam=bam, bai=bai, placed=placed)


# ---- the restatements -----------------------------------------------------------------------------------------------------------------
def window(start, end):
    """sam_itr_querys("%s:%s-%s" % (chrom, start, end)) by hts_parse_reg's rule, restated: 1-based inclusive text -> 0-based half-open."""
    return max(start - 1, 0), end


def fetch(f, chrom, start, end):
    """The fetch of chrom:start-end from a built file: dict(tid, itr_beg, itr_end, chunks) with chunks [(offset in the file, data_len,
    first_uoffset, end_coffset, end_uoffset)], by tabixindex's BAI rule and the cut by BSIZE."""
    names = [n for n, _ in f["refs"]]
    beg, stop = window(start, end)
    if chrom not in names:
        return dict(tid=-1, itr_beg=beg, itr_end=stop, chunks=[])
    tid = names.index(chrom)
    chunks = tabixindex.BamIndex(f["bai"]).query(tid, beg, stop)
    cut = tabixindex.cut_chunks(f["bam"], chunks)
    return dict(tid=tid, itr_beg=beg, itr_end=stop,
                chunks=[(u >> 16, len(d), fu, ec, eu) for (u, _), (d, fu, ec, eu) in zip(chunks, cut)], cut=cut)


def first_chunk_off_the_data(data, chunks):
    """(n, u, v) of the first of a query's chunks [(u, v)] that cannot be cut out of `data` -- no whole block stands at u's coffset, or
    at v's when v's uoffset says the chunk reaches into it, or the offsets leave the data --, None when every chunk can: the rule of
    tabixindex.cut_chunks turned into its refusal, for data that is a prefix of a stream of valid blocks."""
    def block_end(at):
        if at + 26 > len(data) or data[at:at + 4] != b"\x1f\x8b\x08\x04":
            return None
        e = at + struct.unpack_from("<H", data, at + 16)[0] + 1
        return e if e <= len(data) else None
    for n, (u, v) in enumerate(chunks):
        c0, c1, stop = u >> 16, v >> 16, v >> 16
        ok = c0 <= c1 <= len(data)
        if ok and v & 0xffff:
            stop = block_end(c1)
            ok = stop is not None
        if ok and stop > c0:
            ok = block_end(c0) is not None
        if not ok:
            return n, u, v
    return None


NO_CUT = "does not begin and end at BGZF block headers inside the file's data"


def kept_records(f, chrom, start, end):
    """The records of a built file sam_itr_next keeps for chrom:start-end, by the rule: indices into f["records"]."""
    names = [n for n, _ in f["refs"]]
    beg, stop = window(start, end)
    tid = names.index(chrom)
    return [i for i, (t, b, e, _, _) in enumerate(f["placed"]) if t == tid and e > beg and b < stop]


# ---- files whose reads produce VCF records: the reads of committed cases of region_fetched_cases.json.gz ----------------------------------
VCF_REFS = [(str(k), 5000 + 10 * k) for k in range(1, 22)]               # "20" is tid 19, as the cases' reads say (chromID 19)
# The cases the files are written from.  A BAM record has no end field: the decoder derives a read's end by bam_endpos's rule, and in most
# committed cases some reads carry an end that rule does not give, so the record front ends give their lines up to such reads' share (GOF
# of a sample, mostly; tests/test_gpu_bam_records.py prints how many cases come out verbatim).  Cases 3 and 33 are among those the record
# path of plat_call_bam_regions gives verbatim: one sample, and two samples with an option off its default.
ONE_SAMPLE_CASE, TWO_SAMPLE_CASE = 3, 33


def fetched_cases():
    with gzip.open(os.path.join(HERE, "golden", "region_fetched_cases.json.gz"), "rt") as f:
        return json.load(f)


def _rule_end(x):
    cig = x["cigar"]
    rec_pos = x["pos"] + (cig[0][1] if cig and cig[0][0] == 4 else 0)
    return rec_pos + 1 if (x["flag"] & 4) or not cig else rec_pos + sum(ln for op, ln in cig if op in (0, 2, 3, 7, 8))


def case_records(reads, rg=None, extra_tid=20, extra_seq=None, extra_at=()):
    """The reads of one sample of a case as records behind their block_size words, in the case's order, each with RG:Z:<rg> when rg is
    given; then, on reference extra_tid, reads that copy extra_seq at extra_at (they show no variant)."""
    from platypus_amd import hostapi as H
    out = []
    aux = b"RGZ" + rg + b"\0" if rg else b""
    for i, x in enumerate(reads):
        rec = synth.bam_record(K.aligned(x, _rule_end(x)), name=b"r%d\0" % i, aux=aux)
        out.append(struct.pack("<i", len(rec)) + rec)
    for i, p in enumerate(extra_at):
        r = H.AlignedRead(extra_seq[p:p + 60], bytes([35] * 60), p, 60, 3, end=p + 60, cigarOps=[(0, 60)], chromID=extra_tid, mateChromID=extra_tid,
                          insertSize=200, matePos=p + 140)
        rec = synth.bam_record(r, name=b"x%d\0" % i, aux=aux)
        out.append(struct.pack("<i", len(rec)) + rec)
    return out


def other_contig_seq(n=5210, seed=77):
    rng = np.random.default_rng(seed)
    return bytes(b"ACGT"[int(v)] for v in rng.integers(0, 4, n))


def vcf_files(layout):
    """Built files over committed cases, with the golden record lines they must give.  layout:
         "one"        the one-sample case, one file, one @RG
         "two"        the two-sample case, two files with one sample each (S2's file listed first)
         "merged"     the two-sample case, one file, two @RG, the records merged by position
         "split"      the one-sample case, one sample over two files: the first half of its records, then the rest
    Returns dict(files [built], case, samples [sorted names], regions [(chrom, start, end, contig bytes)])."""
    from platypus_amd import fastcaller as F
    cases = fetched_cases()
    other = other_contig_seq()
    extra = dict(extra_seq=other, extra_at=(300, 320, 2000))
    head = "@HD\tVN:1.4\tSO:coordinate\n" + sq_lines(VCF_REFS)
    mk = lambda name, rgs, recs: built(dict(name=name, text=head + "".join("@RG\tID:%s\tSM:%s\n" % g for g in rgs), refs=VCF_REFS, records=recs))
    if layout == "one":
        case = cases[ONE_SAMPLE_CASE]
        files = [mk("one.bam", [("g1", "S1")], case_records(case["regions"][0]["samples"][0]["fetched"], **extra))]
    elif layout == "two":
        case = cases[TWO_SAMPLE_CASE]
        s = case["regions"][0]["samples"]
        files = [mk("second.bam", [("g2", "S2")], case_records(s[1]["fetched"], **extra)), mk("first.bam", [("g1", "S1")], case_records(s[0]["fetched"], **extra))]
    elif layout == "merged":
        case = cases[TWO_SAMPLE_CASE]
        s = case["regions"][0]["samples"]
        reads, aux = F.merge_by_read_group([(0, b"g1", s[0]["fetched"]), (1, b"g2", s[1]["fetched"])], lambda x: x["pos"])
        recs = [r for x, a in zip(reads, aux) for r in case_records([x], rg=a[3:-1])]
        files = [mk("merged.bam", [("g1", "S1"), ("g2", "S2")], recs + case_records([], rg=b"g1", **extra))]
    elif layout == "split":
        case = cases[ONE_SAMPLE_CASE]
        reads = case["regions"][0]["samples"][0]["fetched"]
        h = len(reads) // 2
        files = [mk("split_a.bam", [("ga", "S1")], case_records(reads[:h], rg=b"ga")), mk("split_b.bam", [("gb", "S1")], case_records(reads[h:], rg=b"gb", **extra))]
    else:
        raise ValueError(layout)
    r = case["regions"][0]
    ref = case["ref"].encode()
    regions = [(r["chrom"], r["start"], r["end"], ref), (r["chrom"], r["end"] + 400, r["end"] + 500, ref), ("21", 250, 2100, other)]
    return dict(files=files, case=case, samples=sorted(case["sample_names"]), regions=regions)
