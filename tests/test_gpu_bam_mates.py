"""GPU tests of the broken-mate fetch for whole BAM files (plat_bam_files_mates_plan, plat_call_bam_files_mates:
include/platypus_caller_bamfile.h) over files written in memory (tests/bam_file_cases.py).  The plan's queries and kept records are
compared with a Python restatement of loadBAMData's rule over the files' records (platypusutils.pyx:522-559: the coordinate rule, the
sort, mergeQueries, the second fetch, the filter, the order by mate position), and the call's text byte
for byte with plat_call_bgzf_regions / plat_call_bgzf_regions_rg handed the chunks the test cut itself plus the broken mates the
restatement gives.

The files hold the reads of committed cases (they give record lines) on a contig lengthened to 200 kb, improper pairs in the region whose
mates lie far on the same contig, on the other contig, at mtid -1 and inside the region, and those mates, some of whose own mate
positions lie just outside [start, end]."""
import struct

import numpy as np
import pytest

from platypus_amd import _lib, fastcaller as F, hostapi as H, synth
from platypus_amd.options import default_options
from tests import bam_file_cases as B

pytestmark = pytest.mark.gpu

REFS = [(str(k), 300000) for k in range(1, 22)]                             # "20" is tid 19, "21" tid 20; the names' order is not the tids'
T20, T21 = 19, 20
KT_OTHER = 31
BOTH = dict(assemble=1, assembleBrokenPairs=1)


def _fields(rec):
    """flag, mtid, mpos of a record with its block_size word in front."""
    return struct.unpack_from("<H", rec, 4 + 14)[0], struct.unpack_from("<i", rec, 4 + 20)[0], struct.unpack_from("<i", rec, 4 + 24)[0]


def merge_queries(coords):
    """mergeQueries (platypusutils.pyx:690-707), restated."""
    out = []
    for name, _, p in coords:
        if out and name == out[-1][0] and p - out[-1][2] < 10000 and p - out[-1][1] < 100000:
            out[-1][2] = p + 1
        else:
            out.append([name, p, p + 1])
    return out


def fetched(f, chrom, start, end):
    """The records sam_itr_next returns for chrom:start-end from a built file, in order: the index's chunks (tabixindex's BAI rule) walked
    one after the other, the first record on another contig or at or behind the window's end ending the fetch, a record kept when it
    reaches past the window's begin.  (bam_file_cases.kept_records without the assumption that the file is sorted by record position: the
    committed cases' reads are ordered by the position the decoder gives them, a leading soft clip moved back.)"""
    import bisect
    from platypus_amd import tabixindex
    names = [n for n, _ in f["refs"]]
    tid = names.index(chrom)
    beg, stop = B.window(start, end)
    us = [p[3] for p in f["placed"]]
    out = []
    for cu, cv in tabixindex.BamIndex(f["bai"]).query(tid, beg, stop):
        for i in range(bisect.bisect_left(us, cu), bisect.bisect_left(us, cv)):
            t, b, e = f["placed"][i][:3]
            if t != tid or b >= stop:
                return out
            if e > beg:
                out.append(i)
    return out


def restate(f, chrom, start, end):
    """The broken-mate fetch of chrom:start-end from a built file: (coordinates, queries [(tid, s, e)], mates [record bytes from refID on])."""
    names = [n for n, _ in f["refs"]]
    if chrom not in names:
        return 0, [], []
    tid = names.index(chrom)
    coords = []
    for i in fetched(f, chrom, start, end):
        flag, mtid, mpos = _fields(f["records"][i])
        if (not flag & 2 or flag & 4 or flag & 8) and mtid != -1:
            coords.append((names[mtid], mtid, mpos))
    coords.sort()
    queries = merge_queries(coords)
    mates = []
    for name, s, e in queries:
        for i in fetched(f, name, s, e):
            _, mtid, mpos = _fields(f["records"][i])
            if mtid == tid and start <= mpos <= end:
                mates.append(f["records"][i][4:])
    mates.sort(key=lambda r: struct.unpack_from("<i", r, 24)[0])
    return len(coords), [(names.index(n), s, e) for n, s, e in queries], mates


def _records(recs, with_len=False):
    data = np.frombuffer(b"".join(recs), dtype=np.uint8).copy()
    ln = np.array([len(r) for r in recs], dtype=np.int32)
    off = np.concatenate([[0], np.cumsum(ln)])[:len(recs)].astype(np.int64)
    return (data, off, ln) if with_len else (data, off)


def _read(tid, pos, flag, mtid, mpos, seq, name, rg=None):
    r = H.AlignedRead(seq, bytes([35] * len(seq)), pos, 60, flag, end=pos + len(seq), cigarOps=[(0, len(seq))], chromID=tid, mateChromID=mtid, insertSize=0, matePos=mpos)
    rec = synth.bam_record(r, name=name, aux=b"RGZ" + rg + b"\0" if rg else b"")
    return struct.pack("<i", len(rec)) + rec


def _read_order(rec):
    """(tid, the position the decoder gives the read: the record's, moved back over a leading soft clip) -- the order the caller asks of a fetch."""
    tid, pos = struct.unpack_from("<ii", rec, 4)
    first = struct.unpack_from("<I", rec, 36 + rec[12])[0] if struct.unpack_from("<H", rec, 16)[0] else 0
    return tid, pos - (first >> 4 if first & 15 == 4 else 0)


def long_contig(case):
    rng = np.random.default_rng(20)
    ref = case["ref"].encode()
    return ref + bytes(b"ACGT"[int(v)] for v in rng.integers(0, 4, 200000 - len(ref)))


def mates_input(layout, poison=False):
    """A built file over a committed case ("one": one sample; "merged": two samples by RG) with improper pairs and their mates;
    dict(file, case, samples, groups, regions [(chrom, start, end, contig)]).  poison: one more improper read whose mate position is -1."""
    cases = B.fetched_cases()
    head = "@HD\tVN:1.4\tSO:coordinate\n" + B.sq_lines(REFS)
    if layout == "one":
        case = cases[B.ONE_SAMPLE_CASE]
        rgs, groups = [("g1", "S1")], None
        recs = B.case_records(case["regions"][0]["samples"][0]["fetched"])
        tag = lambda i: None
    else:
        case = cases[B.TWO_SAMPLE_CASE]
        s = case["regions"][0]["samples"]
        rgs, groups = [("g1", "S1"), ("g2", "S2")], [(b"g1", 0), (b"g2", 1)]
        reads, aux = F.merge_by_read_group([(0, b"g1", s[0]["fetched"]), (1, b"g2", s[1]["fetched"])], lambda x: x["pos"])
        recs = [r for x, a in zip(reads, aux) for r in B.case_records([x], rg=a[3:-1])]
        tag = lambda i: (b"g1", b"g2")[i % 2]
    r = case["regions"][0]
    start, end = r["start"], r["end"]
    contig = long_contig(case)
    at = lambda p, n=40: contig[p:p + n]
    # the improper pairs of the region: (flag, mtid, mpos)
    pairs = [(0x41, T20, 150000), (0x41, T20, 150300), (0x41, T21, 7000), (0x49, -1, -1), (0x41, T20, start + 200), (0x07, T20, 180000),
             (0x43, T20, 170000), (0x41, 0, 100)]
    if poison:
        pairs.append((0x41, T20, -1))
    for i, (flag, mtid, mpos) in enumerate(pairs):
        p = start + 60 + 90 * i
        recs.append(_read(T20, p, flag, mtid, mpos, at(p), b"imp%d\0" % i, tag(i)))
    # their mates: (tid, pos, mtid, mpos) -- kept, or dropped by the filter's edges, the contig, or because no query reaches them
    mates = [(T20, 150000, T20, start), (T20, 150010, T20, start - 1), (T20, 150300, T20, end), (T20, 150310, T20, end + 1), (T20, 150320, T21, start + 5),
             (T20, 170000, T20, start + 100), (T20, 180000, T20, start + 400), (T21, 7000, T20, start + 400), (T21, 7030, T20, start + 10)]
    for i, (tid, pos, mtid, mpos) in enumerate(mates):
        recs.append(_read(tid, pos, 0x81, mtid, mpos, at(min(max(mpos, 0), 4000)), b"mate%d\0" % i, tag(i + 1)))
    recs.sort(key=_read_order)                                               # (stable: the case's reads keep their order)
    f = B.built(dict(name=layout + "_mates.bam", text=head + "".join("@RG\tID:%s\tSM:%s\n" % g for g in rgs), refs=REFS, records=recs))
    regions = [(r["chrom"], start, end, contig), ("21", 6900, 7100, B.other_contig_seq(8000))]
    return dict(file=f, case=case, samples=sorted(case["sample_names"]), groups=groups, regions=regions)


def by_hand(nc, v, opts, regions=None, dropped=()):
    """plat_call_bgzf_regions / _rg on the chunks the test cut and the broken mates the restatement gives."""
    f, out = v["file"], []
    for k, (chrom, start, end, contig) in enumerate(regions or v["regions"]):
        ft = B.fetch(f, chrom, start, end)
        mates = [] if k in dropped else restate(f, chrom, start, end)[2]
        if v["groups"] is None:
            out.append(F.BgzfRegion(chrom, start, end, contig, ft["tid"], ft["itr_beg"], ft["itr_end"], [(ft["cut"], _records(mates))]))
        else:
            out.append(F.BgzfFileRegion(chrom, start, end, contig, ft["tid"], ft["itr_beg"], ft["itr_end"], [(ft["cut"], _records(mates, True))]))
    if v["groups"] is None:
        return nc.call_bgzf_regions(out, v["samples"], opts)
    return nc.call_bgzf_regions_rg(out, v["groups"], v["samples"], opts)


@pytest.fixture(scope="module")
def inputs():
    return {layout: mates_input(layout) for layout in ("one", "merged")}


@pytest.mark.parametrize("layout", ["one", "merged"])
def test_plan_and_call_equal_the_restatement(inputs, layout):
    """(a) a pre-split file and (b) a merged file with two samples by RG: the plan's queries and records are the restatement's, the call's
    text is the text of the BGZF call handed the same chunks and those mates; (e) and it differs from the text without the mates."""
    v = inputs[layout]
    f, case = v["file"], v["case"]
    chrom, start, end, _ = v["regions"][0]
    n_coords, queries, mates = restate(f, chrom, start, end)
    # what the input was built to hold: far on the same contig (merged into one query, and one alone), the other contigs, the region itself
    assert {(0, 100, 101), (T20, 150000, 150301), (T20, 180000, 180001), (T21, 7000, 7001)} <= set(queries) and n_coords >= 6
    names = {r[32:r.index(b"\0", 32)] for r in mates}
    assert {b"mate0", b"mate2", b"mate6", b"mate7", b"imp4"} <= names                # the filter's edges, the far query, the other contig, the region itself
    assert not {b"mate1", b"mate3", b"mate4", b"mate5", b"mate8"} & names           # start - 1, end + 1, another contig, and where no query reaches
    mpos = [struct.unpack_from("<i", r, 24)[0] for r in mates]
    assert mpos == sorted(mpos) and mpos[0] == start and mpos[-1] == end and len(set(mpos)) < len(mpos)
    nc = F.NativeCaller(0, 2, 2)
    try:
        h = nc.open_bam(f["bam"], f["bai"], f["name"])
        opts = dict(case["options"], **BOTH)
        plan = nc.bam_mates_plan([h], [r[:3] for r in v["regions"]], default_options(**opts))
        info = nc.bam_mates_info
        total = [0, 0, 0]
        for (c, s, e, _), per in zip(v["regions"], plan):
            want = restate(f, c, s, e)
            assert (per[0]["n_coords"], per[0]["queries"]) == want[:2], (c, s, e)
            assert per[0]["records"] == want[2], (c, s, e)
            total = [total[0] + want[0], total[1] + len(want[1]), total[2] + len(want[2])]
        assert [info["coords"], info["queries"], info["records_kept"]] == total and info["loaded"] == [1, 1]
        assert info["chunks"] > 0 and info["input_bytes"] > 0 and info["records_looked_at"] >= info["records_kept"] and info["device_calls"] >= 3 + 3
        regions = [F.BamFilesRegion(c, s, e, contig) for c, s, e, contig in v["regions"]]
        got = nc.call_bam_files_mates([h], regions, default_options(**opts))
        got_state = (list(nc.loaded), nc.read_counts.copy(), nc.stats["input_bytes"])
        want = by_hand(nc, v, default_options(**opts))
        assert got == want and got_state[0] == list(nc.loaded) == [1, 1] and np.array_equal(got_state[1], nc.read_counts)
        assert got_state[2] == nc.stats["input_bytes"] + info["input_bytes"]  # (the second round's compressed bytes)
        assert len(got.split("\n")) > 2
        # (e) the mates reach the assembler and the likelihoods: without them the text is another
        without = nc.call_bam_files_mates([h], regions, default_options(**dict(opts, assembleBrokenPairs=0)))
        assert without != got and without == by_hand(nc, dict(v, file=dict(f, records=[], placed=[])), default_options(**dict(opts, assembleBrokenPairs=0)))
        h.close()
    finally:
        nc.close()


def test_options_off_is_call_bam_files_with_the_same_launches(inputs):
    """(d) with either option 0: the text of plat_call_bam_files and the same launches in every timer."""
    v = inputs["one"]
    f = v["file"]
    regions = [F.BamFilesRegion(c, s, e, contig) for c, s, e, contig in v["regions"]]
    nc = F.NativeCaller(0, 1, 2)
    try:
        h = nc.open_bam(f["bam"], f["bai"], f["name"])
        nc.time_kernel(KT_OTHER)
        for off in (dict(), dict(assemble=1), dict(assembleBrokenPairs=1)):
            opts = dict(v["case"]["options"], **off)
            a = nc.call_bam_files([h], regions, default_options(**opts))
            la = list(nc.stats["kernel_launches"])
            b = nc.call_bam_files_mates([h], regions, default_options(**opts))
            lb = list(nc.stats["kernel_launches"])
            assert a == b and la == lb and nc.stats["input_bytes"] > 0, off
        h.close()
    finally:
        nc.close()


def _seam_file():
    """(c) one region whose improper pairs point at: two positions 9999 apart behind a query's end (one query) and two 10000 apart (two);
    a chain that the 100000 span cap ends five bases in front of the next coordinate, with one record lying across both queries' windows."""
    refs = [("chrA", 400000), ("chrB", 30000)]
    seq = b"ACGTTGCA" * 5
    targets = [20000, 20000 + 1 + 9999, 50000, 50000 + 1 + 10000] + list(range(100000, 191000, 9000)) + [199000, 199995, 200000]
    recs = [_read(0, 1000 + 10 * i, 0x41, 0, t, seq, b"i%d\0" % i) for i, t in enumerate(targets)]
    there = [20000, 30000, 50000, 60001, 100000, 145000, 199980, 200000]
    recs += [_read(0, p, 0x81, 0, 1000 + 7 * i, seq, b"m%d\0" % i) for i, p in enumerate(there)]
    recs.sort(key=lambda x: B.record_span(x)[:2])
    text = "@HD\tVN:1.4\n" + B.sq_lines(refs) + "@RG\tID:g\tSM:S\n"
    return B.built(dict(name="seams.bam", text=text, refs=refs, records=recs))


def test_merge_seams_and_a_record_returned_by_two_queries():
    f = _seam_file()
    n_coords, queries, mates = restate(f, "chrA", 900, 2000)
    assert queries == [(0, 20000, 30001), (0, 50000, 50001), (0, 60001, 60002), (0, 100000, 199996), (0, 200000, 200001)]
    names = [r[32:r.index(b"\0", 32)] for r in mates]
    assert names.count(b"m6") == 2 and len(mates) == 9                        # the record at 199980 lies in both windows: appended twice
    nc = F.NativeCaller(0, 1, 1)
    try:
        h = nc.open_bam(f["bam"], f["bai"], f["name"])
        plan = nc.bam_mates_plan([h], [("chrA", 900, 2000), ("chrB", 1, 500)], default_options(**BOTH))
        assert (plan[0][0]["n_coords"], plan[0][0]["queries"], plan[0][0]["records"]) == (n_coords, queries, mates)
        assert plan[1][0] == dict(n_coords=0, queries=[], records=[]) and nc.bam_mates_info["queries"] == 5 and nc.bam_mates_info["records_kept"] == 9
        h.close()
    finally:
        nc.close()


def test_a_negative_mate_position_is_refused_by_name_and_the_next_call_succeeds():
    """(f) mpos = -1 with mtid >= 0."""
    v = mates_input("one", poison=True)
    f = v["file"]
    regions = [F.BamFilesRegion(c, s, e, contig) for c, s, e, contig in v["regions"]]
    nc = F.NativeCaller(0, 1, 2)
    try:
        h = nc.open_bam(f["bam"], f["bai"], f["name"])
        opts = dict(v["case"]["options"], **BOTH)
        for _ in range(2):
            with pytest.raises(_lib.PlatypusDeviceError) as e:
                nc.call_bam_files_mates([h], regions, default_options(**opts))
            said = str(e.value)
            assert e.value.code == -9 and "region 0 (20:" in said and "file 0" in said and "mate position -1" in said and "record" in said
        with pytest.raises(_lib.PlatypusDeviceError) as e:
            nc.bam_mates_plan([h], [r[:3] for r in v["regions"]], default_options(**opts))
        assert e.value.code == -9 and "mate position -1" in str(e.value)
        # the region that does not hold the record, and the whole list without the mates
        plan = nc.bam_mates_plan([h], [v["regions"][1][:3]], default_options(**opts))
        assert plan[0][0]["queries"] == restate(f, *v["regions"][1][:3])[1]
        got = nc.call_bam_files_mates([h], regions[1:], default_options(**opts))
        assert got == by_hand(nc, v, default_options(**opts), regions=v["regions"][1:])
        assert nc.call_bam_files_mates([h], regions, default_options(**dict(opts, assembleBrokenPairs=0))) == nc.call_bam_files([h], regions, default_options(**dict(opts, assembleBrokenPairs=0)))
        h.close()
    finally:
        nc.close()


def test_a_region_at_maxReads_is_dropped_before_any_mate_is_fetched(inputs):
    """(g) three regions, the first at maxReads: it is dropped, has no second round in the plan, and the others are what they were."""
    v = inputs["one"]
    f = v["file"]
    chrom, start, end, contig = v["regions"][0]
    three = [v["regions"][0], ("20", 149900, 150400, contig), v["regions"][1]]
    counts = [len(fetched(f, c, s, e)) for c, s, e, _ in three]
    assert counts[0] > counts[1] == 5 and counts[2] == 2
    nc = F.NativeCaller(0, 1, 2)
    try:
        h = nc.open_bam(f["bam"], f["bai"], f["name"])
        opts = dict(v["case"]["options"], maxReads=counts[0], **BOTH)
        plan = nc.bam_mates_plan([h], [r[:3] for r in three], default_options(**opts))
        info = nc.bam_mates_info
        assert info["loaded"] == [0, 1, 1] and plan[0][0] == dict(n_coords=0, queries=[], records=[])
        want = [restate(f, c, s, e) for c, s, e, _ in three[1:]]
        assert [(p[0]["n_coords"], p[0]["queries"], p[0]["records"]) for p in plan[1:]] == want
        assert info["queries"] == sum(len(w[1]) for w in want) > 0 and info["coords"] == sum(w[0] for w in want)
        regions = [F.BamFilesRegion(c, s, e, cg) for c, s, e, cg in three]
        got = nc.call_bam_files_mates([h], regions, default_options(**opts))
        assert nc.loaded == [0, 1, 1]
        assert got == by_hand(nc, v, default_options(**opts), regions=three, dropped=(0,)) and nc.loaded == [0, 1, 1]
        # one read more allowed: the region is back, with its mates
        opts["maxReads"] = counts[0] + 1
        assert nc.bam_mates_plan([h], [r[:3] for r in three], default_options(**opts))[0][0]["queries"] == restate(f, chrom, start, end)[1]
        assert nc.bam_mates_info["loaded"] == [1, 1, 1]
        h.close()
    finally:
        nc.close()


def test_command_line_with_both_options_writes_records_with_the_mates(inputs, tmp_path):
    """--bamFiles with --refFile, --assemble 1 and --assembleBrokenPairs 1 goes to plat_call_bam_files_mates: the records of the call."""
    import os
    import subprocess
    import sys
    from tests.fasta_cases import write_region_fasta
    v = inputs["one"]
    f = v["file"]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = str(tmp_path / f["name"])
    with open(path, "wb") as out:
        out.write(f["bam"])
    with open(path + ".bai", "wb") as out:
        out.write(f["bai"])
    ref = str(tmp_path / "ref.fa")
    write_region_fasta(ref, {"20": v["regions"][0][3], "21": v["regions"][1][3]}, 60)
    chrom, start, end, contig = v["regions"][0]
    opts = dict(v["case"]["options"], **BOTH)
    nc = F.NativeCaller(0, 2, 2)
    try:
        h = nc.open_bam(f["bam"], f["bai"], f["name"])
        want = nc.call_bam_files_mates([h], [F.BamFilesRegion(chrom, start, end, contig)], default_options(**opts))
        h.close()
    finally:
        nc.close()
    out = str(tmp_path / "out.vcf")
    cmd = [sys.executable, "-m", "platypus_amd", "callVariants", "--bamFiles", path, "--refFile", ref, "--regions", "%s:%d-%d" % (chrom, start + 1, end), "-o", out]
    cmd += [x for k, val in opts.items() for x in ("--" + k, str(val))]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=root)
    assert r.returncode == 0, r.stderr[-3000:]
    with open(out) as fh:
        lines = [ln for ln in fh.read().split("\n")[:-1] if not ln.startswith("#")]
    assert lines == want.split("\n")[:-1] and len(lines) >= 2
