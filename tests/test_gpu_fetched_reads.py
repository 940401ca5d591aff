"""GPU tests of the read buffers built from fetched reads: plat_read_buffers_batch (checkAndTrimRead + the stable split of every stream,
cwindow.pyx:332-481,560-595) against the reference's verdicts, and plat_call_fetched_regions (the region loop fed with the reads a BAM fetch
returns) against the reference's record text for the same fetches (tests/golden/region_fetched_cases.json.gz)."""
import copy
import gzip
import json
import os

import numpy as np
import pytest

from platypus_amd import _lib, fastcaller as F, hostapi as H, synth
from platypus_amd.options import default_options

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _qc_cases():
    with gzip.open(os.path.join(HERE, "golden", "readqc_cases.json.gz"), "rt") as f:
        return json.load(f)


def _qc_args(o):
    return (o["minGoodQualBases"], o["minMapQual"], o["minBaseQual"], o["trimOverlapping"], o["trimAdapter"], o["trimReadFlank"],
            o["trimSoftClipped"], o["enabled"])


def _with_end(reads):
    return [dict(r, end=r["pos"] + len(r["qual"])) for r in reads]


def _check_split(res, reads):
    """The split and the gathered buffers of one stream, from its own verdicts: accepted in order, then rejected in order."""
    ok = res["ok"].astype(bool)
    n = len(reads)
    assert list(res["perm"]) == [i for i in range(n) if ok[i]] + [i for i in range(n) if not ok[i]]
    assert res["n_good"] == int(ok.sum())
    assert list(res["hist"]) == [int((res["reason"] == k).sum()) for k in range(8)]
    assert res["unsorted"] == int(any(reads[i]["pos"] < reads[i - 1]["pos"] for i in range(1, n)))
    quals = res["quals"]
    for name, idx in (("reads", [i for i in range(n) if ok[i]]), ("bad", [i for i in range(n) if not ok[i]])):
        t = res[name]
        assert len(t["pos"]) == len(idx)
        assert list(np.diff(t["off"])) == [len(reads[i]["qual"]) for i in idx]
        assert list(np.diff(t["cig_off"])) == [len(reads[i]["cigar"]) for i in idx]
        assert list(t["pos"]) == [reads[i]["pos"] for i in idx] and list(t["end"]) == [reads[i]["end"] for i in idx]
        assert list(t["mapq"]) == [reads[i]["mapq"] for i in idx] and list(t["mate_pos"]) == [reads[i]["matePos"] for i in idx]
        assert list(t["flags"]) == [int(res["flags"][i]) for i in idx]
        assert t["seq"].tobytes() == b"".join(reads[i]["seq"].encode() for i in idx)
        assert t["qual"].tobytes() == b"".join(bytes(quals[i]) for i in idx)
        assert t["cigar"].tolist() == [list(c) for i in idx for c in reads[i]["cigar"]]


def test_read_buffers_match_reference_qc_and_split(golden_dir):
    """All 30 streams of readqc_cases.json.gz: the reference's verdicts, QCFail flags, trimmed qualities and per-type counts, and the split
    "accepted in order, then rejected in order" with the buffers gathered on the device."""
    eng = H.get_engine()
    trimmed = 0
    for c in _qc_cases():
        reads = _with_end(c["reads"])
        res = eng.read_buffers([reads], *_qc_args(c["options"]))[0]
        assert [int(x) for x in res["ok"]] == c["ok"]
        assert [int(x) for x in res["flags"]] == c["flag_out"]
        # trimmed qualities, per read in fetch order (from the gathered buffers through the permutation)
        quals = [None] * len(reads)
        for name, first in (("reads", 0), ("bad", res["n_good"])):
            t = res[name]
            for q in range(len(t["pos"])):
                quals[int(res["perm"][first + q])] = t["qual"][t["off"][q]:t["off"][q + 1]].tolist()
        for got, src, exp in zip(quals, c["reads"], c["qual_out"]):
            assert got == (src["qual"] if exp is None else exp)
            trimmed += exp is not None
        res["quals"] = quals
        _check_split(res, reads)
        for k in range(7):                                   # filteredReadCountsByType (-1: the filter is off, nothing counted)
            assert res["hist"][k] == max(c["counts"][k], 0)
        assert int(res["hist"].sum()) == len(reads) - res["n_good"]
    assert trimmed > 500


def test_read_buffers_many_streams_and_long_streams():
    """Streams of several tiles (thousands of reads), empty streams and an unsorted stream in one call: the same verdicts as one stream per
    call, the split from those verdicts, and the unsorted flag where a position goes down."""
    eng = H.get_engine()
    cases = _qc_cases()
    o = cases[0]["options"]
    streams = [_with_end(c["reads"]) for c in cases[:12]]
    long = [r for st in streams for r in st]                          # ~2 500 reads, positions restart at every case: unsorted
    long_sorted = sorted(copy.deepcopy(long), key=lambda r: r["pos"])
    batch = [streams[3], [], long, streams[5], long_sorted, []]
    got = eng.read_buffers(batch, *_qc_args(o))
    for st, res in zip(batch, got):
        one = eng.read_buffers([st], *_qc_args(o))[0] if st else None
        if not st:
            assert res["n_good"] == 0 and res["unsorted"] == 0 and not res["hist"].any() and len(res["perm"]) == 0
            continue
        assert np.array_equal(res["ok"], one["ok"]) and np.array_equal(res["flags"], one["flags"]) and np.array_equal(res["reason"], one["reason"])
        quals = [None] * len(st)
        for name, first in (("reads", 0), ("bad", res["n_good"])):
            t = res[name]
            for q in range(len(t["pos"])):
                quals[int(res["perm"][first + q])] = t["qual"][t["off"][q]:t["off"][q + 1]].tolist()
        res["quals"] = quals
        _check_split(res, st)
    assert got[2]["unsorted"] == 1 and got[4]["unsorted"] == 0 and got[0]["unsorted"] == 0
    assert len(long) > 4 * 512


def _fetched_reads(lst):
    return [H.AlignedRead(x["seq"].encode(), bytes(ord(c) - 33 for c in x["qual"]), x["pos"], x["mapq"], x["flag"], end=x["end"],
                          cigarOps=[tuple(c) for c in x["cigar"]], chromID=x["chromID"], mateChromID=x["mateChromID"], insertSize=x["insertSize"],
                          matePos=x["matePos"]) for x in lst]


def _fetched_cases():
    with gzip.open(os.path.join(HERE, "golden", "region_fetched_cases.json.gz"), "rt") as f:
        return json.load(f)


def test_fetched_region_loop_matches_reference_text():
    """The 41 region cases from the reads the reference's loader was handed: the same 245 record lines, rlen after the call, the regions
    the loader gave up on (maxReads) skipped, and per sample the sizes of `reads` / `badReads` addReadToBuffer built."""
    cases = _fetched_cases()
    assert len(cases) == 41
    with gzip.open(os.path.join(HERE, "golden", "region_cases.json.gz"), "rt") as f:
        after = json.load(f)
    from tests.region_golden import _reads
    nc = F.NativeCaller(0, 2, 2)
    n_lines = n_skipped = 0
    try:
        for ci, (case, ref) in enumerate(zip(cases, after)):
            fasta = H.FastaFile({"20": case["ref"].encode()})
            # broken mates are handed over sorted by mate position (the reference's sortBrokenMates is a qsort: its order of equal keys is
            # taken from what it left)
            regs = [F.FetchedRegion.from_reads(r["chrom"], r["start"], r["end"], fasta,
                                               [(_fetched_reads(s["fetched"]), _reads(rr["samples"][i]["brokenMates"]) if rr["loaded"] else [])
                                                for i, s in enumerate(r["samples"])])
                    for r, rr in zip(case["regions"], ref["regions"])]
            opts = default_options(**case["options"])
            txt = nc.call_fetched_regions(regs, case["sample_names"], opts)
            lines = txt.split("\n")[:-1]
            assert lines == case["lines"], "case %d: %d lines, want %d" % (ci, len(lines), len(case["lines"]))
            assert opts.rlen == case["rlen_after"], ci
            assert nc.loaded == [int(r["loaded"]) for r in case["regions"]], ci
            for k, r in enumerate(case["regions"]):
                if not r["loaded"]:
                    n_skipped += 1
                    continue
                for i, s in enumerate(r["samples"]):
                    assert list(nc.read_counts[k][i][:2]) == [s["n_reads"], s["n_bad"]], (ci, k, i)
                    assert int(nc.read_counts[k][i][2:].sum()) == s["n_bad"]
            lens = nc.region_text_lengths(len(regs))
            assert int(lens.sum()) == len(txt) and all(ln == 0 for ln, r in zip(lens, case["regions"]) if not r["loaded"])
            n_lines += len(lines)
    finally:
        nc.close()
    assert n_lines == 245 and n_skipped >= 1


def test_python_mirror_builds_the_reference_buffers():
    """hostapi.bamReadBuffer.fromFetchedReads gives the buffers the reference's loader left (region_cases.json.gz) for the same fetches."""
    with gzip.open(os.path.join(HERE, "golden", "region_cases.json.gz"), "rt") as f:
        after = json.load(f)
    for case, ref in zip(_fetched_cases(), after):
        opts = default_options(**case["options"])
        for r, rr in zip(case["regions"], ref["regions"]):
            before, bufs = 0, []
            for s in r["samples"]:
                b = H.bamReadBuffer.fromFetchedReads(_fetched_reads(s["fetched"]), _fetched_reads(s["brokenMates"]), opts, s["sample"], before)
                before += len(s["fetched"])
                bufs.append(b)
                if b is None:
                    break
            assert (None not in bufs) == rr["loaded"]
            if not rr["loaded"]:
                continue
            for b, s in zip(bufs, rr["samples"]):
                for mine, theirs in ((b.reads.array, s["reads"]), (b.badReads.array, s["badReads"])):
                    assert [(x.pos, x.bitFlag, x.qual) for x in mine] == [(y["pos"], y["flag"], bytes(ord(c) - 33 for c in y["qual"])) for y in theirs]


def test_fetched_call_equals_call_on_buffers_split_by_checkAndTrimReads():
    """Synthetic config-4 regions with the loader's trouble injected: the fetched call's text equals call_regions on buffers split on the host
    side by hostapi.checkAndTrimReads."""
    opts = default_options()
    enabled = (opts.filterReadsWithUnmappedMates, opts.filterReadsWithDistantMates, opts.filterReadPairsWithSmallInserts, opts.filterDuplicates)
    fetched, split, names = [], [], None
    for idx, nS in ((0, 1), (1, 2), (2, 1)):
        reg, samples = synth.config4_fetched_region(idx, region_len=20000, n_samples=nS)
        names = names or ["S%d" % (i + 1) for i in range(nS)]
        fasta = H.FastaFile({reg["chrom"]: reg["ref"].tobytes()})
        fetched.append((nS, F.FetchedRegion.from_reads(reg["chrom"], reg["start"], reg["end"], fasta, [(rs, []) for rs in samples])))
        bufs = []
        for rs in samples:
            rs = copy.deepcopy(rs)
            ok, _ = H.checkAndTrimReads(rs, opts, enabled)
            assert 0 < sum(ok) < len(rs)
            bufs.append(H.bamReadBuffer([r for r, g in zip(rs, ok) if g], [r for r, g in zip(rs, ok) if not g], []))
        split.append((nS, F.RegionReads.from_buffers(reg["chrom"], reg["start"], reg["end"], fasta, bufs)))
    nc = F.NativeCaller(0, 2, 2)
    try:
        for nS in (1, 2):
            f = [r for n, r in fetched if n == nS]
            s = [r for n, r in split if n == nS]
            nm = ["S%d" % (i + 1) for i in range(nS)]
            o1, o2 = default_options(), default_options()
            want = nc.call_regions(s, nm, o1)
            got = nc.call_fetched_regions(f, nm, o2)
            assert got == want and o1.rlen == o2.rlen
            assert want.count("\n") > 5
    finally:
        nc.close()


def test_unsorted_fetch_is_refused_and_the_caller_stays_usable():
    ref = b"ACGTTGCA" * 100
    fasta = H.FastaFile({"20": ref})

    def region(order):
        reads = [H.AlignedRead(ref[p:p + 60], bytes([30] * 60), p, bitFlag=3) for p in order]
        return F.FetchedRegion.from_reads("20", 100, 500, fasta, [(reads, [])])
    nc = F.NativeCaller(0, 1, 2)
    try:
        with pytest.raises(_lib.PlatypusDeviceError) as e:
            nc.call_fetched_regions([region([100, 140, 180]), region([200, 150, 250])], ["S1"], default_options())
        assert e.value.code == -9 and "not sorted" in str(e.value) and "region 1" in str(e.value)
        nc.call_fetched_regions([region([100, 140, 180, 200, 220])], ["S1"], default_options())
        assert nc.loaded == [1] and list(nc.read_counts[0][0][:2]) == [5, 0]
    finally:
        nc.close()
