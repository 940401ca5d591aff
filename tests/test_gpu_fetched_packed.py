"""GPU tests of the fetched-reads region loop on PLAT_READS_PACKED input: plat_read_buffers_packed_batch (checkAndTrimRead on the packed
bytes and exceptions, then the split and the gather of the packed bytes) against the reference's verdicts and against the ASCII path on
the same reads, and plat_call_fetched_regions on packed fetched tables against the committed record text.  The committed fixtures hold no
exceptions (bases A/C/G/T, qualities 0-60): the tests inject bases other than A/C/G/T and qualities above 63 and compare with the ASCII
device path, which the other fetched tests pin to the reference."""
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


def _load(name):
    with gzip.open(os.path.join(HERE, "golden", name), "rt") as f:
        return json.load(f)


def _qc_args(o):
    return (o["minGoodQualBases"], o["minMapQual"], o["minBaseQual"], o["trimOverlapping"], o["trimAdapter"], o["trimReadFlank"],
            o["trimSoftClipped"], o["enabled"])


def _with_end(reads):
    return [dict(r, end=r["pos"] + len(r["qual"])) for r in reads]


def _quals_in_fetch_order(res, n):
    quals = [None] * n
    for name, first in (("reads", 0), ("bad", res["n_good"])):
        t = res[name]
        for q in range(len(t["pos"])):
            quals[int(res["perm"][first + q])] = t["qual"][t["off"][q]:t["off"][q + 1]].tolist()
    return quals


def _inject(reads, rng, trimmed=None):
    """Exceptions in a stream of read dicts (seq str, qual list): N bases, qualities 64-127 and >= 128, at the first and last byte of
    reads, inside the stretches the reference trims (`trimmed`: per read the trimmed qualities or None) and elsewhere.  Returns the
    number of bytes changed."""
    changed = 0
    for k, r in enumerate(reads):
        seq, qual = list(r["seq"]), list(r["qual"])
        n = len(qual)
        if not n:
            continue
        spots = []
        if rng.random() < 0.3:
            spots.append(0)
        if rng.random() < 0.3:
            spots.append(n - 1)
        if trimmed is not None and trimmed[k] is not None:
            cut = [i for i in range(n) if trimmed[k][i] == 0 and qual[i] != 0]
            if cut:
                spots += [cut[0], cut[-1], cut[len(cut) // 2]]
        if rng.random() < 0.3:
            spots += list(rng.integers(0, n, size=3))
        for i in spots:
            i = int(i)
            kind = rng.integers(0, 4)
            if kind == 0:
                seq[i] = "N"
            elif kind == 1:
                qual[i] = int(rng.integers(64, 128))
            elif kind == 2:
                qual[i] = int(rng.integers(128, 256))
            else:
                seq[i], qual[i] = "N", int(rng.integers(64, 256))
            changed += 1
        r["seq"], r["qual"] = "".join(seq), qual
    return changed


def _same_buffers(a, b):
    """Two read_buffers results of one stream (packed, ASCII): the same verdicts, split and buffers, bases and trimmed qualities."""
    for k in ("ok", "reason", "flags", "perm", "hist"):
        assert np.array_equal(a[k], b[k]), k
    assert a["n_good"] == b["n_good"] and a["unsorted"] == b["unsorted"]
    for name in ("reads", "bad"):
        for k in ("off", "cig_off", "seq", "qual", "cigar", "pos", "end", "mapq", "flags", "mate_pos"):
            assert np.array_equal(a[name][k], b[name][k]), (name, k)


def test_packed_read_buffers_match_reference_qc_and_ascii_with_exceptions():
    """All 30 streams of readqc_cases.json.gz, packed: the reference's verdicts, QCFail flags, decoded trimmed qualities and counts.  Then
    the same streams with exceptions injected (inside trimmed stretches, at the first and last byte of reads and of the blob): the packed
    call equals the ASCII call on the same reads, and a trimmed base keeps its base bits."""
    eng = H.get_engine()
    cases = _load("readqc_cases.json.gz")
    assert len(cases) == 30
    rng = np.random.default_rng(2024)
    trimmed = injected = 0
    for c in cases:
        reads = _with_end(c["reads"])
        res = eng.read_buffers([reads], *_qc_args(c["options"]), packed=True)[0]
        assert [int(x) for x in res["ok"]] == c["ok"]
        assert [int(x) for x in res["flags"]] == c["flag_out"]
        for got, src, exp in zip(_quals_in_fetch_order(res, len(reads)), c["reads"], c["qual_out"]):
            assert got == (src["qual"] if exp is None else exp)
            trimmed += exp is not None
        for k in range(7):
            assert res["hist"][k] == max(c["counts"][k], 0)
        assert len(res["exc_qual"]) == 0
        # exceptions
        mine = copy.deepcopy(reads)
        injected += _inject(mine, rng, c["qual_out"])
        if mine and mine[0]["qual"] and mine[-1]["qual"]:          # the blob's first and last byte
            mine[0]["qual"][0] = 200
            mine[-1]["seq"] = mine[-1]["seq"][:-1] + "N"
            mine[-1]["qual"][-1] = 99
        a = eng.read_buffers([mine], *_qc_args(c["options"]), packed=True)[0]
        b = eng.read_buffers([copy.deepcopy(mine)], *_qc_args(c["options"]), packed=False)[0]
        _same_buffers(a, b)
        assert len(a["exc_qual"]) > 0
        for name in ("reads", "bad"):                                 # base bits untouched, exceptions where the letters are not A/C/G/T
            t = a[name]
            assert np.array_equal(np.frombuffer(b"ACTG", np.uint8)[t["packed"] & 3][t["seq"] != ord("N")], t["seq"][t["seq"] != ord("N")])
            assert set(np.nonzero(t["seq"] == ord("N"))[0].tolist()) <= set(t["exc_index"].tolist())
    assert trimmed > 500 and injected > 1000


def test_packed_read_buffers_many_streams_equal_ascii():
    """Empty streams, long streams (several tiles) and an unsorted stream in one packed call, with exceptions: the ASCII call's result."""
    eng = H.get_engine()
    cases = _load("readqc_cases.json.gz")
    o = cases[0]["options"]
    rng = np.random.default_rng(7)
    streams = [_with_end(c["reads"]) for c in cases[:12]]
    long = [r for st in streams for r in st]
    long_sorted = sorted(copy.deepcopy(long), key=lambda r: r["pos"])
    batch = copy.deepcopy([[], streams[3], [], long, streams[5], long_sorted, []])
    for st in batch:
        _inject(st, rng)
    a = eng.read_buffers(batch, *_qc_args(o), packed=True)
    b = eng.read_buffers(copy.deepcopy(batch), *_qc_args(o))
    for x, y in zip(a, b):
        _same_buffers(x, y)
    assert a[3]["unsorted"] == 1 and a[5]["unsorted"] == 0 and a[0]["n_good"] == 0 and len(a[0]["perm"]) == 0


def _fetched_reads(lst):
    return [H.AlignedRead(x["seq"].encode(), bytes(ord(c) - 33 for c in x["qual"]), x["pos"], x["mapq"], x["flag"], end=x["end"],
                          cigarOps=[tuple(c) for c in x["cigar"]], chromID=x["chromID"], mateChromID=x["mateChromID"], insertSize=x["insertSize"],
                          matePos=x["matePos"]) for x in lst]


def test_packed_fetched_region_loop_matches_reference_text():
    """The 41 region cases with packed fetched (and broken-mate) tables: the committed 245 lines, rlen after the call, the regions the
    loader gave up on skipped, and per sample the reference's buffer sizes."""
    cases = _load("region_fetched_cases.json.gz")
    after = _load("region_cases.json.gz")
    assert len(cases) == 41
    from tests.region_golden import _reads
    nc = F.NativeCaller(0, 2, 2)
    n_lines = n_skipped = 0
    try:
        for ci, (case, ref) in enumerate(zip(cases, after)):
            fasta = H.FastaFile({"20": case["ref"].encode()})
            regs = [F.FetchedRegion.from_reads(r["chrom"], r["start"], r["end"], fasta,
                                               [(_fetched_reads(s["fetched"]), _reads(rr["samples"][i]["brokenMates"]) if rr["loaded"] else [])
                                                for i, s in enumerate(r["samples"])], packed=True)
                    for r, rr in zip(case["regions"], ref["regions"])]
            assert all(f.encoding == F.READS_PACKED for g in regs for f, *_ in g.samples)
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
            n_lines += len(lines)
    finally:
        nc.close()
    assert n_lines == 245 and n_skipped >= 1


def _inject_aligned(reads, rng):
    """Exceptions in hostapi.AlignedRead objects: N bases and qualities 64-127 (first, last and inner bytes).  (Qualities >= 128 pass the
    QC as the reference's signed chars, tested above; the window kernels after it refuse bytes above 127 and skip such windows, in either
    encoding, so they would leave these regions without records.)"""
    for r in reads:
        if rng.random() < 0.1:
            seq, qual = bytearray(r.seq), bytearray(r.qual)
            for i in [0, r.rlen - 1] + list(rng.integers(0, r.rlen, size=2)):
                if rng.integers(0, 2) == 0:
                    seq[int(i)] = ord("N")
                else:
                    qual[int(i)] = int(rng.integers(64, 128))
            r.seq, r.qual = bytes(seq), bytes(qual)


def test_packed_fetched_call_equals_ascii_and_pre_split_packed():
    """Synthetic config-4 regions (1 and 3 samples) with the loader's trouble and exceptions injected: the packed fetched call's text equals
    the ASCII fetched call's and plat_call_regions' on the packed tables split beforehand; half the input bytes of the ASCII call."""
    opts = default_options()
    enabled = (opts.filterReadsWithUnmappedMates, opts.filterReadsWithDistantMates, opts.filterReadPairsWithSmallInserts, opts.filterDuplicates)
    rng = np.random.default_rng(99)
    nc = F.NativeCaller(0, 2, 2)
    try:
        for nS, idxs in ((1, (0, 1, 2)), (3, (3, 4))):
            ascii_regs, packed_regs, split = [], [], []
            for idx in idxs:
                reg, samples = synth.config4_fetched_region(idx, region_len=20000, n_samples=nS)
                for rs in samples:
                    _inject_aligned(rs, rng)
                fasta = H.FastaFile({reg["chrom"]: reg["ref"].tobytes()})
                args = (reg["chrom"], reg["start"], reg["end"], fasta, [(rs, []) for rs in samples])
                ascii_regs.append(F.FetchedRegion.from_reads(*args))
                packed_regs.append(F.FetchedRegion.from_reads(*args, packed=True))
                bufs = []
                for rs in samples:
                    rs = copy.deepcopy(rs)
                    ok, _ = H.checkAndTrimReads(rs, opts, enabled)
                    bufs.append(H.bamReadBuffer([r for r, g in zip(rs, ok) if g], [r for r, g in zip(rs, ok) if not g], []))
                split.append(F.RegionReads.from_buffers(reg["chrom"], reg["start"], reg["end"], fasta, bufs, packed=True))
            assert sum(len(f.exc[0]) for g in packed_regs for f, *_ in g.samples) > 100
            nm = ["S%d" % (i + 1) for i in range(nS)]
            o1, o2, o3 = default_options(), default_options(), default_options()
            want = nc.call_regions(split, nm, o1)
            got_ascii = nc.call_fetched_regions(ascii_regs, nm, o2)
            ascii_bytes, ascii_counts = nc.stats["input_bytes"], nc.read_counts.copy()
            got = nc.call_fetched_regions(packed_regs, nm, o3)
            assert got == got_ascii == want and o1.rlen == o2.rlen == o3.rlen
            assert want.count("\n") > 5
            assert np.array_equal(nc.read_counts, ascii_counts)
            bases = sum(int(f.off[-1]) for g in packed_regs for f, *_ in g.samples)
            n_exc = sum(len(f.exc[0]) for g in packed_regs for f, *_ in g.samples)
            assert ascii_bytes == 2 * bases and nc.stats["input_bytes"] == bases + 10 * n_exc
            assert 0.45 < nc.stats["input_bytes"] / ascii_bytes < 0.6
    finally:
        nc.close()


def _tiny(order, ref, mapq=60, packed=True, exc=True):
    reads = []
    for p in order:
        seq, qual = bytearray(ref[p:p + 60]), bytearray([30] * 60)
        if exc:
            seq[0], qual[59], qual[30] = ord("N"), 70, 150
        reads.append(H.AlignedRead(bytes(seq), bytes(qual), p, mapq=mapq, bitFlag=3))
    return reads


def test_packed_edge_cases_and_refusals():
    """Empty streams, a stream with every read rejected, a region at maxReads, an unsorted packed fetch (refused; the caller stays usable)
    and a call that mixes encodings (refused with a message naming the table)."""
    ref = b"ACGTTGCAAGCT" * 100
    fasta = H.FastaFile({"20": ref})

    def region(samples, packed=True, start=100, end=900):
        return F.FetchedRegion.from_reads("20", start, end, fasta, [(s, []) for s in samples], packed=packed)
    good = [100, 130, 160, 200, 240, 300, 310, 350]
    nc = F.NativeCaller(0, 1, 2)
    try:
        sets = [[_tiny(good, ref), []], [[], []], [_tiny(good, ref, mapq=5), _tiny(good[:3], ref)]]     # empty streams, every read rejected
        want = nc.call_fetched_regions([region(s, packed=False) for s in sets], ["S1", "S2"], default_options())
        want_counts = nc.read_counts.copy()
        got = nc.call_fetched_regions([region(s) for s in sets], ["S1", "S2"], default_options())
        assert got == want and np.array_equal(nc.read_counts, want_counts)
        assert list(nc.read_counts[2][0][:2]) == [0, len(good)] and nc.read_counts[2][0][2 + 6] == len(good)
        # a region at maxReads (summed over its samples) is skipped, the next is called
        o1, o2 = default_options(maxReads=8), default_options(maxReads=8)
        sets = [[_tiny(good[:5], ref), _tiny(good[:3], ref)], [_tiny(good[:4], ref), _tiny(good[:3], ref)]]
        want = nc.call_fetched_regions([region(s, packed=False) for s in sets], ["S1", "S2"], o1)
        got = nc.call_fetched_regions([region(s) for s in sets], ["S1", "S2"], o2)
        assert nc.loaded == [0, 1] and got == want and o1.rlen == o2.rlen
        assert nc.region_text_lengths(2)[0] == 0
        # unsorted: refused, then the caller still works
        with pytest.raises(_lib.PlatypusDeviceError) as e:
            nc.call_fetched_regions([region([_tiny(good, ref)]), region([_tiny([200, 150, 250], ref)])], ["S1"], default_options())
        assert e.value.code == -9 and "not sorted" in str(e.value) and "region 1" in str(e.value)
        nc.call_fetched_regions([region([_tiny(good, ref)])], ["S1"], default_options())
        assert nc.loaded == [1] and list(nc.read_counts[0][0][:2]) == [len(good), 0]
        # mixed encodings: refused with the table named, then the caller still works
        with pytest.raises(_lib.PlatypusDeviceError) as e:
            nc.call_fetched_regions([region([_tiny(good, ref)]), region([_tiny(good, ref)], packed=False)], ["S1"], default_options())
        msg = str(e.value)
        assert e.value.code == -6 and "region 1" in msg and "PLAT_READS_ASCII" in msg and "PLAT_READS_PACKED" in msg
        # an empty ASCII table next to packed ones is no mix
        nc.call_fetched_regions([region([_tiny(good, ref)]), region([[]], packed=False)], ["S1"], default_options())
        assert nc.loaded == [1, 1]
    finally:
        nc.close()
