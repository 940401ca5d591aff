"""GPU tests of whole BAM files in (include/platypus_caller_bamfile.h): plat_call_bam_files over files written in memory
(tests/bam_file_cases.py) gives the golden record lines of the committed cases whose reads the files hold, and byte for byte the text of
plat_call_bgzf_regions / plat_call_bgzf_regions_rg handed the windows and chunks the TEST cut on the host from the same files
(tabixindex's BAI rule, the cut by BSIZE, the window rule restated in bam_file_cases.window); the fetch plan with the index queries
answered on the device; and the command line from files on disk to a VCF with its header.

The broken-mate fetch (assemble=1 with assembleBrokenPairs=1) is refused by the entry point and not tested here."""
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

from platypus_amd import _lib, fastcaller as F
from platypus_amd.options import default_options
from tests import bam_file_cases as B

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_RECORDS = (np.zeros(0, dtype=np.uint8), np.zeros(0, dtype=np.int64))
NO_FILE_RECORDS = NO_RECORDS + (np.zeros(0, dtype=np.int32),)
# the tables the integrator would have made from the @RG lines of the layouts of bam_file_cases.vcf_files
GROUPS = dict(merged=[(b"g1", 0), (b"g2", 1)], split=[(b"ga", 0), (b"gb", 0)])
SAMPLE_FILE = dict(one=[0], two=[1, 0])                                      # ("two" lists S2's file first)


def _by_hand(nc, layout, v, opts):
    """The existing entry point on what the test cut from the files itself."""
    regions = []
    for chrom, start, end, contig in v["regions"]:
        fetches = [B.fetch(f, chrom, start, end) for f in v["files"]]
        tid, beg, stop = fetches[0]["tid"], fetches[0]["itr_beg"], fetches[0]["itr_end"]
        assert all(ft["tid"] == tid for ft in fetches) and tid >= 0
        if layout in SAMPLE_FILE:
            regions.append(F.BgzfRegion(chrom, start, end, contig, tid, beg, stop, [(fetches[f]["cut"], NO_RECORDS) for f in SAMPLE_FILE[layout]]))
        else:
            regions.append(F.BgzfFileRegion(chrom, start, end, contig, tid, beg, stop, [(ft["cut"], NO_FILE_RECORDS) for ft in fetches]))
    if layout in SAMPLE_FILE:
        return nc.call_bgzf_regions(regions, v["samples"], opts)
    return nc.call_bgzf_regions_rg(regions, GROUPS[layout], v["samples"], opts)


@pytest.mark.parametrize("layout", ["one", "two", "merged", "split"])
def test_call_bam_files_gives_the_golden_lines_and_the_text_of_the_call_on_hand_cut_chunks(layout):
    """Three regions: the case's own with its reads, an empty one behind it, and one on the next contig whose reads copy the reference.
    "one" / "two": one stream per sample (one file; two files with one sample each); "merged" / "split": the split by read group (two
    samples in one file; one sample over two files)."""
    v = B.vcf_files(layout)
    case = v["case"]
    nc = F.NativeCaller(0, 2, 2)
    try:
        files = [nc.open_bam(f["bam"], f["bai"], f["name"]) for f in v["files"]]
        plan = nc.bam_plan(files)
        assert plan["mode"] == ("presplit" if layout in SAMPLE_FILE else "merged") and plan["samples"] == [s.encode() for s in v["samples"]]
        assert plan["sample_file"] == SAMPLE_FILE.get(layout) and plan["read_groups"] == GROUPS.get(layout, [])
        regions = [F.BamFilesRegion(c, s, e, contig) for c, s, e, contig in v["regions"]]
        o1, o2 = default_options(**case["options"]), default_options(**case["options"])
        got = nc.call_bam_files(files, regions, o1)
        got_state = (list(nc.loaded), nc.read_counts.copy(), nc.region_text_lengths(3).copy(), nc.stats["input_bytes"], o1.rlen)
        assert nc.sample_names == v["samples"]
        want = _by_hand(nc, layout, v, o2)
        assert got == want
        assert got_state[0] == list(nc.loaded) == [1, 1, 1] and np.array_equal(got_state[1], nc.read_counts)
        assert np.array_equal(got_state[2], nc.region_text_lengths(3)) and got_state[3] == nc.stats["input_bytes"] > 0
        assert got_state[4] == o2.rlen == 60                                # (rlen follows the last region that holds reads: the 60-base reads on "21")
        # the reference's lines for the case's region; the two other regions show no variant
        assert got.split("\n")[:-1] == case["lines"] and len(case["lines"]) >= 2
        assert got_state[2][0] == len(got) and got_state[2][1] == got_state[2][2] == 0
        # every read of the case reached its sample; the contig behind holds three reads per file that carries them
        # (the loader of the committed case was handed every read of the list; the iterator drops the few that lie outside the window)
        beg, stop = B.window(v["regions"][0][1], v["regions"][0][2])
        for c, s in zip(got_state[1][0], case["regions"][0]["samples"]):
            outside = sum(1 for x in s["fetched"] if not (B._rule_end(x) > beg and x["pos"] + (x["cigar"][0][1] if x["cigar"] and x["cigar"][0][0] == 4 else 0) < stop))
            assert outside <= 1 and s["n_reads"] - outside <= int(c[0]) <= s["n_reads"] and s["n_bad"] - outside <= int(c[1]) <= s["n_bad"]
            assert int(c[0]) + int(c[1]) >= s["n_reads"] + s["n_bad"] - outside
        assert int(got_state[1][1].sum()) == 0 and int(got_state[1][2].sum()) > 0
        # the same call again: handles and caller are unchanged by a call
        assert nc.call_bam_files(files, regions, default_options(**case["options"])) == got
        # the pair of options that asks for the broken-mate fetch is refused by name, and the caller goes on
        with pytest.raises(_lib.PlatypusDeviceError) as e:
            nc.call_bam_files(files, regions, default_options(assemble=1, assembleBrokenPairs=1))
        assert e.value.code == -6 and "assembleBrokenPairs" in str(e.value)
        # a contig no file holds: the region is called without reads
        none = nc.call_bam_files(files, [F.BamFilesRegion("nowhere", 600, 1800, v["regions"][0][3])], default_options(**case["options"]))
        assert none == "" and nc.loaded == [1] and int(nc.read_counts.sum()) == 0
        for f in files:
            f.close()
    finally:
        nc.close()


def test_fetch_plan_with_the_index_queries_on_the_device_equals_the_restatement(monkeypatch):
    monkeypatch.delenv("PLAT_CALLER_HOST_INDEX", raising=False)
    built = [B.built(f) for f in B.hand_files()[:2]] + [B.vcf_files("one")["files"][0]]
    regions = [("chrA", 0, 5000), ("chrA", 5000, 20000), ("chrB", 100, 29000), ("chrA", 39990, 40000), ("20", 600, 2359), ("21", 250, 2100), ("chrZ", 1, 2),
               ("chrA", 0, 1 << 29)]
    nc = F.NativeCaller(0, 1, 1)
    try:
        files = [nc.open_bam(f["bam"], f["bai"], f["name"]) for f in built]
        got = nc.bam_fetch_plan(files, regions)
        assert nc.bam_fetch_info["device_calls"] == 3 and nc.bam_fetch_info["handed_over"] == 0 and nc.bam_fetch_info["queries"] == 5 * 2 + 2
        n = 0
        for (chrom, start, end), per in zip(regions, got):
            for f, g in zip(built, per):
                want = B.fetch(f, chrom, start, end)
                assert (g["tid"], g["itr_beg"], g["itr_end"], g["chunks"]) == (want["tid"], want["itr_beg"], want["itr_end"], want["chunks"]), (chrom, start, end, f["name"])
                n += len(g["chunks"])
        assert n == 13                                                       # (what the restatement gives over these files: counted once on the host)
        for f in files:
            f.close()
    finally:
        nc.close()


@pytest.mark.parametrize("gz", [False, True])
def test_command_line_from_files_on_disk_to_a_vcf(tmp_path, gz):
    from tests.fasta_cases import write_region_fasta
    v = B.vcf_files("two")
    names = []
    for f in v["files"]:
        path = str(tmp_path / f["name"])
        with open(path, "wb") as out:
            out.write(f["bam"])
        with open(path + ".bai" if f is v["files"][0] else path[:-4] + ".bai", "wb") as out:      # (both places an index is looked for)
            out.write(f["bai"])
        names.append(path)
    ref = str(tmp_path / "ref.fa")
    write_region_fasta(ref, {"20": v["regions"][0][3], "21": v["regions"][2][3]}, 60)
    chrom, start, end, _ = v["regions"][0]
    out = str(tmp_path / ("out.vcf.gz" if gz else "out.vcf"))
    cmd = [sys.executable, "-m", "platypus_amd", "callVariants", "--bamFiles", ",".join(names), "--refFile", ref,
           "--regions", "%s:%d-%d,21:251-2100" % (chrom, start + 1, end), "-o", out] + (["--outputIndex", "1"] if gz else [])
    cmd += [x for k, val in v["case"]["options"].items() for x in ("--" + k, str(val))]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    assert '"mode": "presplit"' in r.stdout and '"samples": 2' in r.stdout
    with (gzip.open(out, "rt") if gz else open(out)) as f:
        lines = f.read().split("\n")[:-1]
    head = [ln for ln in lines if ln.startswith("#")]
    assert head[-1].split("\t")[:9] == ["#CHROM", "POS", "ID", "REF", "ALT", "QUAL", "FILTER", "INFO", "FORMAT"] and head[-1].split("\t")[9:] == v["samples"] == ["S1", "S2"]
    assert [ln for ln in lines if not ln.startswith("#")] == v["case"]["lines"]
    if gz:
        from platypus_amd import tabixindex
        with open(out, "rb") as f, open(out + ".tbi", "rb") as t:
            tf = tabixindex.TabixFile(f.read(), t.read())
        assert tf.index.names == [b"20"] and tf.fetch_blocks(b"20", start, end) is not None
    # a region file is refused with a message
    bed = str(tmp_path / "r.bed")
    with open(bed, "w") as f:
        f.write("20\t600\t1800\n")
    r = subprocess.run(cmd[:cmd.index("--regions") + 1] + [bed, "-o", out], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode != 0 and "region files (.txt / .bed) are not read" in r.stderr
