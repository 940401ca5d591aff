"""Generate tests/golden/region_fetched_cases.json.gz: the region cases of region_cases.json.gz as the reference's loader RECEIVED them.

Runs only in the build container (needs the reference tree, gcc, Cython), like gen_golden.py, whose region driver it reuses unchanged:
gen_golden.gen_region is run once more with rgn_drv.Loader wrapped so that what it is handed -- per region and sample the raw read dicts
of the fetch, in fetch order, and the broken mates -- is kept.  The record lines it writes into a scratch directory are asserted to be the
ones of the committed region_cases.json.gz (41 cases, 245 lines), so the stored inputs are exactly what produced those lines.

Stored per case: the case's `options`, `ref`, `sample_names`, `rlen_after` and `lines` (as in region_cases.json.gz), and per region
`chrom`, `start`, `end`, `loaded` and per sample {sample, fetched, brokenMates}: every field rgn_make_read reads (seq, qual as phred+33
text, pos, end, mapq, flag, chromID, mateChromID, insertSize, matePos, cigar) -- plus, per loaded sample, the sizes of the buffers the
reference's addReadToBuffer made of them (n_reads, n_bad).

Usage:  python tests/golden/gen_golden_fetched.py [--scratch DIR]
"""
import argparse
import gzip
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as G  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scratch", default="/tmp/platgold")
    a = ap.parse_args()
    if not os.path.isdir(G.REF):
        sys.exit("reference tree not found at %s: golden vectors can only be regenerated in the build container" % G.REF)
    subprocess.check_call(["make", "-C", os.path.join(G.ROOT, "oracle")])
    G.build_scratch(a.scratch)
    import rgn_drv

    handed = []                                   # one Loader per case, in case order
    base = rgn_drv.Loader

    class RecordingLoader(base):
        def __init__(self, regions):
            base.__init__(self, regions)
            handed.append(self)
    rgn_drv.Loader = RecordingLoader
    with tempfile.TemporaryDirectory() as tmp:
        G.gen_region(tmp)
        with gzip.open(os.path.join(tmp, "region_cases.json.gz"), "rt") as f:
            fresh = json.load(f)
    with gzip.open(os.path.join(HERE, "region_cases.json.gz"), "rt") as f:
        committed = json.load(f)
    assert len(fresh) == len(committed) == len(handed) == 41, (len(fresh), len(committed), len(handed))
    assert sum(len(c["lines"]) for c in committed) == 245
    for k, (x, y) in enumerate(zip(fresh, committed)):
        assert x["lines"] == y["lines"] and x["rlen_after"] == y["rlen_after"], "case %d: the driver no longer writes the committed lines" % k

    enc = lambda rs: [dict(seq=r["seq"].decode(), qual="".join(chr(33 + q) for q in r["qual"]), pos=r["pos"], end=r["end"], mapq=r["mapq"],
                           flag=r["flag"], chromID=r["chromID"], mateChromID=r["mateChromID"], insertSize=r["insertSize"], matePos=r["matePos"],
                           cigar=[list(c) for c in r["cigar"]]) for r in rs]
    cases = []
    for case, loader in zip(committed, handed):
        regions = []
        for reg in case["regions"]:
            key = (reg["chrom"].encode(), reg["start"], reg["end"])
            after = dict((s["sample"], s) for s in reg["samples"])
            samples = []
            for name, reads, broken in loader.regions[key]:
                d = dict(sample=name.decode(), fetched=enc(reads), brokenMates=enc(broken))
                if reg["loaded"]:
                    d["n_reads"], d["n_bad"] = len(after[d["sample"]]["reads"]), len(after[d["sample"]]["badReads"])
                samples.append(d)
            regions.append(dict(chrom=reg["chrom"], start=reg["start"], end=reg["end"], loaded=reg["loaded"], samples=samples))
        cases.append(dict(options=case["options"], ref=case["ref"], sample_names=case["sample_names"], regions=regions,
                          rlen_after=case["rlen_after"], lines=case["lines"]))
    with gzip.open(os.path.join(HERE, "region_fetched_cases.json.gz"), "wt") as f:
        json.dump(cases, f)
    print("region_fetched: %d cases, %d fetched reads, %d record lines" % (
        len(cases), sum(len(s["fetched"]) for c in cases for r in c["regions"] for s in r["samples"]), sum(len(c["lines"]) for c in cases)))


if __name__ == "__main__":
    main()
