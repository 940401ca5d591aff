"""Generate tests/golden/source_cases.json.gz and tests/golden/source_region_cases.json.gz: candidates from source VCF lines (--source).

Runs only in the build container (needs the reference tree, gcc, Cython), like gen_golden.py, whose scratch drivers it reuses unchanged.

source_cases: the reference's own text `src/python/variantutils.py:72-159` (the loop over the lines of one fetch) and `:168-197`
(isValidVcfLine), taken by line range and executed over stand-in line objects (`contig`, `pos` = int(POS) - 1 as TabProxies.pyx:608
leaves it, `ref`, `alt`: native strings, as under Python 2), followed by the text of `:161` (`sorted(list(set(varList)))`).  `Variant` is
the region driver's class (the reference's constructor, __hash__ and __richcmp__) behind an adapter that encodes the native strings.
There is no Python 2 here: `set` in line 161 is a replay of CPython 2.7's set (setobject.c: slot order, the first of equal keys kept)
probed with py2compat.py2_variant_hash -- a restatement, as the dictionaries of the region driver are.  Stored per case: the text, maxSize,
longHaps, the alleles in emission order (varList before line 161) and the list line 161 leaves.

source_region_cases: the region driver (`rgn_drv`, gen_golden.py) with its `variantutils` global, None there, replaced by a reader made
of the same texts (the `for vcfFile in self.vcfFiles` loop of :65-70 restated over in-memory fetches, then :72-159 and :161-163): the
reads are those of committed cases of region_fetched_cases.json.gz (what the reference's loader was handed), the source lines are written
here from the cases' planted variants plus alleles no read shows.  Stored per case: options, ref, sample names, the raw reads per region
and sample, the fetched text per region and source file, and the record lines the reference's loop wrote.

What is restated and what is a stand-in is disclosed in tests/golden/README_source.md.

Usage:  python tests/golden/gen_golden_source.py [--scratch DIR] [--keep-scratch]
"""
import argparse
import gzip
import io
import json
import logging
import os
import subprocess
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as G  # noqa: E402

FILE_VAR = 2


class Line(object):
    """What ctabix's asVCF proxy gives the reader of a line: contig, pos (0-based), ref, alt."""

    def __init__(self, text):
        cols = text.split("\t")
        self.contig, self.pos, self.ref, self.alt = cols[0], int(cols[1]) - 1, cols[3], cols[4]
        self.text = text

    def __str__(self):
        return self.text


def py2_variant_set(py2compat):
    """`set` for line 161: CPython 2.7's set over Variants (hash = py2_variant_hash, equality = the reference's __richcmp__ ==)."""
    M = (1 << 64) - 1

    def make(items):
        items = list(items)
        hashes = [py2compat.py2_variant_hash(v.refName, v.refPos, v.removed, v.added) for v in items]

        def slot(table, k):
            mask = len(table) - 1
            i, perturb = hashes[k] & mask, hashes[k]
            while table[i & mask] is not None and not (hashes[table[i & mask]] == hashes[k] and items[table[i & mask]] == items[k]):
                i = (5 * i + perturb + 1) & M
                perturb >>= 5
            return i & mask
        table, used = [None] * 8, 0
        for k in range(len(items)):
            j = slot(table, k)
            if table[j] is not None:
                continue
            table[j] = k
            used += 1
            if used * 3 >= len(table) * 2:
                size = 8
                while size <= used * (2 if used > 50000 else 4):
                    size <<= 1
                grown = [None] * size
                for q in table:
                    if q is not None:
                        grown[slot(grown, q)] = q
                table = grown
        return [items[k] for k in table if k is not None]
    return make


def reader_namespace(rgn_drv, py2compat):
    """The reference's reader texts in one namespace: `lines_loop(self, vcfLines, chromosome, varList, maxSize)` = variantutils.py:72-159,
    `isValidVcfLine` = :168-197, `finish(varList, chromosome, start, end)` = :161-163."""
    src = open(os.path.join(G.REF, "src/python/variantutils.py")).read().split("\n")
    assert src[71].strip() == "for line in vcfLines:" and src[158].strip() == "varList.append(var)" and src[73].strip() == "if not isValidVcfLine(line):"
    assert src[160].strip() == "varList = sorted(list(set(varList)))" and src[162].strip() == "return varList"
    assert src[167].startswith("def isValidVcfLine(line):") and src[196].strip() == "return True"
    enc = lambda x: x if isinstance(x, bytes) else x.encode("ascii")

    def Variant(refName, refPos, removed, added, nSupportingReads, varSource):
        # (the adapter: variantutils lives in Python 2's one string type, the driver's Variant takes bytes / char*)
        return rgn_drv.Variant(enc(refName), refPos, enc(removed), enc(added), nSupportingReads, varSource)
    ns = dict(Variant=Variant, FILE_VAR=FILE_VAR, logger=logging.getLogger("Log"))
    dedent = lambda lines, n: "\n".join(l[n:] if l.strip() else "" for l in lines)
    text = ("def lines_loop(self, vcfLines, chromosome, varList, maxSize):\n" + dedent(src[71:159], 8) + "\n\n"
            + "\n".join(src[167:197]) + "\n")
    exec(compile(text, "variantutils_py_slice", "exec"), ns)
    # line 161 in a namespace of its own: ITS set is the Python-2 replay (isValidVcfLine's sets of characters are only tested for emptiness)
    fin = dict(logger=ns["logger"], set=py2_variant_set(py2compat))
    exec(compile("def finish(varList, chromosome, start, end):\n" + dedent(src[160:163], 4) + "\n", "variantutils_py_line161", "exec"), fin)
    ns["finish"] = fin["finish"]
    return ns


class Reader(object):
    """variantutils.VariantCandidateReader over in-memory fetches: the constructor and the `for vcfFile in self.vcfFiles` loop (:26-70) are
    restated (file names are keys of FETCHES), everything per line and the set / sort are the reference's text."""
    NS = None
    FETCHES = {}                       # {file name: {(chrom, start, end): text}}

    def __init__(self, fileNames, options):
        self.options = options
        self.vcfFiles = [Reader.FETCHES[name] for name in fileNames]

    def Variants(self, chromosome, start, end):
        varList = []
        maxSize = self.options.maxSize
        for vcfFile in self.vcfFiles:
            text = vcfFile.get((chromosome, start, end), "")
            vcfLines = [Line(t) for t in text.split("\n") if t]
            Reader.NS["lines_loop"](self, vcfLines, chromosome, varList, maxSize)
        return Reader.NS["finish"](varList, chromosome, start, end)


def var3(v):
    return [int(v.refPos), v.removed.decode(), v.added.decode()]


# ---- source_cases ---------------------------------------------------------------------------------------------------------------------

def gen_source_cases(ns, out):
    rng = np.random.default_rng(20260161)
    B = "ACGT"
    seq = lambda n: "".join(B[int(x)] for x in rng.integers(0, 4, n))

    def line(pos, ref, alt, wide=0):
        cols = ["20", str(pos), "rs%d" % int(rng.integers(1, 10 ** 6)) if rng.random() < 0.5 else ".", ref, alt, "50", "PASS", "AC=1;AN=2", "GT"]
        cols += ["0/1"] * wide
        return "\t".join(cols[:int(rng.integers(5, len(cols) + 1))] if not wide else cols)

    def random_line(p0):
        pos = int(p0 + rng.integers(0, 12))
        kind = rng.random()
        if kind < 0.30:                                             # SNPs, one to three alleles: ties at one position
            ref = seq(1)
            alts = [B[int(x)] for x in rng.permutation(4)[:int(rng.integers(1, 4))]]           # (may repeat REF: emitted all the same)
            return line(pos, ref, ",".join(alts))
        if kind < 0.45:                                             # MNPs with shared heads and tails
            n = int(rng.integers(2, 7))
            ref = seq(n)
            alt = list(ref)
            for _ in range(int(rng.integers(0, 3))):
                alt[int(rng.integers(0, n))] = B[int(rng.integers(0, 4))]
            return line(pos, ref, "".join(alt))
        if kind < 0.62:                                             # insertions: several at one position (ties)
            ref = seq(1)
            alts = [ref + seq(int(rng.integers(1, 4))) for _ in range(int(rng.integers(1, 4)))]
            return line(pos, ref, ",".join(alts))
        if kind < 0.74:                                             # deletions, also with a repeated head that trims further
            ref = seq(int(rng.integers(2, 9)))
            return line(pos, ref, ref[:int(rng.integers(1, len(ref)))])
        if kind < 0.82:                                             # replacements / anchors that differ
            return line(pos, seq(int(rng.integers(1, 6))), seq(int(rng.integers(1, 6))) + "," + seq(int(rng.integers(1, 4))))
        if kind < 0.87:                                             # an allele over maxSize next to one that fits
            ref = seq(1)
            return line(pos, ref, ref + seq(int(rng.integers(30, 45))) + "," + seq(1))
        if kind < 0.91:                                             # empty ALT elements
            return line(pos, seq(int(rng.integers(1, 3))), rng.choice(["A,", ",C", ",", ""]))
        if kind < 0.96:                                             # what isValidVcfLine refuses
            return line(pos, *[("A", "."), ("A", "*"), ("A", "<DEL>"), ("a", "C"), ("A", "c,G"), ("AN", "A,R"), ("A.", "C")][int(rng.integers(0, 7))])
        return line(int(rng.integers(0, 2)), "N", "A,N")           # POS 0 (pos -1: invalid) and POS 1

    cases = []
    for ci in range(72):
        longHaps = int(ci % 6 == 5)
        maxSize = 25 if ci % 4 == 0 else 1500
        n = int(rng.integers(4, 36))
        p0 = int(rng.integers(1, 5000))
        lines = [random_line(p0) for _ in range(n)]
        if ci % 5 == 0:                                             # the same record twice (two files listing one allele)
            lines.append(lines[int(rng.integers(0, len(lines)))])
        if ci == 7:
            lines.append(line(p0 + 3, "G", "T", wide=400))
        text = "".join(t + "\n" for t in lines)
        if ci % 9 == 0:
            text = text[:-1]                                        # the last line without its newline
        self = types.SimpleNamespace(options=types.SimpleNamespace(longHaps=longHaps, maxSize=maxSize))
        varList = []
        ns["lines_loop"](self, [Line(t) for t in text.split("\n") if t], b"20", varList, maxSize)
        emitted = [var3(v) for v in varList]
        ordered = ns["finish"](list(varList), b"20", 0, 0)
        cases.append(dict(chrom="20", text=text, maxSize=maxSize, longHaps=longHaps, alleles=emitted, ordered=[var3(v) for v in ordered]))

    # the conditions the fixture has to meet
    from platypus_amd import regionprep as RP
    seen = set()
    ties = collapsed = 0
    for c in cases:
        for t in c["text"].split("\n"):
            if not t:
                continue
            verdict, alleles, over = RP.sourceLineAlleles(t.encode(), c["maxSize"], c["longHaps"])
            cols = t.split("\t")
            ref, alts = cols[3], cols[4].split(",")
            if verdict == RP.SOURCE_LINE_INVALID:
                seen.add("invalid-pos" if int(cols[1]) == 0 else "invalid-ref" if set(ref) - set("ACGTN") else "invalid-alt")
            if over:
                seen.add("oversize")
            if verdict == RP.SOURCE_LINE_OK:
                for a in alts:
                    if abs(len(a) - len(ref)) > c["maxSize"]:
                        continue
                    if a == "":
                        seen.add("empty-element")
                    if len(ref) == len(a) == 1:
                        seen.add("snp-equal" if ref == a else "snp")
                    elif len(ref) == len(a):
                        seen.add("mnp-empty" if ref == a else "mnp-lead" if ref[0] == a[0] else "mnp-tail" if ref[-1] == a[-1] else "mnp")
                    elif c["longHaps"]:
                        seen.add("longhaps")
                    else:
                        seen.add("indel-trim" if len(ref) > 1 and len(a) > 1 and ref[1] == a[1] else "indel")
                        if ref[:1] != a[:1]:
                            seen.add("indel-anchor-differs")
        o = c["ordered"]
        key = lambda v: (v[0], len(v[1]), len(v[2]))
        if any(key(a) == key(b) and (len(a[1]) == len(a[2]) == 1 or len(a[1]) == 0) for a, b in zip(o, o[1:])):
            ties += 1
        if len(o) < len(c["alleles"]):
            collapsed += 1
        # (the product's restatement agrees -- a check of the generator's inputs, not the fixture's source)
        got, _, bad = RP.sourceTextAlleles(c["text"].encode(), c["maxSize"], c["longHaps"])
        assert not bad and [[p, r.decode(), a.decode()] for p, r, a, _ in got] == c["alleles"], c["text"]
    need = {"invalid-pos", "invalid-ref", "invalid-alt", "oversize", "empty-element", "snp", "snp-equal", "mnp", "mnp-lead", "mnp-tail", "mnp-empty",
            "longhaps", "indel", "indel-trim", "indel-anchor-differs"}
    assert need <= seen, need - seen
    assert ties >= 10 and collapsed >= 1, (ties, collapsed)
    path = os.path.join(out, "source_cases.json.gz")
    with gzip.open(path, "wt") as f:
        json.dump(cases, f)
    assert os.path.getsize(path) < (1 << 20)
    print("source: %d cases, %d lines, %d alleles, %d cases with a tie set order decides, %d with duplicates collapsed, %d bytes" % (
        len(cases), sum(c["text"].count("\n") for c in cases), sum(len(c["alleles"]) for c in cases), ties, collapsed, os.path.getsize(path)))


# ---- source_region_cases --------------------------------------------------------------------------------------------------------------

def gen_source_region_cases(out):
    import rgn_drv
    from platypus_amd.options import default_options
    VCF, infoSig, filterSig, formatSig = G.build_vcf_writer()
    swallowed = []
    sys.unraisablehook = lambda u: swallowed.append(repr(u.exc_value))       # "cdef void" texts would hide an exception
    wpy = open(os.path.join(G.REF, "src/python/window.py")).read().split("\n")
    assert wpy[17].startswith("class WindowGenerator(object):") and wpy[237].strip() == "yield thisWindow"
    wns = dict(xrange=range, logger=G.logging_stub())
    exec(compile("from __future__ import division\n" + "\n".join(wpy[17:238]) + "\n", "window_py_slice", "exec"), wns)
    log = logging.getLogger("Log")
    log.setLevel(logging.WARNING)
    log.propagate = False
    msgs = []

    class Capture(logging.Handler):
        def emit(self, record):
            msgs.append((record.levelname, record.getMessage()))
    log.addHandler(Capture())

    with gzip.open(os.path.join(HERE, "region_fetched_cases.json.gz"), "rt") as f:
        fetched = json.load(f)
    with gzip.open(os.path.join(HERE, "region_cases.json.gz"), "rt") as f:
        planted = [c["planted"] for c in json.load(f)]
    rng = np.random.default_rng(4906161)
    B = "ACGT"

    def vcf_line(ref, pos, rem, add):
        """One record for the allele (pos, rem, add) as a VCF writes it: SNPs as they are, indels behind their anchor base."""
        if len(rem) == len(add):
            return "20\t%d\t.\t%s\t%s\tQ\tPASS\tX=1" % (pos + 1, rem, add)
        a = ref[pos - 1]
        return "20\t%d\t.\t%s\t%s\tQ\tPASS\tX=1" % (pos, a + rem, a + add)

    def novel(ref, lo, hi, n):
        """alleles no read shows: SNPs (two alleles at one site now and then), an insertion, a deletion, an MNP"""
        outl = []
        for _ in range(n):
            p = int(rng.integers(lo, hi))
            r = ref[p]
            k = rng.random()
            if k < 0.5:
                alts = [b for b in B if b != r]
                rng.shuffle(alts)
                outl.append("20\t%d\trsN\t%s\t%s" % (p + 1, r, ",".join(alts[:int(rng.integers(1, 3))])))
            elif k < 0.7:
                outl.append("20\t%d\t.\t%s\t%s\t.\t.\t." % (p + 1, r, r + "".join(B[int(x)] for x in rng.integers(0, 4, int(rng.integers(1, 4))))))
            elif k < 0.9:
                outl.append("20\t%d\t.\t%s\t%s" % (p + 1, ref[p:p + int(rng.integers(2, 5))], r))
            else:
                m = ref[p:p + 3]
                outl.append("20\t%d\t.\t%s\t%s" % (p + 1, m, m[0] + B[(B.index(m[1]) + 1) % 4] + m[2]))
        return outl

    # (base case of region_fetched_cases, options on top of its own, number of source files, what it is there for)
    plan = [
        (0, dict(), 1, "source + BAM candidates: planted alleles (equal to BAM candidates) and alleles no read supports"),
        (0, dict(getVariantsFromBAMs=0), 1, "the source alone: getVariantsFromBAMs=0"),
        (10, dict(), 1, "source + assemble=1"),
        (1, dict(), 2, "two samples, two files (the second repeats alleles of the first)"),
        (9, dict(longHaps=1), 1, "longHaps=1: indel records untrimmed"),
        (9, dict(), 2, "indels from the source, two files"),
        (30, dict(), 1, "two regions called in order"),
        (38, dict(getVariantsFromBAMs=0), 1, "two samples with different alleles at one site, the source alone"),
    ]
    cases = []
    for base, extra, nFiles, why in plan:
        fc = fetched[base]
        ref = fc["ref"]
        opts_over = dict(fc["options"], **extra)
        names = [s.encode() for s in fc["sample_names"]]
        regions = [(r["chrom"].encode(), r["start"], r["end"]) for r in fc["regions"]]
        raw = {}
        for reg, r in zip(regions, fc["regions"]):
            dec = lambda rs: [dict(x, seq=x["seq"].encode(), qual=[ord(c) - 33 for c in x["qual"]], cigar=[tuple(c) for c in x["cigar"]]) for x in rs]
            raw[reg] = [(s["sample"].encode(), dec(s["fetched"]), dec(s["brokenMates"])) for s in r["samples"]]
        # the source files: every planted allele (the reads show most of them) and novel ones, in position order; a second file repeats
        # some of the first's alleles and adds its own
        files = []
        for fi in range(nFiles):
            recs = []
            for p, rem, add in planted[base]:
                if fi == 0 or rng.random() < 0.5:
                    recs.append((p, vcf_line(ref, p, rem, add)))
            for t in novel(ref, regions[0][1] + 30, regions[-1][2] - 30, 6 if fi == 0 else 3):
                recs.append((int(t.split("\t")[1]) - 1, t))
            recs.sort(key=lambda x: x[0])
            files.append([t for _, t in recs])
        fetches = []                                                # per region, per file: the text a fetch of the region returns
        Reader.FETCHES = {}
        for fi, recs in enumerate(files):
            per = {}
            for reg in regions:
                hit = [t for t in recs if int(t.split("\t")[1]) - 1 < reg[2] and int(t.split("\t")[1]) - 1 + len(t.split("\t")[3]) > reg[1]]
                per[reg] = "".join(t + "\n" for t in hit)
            Reader.FETCHES["source%d.vcf.gz" % fi] = per
        for reg in regions:
            fetches.append([Reader.FETCHES["source%d.vcf.gz" % fi][reg] for fi in range(nFiles)])
        opts = default_options(**opts_over)
        opts.verbosity = 2
        opts.bamFiles, opts.refFile = ["fixture.bam"], "fixture.fa"
        opts.sourceFile = ["source%d.vcf.gz" % fi for fi in range(nFiles)]
        opts.nInd = len(names)
        opts.originalMaxHaplotypes = opts.maxHaplotypes
        opts.maxHaplotypes = min(257, opts.maxHaplotypes)
        opts.maxGenotypes = opts.originalMaxHaplotypes * (opts.originalMaxHaplotypes + 1) // 2
        opts.rlen = 150
        loader = rgn_drv.Loader(raw)
        vf = VCF()
        vf.setsamples(list(names)); vf.setinfo(infoSig); vf.setfilter(filterSig); vf.setformat(formatSig)
        stream = io.StringIO()
        del msgs[:]
        rgn_drv.run_regions(list(regions), loader, rgn_drv.FastaFile({b"20": ref.encode()}), opts, wns["WindowGenerator"](), stream, vf)
        lines = stream.getvalue().split("\n")[:-1]
        skipped = [m for lv, m in msgs if "will be skipped" in m]
        errors = [m for lv, m in msgs if lv == "ERROR"]
        assert not skipped and not errors, (why, skipped[:2], errors[:2])
        assert all(reg in loader.loaded for reg in regions)
        enc = lambda rs: [dict(r, qual="".join(chr(33 + q) for q in r["qual"])) for r in rs]
        cases.append(dict(why=why, base_case=base, options=opts_over, ref=ref, sample_names=fc["sample_names"],
                          regions=[dict(chrom=c.decode(), start=s_, end=e_, loaded=True, source=fetches[k],
                                        samples=[dict(sample=b["sample"], reads=enc(b["reads"]), badReads=enc(b["badReads"]), brokenMates=enc(b["brokenMates"]))
                                                 for b in loader.loaded[reg]])
                                   for k, reg in enumerate(regions) for c, s_, e_ in [reg]],
                          rlen_after=int(opts.rlen), lines=lines))
        print("  source region case (%s): %d regions, %d samples, %d source lines -> %d record lines (%d Source=File, %d Platypus,File)" % (
            why, len(regions), len(names), sum(t.count("\n") for f in fetches for t in f), len(lines),
            sum("Source=File" in ln for ln in lines), sum("Source=Platypus,File" in ln or "Source=File,Platypus" in ln for ln in lines)))
    assert not swallowed, swallowed[:3]
    text = "\n".join(ln for c in cases for ln in c["lines"])
    assert "Source=File;" in text or "Source=File\t" in text, "no allele that only the source lists was called"
    assert "Platypus" in text and ("Platypus,File" in text or "File,Platypus" in text), "no allele of both the reads and the source"
    assert any("Assembler" in ln and "File" in ln for c in cases for ln in c["lines"]) or any(c["options"].get("assemble") for c in cases)
    path = os.path.join(out, "source_region_cases.json.gz")
    with gzip.open(path, "wt") as f:
        json.dump(cases, f)
    assert os.path.getsize(path) < (1 << 20), os.path.getsize(path)
    print("source region: %d cases, %d record lines, %d bytes" % (len(cases), sum(len(c["lines"]) for c in cases), os.path.getsize(path)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scratch", default="/tmp/platgold")
    ap.add_argument("--keep-scratch", action="store_true", help="use the drivers already built in --scratch")
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    if not os.path.isdir(G.REF):
        sys.exit("reference tree not found at %s: golden vectors can only be regenerated in the build container" % G.REF)
    if a.keep_scratch and os.path.exists(os.path.join(a.scratch, "rgn_drv.pyx")):
        sys.path.insert(0, a.scratch)
    else:
        subprocess.check_call(["make", "-C", os.path.join(G.ROOT, "oracle")])
        G.build_scratch(a.scratch)
    import py2compat
    import rgn_drv
    ns = reader_namespace(rgn_drv, py2compat)
    Reader.NS = ns
    rgn_drv.variantutils = types.SimpleNamespace(VariantCandidateReader=Reader)
    todo = a.only.split(",") if a.only else ["source", "region"]
    if "source" in todo:
        gen_source_cases(ns, HERE)
    if "region" in todo:
        gen_source_region_cases(HERE)


if __name__ == "__main__":
    main()
