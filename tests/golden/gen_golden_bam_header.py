"""Generate tests/golden/bam_header_cases.json.gz: BAM header text -> read groups and samples, loadBAMData's mode decision, and the region
list of getRegions, for the tests of include/platypus_caller_bamfile.h.

Runs only where the reference tree is (PLATYPUS_REF), like the other generators.  It takes the reference's own text by line range and
executes it over stand-ins, as gen_golden_source.py does:

  htslibWrapper.pyx:16-20, :26-29   VALID_HEADER_TYPES, VALID_HEADER_FIELDS (dict literals, executed as they are)
  htslibWrapper.pyx:251-289         Samfile.header's getter
  platypusutils.pyx:114-147         the try / except of getSampleNamesAndLoadIterators, inside a restated loop over the files
  platypusutils.pyx:462-463, :478-484   uniqueSamples, uniqueBAMs, the decision and the choice of a sample's file
  platypusutils.pyx:999-1085        getRegions from `options.regions == None` on

What is rewritten so that Python 3 compiles Python-2 text, and what stands in for what, is disclosed in README_bam_header.md.

Usage:  python tests/golden/gen_golden_bam_header.py
"""
import gzip
import json
import logging
import os
import re
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("PLATYPUS_REF", "/root/reference")


def py3(lines):
    """Python-2 statements Python 3 does not parse, rewritten one for one: `raise X, msg` -> `raise X(msg)`, `except X, e:` -> `except X as e:`,
    `cdef <type> name = ...` -> `name = ...`."""
    out = []
    for ln in lines:
        ln = re.sub(r"^(\s*)raise (\w+), (.*)$", r"\1raise \2(\3)", ln)
        ln = re.sub(r"^(\s*)except (\w+), (\w+):", r"\1except \2 as \3:", ln)
        ln = re.sub(r"^(\s*)cdef (?:list|dict|str|int) (\w+ = )", r"\1\2", ln)
        out.append(ln)
    return out


def dedent(lines, n):
    return [l[n:] if l.strip() else "" for l in lines]


def namespaces():
    hts = open(os.path.join(REF, "src/cython/htslibWrapper.pyx")).read().split("\n")
    utl = open(os.path.join(REF, "src/cython/platypusutils.pyx")).read().split("\n")
    assert hts[15].startswith("VALID_HEADER_TYPES = {") and hts[19].strip() == '"CO" : list }'
    assert hts[25].startswith("VALID_HEADER_FIELDS = {") and hts[28].strip().startswith('"PG" :')
    assert hts[250].strip() == "def __get__(self):" and hts[288].strip() == "return result"
    assert utl[113].strip() == "try:" and utl[146].strip().startswith("logger.debug(\"Adding sample name %s, from BAM file")
    assert utl[461].strip() == "cdef list uniqueSamples = sorted(set(samples))" and utl[462].strip() == "cdef list uniqueBAMs = sorted(set(bamFiles))"
    assert utl[477].strip() == "if len(set(samples)) == len(set(bamFiles)):" and utl[483].strip() == "reader = bamsThisSample[0]"
    assert utl[998].strip() == "elif options.regions == None:" and utl[1084].strip() == "return finalRegions"
    log = logging.getLogger("Log")
    log.setLevel(logging.CRITICAL)
    ns = dict(StandardError=Exception, NULL=None, logger=log, bytes=str, os=os)
    text = "\n".join(hts[15:20] + hts[25:29]) + "\n"
    text += "def header_get(self):\n" + "\n".join(py3(dedent(hts[251:289], 8))) + "\n"
    # the loop over the files restated (platypusutils.pyx:103-112 opens them), its try / except the reference's
    text += ("def sample_names(bamFileNames, opened):\n    samples = []\n    samplesByID = {}\n    samplesByBAM = {}\n"
             "    for index,fileName in enumerate(bamFileNames):\n        bamFile = opened[index]\n" + "\n".join(py3(utl[113:147])) + "\n"
             "    return samples,samplesByID,samplesByBAM\n")
    # the decision: 462-463 and 478-484, the reader kept per sample where the reference goes on to fetch from it
    text += ("def decide(samples, bamFiles, samplesByBAM):\n" + "\n".join(py3(utl[461:463])) + "\n    chosen = {}\n" + "\n".join(py3(utl[477:484])) + "\n"
             "            chosen[sample] = reader\n        return 'presplit', uniqueSamples, chosen\n    return 'merged', uniqueSamples, None\n")
    body = py3(utl[998:1085])
    body[0] = body[0].replace("elif", "if", 1)
    text += "def get_regions(options, file, refFile):\n    regions = []\n" + "\n".join(body) + "\n"
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", SyntaxWarning)                  # (platypusutils.pyx:1023 calls a string)
        exec(compile(text, "reference_slices", "exec"), ns)
    return ns


class Sam(object):
    """What the slices read of a Samfile: theHeader.text, text, header (the getter above), close; ordered and hashed by its place in the list."""
    NS = None

    def __init__(self, index, text):
        self.index, self.text = index, text
        self.theHeader = types.SimpleNamespace(text=text)
        self.filename, self.lock = "file%d" % index, None

    header = property(lambda self: Sam.NS["header_get"](self))

    def __lt__(self, other):
        return self.index < other.index

    def close(self):
        pass


class Refs(dict):
    iteritems = dict.items


SQ = "@SQ\tSN:chrA\tLN:40000\n@SQ\tSN:chrB\tLN:30000\n"
HEADERS = [
    ("one read group", "@HD\tVN:1.4\tSO:coordinate\n" + SQ + "@RG\tID:g1\tSM:NA1\tPL:X\n@PG\tID:w\tPN:w\n@CO\tany text: here\n"),
    ("no @RG", "@HD\tVN:1.0\n" + SQ),
    ("an @RG without SM", SQ + "@RG\tID:g1\tLB:l\n"),
    ("an @RG without SM behind one with", SQ + "@RG\tID:g1\tSM:a\n@RG\tID:g2\n"),
    ("an unknown field code", SQ + "@RG\tID:g1\tSM:a\tXX:1\n"),
    ("an unknown field code in @SQ", "@SQ\tSN:chrA\tLN:40000\tAN:alt\n@RG\tID:g1\tSM:a\n"),
    ("a line without @", SQ + "RG\tID:g1\tSM:a\n@RG\tID:g2\tSM:b\n"),
    ("two @HD", "@HD\tVN:1.0\n@HD\tVN:1.4\n" + SQ + "@RG\tID:g1\tSM:a\n"),
    ("a duplicate ID", SQ + "@RG\tID:g1\tSM:a\n@RG\tID:g2\tSM:b\n@RG\tID:g1\tSM:b\n"),
    ("a duplicate ID, one sample", SQ + "@RG\tID:g1\tSM:a\n@RG\tID:g1\tSM:a\n"),
    ("SM containing ':'", SQ + "@RG\tID:g:1\tSM:fam:child:2\n"),
    ("CRLF", "@HD\tVN:1.4\r\n" + SQ.replace("\n", "\r\n") + "@RG\tID:g1\tSM:a\r\n"),
    ("CRLF, SM in the middle", SQ.replace("\n", "\r\n") + "@RG\tSM:a\tID:g1\r\n"),
    ("two samples", SQ + "@RG\tID:ga\tSM:T2\n@RG\tID:gb\tSM:T1\n"),
    ("three groups, two samples", SQ + "@RG\tID:g1\tSM:T1\n@RG\tID:g2\tSM:T2\n@RG\tID:g3\tSM:T1\n"),
    ("blank and whitespace lines", "\n" + SQ + "   \n\t\n@RG\tID:g1\tSM:a\n\n\n"),
    ("no newline at the end", SQ + "@RG\tID:g1\tSM:a"),
    ("an invalid record type", SQ + "@XY\tID:1\n@RG\tID:g1\tSM:a\n"),
    ("a field without ':'", SQ + "@RG\tID:g1\tSM:a\tnocolon\n"),
    ("an empty field", SQ + "@RG\tID:g1\t\tSM:a\n"),
    ("LN that is no int", "@SQ\tSN:chrA\tLN:4e4\n@RG\tID:g1\tSM:a\n"),
    ("LN with blanks and a sign", "@SQ\tSN:chrA\tLN: +40000 \n@RG\tID:g1\tSM:a\n"),
    ("an @RG without ID behind one with", SQ + "@RG\tID:g1\tSM:a\n@RG\tSM:a\tLB:x\n"),
    ("SM twice in a line", SQ + "@RG\tID:g1\tSM:a\tSM:b\n"),
    ("an empty text", ""),
    ("only @CO", "@CO\tfree\ttext without colons\n"),
    ("an empty SM", SQ + "@RG\tID:g1\tSM:\n"),
]
NAMES = ["/data/run1/NA12878.bam", "relative/sample_two.cram", "x.bam", "ab.bam", "a.b.c.bam", "dir.with.dots/plain", "T1.bam"]

# the files of one call: (header label, file name)
PLANS = [
    [("one read group", "a.bam")],
    [("no @RG", "/data/run1/NA12878.bam")],
    [("one read group", "a.bam"), ("SM containing ':'", "b.bam")],
    [("two samples", "m.bam")],
    [("two samples", "m.bam"), ("one read group", "a.bam")],
    [("a duplicate ID", "d.bam"), ("two samples", "m.bam")],
    [("a duplicate ID, one sample", "x1.bam"), ("a duplicate ID, one sample", "x2.bam")],
    [("two samples", "m1.bam"), ("two samples", "m2.bam")],
    [("three groups, two samples", "t.bam"), ("no @RG", "T1.bam")],
    [("no @RG", "dir/ab.bam"), ("an empty SM", "e.bam")],
    [("no @RG", "dir/ab.bam"), ("CRLF", "c.bam")],
    [("an @RG without ID behind one with", "p.bam"), ("one read group", "a.bam")],
    [("an @RG without ID behind one with", "p.bam"), ("two samples", "m.bam")],
    [("an unknown field code", "u1.bam"), ("an unknown field code", "u1.bam")],
    [("two samples", "m.bam"), ("three groups, two samples", "t.bam"), ("no @RG", "z9.bam")],
]

FAI = [("chrA", 40000), ("chrB", 30000), ("chrC", 500)]
REGION_CASES = [
    ("one read group", None, 100000), ("one read group", None, 12000), ("no @RG", None, 7000),
    ("one read group", ["chrA"], 100000), ("one read group", ["chrB"], 9000), ("one read group", ["chrA:100-2000"], 100000),
    ("one read group", ["chrA:100-30000", "chrB:1-500"], 10000), ("one read group", ["chrB:1-30000", "chrA"], 16384),
    ("one read group", ["chrZ:1-10", "chrA:5-6"], 100000), ("one read group", ["chrC:600-700", "chrC:400-900"], 100000),
    ("one read group", ["chrC"], 100000), ("an unknown field code in @SQ", ["chrC"], 100), ("an unknown field code in @SQ", ["chrA:1-10", "chrC"], 100),
    ("one read group", ["chr:with:colons:3-9"], 100000), ("an unknown field code in @SQ", None, 100),
]


def main():
    if not os.path.isdir(REF):
        sys.exit("reference tree not found at %s: golden vectors can only be regenerated where it is" % REF)
    ns = namespaces()
    Sam.NS = ns
    texts = dict(HEADERS)
    headers = []
    for k, (label, text) in enumerate(HEADERS):
        name = NAMES[k % len(NAMES)]
        sam = Sam(0, text)
        try:
            rg = [[g.get("ID"), g.get("SM")] for g in ns["header_get"](sam).get("RG", [])]
            raised = None
        except Exception as e:
            rg, raised = None, type(e).__name__
        samples, byID, byBAM = ns["sample_names"]([name], [sam])
        headers.append(dict(label=label, text=text, file_name=name, header_rg=rg, header_raised=raised, samples=sorted(samples),
                            samplesByID=byID, samplesByBAM=byBAM[sam] if isinstance(byBAM[sam], str) else sorted(byBAM[sam])))
    plans = []
    for files in PLANS:
        opened = [Sam(i, texts[label]) for i, (label, _) in enumerate(files)]
        samples, byID, byBAM = ns["sample_names"]([n for _, n in files], opened)
        try:
            mode, order, chosen = ns["decide"](samples, opened, byBAM)
            chosen = {s: r.index for s, r in chosen.items()} if chosen is not None else None
        except AssertionError:
            mode, order, chosen = "assertion", sorted(set(samples)), None
        plans.append(dict(files=[dict(label=l, file_name=n) for l, n in files], samples=sorted(samples), samplesByID=byID, mode=mode, order=order, chosen=chosen))
    regions = []
    for label, asked, buffer_size in REGION_CASES:
        opts = types.SimpleNamespace(regions=asked, bufferSize=buffer_size, verbosity=2)
        refs = Refs((n, types.SimpleNamespace(SeqLength=l)) for n, l in (FAI if asked is not None or label != "an unknown field code in @SQ" else FAI[2:]))     # (one contig where the order would be a Python-2 dict's)
        got = ns["get_regions"](opts, Sam(0, texts[label]), types.SimpleNamespace(refs=refs))
        regions.append(dict(label=label, regions=asked, bufferSize=buffer_size, fai=[[n, v.SeqLength] for n, v in refs.items()], final=[list(r) for r in got]))
    seen = {h["header_raised"] for h in headers}
    assert {"ValueError", "AssertionError", "Exception", None} <= seen, seen
    assert {p["mode"] for p in plans} == {"presplit", "merged", "assertion"}
    path = os.path.join(HERE, "bam_header_cases.json.gz")
    with gzip.open(path, "wt") as f:
        json.dump(dict(headers=headers, plans=plans, regions=regions), f)
    print("bam header: %d header texts (%d raise), %d plans, %d region lists, %d bytes" % (
        len(headers), sum(h["header_raised"] is not None for h in headers), len(plans), len(regions), os.path.getsize(path)))


if __name__ == "__main__":
    main()
