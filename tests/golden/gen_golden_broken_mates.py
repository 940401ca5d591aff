"""Generate tests/golden/broken_mate_cases.json.gz: which fetched reads give a mate coordinate, the sorted coordinates, the queries
mergeQueries makes of them and which records of a second-round fetch are broken mates, for the tests of csrc/mate_rule.hpp and
plat_bam_files_mates_plan (include/platypus_caller_bamfile.h).

Runs only where the reference tree is (PLATYPUS_REF), like the other generators.  It takes the reference's own text by line range and
executes it over stand-in reads, as gen_golden_bam_header.py does:

  htslibWrapper.pxd:235-237, :256-257, :262-263, :265-266   BAM_FPROPER_PAIR / BAM_FUNMAP / BAM_FMUNMAP and the three flag tests
  platypusutils.pyx:522-533    the append rule of loadBAMData's first branch (the second branch, :617-627, is the same text)
  platypusutils.pyx:545        brokenMateCoords.sort()
  platypusutils.pyx:690-707    mergeQueries
  platypusutils.pyx:556        the filter predicate of the second round

What is rewritten so that Python 3 compiles Cython text, and what stands in for what, is disclosed in README_broken_mates.md.  Only data is
stored: the inputs written here and what the executed text made of them.

Usage:  python tests/golden/gen_golden_broken_mates.py
"""
import gzip
import json
import os
import random
import re
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("PLATYPUS_REF", "/root/reference")


def dedent(lines, n):
    return [l[n:] if l.strip() else "" for l in lines]


def namespace():
    pxd = open(os.path.join(REF, "src/cython/htslibWrapper.pxd")).read().split("\n")
    utl = open(os.path.join(REF, "src/cython/platypusutils.pyx")).read().split("\n")
    assert pxd[234].startswith("DEF BAM_FPROPER_PAIR = 2") and pxd[236].startswith("DEF BAM_FMUNMAP = 8")
    assert pxd[255].startswith("cdef inline int Read_IsProperPair(") and pxd[261].startswith("cdef inline int Read_IsUnmapped(") and pxd[264].startswith("cdef inline int Read_MateIsUnmapped(")
    assert utl[521].strip() == "if fetchBrokenMates:" and utl[532].strip().startswith("brokenMateCoords.append(")
    assert utl[544].strip() == "brokenMateCoords.sort()"
    assert utl[555].strip() == "if readIterator.b.core.mtid == chromID and start <= readIterator.b.core.mpos <= end:"
    assert utl[689].strip() == "cdef list mergeQueries(list coords):" and utl[706].strip() == "return queries"
    flag_fn = lambda a, b: [re.sub(r"^cdef inline int (\w+)\(cAlignedRead\* theRead\) nogil:", r"def \1(theRead):", pxd[a])] + pxd[a + 1:b]
    text = "\n".join(re.sub(r"^DEF ", "", l) for l in pxd[234:237]) + "\n"
    text += "\n".join(flag_fn(255, 257) + flag_fn(261, 263) + flag_fn(264, 266)) + "\n"
    text += "def append_rule(fetchBrokenMates, theRead, reader, brokenMateCoords):\n" + "\n".join(dedent(utl[521:533], 12)) + "\n"
    text += "def sort_coords(brokenMateCoords):\n" + "\n".join(dedent(utl[544:545], 12)) + "\n"
    text += "def mergeQueries(coords):\n" + "\n".join(utl[690:707]) + "\n"
    text += "def is_mate(readIterator, chromID, start, end):\n" + "\n".join(dedent(utl[555:556], 20)) + "\n        return True\n    return False\n"
    ns = {}
    exec(compile(text, "reference_slices", "exec"), ns)
    return ns


FLAGS8 = [a | b | c for a in (0, 2) for b in (0, 4) for c in (0, 8)]         # every combination of 0x2 / 0x4 / 0x8


def chain(start, step, last):
    """Positions from start in steps that keep mergeQueries' gap test true, then `last`."""
    return list(range(start, last - 1000, step)) + [last]


def cases():
    AB, BA = ["chrA", "chrB"], ["chrB", "chrA"]                              # BA: name order differs from tid order
    R = lambda mpos, mtid=0, flag=1: [flag, mtid, mpos]
    out = []
    add = lambda label, contigs, chrom_id, start, end, reads, second=(): out.append(dict(label=label, contigs=contigs, chrom_id=chrom_id, start=start, end=end,
                                                                                         reads=[list(r) for r in reads], second=[list(s) for s in second]))
    edge = lambda s, e, tid, other: [[t, p] for t in (tid, other, -1) for p in (s - 1, s, e, e + 1, (s + e) // 2)]
    add("the empty list", AB, 0, 1000, 2000, [], edge(1000, 2000, 0, 1))
    add("one coordinate", AB, 0, 1000, 2000, [R(50000)], edge(1000, 2000, 0, 1))
    add("equal coordinates", AB, 0, 1000, 2000, [R(50000), R(50000), R(50000)])
    add("mate position 0", AB, 0, 1000, 2000, [R(0), R(1), R(2)])
    for gap in (9999, 10000, 10001):
        add("a gap of %d" % gap, AB, 0, 1000, 2000, [R(100), R(101 + gap)])
    for span in (99999, 100000, 100001):
        add("a span of %d" % span, AB, 0, 500, 900, [R(p) for p in chain(1000, 9000, 1000 + span)])
    add("a span of 100000 reached in one step too many", AB, 0, 500, 900, [R(p) for p in chain(1000, 9000, 101000)] + [R(101001), R(110999), R(111000)])
    add("two contigs, tid order", AB, 0, 1000, 2000, [R(700, 1), R(300, 0), R(800, 1), R(200, 0), R(20000, 1)])
    add("two contigs, name order against tid order", BA, 1, 1000, 2000, [R(700, 1), R(300, 0), R(800, 1), R(200, 0), R(20000, 0), R(5, 1)], edge(1000, 2000, 1, 0))
    add("equal names under two tids", ["dup", "dup", "x"], 2, 10, 20, [R(500, 1), R(400, 0), R(450, 1), R(90000, 0), R(100, 2), R(460, 0)], edge(10, 20, 2, 0))
    add("mtid -1 under every flag", AB, 0, 1000, 2000, [R(5000 + f, -1, f | 1) for f in FLAGS8])
    add("every flag, mate on the same contig", AB, 0, 1000, 2000, [R(5000 + 20000 * i, 0, f | 0x41) for i, f in enumerate(FLAGS8)])
    add("every flag, mate on the other contig", AB, 0, 1000, 2000, [R(5000 + 20000 * i, 1, f | 0x81) for i, f in enumerate(FLAGS8)])
    add("every flag on tid 1, mates everywhere", BA, 1, 1000, 2000, [R(3000 + 7 * i + 50000 * t, t, f) for i, f in enumerate(FLAGS8) for t in (-1, 0, 1)])
    add("the filter's edges, region at 0", AB, 1, 0, 10, [R(5, 1)], edge(0, 10, 1, 0))
    add("the filter's edges, start == end", AB, 0, 777, 777, [R(5)], edge(777, 777, 0, 1))
    add("the largest position", AB, 0, 1000, 2000, [R(2147483647), R(2147483646), R(2147473647)], [[0, 2147483647]])
    add("descending input", AB, 0, 1000, 2000, [R(p) for p in range(300000, 0, -7001)])
    add("a run that ends by the gap, then by the span", AB, 0, 1000, 2000, [R(p) for p in chain(0, 9999, 99998)] + [R(99999), R(100000), R(109999), R(120000)])
    rng = random.Random(690)
    for k in range(9):
        contigs = [AB, BA, ["c3", "c1", "c2"], ["dup", "dup", "x"]][k % 4]
        n_ref = len(contigs)
        chrom_id = rng.randrange(n_ref)
        start = rng.randrange(0, 50000)
        end = start + rng.randrange(0, 3000)
        centres = [rng.randrange(0, 400000) for _ in range(1 + k)]
        reads = []
        for _ in range(rng.randrange(20, 160)):
            flag = rng.choice(FLAGS8) | rng.choice((0, 1, 0x10, 0x41, 0x400))
            mtid = rng.choice([-1] + list(range(n_ref)) * 2 + [chrom_id] * 3)
            mpos = max(0, rng.choice(centres) + int(rng.gauss(0, 1) * rng.choice((10, 4000, 60000))))
            reads.append([flag, mtid, mpos])
        second = [[rng.choice([-1, chrom_id, chrom_id] + list(range(n_ref))), rng.choice((start - 1, start, end, end + 1, rng.randrange(max(start - 50, 0), end + 50)))] for _ in range(40)]
        add("random %d" % k, contigs, chrom_id, start, end, reads, second)
    return out


def main():
    if not os.path.isdir(REF):
        sys.exit("reference tree not found at %s: golden vectors can only be regenerated where it is" % REF)
    ns = namespace()
    done = []
    for c in cases():
        reader = types.SimpleNamespace(getrname=lambda tid, names=c["contigs"]: names[tid])
        coords = []
        for flag, mtid, mpos in c["reads"]:
            read = types.SimpleNamespace(bitFlag=flag, chromID=c["chrom_id"], mateChromID=mtid, matePos=mpos)
            ns["append_rule"](1, read, reader, coords)
        picked = [[t, p] for _, t, p in coords]
        off = []
        for flag, mtid, mpos in c["reads"]:                                  # (with the option off nothing is appended)
            ns["append_rule"](0, types.SimpleNamespace(bitFlag=flag, chromID=c["chrom_id"], mateChromID=mtid, matePos=mpos), reader, off)
        assert off == []
        ns["sort_coords"](coords)
        queries = ns["mergeQueries"](coords)
        mates = []
        for mtid, mpos in c["second"]:
            it = types.SimpleNamespace(b=types.SimpleNamespace(core=types.SimpleNamespace(mtid=mtid, mpos=mpos)))
            mates.append(1 if ns["is_mate"](it, c["chrom_id"], c["start"], c["end"]) else 0)
        done.append(dict(c, picked=picked, sorted=[[t, p] for _, t, p in coords], queries=[[n, s, e] for n, s, e in queries], is_mate=mates))
    labels = [c["label"] for c in done]
    assert len(set(labels)) == len(labels) and 28 <= len(done) <= 34, len(done)
    assert any(not c["picked"] for c in done) and any(len(c["queries"]) > 3 for c in done)
    assert any(sum(c["is_mate"]) for c in done) and any(0 in c["is_mate"] for c in done)
    path = os.path.join(HERE, "broken_mate_cases.json.gz")
    with gzip.GzipFile(path, "wb", mtime=0) as f:
        f.write(json.dumps(dict(cases=done), separators=(",", ":")).encode())
    print("broken mates: %d cases, %d reads, %d coordinates, %d queries, %d second-round records, %d bytes" % (
        len(done), sum(len(c["reads"]) for c in done), sum(len(c["picked"]) for c in done), sum(len(c["queries"]) for c in done),
        sum(len(c["second"]) for c in done), os.path.getsize(path)))


if __name__ == "__main__":
    main()
