"""Generate tests/golden/tabix_index_cases.json.gz: the .tbi the reference's own ti_index_build writes for small bgzipped VCFs that
tests/golden/tabix_cases.json.gz lacks, and the files it exits on.

Runs only in the build container (needs the reference tree and gcc).  A driver of a few lines -- written here, it defines `pysamerr` and
calls ti_index_build, ti_open, ti_lazy_index_load, ti_queryi and ti_read -- is compiled in a scratch directory together with the
reference's src/tabix/{index,bgzf,kstring,knetfile}.c.pysam.c; nothing compiled from the reference and none of its text is kept.  The
texts are those of tests/tabix_index_cases.py (hand_texts: the corners of the rule), bgzipped by platypus_amd.synth.bgzf_stream at
payloads 65280 (a whole file inside one block) and 37 (every run across blocks), plus files laid out as the project's own output is: a
header piece and per-region pieces, every piece a whole number of blocks, the EOF block at the end.  Stored per case: the .vcf.gz bytes
and the .tbi bytes, or for a file the reference exits on its non-zero exit status and no .tbi.  At generation time the rule's mirror must
give the same parsed index, and the reference's reader (ti_queryi / ti_read) must return the same lines through the mirror's serialised
index as through its own.  tests/golden/README_tabix_index.md says what each case covers.

Usage:  python tests/golden/gen_golden_tabix_index.py [--reference DIR] [--scratch DIR] [--keep-scratch]
"""
import argparse
import base64
import gzip
import json
import os
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from platypus_amd import synth, tabixindex  # noqa: E402
from tests import tabix_index_cases as K  # noqa: E402
from tests.golden.gen_golden_tabix import DRIVER, parse_answers  # noqa: E402


def own_layout(payload):
    """A file as the command line writes it: the header a piece of its own, then each region's records, every piece whole blocks."""
    regions = [K._lines(*[K.L(b"r%d" % r, 1000 * r + 37 * k + 1, ref=b"ACG"[:1 + k % 3]) for k in range(40)]) for r in range(4)]
    regions.insert(2, b"")                                                   # (a region without records: no block)
    pieces = [K.HEADER] + regions
    return b"".join(synth.bgzf_stream(p, payload, eof=False)[0] for p in pieces if p) + synth.BGZF_EOF


def cases():
    out = []
    for label, text, line, kind in K.hand_texts():
        if kind == K.KIND_WIDE or label in ("an empty file", "only a header"):
            continue                                                        # (the reference does not exit on a wide POS: it narrows it)
        for payload in (65280, 37):
            out.append(("%s @%d" % (label, payload), synth.bgzf_stream(text, payload)[0], line is not None))
    for payload in (65280, 100):
        out.append(("the project's own layout @%d" % payload, own_layout(payload), False))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("PLATYPUS_REF", "/root/reference"))
    ap.add_argument("--scratch")
    ap.add_argument("--keep-scratch", action="store_true")
    a = ap.parse_args()
    scratch = a.scratch or tempfile.mkdtemp(prefix="tabix_index_golden_")
    os.makedirs(scratch, exist_ok=True)
    src = os.path.join(a.reference, "src", "tabix")
    with open(os.path.join(scratch, "drv.c"), "w") as f:
        f.write(DRIVER)
    drv = os.path.join(scratch, "drv")
    subprocess.check_call(["gcc", "-O1", "-w", "-I" + src, os.path.join(scratch, "drv.c")] + [os.path.join(src, n + ".c.pysam.c") for n in ("index", "bgzf", "kstring", "knetfile")] +
                          ["-o", drv, "-lz", "-lm"])
    stored, rows = [], []
    for k, (label, data, expect_refused) in enumerate(cases()):
        path = os.path.join(scratch, "c%d.vcf.gz" % k)
        with open(path, "wb") as f:
            f.write(data)
        r = subprocess.run([drv, "index", path], capture_output=True)
        st, raw = K.index_of(data)
        if r.returncode != 0:
            assert not os.path.exists(path + ".tbi") and expect_refused and st[K.ST_VERDICT] == K.ERR_BAD_INPUT, (label, r.returncode, r.stderr)
            stored.append({"label": label, "vcf_gz": base64.b64encode(data).decode(), "tbi": None, "refused": True, "exit": r.returncode})
            rows.append((label, len(data), "exit %d, line %d" % (r.returncode, st[K.ST_LINE])))
            continue
        assert not expect_refused and st[K.ST_VERDICT] == 0, label
        with open(path + ".tbi", "rb") as f:
            tbi = f.read()
        theirs, ours = tabixindex.TabixIndex(tbi), tabixindex.TabixIndex(gzip.compress(raw))
        assert K.parsed(ours) == K.parsed(theirs), label
        # the reference's reader over its own index and over the mirror's
        asked = [(t, b, e) for t in range(len(theirs.names)) for b, e in [(0, 1 << 29), (0, 50), (99, 121), (39999, 50011)] + [(16384 * w, 16384 * (w + 1)) for w in range(4)]]
        ask = "".join("%d %d %d\n" % q for q in asked).encode()
        own = parse_answers(subprocess.run([drv, "query", path], input=ask, capture_output=True, check=True).stdout)
        twin = os.path.join(scratch, "m%d.vcf.gz" % k)
        shutil.copy(path, twin)
        with open(twin + ".tbi", "wb") as f:
            f.write(synth.bgzf_stream(raw)[0])
        assert parse_answers(subprocess.run([drv, "query", twin], input=ask, capture_output=True, check=True).stdout) == own, label
        stored.append({"label": label, "vcf_gz": base64.b64encode(data).decode(), "tbi": base64.b64encode(tbi).decode(), "refused": False, "exit": 0})
        rows.append((label, len(data), "%d contigs, %d bins, %d windows, %d lines over %d queries" % (
            len(theirs.names), sum(len(b) for b in theirs.bins), sum(len(l) for l in theirs.linear), sum(len(x) for x in own), len(asked))))
    out = os.path.join(HERE, "tabix_index_cases.json.gz")
    with gzip.GzipFile(out, "wb", mtime=0) as f:
        f.write(json.dumps({"cases": stored}, sort_keys=True).encode())
    with open(os.path.join(HERE, "README_tabix_index.md"), "w") as f:
        f.write("# tabix_index_cases.json.gz\n\nWritten by `gen_golden_tabix_index.py`: bgzipped VCFs with the `.tbi` the reference's `ti_index_build` wrote for each, or its\n"
                "non-zero exit and no `.tbi`.  `tests/tabix_index_cases.py` (`hand_texts`, `golden_cases`) holds the texts and the loader.\n\n| case | bytes | the reference |\n|---|---|---|\n")
        for row in rows:
            f.write("| %s | %d | %s |\n" % row)
    print(out, os.path.getsize(out), "bytes,", len(stored), "cases")
    if not a.keep_scratch and not a.scratch:
        shutil.rmtree(scratch)


if __name__ == "__main__":
    main()
