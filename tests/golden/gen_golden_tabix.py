"""Generate tests/golden/tabix_cases.json.gz: what the reference's own tabix returns for queries over small bgzipped VCFs.

Runs only in the build container (needs the reference tree and gcc).  A driver of a few lines -- written here, it defines `pysamerr` and
calls ti_index_build, ti_open, ti_lazy_index_load, ti_queryi and ti_read -- is compiled in a scratch directory together with the
reference's src/tabix/{index,bgzf,kstring,knetfile}.c.pysam.c; nothing compiled from the reference and none of its text is kept.  The
VCFs are written here and bgzipped by platypus_amd.synth.bgzf_stream at chosen block payloads, so that lines span blocks and end exactly
on block ends.  Stored per file: the .vcf.gz bytes, the .tbi bytes ti_index_build wrote, the index's names, and per query (tid, beg, end)
the lines ti_read returned; and, for the command line's test, a source VCF of the SNPs planted in the synthetic regions of config 4 with
its .tbi ("cli").  tests/golden/README_tabix.md says what each file covers.

Usage:  python tests/golden/gen_golden_tabix.py [--reference DIR] [--scratch DIR] [--keep-scratch]
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

DRIVER = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "tabix.h"
FILE* pysamerr;
int main(int argc, char** argv) {
    pysamerr = stderr;
    if (argc < 3) return 9;
    if (!strcmp(argv[1], "index")) return ti_index_build(argv[2], &ti_conf_vcf) ? 3 : 0;
    tabix_t* t = ti_open(argv[2], 0);
    if (!t || ti_lazy_index_load(t) < 0) return 2;
    int tid, beg, end;
    while (scanf("%d %d %d", &tid, &beg, &end) == 3) {        /* one query per line of stdin */
        ti_iter_t it = ti_queryi(t, tid, beg, end);
        const char* s;
        int len;
        printf("Q\n");
        while (it && (s = ti_read(t, it, &len)) != 0) { printf("L %d\n", len); fwrite(s, 1, (size_t)len, stdout); printf("\n"); }
        if (it) ti_iter_destroy(it);
    }
    printf("E\n");
    ti_close(t);
    return 0;
}
"""

HEADER = b"##fileformat=VCFv4.1\n##source=gen_golden_tabix\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + b"\t".join(b"S%d" % i for i in range(6)) + b"\n"


def line(chrom, pos, ref=b"A", alt=b"C", info=b"DP=10", samples=6, pad=0):
    gt = b"\t".join(b"0/1:%d" % (7 * i % 50) for i in range(samples))
    return b"\t".join([chrom, pos, b".", ref, alt, b"50", b"PASS", info + (b";P=" + b"p" * pad if pad else b""), b"GT:DP", gt]) + b"\n"


def pad_to_block(text, payload, make):
    """make(pad) appended to text with the pad chosen so that the line ends exactly on a block end."""
    for pad in range(1, payload + 2):
        if (len(text) + len(make(pad))) % payload == 0:
            return text + make(pad)
    raise AssertionError("no pad fits")


def body(payload, long_lines, last_newline=True):
    """Three contigs whose names are prefixes of each other; positions over several 16 kb bins; the corners README_tabix.md lists."""
    t = HEADER
    t = pad_to_block(t, payload, lambda pad: line(b"2", b"100", pad=pad))
    t += line(b"2", b"5000", info=b"SVTYPE=DEL;END=90000") + line(b"2", b"7000") + line(b"2", b"20000", ref=b"ACGT") + line(b"2", b"70500")
    t += line(b"2", b"70600", info=b"END=70900") + line(b"2", b"70700", info=b"SVEND=7") + line(b"2", b"70800", info=b"CIEND=1;END=7")
    t += b"#a meta line inside the data\n"
    t += line(b"2", b"131072") + line(b"2", b"300000")
    # POS forms: 0 (b = 0), 010 (octal 8), " 12", 0x10 (16); an empty REF
    t += line(b"20", b"0") + line(b"20", b"010") + line(b"20", b" 12", ref=b"") + line(b"20", b"0x10")
    t = pad_to_block(t, payload, lambda pad: line(b"20", b"200", pad=pad))
    for p in range(205, 230, 5):
        t += line(b"20", b"%d" % p, ref=b"A" * (1 + p % 4))
    if long_lines >= 1:
        t += line(b"20", b"16000", samples=300)                          # longer than 1024 bytes
    if long_lines >= 2:
        t += line(b"20", b"16500", samples=14000)                        # longer than 65536 bytes
    t += b"#another one\n"
    t += line(b"20", b"17000", info=b"END=40000;DP=3") + line(b"20", b"33000") + line(b"20", b"49152") + line(b"20", b"1000000")
    t += line(b"20_alt", b"50") + line(b"20_alt", b"16384") + line(b"20_alt", b"16385", ref=b"AC")
    return t if last_newline else t[:-1]


QUERIES = [  # (name, beg, end), 0-based half-open
    (b"2", 0, 50), (b"2", 99, 100), (b"2", 100, 101), (b"2", 6999, 7001), (b"2", 8000, 8100), (b"2", 70000, 71000), (b"2", 89999, 90001), (b"2", 90000, 90001),
    (b"2", 131071, 131073), (b"2", 299999, 400000), (b"2", 400000, 500000), (b"2", 0, 1 << 29),
    (b"20", 0, 1), (b"20", 7, 8), (b"20", 8, 9), (b"20", 11, 12), (b"20", 15, 16), (b"20", 199, 215), (b"20", 210, 211), (b"20", 15999, 16001),
    (b"20", 16499, 16500), (b"20", 30000, 30001), (b"20", 32999, 49153), (b"20", 999999, 1000000), (b"20", 1000000, 2000000), (b"20", 0, 1 << 29),
    (b"20_alt", 0, 49), (b"20_alt", 49, 50), (b"20_alt", 16383, 16386), (b"20_alt", 16386, 20000), (b"20_alt", 0, 1 << 29),
]
FILES = [("payload 65280, a line over 64 KiB", 65280, 2, True), ("payload 100", 100, 1, True), ("payload 37, no last newline", 37, 0, False)]


def run(cmd, **kw):
    r = subprocess.run(cmd, capture_output=True, **kw)
    if r.returncode != 0:
        raise RuntimeError("%s failed (%d):\n%s" % (" ".join(cmd), r.returncode, r.stderr.decode("latin-1")[-2000:]))
    return r.stdout


def parse_answers(out):
    queries, at = [], 0
    while True:
        nl = out.index(b"\n", at)
        tag = out[at:nl]
        at = nl + 1
        if tag == b"E":
            return queries
        if tag == b"Q":
            queries.append([])
            continue
        n = int(tag[2:])
        queries[-1].append(out[at:at + n])
        assert out[at + n:at + n + 1] == b"\n"
        at += n + 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("PLATYPUS_REF", "/root/reference"))
    ap.add_argument("--scratch")
    ap.add_argument("--keep-scratch", action="store_true")
    a = ap.parse_args()
    scratch = a.scratch or tempfile.mkdtemp(prefix="tabix_golden_")
    os.makedirs(scratch, exist_ok=True)
    src = os.path.join(a.reference, "src", "tabix")
    with open(os.path.join(scratch, "drv.c"), "w") as f:
        f.write(DRIVER)
    drv = os.path.join(scratch, "drv")
    run(["gcc", "-O1", "-w", "-I" + src, os.path.join(scratch, "drv.c")] + [os.path.join(src, n + ".c.pysam.c") for n in ("index", "bgzf", "kstring", "knetfile")] +
        ["-o", drv, "-lz", "-lm"])
    files = []
    for label, payload, long_lines, last_newline in FILES:
        text = body(payload, long_lines, last_newline)
        data, _ = synth.bgzf_stream(text, payload)
        path = os.path.join(scratch, "f%d.vcf.gz" % payload)
        with open(path, "wb") as f:
            f.write(data)
        run([drv, "index", path])
        with open(path + ".tbi", "rb") as f:
            tbi = f.read()
        index = tabixindex.TabixIndex(tbi)
        asked = [(index.tid(n), b, e) for n, b, e in QUERIES]
        got = parse_answers(run([drv, "query", path], input="".join("%d %d %d\n" % q for q in asked).encode()))
        assert len(got) == len(asked)
        files.append({"label": label, "payload": payload, "vcf_gz": base64.b64encode(data).decode(), "tbi": base64.b64encode(tbi).decode(),
                      "names": [n.decode("latin-1") for n in index.names],
                      "queries": [{"tid": q[0], "beg": q[1], "end": q[2], "lines": [x.decode("latin-1") for x in lines]} for q, lines in zip(asked, got)]})
        print("%-36s %7d bytes of text, %6d compressed, %5d of index, %d queries, %d lines returned" %
              (label, len(text), len(data), len(tbi), len(asked), sum(len(x) for x in got)))
    # for the command line's test: the SNPs planted in the two regions of `--synthetic=config4:2 --bufferSize 4000` as a source VCF
    known = b"##fileformat=VCFv4.1\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n"
    for i in range(2):
        r = synth.config4_region_arrays(i, region_len=4000, n_samples=1, read_len=150)      # (the native loop's generator)
        for pos, removed, added in r["variants"]:
            if len(removed) == len(added) == 1:
                known += b"\t".join([r["chrom"].encode(), b"%d" % (pos + 1), b".", removed, added, b".", b".", b"."]) + b"\n"
    data, _ = synth.bgzf_stream(known, 100)
    path = os.path.join(scratch, "known.vcf.gz")
    with open(path, "wb") as f:
        f.write(data)
    run([drv, "index", path])
    with open(path + ".tbi", "rb") as f:
        cli = {"vcf": known.decode(), "vcf_gz": base64.b64encode(data).decode(), "tbi": base64.b64encode(f.read()).decode()}
    out = os.path.join(HERE, "tabix_cases.json.gz")
    with gzip.GzipFile(out, "wb", mtime=0) as f:
        f.write(json.dumps({"files": files, "cli": cli}, sort_keys=True).encode())
    print(out, os.path.getsize(out), "bytes")
    if not a.keep_scratch and not a.scratch:
        shutil.rmtree(scratch)


if __name__ == "__main__":
    main()
