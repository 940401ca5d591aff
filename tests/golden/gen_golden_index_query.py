"""Generate tests/golden/index_query_cases.json.gz: the chunk lists the reference's own ti_iter_query returns over indexes its own
ti_index_build wrote.

Runs only in the build container (needs the reference tree and gcc).  A driver of a few lines -- written here; it defines `pysamerr`,
includes the reference's index source so that it can read the iterator's chunk list, and calls ti_index_build, ti_index_load_local and
ti_iter_query -- is compiled in a scratch directory together with the reference's src/tabix/{bgzf,kstring,knetfile}.c.pysam.c; nothing
compiled from the reference and none of its text is kept.  The VCFs are written by tests/index_query_cases.py (fixture_texts) and bgzipped
by platypus_amd.synth.bgzf_stream at small block payloads; they are not stored.  Stored per file: the .tbi bytes ti_index_build wrote,
the queries (tid, beg, end) and per query the chunk list (u, v) the iterator held, or null where ti_iter_query returned no iterator.
At generation time platypus_amd.tabixindex.TabixIndex.query must return the same lists.  README_index_query.md says what each file covers.

Usage:  python tests/golden/gen_golden_index_query.py [--reference DIR] [--scratch DIR] [--keep-scratch]
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
from tests import index_query_cases as Q  # noqa: E402

DRIVER = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "index.c.pysam.c"
FILE* pysamerr;
int main(int argc, char** argv) {
    pysamerr = stderr;
    if (argc < 3) return 9;
    if (!strcmp(argv[1], "index")) return ti_index_build(argv[2], &ti_conf_vcf) ? 3 : 0;
    ti_index_t* idx = ti_index_load_local(argv[2]);
    if (!idx) return 2;
    int tid, beg, end, i;
    while (scanf("%d %d %d", &tid, &beg, &end) == 3) {        /* one query per line of stdin */
        ti_iter_t it = ti_iter_query(idx, tid, beg, end);
        if (!it) { printf("Q -1\n"); continue; }
        printf("Q %d\n", it->n_off);
        for (i = 0; i < it->n_off; ++i) printf("%llu %llu\n", (unsigned long long)it->off[i].u, (unsigned long long)it->off[i].v);
        ti_iter_destroy(it);
    }
    ti_index_destroy(idx);
    return 0;
}
"""


def run(cmd, **kw):
    r = subprocess.run(cmd, capture_output=True, **kw)
    if r.returncode != 0:
        raise RuntimeError("%s failed (%d):\n%s" % (" ".join(cmd), r.returncode, r.stderr.decode("latin-1")[-2000:]))
    return r.stdout


def parse_answers(out):
    answers, lines, at = [], out.decode().split("\n"), 0
    while at < len(lines) and lines[at]:
        n = int(lines[at].split()[1])
        at += 1
        if n < 0:
            answers.append(None)
            continue
        answers.append([tuple(int(x) for x in lines[at + k].split()) for k in range(n)])
        at += n
    return answers


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("PLATYPUS_REF", "/root/reference"))
    ap.add_argument("--scratch")
    ap.add_argument("--keep-scratch", action="store_true")
    a = ap.parse_args()
    scratch = a.scratch or tempfile.mkdtemp(prefix="index_query_golden_")
    os.makedirs(scratch, exist_ok=True)
    src = os.path.join(a.reference, "src", "tabix")
    with open(os.path.join(scratch, "drv.c"), "w") as f:
        f.write(DRIVER)
    drv = os.path.join(scratch, "drv")
    run(["gcc", "-O1", "-w", "-I" + src, os.path.join(scratch, "drv.c")] + [os.path.join(src, n + ".c.pysam.c") for n in ("bgzf", "kstring", "knetfile")] +
        ["-o", drv, "-lz", "-lm"])
    files, rows = [], []
    for k, (label, payload, text) in enumerate(Q.fixture_texts()):
        data, _ = synth.bgzf_stream(text, payload)
        path = os.path.join(scratch, "f%d.vcf.gz" % k)
        with open(path, "wb") as f:
            f.write(data)
        run([drv, "index", path])
        with open(path + ".tbi", "rb") as f:
            tbi = f.read()
        index = tabixindex.TabixIndex(tbi)
        asked = Q.fixture_queries(label, index)
        got = parse_answers(run([drv, "query", path + ".tbi"], input="".join("%d %d %d\n" % q for q in asked).encode()))
        assert len(got) == len(asked)
        gathered = []
        for q, chunks in zip(asked, got):
            mine = index.query(*q)
            assert mine == chunks, (label, q, mine and mine[:3], chunks and chunks[:3])
            gathered.append(Q.gathered_of(index, *q))
        assert max(gathered) <= Q.MAX_CHUNKS, (label, max(gathered))
        files.append({"label": label, "payload": payload, "tbi": base64.b64encode(tbi).decode(),
                      "queries": [{"tid": q[0], "beg": q[1], "end": q[2], "chunks": c} for q, c in zip(asked, got)]})
        rows.append((label, payload, len(text), len(tbi), sum(len(b) for b in index.bins), sum(len(c) for b in index.bins for c in b.values()), gathered,
                     [None if c is None else len(c) for c in got]))
        print("%-8s %8d bytes of text, %6d of index, %d queries, gathered %s" % (label, len(text), len(tbi), len(asked), gathered))
    out = os.path.join(HERE, "index_query_cases.json.gz")
    with gzip.GzipFile(out, "wb", mtime=0) as f:
        f.write(json.dumps({"files": files}, sort_keys=True).encode())
    print(out, os.path.getsize(out), "bytes")
    with open(os.path.join(HERE, "README_index_query.md"), "w") as f:
        f.write("# index_query_cases.json.gz\n\nWritten by `gen_golden_index_query.py`: `.tbi` files the reference's `ti_index_build` wrote for bgzipped VCFs made by\n"
                "`tests/index_query_cases.py` (`fixture_texts`; the VCFs are not stored), queries, and per query the chunk list the reference's\n"
                "`ti_iter_query` returned (`null`: no iterator).  `tests/index_query_cases.py` (`golden_files`) is the loader.\n\n"
                "| file | block payload | text bytes | `.tbi` bytes | bins | chunks | gathered per query | chunks returned per query |\n|---|---|---|---|---|---|---|---|\n")
        for r in rows:
            f.write("| %s | %d | %d | %d | %d | %d | %s | %s |\n" % (r[0], r[1], r[2], r[3], r[4], r[5], " ".join(map(str, r[6])), " ".join("-" if x is None else str(x) for x in r[7])))
        f.write("\nThe queries cover: nothing touched, `beg == end`, `end < beg`, `beg < 0`, `end` beyond 2^29, `beg >> 14` at and beyond the linear\n"
                "index's length, one 16 kb bin, about 13 bins, 60-70 gathered chunks, about 1500 gathered chunks, and whole contigs.\n\n"
                "Caveat: the reference's indexer never writes a chunk contained in another, chunks tied in `u`, or zero-length chunks, and its linear\n"
                "index has no zero entry above a non-zero one.  Those corners of the rule are made by hand (`tests/index_query_cases.py`, `hand_cases`)\n"
                "and checked against `platypus_amd/tabixindex.py`, which this file pins to the reference first.\n")
    if not a.keep_scratch and not a.scratch:
        shutil.rmtree(scratch)


if __name__ == "__main__":
    main()
