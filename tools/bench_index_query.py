"""What a whole call's index queries cost (plat_index_query_batch, plat_index_query): 31 000 windows of 100 kb -- one pass of the whole-genome
job over one source file -- against a tabix index of the fixture's kind (a record every 20 kb with long END= records between, the VCF
written here and indexed by the library itself, plat_caller_index_bgzf), answered three ways:

    the device batch     plat_index_query as it stands: upload of the queries, seven kernels, the wait, the copy-back (plat_index_query_info.seconds)
    the host twin        the same call under PLAT_CALLER_HOST_INDEX=1: idxq::query (csrc/index_query.hpp) per query on one thread
    Python               platypus_amd.tabixindex.TabixIndex.query per query

Warmed (the first calls load code objects and grow buffers), then `--repeats` timed calls each, medians; the three must agree on every
chunk list.  A record, not a gate: the claim it supports or withdraws is host CPU time per region removed, not kernel speed.

    python tools/bench_index_query.py [--windows 31000] [--window 100000] [--contig-mb 240] [--out profiles/index_query.json]"""
import argparse
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HEADER = b"##fileformat=VCFv4.1\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n"


def source_text(contig_mb, seed=5):
    """Two contigs of contig_mb Mb: a record every 20 kb, an END= record of 100 kb .. 3 Mb behind every fourth (tests/index_query_cases.py's "wide")."""
    rng, out = random.Random(seed), [HEADER]
    for chrom in (b"1", b"2"):
        for i in range(contig_mb * 50):
            pos = 1000 + 20000 * i
            out.append(b"%s\t%d\t.\tA\tC\t.\t.\t.\n" % (chrom, pos))
            if i % 4 == 3:
                out.append(b"%s\t%d\t.\tA\t<DEL>\t.\t.\tEND=%d\n" % (chrom, pos + 7, pos + rng.choice((100000, 130000, 1000000, 3000000))))
    return b"".join(out)


def timed(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    v = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        r = fn()
        v.append((r if isinstance(r, float) else time.perf_counter() - t0) * 1e3)
    return dict(median_ms=round(statistics.median(v), 3), best_ms=round(min(v), 3), runs=repeats)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=31000)
    ap.add_argument("--window", type=int, default=100000)
    ap.add_argument("--contig-mb", type=int, default=240)
    ap.add_argument("--payload", type=int, default=4096, help="bytes of text per BGZF block of the source file")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "index_query.json"))
    a = ap.parse_args()
    from platypus_amd import fastcaller as F, synth, tabixindex
    packed = synth.bgzf_stream(source_text(a.contig_mb), a.payload, eof=True)[0]
    rng = random.Random(11)
    queries = [(rng.randrange(2), b, b + a.window) for b in (rng.randrange(a.contig_mb * 1000000) for _ in range(a.windows))]
    nc = F.NativeCaller(0, 1, 1)
    try:
        tbi = nc.index_bgzf(packed)
        mirror = tabixindex.TabixIndex(tbi)
        idx = nc.open_index(tbi)
        want, info = nc.query_index(idx, queries, info=True)
        res = dict(tool="bench_index_query", windows=a.windows, window=a.window, file_bytes=len(packed), tbi_bytes=len(tbi),
                   bins=sum(len(b) for b in mirror.bins), chunks=sum(len(c) for b in mirror.bins for c in b.values()), linear=sum(len(l) for l in mirror.linear),
                   chunks_returned=info["chunks"], handed_over=info["handed_over"], device_calls=info["device_calls"], warmup=a.warmup)
        call = lambda: nc.query_index(idx, queries, info=True)[1]["seconds"]
        res["device_batch"] = timed(call, a.warmup, a.repeats)
        t0 = time.perf_counter()
        call()
        res["device_batch_with_python_ms"] = round((time.perf_counter() - t0) * 1e3, 3)      # (the ctypes round trip and the lists made of the answer)
        os.environ["PLAT_CALLER_HOST_INDEX"] = "1"
        try:
            assert nc.query_index(idx, queries) == want
            res["host_twin"] = timed(call, 1, max(3, a.repeats // 2))
        finally:
            del os.environ["PLAT_CALLER_HOST_INDEX"]
        t0 = time.perf_counter()
        got = [mirror.query(*q) for q in queries]
        res["python_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
        assert got == want
        res["host_twin_us_per_query"] = round(res["host_twin"]["median_ms"] * 1e3 / a.windows, 3)
        res["device_us_per_query"] = round(res["device_batch"]["median_ms"] * 1e3 / a.windows, 3)
        res["python_us_per_query"] = round(res["python_ms"] * 1e3 / a.windows, 3)
        idx.close()
    finally:
        nc.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
