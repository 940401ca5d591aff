#!/usr/bin/env python3
"""What the loader's work on the device costs: plat_call_fetched_regions (reads as a fetch returns them: QC, split and gather on the
device in front of the loop) against plat_call_regions on the same reads split beforehand (hostapi.checkAndTrimReads), on synthetic
config-4 regions with the loader's trouble injected (synth.config4_fetched_region).  Prints one JSON line: windows/s, process CPU
seconds per region and the input bytes (bases and qualities over the link) of both calls (best of --reps), and the bytes
plat_read_buffers_batch reads.  --packed: both calls take PLAT_READS_PACKED tables (one byte per base; the fetched call then runs
plat_read_buffers_packed_batch).

The kernels on their own (k_read_qc or k_read_qc_packed, k_read_split, k_read_gather against the chunk's other kernels), in a run of
their own:
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/fetched_cost.py --reps 1 [--packed]
"""
import argparse
import copy
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from platypus_amd import fastcaller as F, hostapi as H, synth  # noqa: E402
from platypus_amd.options import default_options  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=8)
    ap.add_argument("--region-len", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--workers", type=int, default=4)
    ap.add_argument("--per-chunk", type=int, default=4)
    ap.add_argument("--packed", action="store_true", help="PLAT_READS_PACKED tables for both calls")
    a = ap.parse_args()
    opts = default_options()
    enabled = (opts.filterReadsWithUnmappedMates, opts.filterReadsWithDistantMates, opts.filterReadPairsWithSmallInserts, opts.filterDuplicates)
    fetched, split, n_reads, n_bytes = [], [], 0, 0
    for i in range(a.regions):
        reg, samples = synth.config4_fetched_region(i, region_len=a.region_len)
        fasta = H.FastaFile({reg["chrom"]: reg["ref"].tobytes()})
        fetched.append(F.FetchedRegion.from_reads(reg["chrom"], reg["start"], reg["end"], fasta, [(rs, []) for rs in samples], packed=a.packed))
        bufs = []
        for rs in samples:
            rs = copy.deepcopy(rs)
            n_reads += len(rs)
            n_bytes += sum(r.rlen for r in rs)
            ok, _ = H.checkAndTrimReads(rs, opts, enabled)
            bufs.append(H.bamReadBuffer([r for r, g in zip(rs, ok) if g], [r for r, g in zip(rs, ok) if not g], []))
        split.append(F.RegionReads.from_buffers(reg["chrom"], reg["start"], reg["end"], fasta, bufs, packed=a.packed))
    nc = F.NativeCaller(0, a.workers, a.per_chunk)
    out = dict(regions=a.regions, region_len=a.region_len, reads=n_reads, read_bases=n_bytes, packed=a.packed)
    try:
        for name, call, regs in (("pre_split", nc.call_regions, split), ("fetched", nc.call_fetched_regions, fetched)):
            best = None
            for _ in range(a.reps):
                o = default_options()
                w0, c0 = time.perf_counter(), time.process_time()
                txt = call(regs, ["S1"], o)
                w, c = time.perf_counter() - w0, time.process_time() - c0
                if best is None or w < best[0]:
                    best = (w, c, nc.stats["n_windows_called"], len(txt), nc.stats["input_bytes"])
            w, c, nw, nt, ib = best
            out[name] = dict(seconds=w, windows_per_sec=nw / w, cpu_seconds_per_region=c / a.regions, windows=nw, text_bytes=nt, input_bytes=ib)
        # QC reads qualities, flags and the per-read fields once and writes trimmed qualities in place; the gather reads bases, qualities
        # and CIGARs once more and writes them once (algorithmic bytes, not measured traffic)
        # (packed: one byte per base for both, the gather's bases and qualities in one byte; exceptions left out)
        out["read_buffers_bytes"] = dict(qc=n_bytes + 40 * n_reads, split=20 * n_reads, gather=(2 if a.packed else 4) * n_bytes + 60 * n_reads)
        out["same_text"] = out["pre_split"]["text_bytes"] == out["fetched"]["text_bytes"]
    finally:
        nc.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
