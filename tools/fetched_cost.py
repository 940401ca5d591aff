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

--bam: the three ways to hand fetched reads over, in one run: plat_call_fetched_regions on ASCII tables ("fetched_ascii") and on packed
tables ("fetched_packed"), and plat_call_bam_regions on the raw BAM alignment records of the same reads ("bam": ReadIterator.get on the
device, plat_bam_decode_batch) -- wall time, process CPU per region and input bytes of each.  The reads' `end` is the decode rule's
(a record holds none), for all three.  Under rocprofv3 the same run gives k_bam_core / k_bam_scan / k_bam_expand next to k_unpack_pieces
(the packed call expands a table of the same bases); "bam_expand_bytes" / "unpack_pieces_bytes" are their algorithmic bytes (3.5 and 3
per base).

--bgzf (with --bam): a fourth way, plat_call_bgzf_regions on the same records as BGZF blocks (zlib level --level, the same names and aux
data as "bam"): "bgzf" next to the three, with its link bytes (the compressed bytes), and "host_zlib": single-thread zlib inflate of the
same blocks on the host (seconds, bytes in and out) -- what the device takes off the CPU.  Under rocprofv3 the run gives k_bgzf_inflate,
k_bam_find and the other new kernels next to the decode's.

--read-groups (with --bam --bgzf): the merged-file calls.  The regions get --samples samples; "bam" and "bgzf" are the existing calls on the
pre-split samples (the baseline), "bam_rg" and "bgzf_rg" are plat_call_bam_regions_rg / plat_call_bgzf_regions_rg on the same reads as
ONE merged file per region, two read-group IDs per sample, every record carrying its RG field (the pre-split records carry it too: the
same bytes ride on the link) -- wall time, process CPU per region and link bytes of each, in one run.  --out FILE also writes the JSON
there.  Under rocprofv3 the run gives k_route_tag, k_route_hist, k_route_place and the route's scans next to k_bam_core.
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
    ap.add_argument("--bam", action="store_true", help="ASCII fetched, packed fetched and raw BAM records in one run")
    ap.add_argument("--bgzf", action="store_true", help="with --bam: the BGZF call on the same records, and host zlib inflate of the same blocks")
    ap.add_argument("--level", type=int, default=6, help="zlib level of the BGZF blocks")
    ap.add_argument("--read-groups", action="store_true", help="with --bam --bgzf: the merged-file calls next to the pre-split ones")
    ap.add_argument("--samples", type=int, default=3, help="samples per region of the --read-groups run")
    ap.add_argument("--out", help="also write the JSON line to this file")
    a = ap.parse_args()
    if a.read_groups:
        return rg_main(a)
    if a.bam or a.bgzf:
        return bam_main(a)
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


def bam_main(a):
    ascii_, packed, bam, bgzf, n_reads, n_bytes = [], [], [], [], 0, 0
    for i in range(a.regions):
        reg, samples = synth.config4_fetched_region(i, region_len=a.region_len)
        fasta = H.FastaFile({reg["chrom"]: reg["ref"].tobytes()})
        for rs in samples:
            for r in rs:                                                 # bam_endpos as plat_bam_decode_batch states it
                clip = r.cigarOps[0][1] if r.cigarOps and r.cigarOps[0][0] == 4 else 0
                r.end = r.pos + clip + (1 if (r.bitFlag & 4) or not r.cigarOps else sum(ln for op, ln in r.cigarOps if op in (0, 2, 3, 7, 8)))
            n_reads += len(rs)
            n_bytes += sum(r.rlen for r in rs)
        pairs = [(rs, []) for rs in samples]
        ascii_.append(F.FetchedRegion.from_reads(reg["chrom"], reg["start"], reg["end"], fasta, pairs))
        packed.append(F.FetchedRegion.from_reads(reg["chrom"], reg["start"], reg["end"], fasta, pairs, packed=True))
        # names as a sequencer writes them (~40 bytes) and an aux block of the usual tags' size: what rides along on the link
        names = [[("HWI-ST1234:100:C1ABCACXX:%d:%04d:%05d" % (1 + k % 8, k % 2316, k % 99991)).encode() + b"\0" for k in range(len(rs))] for rs in samples]
        aux = [[b"NMC\x00MDZ150\x00ASC\x96XSC\x00RGZgrp1\x00"] * len(rs) for rs in samples]
        bam.append(F.BamRegion(reg["chrom"], reg["start"], reg["end"], fasta._seq[reg["chrom"]],
                               [(synth.bam_records(rs, names=nm, aux=ax, block_size=True), synth.bam_records([])) for rs, nm, ax in zip(samples, names, aux)]))
        if a.bgzf:
            bgzf.append(F.BgzfRegion.from_reads(reg["chrom"], reg["start"], reg["end"], fasta, pairs, level=a.level, names=names[0], aux=aux[0]))
    nc = F.NativeCaller(0, a.workers, a.per_chunk)
    out = dict(regions=a.regions, region_len=a.region_len, reads=n_reads, read_bases=n_bytes)
    texts = {}
    try:
        for name, call, regs in (("fetched_ascii", nc.call_fetched_regions, ascii_), ("fetched_packed", nc.call_fetched_regions, packed),
                                 ("bam", nc.call_bam_regions, bam)) + ((("bgzf", nc.call_bgzf_regions, bgzf),) if a.bgzf else ()):
            best = None
            for _ in range(a.reps):
                o = default_options()
                w0, c0 = time.perf_counter(), time.process_time()
                texts[name] = call(regs, ["S1"], o)
                w, c = time.perf_counter() - w0, time.process_time() - c0
                if best is None or w < best[0]:
                    best = (w, c, nc.stats["n_windows_called"], nc.stats["input_bytes"])
            w, c, nw, ib = best
            out[name] = dict(seconds=w, windows_per_sec=nw / w, cpu_seconds_per_region=c / a.regions, windows=nw, text_bytes=len(texts[name]), input_bytes=ib)
        out["same_text"] = texts["bam"] == texts["fetched_ascii"] == texts["fetched_packed"]
        out["bam_expand_bytes"], out["unpack_pieces_bytes"] = int(3.5 * n_bytes), 3 * n_bytes
        if a.bgzf:
            import zlib
            out["same_text"] = out["same_text"] and texts["bgzf"] == texts["bam"]
            out["bgzf_level"] = a.level
            # single-thread zlib over the same blocks: the deflate data of every block, the CRC32 over its output
            blocks = []
            for reg in bgzf:
                for chunks, _ in reg.samples:
                    for d, _, _, _ in chunks:
                        d, at = d.tobytes(), 0
                        while at < len(d):
                            n = int.from_bytes(d[at + 16:at + 18], "little") + 1
                            blocks.append(d[at + 18:at + n - 8])
                            at += n
            best, n_out = None, 0
            for _ in range(a.reps):
                w0 = time.perf_counter()
                n_out = 0
                for b in blocks:
                    o = zlib.decompress(b, -15)
                    zlib.crc32(o)
                    n_out += len(o)
                w = time.perf_counter() - w0
                best = w if best is None or w < best else best
            n_in = sum(len(b) for b in blocks)
            out["host_zlib"] = dict(seconds=best, blocks=len(blocks), compressed_bytes=n_in, inflated_bytes=n_out, inflated_mb_per_sec=n_out / best / 1e6,
                                    seconds_per_region=best / a.regions)
    finally:
        nc.close()
    print(json.dumps(out))


def rg_main(a):
    pre_bam, pre_bgzf, rg_bam, rg_bgzf, n_reads, n_bytes = [], [], [], [], 0, 0
    nS = a.samples
    for i in range(a.regions):
        reg, samples = synth.config4_fetched_region(i, region_len=a.region_len, n_samples=nS)
        fasta = H.FastaFile({reg["chrom"]: reg["ref"].tobytes()})
        at = (reg["chrom"], reg["start"], reg["end"], fasta)
        for rs in samples:
            for r in rs:                                                 # bam_endpos as plat_bam_decode_batch states it
                clip = r.cigarOps[0][1] if r.cigarOps and r.cigarOps[0][0] == 4 else 0
                r.end = r.pos + clip + (1 if (r.bitFlag & 4) or not r.cigarOps else sum(ln for op, ln in r.cigarOps if op in (0, 2, 3, 7, 8)))
            n_reads += len(rs)
            n_bytes += sum(r.rlen for r in rs)
        # two read groups per sample: the first and the second half of its reads
        entries = [(k, "s%d.%s" % (k, ab), rs[:len(rs) // 2] if j == 0 else rs[len(rs) // 2:], []) for k, rs in enumerate(samples) for j, ab in enumerate("ab")]
        split = [F.merge_by_read_group([e[:3] for e in entries if e[0] == k], F._read_pos) for k in range(nS)]      # (reads, aux) per sample
        pre_bam.append(F.BamRegion(at[0], at[1], at[2], fasta._seq[at[0]], [(synth.bam_records(rs, aux=ax), synth.bam_records([])) for rs, ax in split]))
        ones = [F.BgzfRegion.from_reads(*at, [(rs, [])], level=a.level, aux=ax) for rs, ax in split]
        with_reads = [o for o, (rs, _) in zip(ones, split) if rs]
        itr = (with_reads[0].tid, min(o.itr_beg for o in with_reads), max(o.itr_end for o in with_reads)) if with_reads else (0, at[1], at[2])
        pre_bgzf.append(F.BgzfRegion(at[0], at[1], at[2], fasta._seq[at[0]], itr[0], itr[1], itr[2], [o.samples[0] for o in ones]))
        rg_bam.append(F.BamFileRegion.from_reads(*at, [entries]))
        rg_bgzf.append(F.BgzfFileRegion.from_reads(*at, [entries], level=a.level))
    groups = [("s%d.%s" % (k, ab), k) for k in range(nS) for ab in "ab"]
    names = ["S%d" % (k + 1) for k in range(nS)]
    nc = F.NativeCaller(0, a.workers, a.per_chunk)
    out = dict(regions=a.regions, region_len=a.region_len, samples=nS, read_groups=len(groups), reads=n_reads, read_bases=n_bytes, bgzf_level=a.level)
    texts = {}
    try:
        for name, call, regs in (("bam", lambda r, n, o: nc.call_bam_regions(r, n, o), pre_bam), ("bgzf", lambda r, n, o: nc.call_bgzf_regions(r, n, o), pre_bgzf),
                                 ("bam_rg", lambda r, n, o: nc.call_bam_regions_rg(r, groups, n, o), rg_bam),
                                 ("bgzf_rg", lambda r, n, o: nc.call_bgzf_regions_rg(r, groups, n, o), rg_bgzf)):
            best = None
            for _ in range(a.reps):
                o = default_options()
                w0, c0 = time.perf_counter(), time.process_time()
                texts[name] = call(regs, names, o)
                w, c = time.perf_counter() - w0, time.process_time() - c0
                if best is None or w < best[0]:
                    best = (w, c, nc.stats["n_windows_called"], nc.stats["input_bytes"])
            w, c, nw, ib = best
            out[name] = dict(seconds=w, windows_per_sec=nw / w, cpu_seconds_per_region=c / a.regions, windows=nw, text_bytes=len(texts[name]), input_bytes=ib)
        out["same_text"] = texts["bam"] == texts["bgzf"] == texts["bam_rg"] == texts["bgzf_rg"]
    finally:
        nc.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
