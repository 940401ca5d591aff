"""What the broken-mate fetch of whole BAM files costs (plat_bam_mates_batch, plat_bam_files_mates_plan, plat_call_bam_files_mates): a
seeded BAM file of --records records (default 10^5) of 100 bases on one contig, --improper of them (default 5 %) improper pairs whose
mates lie 150 kb further on, is written in memory with its .bai and called in regions of --region-len bases.

    the device pass      plat_bam_mates_batch alone over the file's records, resident on the device, in both modes: the call's three
                         launches between two device events, and plat_kernel_times for the timer they run under (PLAT_KT_OTHER: the three
                         kernels share it, so the figure is their sum; launches says how many were timed), after a warm-up, median of
                         --repeats.  Bytes touched are computed from the shapes -- per pass and record 16 bytes of offsets and the 64-byte
                         line that holds its 10 bytes of fixed fields, twice (count and write), plus what is written (and, in FETCH mode,
                         read and written for the kept records) -- and given over that time and as a share of the HBM peak (8.0 TB/s, the
                         specification's figure).  No threshold: COORDS reads 12 bytes at record stride and sits far from the peak
    the plan and the call   plat_bam_files_mates_plan's wall time (plat_bam_mates_plan.seconds) next to the whole
                         plat_call_bam_files_mates and next to the BGZF call that follows it (the difference)
    options off          plat_call_bam_files_mates against plat_call_bam_files with assembleBrokenPairs = 0 on the same file, alternating,
                         with the run-to-run spread of each: the same launches (tests/test_gpu_bam_mates.py), so the two must overlap
                         within that spread.  --label names the code the figures belong to (any name: this, parent, head_2 ...): a run
                         of another build adds its own entry to the same file (options_off, and runs: the plan and the call too)

One process, one GPU; a record, not a bar.

    python tools/bam_mates_bench.py [--records 100000] [--improper 0.05] [--repeats 5] [--label this] [--out profiles/bam_mates.json]"""
import argparse
import json
import os
import statistics
import struct
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12
KT_OTHER = 31
READ = 100


def seeded_file(n_records, improper, seed=17):
    """(built file, contig bytes, regions' span): n_records reads of READ bases that copy the contig, every 1/improper-th the first read of an
    improper pair whose mate lies 150 kb further on, or such a mate, pointing back."""
    from tests import bam_file_cases as B
    rng = np.random.default_rng(seed)
    span = n_records * 10                                                     # 10x coverage of READ-base reads
    contig = bytes(b"ACGT"[int(v)] for v in rng.integers(0, 4, span + 200000))
    every = max(int(round(2 / improper)), 2)                                 # half of the improper reads point forward, half are their mates and point back
    cig = struct.pack("<I", READ << 4)
    qual = bytes([35] * READ)
    code = bytes.maketrans(b"ACGT", bytes([1, 2, 4, 8]))
    recs = []
    for i in range(n_records):
        pos = i * 10
        codes = np.frombuffer(contig[pos:pos + READ].translate(code), dtype=np.uint8)
        seq = ((codes[0::2] << 4) | codes[1::2]).tobytes()
        flag, mpos = 0x43, pos + 200
        if i % every == 0:
            flag, mpos = 0x41, pos + 150000
        elif i % every == 1 and pos >= 150000:
            flag, mpos = 0x81, pos - 150000 - 10
        name = b"r%d\0" % i
        rec = struct.pack("<iiBBHHHiiii", 0, pos, len(name), 60, 0, 1, flag, READ, 0, mpos, 0) + name + cig + seq + qual
        recs.append(struct.pack("<i", len(rec)) + rec)
    refs = [("chr1", len(contig))]
    text = "@HD\tVN:1.4\tSO:coordinate\n" + B.sq_lines(refs) + "@RG\tID:g\tSM:S\n"
    return B.built(dict(name="bench.bam", text=text, refs=refs, records=recs), block_payload=0xff00), contig, span


def device_pass(eng, f, mode, warmup, repeats):
    import torch
    blob = np.frombuffer(b"".join(f["records"]), dtype=np.uint8)
    ln = np.array([len(r) for r in f["records"]], dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(ln)])[:-1] + 4
    lim = off - 4 + ln
    n = len(off)
    begin = np.array([0, n], dtype=np.int32)
    want, lo, hi = np.zeros(1, np.int32), np.full(1, 140000, np.int32), np.full(1, 400000, np.int32)
    eng.lib.plat_kernel_timer_only(eng.ctx, KT_OTHER)
    ms, kt, out = [], [], None
    for k in range(warmup + repeats):
        eng.lib.plat_kernel_times(eng.ctx, (C_double * 32)(), (C_int64 * 32)())    # (drop what is pending)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        out = eng.bam_mates(blob, off, lim, begin, mode, want, lo, hi)
        t1.record()
        torch.cuda.synchronize(eng.device)
        a, b = (C_double * 32)(), (C_int64 * 32)()
        eng.lib.plat_kernel_times(eng.ctx, a, b)
        if k >= warmup:
            ms.append(t0.elapsed_time(t1))
            kt.append((a[KT_OTHER], b[KT_OTHER]))
    eng.lib.plat_kernel_timer_only(eng.ctx, -1)
    kept, kept_bytes = int(out["status"][2]), int(out["need_bytes"])
    touched = 2 * n * (16 + 64) + (kept * 8 if mode == "coords" else kept * 16 + 2 * kept_bytes)
    med = statistics.median(t for t, _ in kt)
    return dict(records=n, kept=kept, kept_bytes=kept_bytes, kernels_ms_median=round(med, 4), kernels_ms_best=round(min(t for t, _ in kt), 4), launches=int(kt[-1][1]),
                call_with_transfers_ms_median=round(statistics.median(ms), 3), bytes_touched=touched, tb_per_s=round(touched / (med * 1e-3) / 1e12, 4),
                share_of_hbm_peak=round(touched / (med * 1e-3) / HBM_PEAK, 4)) if med > 0 else dict(records=n, kept=kept, not_timed=True)


def spread(xs):
    return dict(median_s=round(statistics.median(xs), 4), min_s=round(min(xs), 4), max_s=round(max(xs), 4), runs=len(xs))


def main():
    global C_double, C_int64
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=100000)
    ap.add_argument("--improper", type=float, default=0.05)
    ap.add_argument("--region-len", type=int, default=100000)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--label", default="this")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bam_mates.json"))
    a = ap.parse_args()
    import ctypes as C
    C_double, C_int64 = C.c_double, C.c_int64
    from platypus_amd import fastcaller as F
    from platypus_amd.engine import Engine
    from platypus_amd.options import default_options
    f, contig, span = seeded_file(a.records, a.improper)
    res = dict(tool="bam_mates_bench", records=a.records, improper=a.improper, file_bytes=len(f["bam"]), region_len=a.region_len, warmup=a.warmup, repeats=a.repeats)
    has_mates = hasattr(F.load(), "plat_call_bam_files_mates")
    if has_mates:
        eng = Engine(0)
        res["device_pass"] = {mode: device_pass(eng, f, mode, a.warmup, a.repeats) for mode in ("coords", "fetch")}
    regions = [F.BamFilesRegion("chr1", s, min(s + a.region_len, span), contig) for s in range(0, span, a.region_len)]
    nc = F.NativeCaller(0, 4, 4)
    try:
        h = nc.open_bam(f["bam"], f["bai"], f["name"])
        on, off = dict(assemble=1, assembleBrokenPairs=1, maxReads=10 ** 9), dict(assemble=1, assembleBrokenPairs=0, maxReads=10 ** 9)
        nc.call_bam_files([h], regions, default_options(**off))             # warm-up
        plain, mates, whole, plan = [], [], [], []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            text = nc.call_bam_files([h], regions, default_options(**off))
            plain.append(time.perf_counter() - t0)
            if has_mates:
                t0 = time.perf_counter()
                assert nc.call_bam_files_mates([h], regions, default_options(**off)) == text
                mates.append(time.perf_counter() - t0)
        if has_mates:
            for _ in range(a.repeats):
                t0 = time.perf_counter()
                nc.call_bam_files_mates([h], regions, default_options(**on))
                whole.append(time.perf_counter() - t0)
                nc.bam_mates_plan([h], [(r.chrom, r.start, r.end) for r in regions], default_options(**on))
                plan.append(nc.bam_mates_info["seconds"])
            info = {k: v for k, v in nc.bam_mates_info.items() if k != "loaded"}
            res["plan_and_call"] = dict(plan=spread(plan), whole_call=spread(whole), bgzf_call_behind_it_median_s=round(statistics.median(whole) - statistics.median(plan), 4),
                                        counters=info)
        entry = dict(call_bam_files=spread(plain))
        if has_mates:
            entry["call_bam_files_mates"] = spread(mates)
            entry["overlap"] = max(min(plain), min(mates)) <= min(max(plain), max(mates))
        h.close()
    finally:
        nc.close()
    old, runs = {}, {}
    if a.out and os.path.exists(a.out):
        with open(a.out) as fh:
            prev = json.loads(fh.read() or "{}")
        old, runs = prev.get("options_off", {}), prev.get("runs", {})
    res["options_off"] = dict(old, **{a.label: entry})
    res["runs"] = dict(runs, **{a.label: dict(plan_and_call=res.get("plan_and_call"), options_off=entry)})       # every label's own figures, whichever ran last
    if not any(k.startswith("parent") for k in res["options_off"]):
        res["options_off"]["parent"] = "not measured"
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
