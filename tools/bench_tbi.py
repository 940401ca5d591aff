"""What the tabix index of the compressed output costs (plat_tabix_index_batch, plat_caller_index_bgzf): tools/bench_bgzf_out.py's record
text (a few thousand config-4 regions, taken several times over with the contigs renamed so that the file stays sorted), compressed by
plat_caller_compress_text behind a header piece, then indexed
  * on the device through plat_caller_index_bgzf (chain walk, one upload, inflate and index kernels, copies back, finishing stage);
  * split between HIP events into upload, inflate and index kernels, all buffers resident, the rest of the call by subtraction;
  * by the host twin (PLAT_CALLER_HOST_TBI=1): one core inflating and walking every byte, the bar the device path is compared with.
Every timing: `warmup` runs thrown away, then `repeats` runs; median and best are kept.  Prints one JSON line and writes it to --out.

    python tools/bench_tbi.py [--regions 3000] [--region-len 4000] [--group 25] [--repeat 8] [--out profiles/tbi_index.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import struct
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
HEADER = b"##fileformat=VCFv4.0\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS1\n"


def sorted_text(n_regions, region_len, group, repeat):
    """(text, piece lengths): bench_bgzf_out's pieces `repeat` times over, copy k's contigs prefixed with k<k> (a contig may not come back)."""
    from bench_bgzf_out import record_text
    text, lens = record_text(n_regions, region_len, group, 1)
    pieces, at = [], 0
    for n in lens.tolist():
        pieces.append(text[at:at + n])
        at += n
    out = []
    for k in range(repeat):
        pre = b"k%d" % k
        out += [b"".join(pre + ln + b"\n" for ln in p.split(b"\n")[:-1]) for p in pieces]
    return b"".join(out), [len(p) for p in out]


def timed(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return dict(median_ms=round(statistics.median(ts), 3), best_ms=round(min(ts), 3), runs=repeats)


def device_split(eng, packed, warmup, repeats):
    """Upload, inflate and index kernels between HIP events; buffers allocated once."""
    import torch
    from platypus_amd import _lib
    from platypus_amd import tabixindex
    blocks, at = [], 0
    while at < len(packed):                                               # (offset, length, ISIZE) of the file's blocks
        k = tabixindex.block_length(packed, at)
        blocks.append((at, k, struct.unpack_from("<I", packed, at + k - 4)[0]))
        at += k
    while blocks and blocks[-1][2] == 0:
        end = blocks.pop()[0]
    n, total = len(blocks), sum(b[2] for b in blocks)
    host = torch.from_numpy(np.frombuffer(packed, dtype=np.uint8).copy()).pin_memory()
    d_file = torch.empty(len(packed), dtype=torch.uint8, device=eng.device)
    d_off = torch.tensor([b[0] for b in blocks], dtype=torch.int64, device=eng.device)
    d_addr = torch.tensor([b[0] for b in blocks] + [end], dtype=torch.int64, device=eng.device)
    d_data = torch.empty(total + _lib.PLAT_BLOB_PAD, dtype=torch.uint8, device=eng.device)
    d_out_off = torch.zeros(n + 1, dtype=torch.int64, device=eng.device)
    d_ist = torch.zeros(4, dtype=torch.int64, device=eng.device)
    io = _lib.BgzfInflateOut(total, d_data.data_ptr(), d_out_off.data_ptr(), d_ist.data_ptr())
    cap_r, cap_n, cap_w, cap_b = total // 64 + 1024, _lib.TBI_MAX_REF, 1 << 18, 1 << 20
    i32 = lambda k: torch.zeros(k + 1, dtype=torch.int32, device=eng.device)
    i64 = lambda k: torch.zeros(k + 1, dtype=torch.int64, device=eng.device)
    keep = [i32(cap_r), i32(cap_r), i64(cap_r), i64(cap_n), i32(cap_n), torch.zeros(cap_b + 1, dtype=torch.uint8, device=eng.device), i64(cap_n + 1), i64(cap_w),
            i64(_lib.TBI_STATUS_WORDS)]
    ti = _lib.TabixIndexIn(n, 0, d_data.data_ptr(), total, d_out_off.data_ptr(), d_addr.data_ptr())
    to = _lib.TabixIndexOut(cap_r, cap_n, cap_w, cap_b, *[t.data_ptr() for t in keep])
    stream = torch.cuda.current_stream(eng.device)
    rows = {"upload": [], "inflate": [], "index": []}
    for it in range(warmup + repeats):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        ev[0].record(stream)
        d_file.copy_(host, non_blocking=True)
        ev[1].record(stream)
        _lib.check(eng.lib.plat_bgzf_inflate_batch(eng.ctx, n, d_file.data_ptr(), len(packed), d_off.data_ptr(), None, C.byref(io), eng._stream()), "plat_bgzf_inflate_batch")
        ev[2].record(stream)
        _lib.check(eng.lib.plat_tabix_index_batch(eng.ctx, C.byref(ti), C.byref(to), eng._stream()), "plat_tabix_index_batch")
        ev[3].record(stream)
        eng._sync()
        torch.cuda.synchronize()
        if it >= warmup:
            for k, name in enumerate(("upload", "inflate", "index")):
                rows[name].append(ev[k].elapsed_time(ev[k + 1]))
    st = keep[-1].cpu().numpy()
    assert int(d_ist.cpu()[0]) == 0 and int(st[0]) == 0, st
    out = {name: dict(median_ms=round(statistics.median(v), 3), best_ms=round(min(v), 3), runs=repeats) for name, v in rows.items()}
    out.update(blocks=n, inflated_bytes=total, records=int(st[3]), runs=int(st[4]), contigs=int(st[5]), windows=int(st[6]), records_per_run=round(int(st[3]) / max(int(st[4]), 1), 2))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=3000)
    ap.add_argument("--region-len", type=int, default=4000)
    ap.add_argument("--group", type=int, default=25)
    ap.add_argument("--repeat", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tbi_index.json"))
    a = ap.parse_args()
    from platypus_amd import fastcaller as F, hostapi as H
    text, lens = sorted_text(a.regions, a.region_len, a.group, a.repeat)
    nc = F.NativeCaller(0, 8, 4)
    try:
        z, _ = nc.compress_text(HEADER + text, [len(HEADER)] + lens)
        packed = bytes(z)
        res = dict(tool="bench_tbi", regions=a.regions, region_len=a.region_len, text_bytes=len(HEADER) + len(text), file_bytes=len(packed), warmup=a.warmup)
        tbi = nc.index_bgzf(packed)
        res["tbi_bytes"] = len(tbi)
        res["device_call"] = timed(lambda: nc.index_bgzf(packed), a.warmup, a.repeats)
        os.environ["PLAT_CALLER_HOST_TBI"] = "1"
        try:
            assert nc.index_bgzf(packed) == tbi
            res["host_twin_call"] = timed(lambda: nc.index_bgzf(packed), 1, max(3, a.repeats // 3))
        finally:
            del os.environ["PLAT_CALLER_HOST_TBI"]
    finally:
        nc.close()
    res["device_split"] = device_split(H.get_engine(), packed, a.warmup, a.repeats)
    s = res["device_split"]
    res["device_rest_ms"] = round(res["device_call"]["median_ms"] - s["upload"]["median_ms"] - s["inflate"]["median_ms"] - s["index"]["median_ms"], 3)
    res["host_over_device"] = round(res["host_twin_call"]["median_ms"] / res["device_call"]["median_ms"], 2)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
