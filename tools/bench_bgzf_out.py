"""What writing the record text as BGZF costs (plat_bgzf_deflate_batch, plat_caller_compress_text): the record text of a few thousand
config-4 regions, grouped into pieces the size of the whole-genome job's regions, compressed
  * on the device: the kernels alone between two HIP events (text and offsets resident), and end to end through plat_caller_compress_text
    (upload, kernels, download; the caller's workers take slices in turn);
  * by zlib level 1 and 6 on the same 0xff00-byte blocks, one core: its ratio and its throughput x 16 -- the box's CPUs, the bar the
    device path is compared with;
  * by the host twin of the device's rule (PLAT_CALLER_HOST_DEFLATE=1), one worker.
Prints one JSON line and writes it to --out.

    python tools/bench_bgzf_out.py [--regions 3000] [--region-len 4000] [--group 25] [--repeat 8] [--out profiles/bgzf_out.json]"""
import argparse
import ctypes as C
import json
import os
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PAYLOAD = 0xff00


def record_text(n_regions, region_len, group, repeat):
    """(text, piece lengths): the native region loop's records of n_regions synthetic regions, `group` regions to a piece, `repeat` times over."""
    from platypus_amd import fastcaller as F, synth
    from platypus_amd.options import default_options
    nc = F.NativeCaller(0, 8, 4)
    try:
        opts = default_options(rlen=100)
        opts.originalMaxHaplotypes = opts.maxHaplotypes
        regs = [F.region_from_arrays(synth.config4_region_arrays(i, region_len=region_len, n_samples=1, read_len=100)) for i in range(n_regions)]
        text = nc.call_regions(regs, ["S1"], opts).encode("ascii")
        lens = nc.region_text_lengths(n_regions)
    finally:
        nc.close()
    pieces = np.add.reduceat(lens, np.arange(0, n_regions, group)) if n_regions else lens
    return text * repeat, np.tile(pieces, repeat)


def device_kernels(eng, text, lens, repeats):
    """plat_bgzf_deflate_batch between two HIP events, text and offsets resident: (best ms, compressed bytes, blocks)."""
    import torch
    from platypus_amd import _lib
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    d_text = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).to(eng.device)
    d_off = torch.from_numpy(off).to(eng.device)
    cap = len(text) + 31 * (len(text) // PAYLOAD + len(lens))
    d_data = torch.empty(cap + _lib.PLAT_BLOB_PAD, dtype=torch.uint8, device=eng.device)
    d_out_off = torch.zeros(len(off), dtype=torch.int64, device=eng.device)
    d_status = torch.zeros(4, dtype=torch.int64, device=eng.device)
    i = _lib.BgzfDeflateIn(d_text.data_ptr(), len(text), len(lens), 1, d_off.data_ptr())
    o = _lib.BgzfDeflateOut(cap, d_data.data_ptr(), d_out_off.data_ptr(), d_status.data_ptr())
    best = None
    stream = torch.cuda.current_stream(eng.device)
    for _ in range(repeats + 1):                                          # (the first run sizes the scratch)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        _lib.check(eng.lib.plat_bgzf_deflate_batch(eng.ctx, C.byref(i), C.byref(o), eng._stream()), "plat_bgzf_deflate_batch")
        b.record(stream)
        eng._sync()
        torch.cuda.synchronize()
        ms = a.elapsed_time(b)
        best = ms if best is None else min(best, ms)
    st = d_status.cpu().numpy()
    assert int(st[0]) == 0
    return best, int(st[2]), int(st[3])


def wall(fn, repeats):
    best = None
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best, out


def zlib_blocks(text, lens, level, budget_bytes):
    """zlib on the pieces' 0xff00-byte blocks (raw deflate, as a BGZF writer calls it), one core, over the first budget_bytes of the text."""
    blocks, at = [], 0
    for n in lens.tolist():
        for k in range(at, at + n, PAYLOAD):
            blocks.append(text[k:min(at + n, k + PAYLOAD)])
        at += n
        if at >= budget_bytes:
            break
    t0 = time.perf_counter()
    out = 0
    for b in blocks:
        c = zlib.compressobj(level, zlib.DEFLATED, -15)
        out += len(c.compress(b)) + len(c.flush()) + 26
    dt = time.perf_counter() - t0
    n_in = sum(len(b) for b in blocks)
    return dict(bytes_in=n_in, ratio=round(out / n_in, 4), one_core_MBps=round(n_in / dt / 1e6, 1), sixteen_cores_GBps=round(16 * n_in / dt / 1e9, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=3000)
    ap.add_argument("--region-len", type=int, default=4000)
    ap.add_argument("--group", type=int, default=25, help="regions per piece (25 x 4 kb: the whole-genome job's 100 kb regions)")
    ap.add_argument("--repeat", type=int, default=8, help="the text is taken this many times over")
    ap.add_argument("--repeats", type=int, default=5, help="timed runs of each measurement (the best counts)")
    ap.add_argument("--workers", type=int, default=8)
    ap.add_argument("--zlib-budget", type=int, default=32 << 20, help="bytes of text the zlib passes run over")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bgzf_out.json"))
    a = ap.parse_args()
    from platypus_amd import fastcaller as F, hostapi as H
    text, lens = record_text(a.regions, a.region_len, a.group, a.repeat)
    eng = H.get_engine()
    ms, packed, blocks = device_kernels(eng, text, lens, a.repeats)
    res = dict(tool="bench_bgzf_out", regions=a.regions, region_len=a.region_len, pieces=int(len(lens)), text_bytes=len(text), blocks=blocks,
               device=dict(level=1, compressed_bytes=packed, ratio=round(packed / len(text), 4), kernels_ms=round(ms, 3),
                           kernels_GBps=round(len(text) / ms / 1e6, 2)))
    nc = F.NativeCaller(0, a.workers, 4)
    try:
        dt, (z, _) = wall(lambda: nc.compress_text(text, lens), a.repeats)
        assert len(z) == packed + 28
        res["device"].update(end_to_end_ms=round(dt * 1e3, 2), end_to_end_GBps=round(len(text) / dt / 1e9, 3), workers=a.workers)
    finally:
        nc.close()
    os.environ["PLAT_CALLER_HOST_DEFLATE"] = "1"
    nc = F.NativeCaller(0, 1, 4)
    try:
        small = int(np.searchsorted(np.cumsum(lens), a.zlib_budget)) + 1
        sub = lens[:small]
        n_sub = int(sub.sum())
        dt, (hz, _) = wall(lambda: nc.compress_text(text[:n_sub], sub), 2)
        res["host_twin"] = dict(bytes_in=n_sub, ratio=round((len(hz) - 28) / n_sub, 4), one_core_MBps=round(n_sub / dt / 1e6, 1),
                                sixteen_cores_GBps=round(16 * n_sub / dt / 1e9, 3))
    finally:
        nc.close()
        del os.environ["PLAT_CALLER_HOST_DEFLATE"]
    res["zlib_level_1"] = zlib_blocks(text, lens, 1, a.zlib_budget)
    res["zlib_level_6"] = zlib_blocks(text, lens, 6, a.zlib_budget)
    bar = res["zlib_level_1"]["sixteen_cores_GBps"]
    res["device_end_to_end_over_16_core_zlib1"] = round(res["device"]["end_to_end_GBps"] / bar, 2)
    res["device_kernels_over_16_core_zlib1"] = round(res["device"]["kernels_GBps"] / bar, 2)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
