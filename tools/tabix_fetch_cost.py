"""What taking a source VCF as BGZF blocks costs: one chunk of regions of panel-like text (lines of ~10 KB: a few thousand sample columns)
handed to plat_caller_set_source_blocks, on the device and -- PLAT_CALLER_HOST_TABIX=1 -- on the host, plus the two device entry points
timed alone with HIP events.  A record, not a gate.  Prints one JSON line and writes it to --out.

    python tools/tabix_fetch_cost.py [--regions 128] [--lines 200] [--line-bytes 10000] [--out profiles/tabix_fetch_cost.json]
"""
import argparse
import ctypes as C
import json
import os
import random
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from platypus_amd import _lib, fastcaller as F, hostapi as H, synth  # noqa: E402


def region_text(k, n_lines, line_bytes, rng):
    """n_lines data lines of ~line_bytes each on contig 20, from position 1000 * k on: eight columns and genotype columns behind them."""
    gts = [b"0/0:%d:%d" % (rng.randrange(60), rng.randrange(99)) for _ in range(64)] + [b"0/1:%d:%d" % (rng.randrange(60), rng.randrange(99)) for _ in range(8)]
    out = []
    for i in range(n_lines):
        head = b"\t".join([b"20", b"%d" % (100000 * k + 1000 + 3 * i), b"rs%d" % i, b"ACGT"[i % 4:i % 4 + 1], b"TGCA"[i % 4:i % 4 + 1], b"50", b"PASS",
                           b"AC=%d;AN=2000" % rng.randrange(2000), b"GT:DP:GQ"])
        cols = []
        size = len(head)
        while size < line_bytes:
            g = gts[rng.randrange(len(gts))]
            cols.append(g)
            size += len(g) + 1
        out.append(head + b"\t" + b"\t".join(cols) + b"\n")
    return b"".join(out)


def block_offsets(data):
    off, at = [], 0
    while at < len(data):
        off.append(at)
        at += int.from_bytes(data[at + 16:at + 18], "little") + 1
    return off


def time_entry_points(eng, texts, blobs, repeats):
    """plat_bgzf_inflate_batch and plat_tabix_fetch_batch over the same blocks, each between two HIP events: the best of `repeats`."""
    import torch
    blob = b"".join(blobs)
    blk_off, chunk_first, chunk_end, base = [], [], [], 0
    for b in blobs:
        offs = block_offsets(b)
        chunk_first.append(len(blk_off))
        blk_off += [base + o for o in offs]
        chunk_end.append(len(blk_off))
        base += len(b)
    n, inflated = len(blobs), sum(len(t) for t in texts)
    dev = lambda a, dt: torch.from_numpy(np.append(np.asarray(a, dtype=dt), np.zeros(1, dtype=dt))).to(eng.device)
    d_blob, d_off = dev(np.frombuffer(blob, dtype=np.uint8), np.uint8), dev(blk_off, np.int64)
    d_data = torch.zeros(inflated + _lib.PLAT_BLOB_PAD + 16, dtype=torch.uint8, device=eng.device)
    d_out_off, d_st = torch.zeros(len(blk_off) + 1, dtype=torch.int64, device=eng.device), torch.zeros(8, dtype=torch.int64, device=eng.device)
    io = _lib.BgzfInflateOut(inflated, d_data.data_ptr(), d_out_off.data_ptr(), d_st.data_ptr())
    g = dict(scb=dev(np.arange(n + 1), np.int32), cf=dev(chunk_first, np.int32), ce=dev(chunk_end, np.int32), zero=dev(np.zeros(n), np.int32),
             minus=dev(-np.ones(n), np.int32), names=dev(np.frombuffer(b"20" * n, dtype=np.uint8), np.uint8), noff=dev(2 * np.arange(n + 1), np.int32),
             end=dev(np.full(n, 1 << 29), np.int32))
    cap = inflated + n
    d_text = torch.zeros(cap + _lib.PLAT_BLOB_PAD + 16, dtype=torch.uint8, device=eng.device)
    d_toff, d_counts = torch.zeros(n + 1, dtype=torch.int64, device=eng.device), torch.zeros(2 * n, dtype=torch.int64, device=eng.device)
    fi = _lib.TabixFetchIn(n, n, len(blk_off), 0, d_data.data_ptr(), inflated, d_out_off.data_ptr(), g["scb"].data_ptr(), g["cf"].data_ptr(), g["ce"].data_ptr(),
                           g["zero"].data_ptr(), g["minus"].data_ptr(), g["zero"].data_ptr(), g["names"].data_ptr(), g["noff"].data_ptr(), g["zero"].data_ptr(),
                           g["end"].data_ptr())
    fo = _lib.TabixFetchOut(cap, d_text.data_ptr(), d_toff.data_ptr(), d_counts.data_ptr(), d_st.data_ptr() + 32)
    ms = {"inflate": [], "fetch": []}
    for _ in range(repeats + 1):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        ev[0].record()
        _lib.check(eng.lib.plat_bgzf_inflate_batch(eng.ctx, len(blk_off), d_blob.data_ptr(), len(blob), d_off.data_ptr(), None, C.byref(io), eng._stream()), "inflate")
        ev[1].record()
        _lib.check(eng.lib.plat_tabix_fetch_batch(eng.ctx, C.byref(fi), C.byref(fo), eng._stream()), "fetch")
        ev[2].record()
        eng._sync()
        ms["inflate"].append(ev[0].elapsed_time(ev[1]))
        ms["fetch"].append(ev[1].elapsed_time(ev[2]))
    st = d_st.cpu().numpy()
    assert st[0] == 0 and st[4] == 0 and int(st[7]) == inflated, st            # every line of every region is kept
    return {k: round(min(v[1:]), 4) for k, v in ms.items()}                  # (the first round pays the scratch's allocation)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=128)
    ap.add_argument("--lines", type=int, default=200)
    ap.add_argument("--line-bytes", type=int, default=10000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "tabix_fetch_cost.json"))
    a = ap.parse_args()
    rng = random.Random(8)
    distinct = [region_text(k, a.lines, a.line_bytes, rng) for k in range(4)]  # (four texts, dealt to the regions in turn: the generator is Python)
    packed = [synth.bgzf_stream(t, 0xff00, level=6)[0] for t in distinct]
    texts, blobs = [distinct[k % 4] for k in range(a.regions)], [packed[k % 4] for k in range(a.regions)]
    arrays = [np.frombuffer(b, dtype=np.uint8) for b in packed]
    blocks = [[(b"20", 0, 1 << 29, [(arrays[k % 4], 0, -1, 0)])] for k in range(a.regions)]
    out = {"regions": a.regions, "lines_per_region": a.lines, "line_bytes": a.line_bytes}
    nc = F.NativeCaller(0, 2, 4)
    try:
        for path, env in (("device", None), ("host", "1")):
            if env:
                os.environ["PLAT_CALLER_HOST_TABIX"] = env
            else:
                os.environ.pop("PLAT_CALLER_HOST_TABIX", None)
            secs = []
            for _ in range(a.repeats):
                t0 = time.perf_counter()
                nc.set_source_blocks(blocks)
                wall = time.perf_counter() - t0
                info = dict(nc.source_blocks_info)
                secs.append((info["seconds"], wall))
                nc.set_source_blocks([])
            assert info["kept_bytes"] == info["inflated_bytes"] == sum(len(t) for t in texts) and info["lines_kept"] == a.regions * a.lines
            out[path] = {"seconds": round(min(s for s, _ in secs[1:] or secs), 5), "seconds_first_call": round(secs[0][0], 5), "python_wall": round(min(w for _, w in secs), 5),
                         "compressed_bytes": info["compressed_bytes"], "inflated_bytes": info["inflated_bytes"], "n_blocks": info["n_blocks"],
                         "lines_kept": info["lines_kept"]}
        os.environ.pop("PLAT_CALLER_HOST_TABIX", None)
    finally:
        nc.close()
    out["kernels_ms"] = time_entry_points(H.get_engine(), texts, blobs, a.repeats)
    line = json.dumps(out, sort_keys=True)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
