"""What loading a reference genome costs (plat_fasta_fetch_batch, plat_fasta_load): a seeded FASTA of --contigs contigs and about --mb MB
at 60/61 is built in memory (default: 24 contigs, about 3 GB -- a human genome's shape) and all its contigs are fetched whole.

    the device batch     plat_fasta_fetch_batch alone, the file and the queries resident on the device: the five launches between two
                         device events, after a warm-up, median of --repeats.  Bytes moved are computed from the shapes -- the file's
                         bytes once per pass (the count pass and the write pass each read them) plus the bytes written -- and given over
                         that time, and as a share of the HBM peak (8.0 TB/s, the specification's figure)
    the whole call       plat_fasta_load as it stands: the upload of the file, the batch, the wait, the copy back into pinned host
                         memory (plat_fasta_info.seconds)
    the host twin        the same call under PLAT_CALLER_HOST_FASTA=1: the rule's loop on one thread -- the thing the call replaces

One process, one GPU; a record, not a bar.

    python tools/fasta_fetch_bench.py [--mb 3000] [--contigs 24] [--warmup 2] [--repeats 5] [--out profiles/fasta_fetch.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12


def seeded_fasta(contigs, total_bytes, line_len=60, seed=9):
    """(the file as a uint8 array, its .fai's bytes): `contigs` contigs of decreasing length, lines of line_len bases."""
    rng = np.random.Generator(np.random.PCG64(seed))
    weights = np.linspace(2.5, 0.5, contigs)
    lengths = (weights / weights.sum() * total_bytes * line_len / (line_len + 1)).astype(np.int64) // line_len * line_len + 17
    parts, fai, at = [], [], 0
    lut = np.frombuffer(b"ACGTacgtNn", dtype=np.uint8)
    for k, n in enumerate(lengths.tolist()):
        head = np.frombuffer(b">chr%d seeded\n" % (k + 1), dtype=np.uint8)
        full = n // line_len
        body = np.empty((full, line_len + 1), dtype=np.uint8)
        body[:, :line_len] = lut[rng.integers(0, 4, size=(full, line_len), dtype=np.uint8) + (rng.integers(0, 64, size=(full, 1), dtype=np.uint8) == 0) * 4]
        body[:, line_len] = 0x0A
        tail = np.concatenate([lut[rng.integers(0, 4, size=n - full * line_len, dtype=np.uint8)], np.frombuffer(b"\n", dtype=np.uint8)])
        fai.append(b"chr%d\t%d\t%d\t%d\t%d\n" % (k + 1, n, at + len(head), line_len, line_len + 1))
        parts += [head, body.reshape(-1), tail]
        at += len(head) + body.size + len(tail)
    return np.concatenate(parts), b"".join(fai), lengths.tolist()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=int, default=3000)
    ap.add_argument("--contigs", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fasta_fetch.json"))
    a = ap.parse_args()
    import torch
    from platypus_amd import _lib, fastcaller as F
    from platypus_amd.engine import Engine
    data, fai, lengths = seeded_fasta(a.contigs, a.mb * 1000000)
    res = dict(tool="fasta_fetch_bench", contigs=a.contigs, file_bytes=int(data.size), bases=int(sum(lengths)), line="60/61", warmup=a.warmup, repeats=a.repeats)
    # the device batch alone
    eng = Engine(0)
    rows = [ln.split(b"\t") for ln in fai.split(b"\n") if ln]
    q = np.asarray([[int(r[2]), int(r[3]), int(r[4]), int(r[1]), 0, 0] for r in rows], dtype=np.int64)
    n = len(rows)
    d_file = torch.from_numpy(data).to(eng.device)
    d_q = [torch.from_numpy(np.ascontiguousarray(q[:, k])).to(eng.device) for k in range(6)]
    d_mode = torch.ones(n, dtype=torch.uint8, device=eng.device)
    cap = int(sum(lengths))
    d_off, d_status = torch.zeros(n + 1, dtype=torch.int64, device=eng.device), torch.zeros(n, dtype=torch.int32, device=eng.device)
    d_totals, d_out = torch.zeros(_lib.FASTA_STATUS_WORDS, dtype=torch.int64, device=eng.device), torch.empty(cap, dtype=torch.uint8, device=eng.device)
    i = _lib.FastaFetchIn(d_file.data_ptr(), int(data.size), 0, int(data.size), n, *[t.data_ptr() for t in d_q], d_mode.data_ptr())
    o = _lib.FastaFetchOut(cap, d_off.data_ptr(), d_status.data_ptr(), d_out.data_ptr(), d_totals.data_ptr())
    ms = []
    for k in range(a.warmup + a.repeats):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        _lib.check(eng.lib.plat_fasta_fetch_batch(eng.ctx, C.byref(i), C.byref(o), eng._stream()), "plat_fasta_fetch_batch")
        t1.record()
        torch.cuda.synchronize(eng.device)
        if k >= a.warmup:
            ms.append(t0.elapsed_time(t1))
    totals = d_totals.cpu().numpy().tolist()
    assert totals[0] == 0 and totals[1] == cap, totals
    moved = 2 * int(data.size) + cap
    med = statistics.median(ms)
    res["device_batch"] = dict(median_ms=round(med, 3), best_ms=round(min(ms), 3), tiles=int(totals[2]), bytes_moved=moved,
                               tb_per_s=round(moved / (med * 1e-3) / 1e12, 3), share_of_hbm_peak=round(moved / (med * 1e-3) / HBM_PEAK, 3))
    first = d_out[:lengths[0]].cpu().numpy()
    del d_file, d_out
    torch.cuda.empty_cache()
    # the whole call, and the host twin
    nc = F.NativeCaller(0, 1, 1)
    try:
        secs = []
        for k in range(1 + max(2, a.repeats // 2)):
            fa = nc.open_fasta(data, fai)
            fa.load()
            if k:
                secs.append(fa.info["seconds"])
            else:
                assert np.array_equal(fa.contig(0)[0], first) and fa.info["out_bytes"] == cap
            fa.close()
        res["whole_call"] = dict(median_ms=round(statistics.median(secs) * 1e3, 1), best_ms=round(min(secs) * 1e3, 1), runs=len(secs), uploaded_bytes=int(data.size), copied_back=cap)
        os.environ["PLAT_CALLER_HOST_FASTA"] = "1"
        try:
            fa = nc.open_fasta(data, fai)
            fa.load()
            assert np.array_equal(fa.contig(0)[0], first)
            res["host_twin_one_thread_ms"] = round(fa.info["seconds"] * 1e3, 1)
            fa.close()
        finally:
            del os.environ["PLAT_CALLER_HOST_FASTA"]
    finally:
        nc.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
