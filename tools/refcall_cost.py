#!/usr/bin/env python3
"""What --outputRefCalls=1 costs in the native region loop: synthetic config-4 regions (tools/synth, one sample, generated on demand) through
plat_call_regions_stream with outputRefCalls=1 and with outputRefCalls=0, --reps runs each.  Per mode: worker CPU seconds per region
(plat_caller_stats.seconds_worker_cpu / regions), windows/s (windows called / wall seconds) -- every run, and their median and spread
(max - min) -- the REFCALL records, the stage-B regions on the device and on the host, the read-count intervals from the device and the
decisions left to the host's loop.  One more run per mode times the kernels filed under "other" (plat_caller_time_kernel) with the device
read counts and once more with PLAT_CALLER_HOST_REFCOV=1: the difference is plat_refcall_coverage_batch's kernels, reported per chunk.

Writes profiles/refcall_cost.json (--out) under --label: run it once on the commit before the device read counts ("parent": the switch and the
new counters do not exist there, the fields come out as null) and once on this one ("this"); the file keeps both.

    python tools/refcall_cost.py --label this [--regions 256] [--region-len 100000] [--reps 3]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from platypus_amd import _lib, fastcaller as F  # noqa: E402
from platypus_amd.options import default_options  # noqa: E402
from tools.synth import source  # noqa: E402


def other_kernel_id():
    lib = _lib.load()
    for k in range(64):
        name = lib.plat_kernel_timer_name(k)
        if name is None:
            break
        if b"other" in name.lower():
            return k
    return -1


def one_run(a, refcalls, host_refcov=False, time_other=-1):
    if host_refcov:
        os.environ["PLAT_CALLER_HOST_REFCOV"] = "1"
    else:
        os.environ.pop("PLAT_CALLER_HOST_REFCOV", None)
    src = source.RegionSource(list(range(a.regions)), a.slots, region_len=a.region_len)
    nc = F.NativeCaller(0, a.workers, a.per_chunk)
    try:
        if time_other >= 0:
            nc.time_kernel(time_other)
        t0 = time.perf_counter()
        txt = nc.call_stream(a.regions, src.load_fn, src.h, ["S1"], default_options(outputRefCalls=1 if refcalls else 0), a.slots, a.loaders, raw=True)
        wall = time.perf_counter() - t0
        st = nc.stats
    finally:
        nc.close()
        src.close()
        os.environ.pop("PLAT_CALLER_HOST_REFCOV", None)
    out = dict(wall_seconds=wall, worker_cpu_seconds_per_region=st["seconds_worker_cpu"] / a.regions, windows_per_second=st["n_windows_called"] / wall,
               windows_called=st["n_windows_called"], records=st["n_records"], refcall_records=st["n_refcall_records"], text_bytes=len(txt),
               stage_b_regions_device=st["n_regions_stage_b_device"], stage_b_regions_host=st["n_regions_stage_b_host"],
               refcall_intervals_device=st.get("n_refcall_intervals_device"), refcall_positions_device=st.get("n_refcall_positions_device"),
               refcall_decisions_host=st.get("n_refcall_intervals_host"))
    if time_other >= 0:
        out["other_kernels_ms"] = st["kernel_ms"][time_other]
        out["other_kernels_launches"] = st["kernel_launches"][time_other]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--label", required=True, help="the key this run is kept under in the output file (parent / this)")
    ap.add_argument("--regions", type=int, default=256)
    ap.add_argument("--region-len", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--workers", type=int, default=4)
    ap.add_argument("--per-chunk", type=int, default=4)
    ap.add_argument("--slots", type=int, default=32)
    ap.add_argument("--loaders", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "refcall_cost.json"))
    a = ap.parse_args()
    one_run(a, False)                                                       # (warm-up: the worker's buffers, the code objects)
    res = dict(regions=a.regions, region_len=a.region_len, workers=a.workers, regions_per_chunk=a.per_chunk, reps=a.reps)
    for refcalls in (1, 0):
        runs = [one_run(a, refcalls) for _ in range(a.reps)]
        mode = dict(runs=runs)
        for k in ("worker_cpu_seconds_per_region", "windows_per_second"):
            v = [r[k] for r in runs]
            mode[k] = dict(median=statistics.median(v), spread=max(v) - min(v), values=v)
        res["outputRefCalls=%d" % refcalls] = mode
    kid = other_kernel_id()
    if kid >= 0 and hasattr(F.CallerStats, "n_refcall_intervals_device"):
        dev, host = one_run(a, 1, False, kid), one_run(a, 1, True, kid)
        chunks = -(-a.regions // a.per_chunk)
        ms = dev["other_kernels_ms"] - host["other_kernels_ms"]
        res["coverage_kernels"] = dict(ms_total=ms, launches=dev["other_kernels_launches"] - host["other_kernels_launches"], chunks=chunks,
                                       ms_per_chunk=ms / chunks, other_kernels_ms_with_host_loop=host["other_kernels_ms"])
    keep = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            keep = json.load(f)
    keep.setdefault("what", "tools/refcall_cost.py: the native region loop on synthetic config-4 regions with outputRefCalls=1 and 0, MI355X; worker CPU seconds per "
                            "region, windows/s (median and max - min of the runs), and the read-count kernels' time per chunk")
    keep[a.label] = res
    with open(a.out, "w") as f:
        json.dump(keep, f, indent=1)
        f.write("\n")
    print(json.dumps({a.label: {k: v for k, v in res.items() if not isinstance(v, dict) or k == "coverage_kernels"} |
                      {k: {m: v[m] for m in ("worker_cpu_seconds_per_region", "windows_per_second")} for k, v in res.items() if k.startswith("outputRefCalls")}}))


if __name__ == "__main__":
    main()
