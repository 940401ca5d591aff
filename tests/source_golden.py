"""Shared by the CPU and GPU tests of candidates from source VCF lines: the fixtures tests/golden/source_cases.json.gz (the reference's
reader text over lines) and source_region_cases.json.gz (the reference's region loop with that reader), written by
tests/golden/gen_golden_source.py; the region loops fed from a case; the host parser behind its debug export."""
import ctypes as C
import gzip
import io
import json
import os

import numpy as np

from platypus_amd import caller, fastcaller as F, hostapi as H
from platypus_amd.options import default_options
from platypus_amd.vcfrecords import VCF, _py2_string_hash
from tests import region_golden as R

HERE = os.path.dirname(os.path.abspath(__file__))


def load(name):
    with gzip.open(os.path.join(HERE, "golden", name), "rt") as f:
        return json.load(f)


def region_source(case):
    """Per loaded region the fetched texts (bytes, one per source file)."""
    return [[t.encode() for t in reg["source"]] for reg in case["regions"] if reg["loaded"]]


def python_loop_text(case):
    fasta, work, names = R.case_work(case)
    opts = default_options(**case["options"])
    files = len(case["regions"][0]["source"])
    opts.sourceFile = [{(reg["chrom"], reg["start"], reg["end"]): reg["source"][f].encode() for reg in case["regions"]} for f in range(files)]
    out = io.StringIO()
    caller.callVariantsInRegions(work, fasta, opts, VCF(names), out)
    return out.getvalue().split("\n")[:-1], opts.rlen


def native_loop_text(case, lib=None, workers=2, per_chunk=2, nc=None, source=True):
    """The native loop over the case (its source lines set unless source=False); returns (lines, rlen, stats)."""
    fasta, work, names = R.case_work(case)
    opts = default_options(**case["options"])
    own = nc is None
    if own:
        nc = F.NativeCaller(0, workers, per_chunk, lib=lib) if lib is not None else F.NativeCaller(0, workers, per_chunk)
    try:
        txt = nc.call_regions([F.RegionReads.from_buffers(c, s, e, fasta, b) for c, s, e, b in work], names, opts,
                              source_lines=region_source(case) if source else None)
        st = nc.stats
    finally:
        if own:
            nc.close()
    return txt.split("\n")[:-1], opts.rlen, st


def host_parse(lib, regions, names, max_size=1500, long_haps=0, cap=None, text_off=None):
    """plat_caller_debug_source_parse: the host parser over regions' texts; the dict Engine.source_variants returns (no guards)."""
    blobs = [bytes(r) for r in regions]
    n = len(blobs)
    text = b"".join(blobs)
    off = np.concatenate([[0], np.cumsum([len(b) for b in blobs])]).astype(np.int64) if text_off is None else np.asarray(text_off, dtype=np.int64)
    hashes = np.array([_py2_string_hash(h.decode("latin-1") if isinstance(h, bytes) else h) for h in names] + [0], dtype=np.uint64).view(np.int64)
    cap = len(text) + 1 if cap is None else int(cap)
    buf = np.frombuffer(text + b"\0" * 64, dtype=np.uint8).copy()
    i32, i64 = (lambda k: np.zeros(k + 1, dtype=np.int32)), (lambda k: np.zeros(k + 1, dtype=np.int64))
    g = dict(region_begin=i32(n + 1), pos=i32(cap), rem_off=i64(cap), n_rem=i32(cap), add_off=i64(cap), n_add=i32(cap), hash=i32(cap), line=i32(cap),
             region_stats=i32(4 * n), status=i64(4))
    fn = lib.plat_caller_debug_source_parse
    fn.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64] + [C.c_void_p] * 10
    fn.restype = C.c_int
    rc = fn(buf.ctypes.data, len(text), off.ctypes.data, hashes.ctypes.data, n, int(max_size), int(long_haps), cap,
            *[g[k].ctypes.data for k in ("region_begin", "pos", "rem_off", "n_rem", "add_off", "n_add", "hash", "line", "region_stats", "status")])
    st = g["status"][:4]
    assert rc == int(st[0])
    written = 0 if rc == -1 else min(int(st[2]), cap)
    out = {k: g[k][:written] for k in ("pos", "rem_off", "n_rem", "add_off", "n_add", "hash", "line")}
    out.update(region_begin=g["region_begin"][:n + 1], stats=g["region_stats"][:4 * n].reshape(-1, 4), status=st, text=text)
    return out


def host_order(lib, text, d, first, last):
    """plat_caller_debug_source_order over alleles [first, last) of a parse: indices (into the parse) in the order of variantutils.py:161."""
    n = last - first
    out = np.zeros(max(n, 1), dtype=np.int32)
    buf = np.frombuffer(text + b"\0" * 64, dtype=np.uint8).copy()
    fn = lib.plat_caller_debug_source_order
    fn.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 7
    fn.restype = C.c_int
    arr = [np.ascontiguousarray(d[k][first:last]) for k in ("pos", "rem_off", "n_rem", "add_off", "n_add", "hash")]
    m = fn(buf.ctypes.data, n, *[a.ctypes.data for a in arr], out.ctypes.data)
    return [first + int(i) for i in out[:m]]


def alleles_of(d, first=0, last=None):
    """[(pos, removed, added, line)] of a parse (device or host)."""
    t = d["text"]
    last = len(d["pos"]) if last is None else last
    return [(int(d["pos"][i]), t[int(d["rem_off"][i]):int(d["rem_off"][i]) + int(d["n_rem"][i])],
             t[int(d["add_off"][i]):int(d["add_off"][i]) + int(d["n_add"][i])], int(d["line"][i])) for i in range(first, last)]


def python_parse(regions, names, max_size=1500, long_haps=0):
    """The plain-Python restatement in the shape of a parse: (per region [(pos, removed, added, line)], stats [n, 4], hashes, lowest BAD
    (region << 32 | line) or -1)."""
    from platypus_amd import regionprep as RP
    from platypus_amd.vcfrecords import py2_variant_hash
    per, stats, hashes, bad = [], [], [], -1
    for k, (text, name) in enumerate(zip(regions, names)):
        alleles, st, bads = RP.sourceTextAlleles(bytes(text), max_size, long_haps)
        per.append(alleles)
        stats.append([st["lines"], st["skipped"], st["invalid"], st["oversize"]])
        for p, r, a, _ in alleles:
            h = py2_variant_hash(name, p, r, a) & 0xFFFFFFFF
            hashes.append(h - (1 << 32) if h >= 1 << 31 else h)
        if bads and bad < 0:
            bad = (k << 32) | bads[0]
    return per, np.array(stats, dtype=np.int32).reshape(-1, 4), hashes, bad
