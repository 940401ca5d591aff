"""CPU tests of the read counts of reference-call blocks (plat_refcall_coverage_batch, csrc/refcov_rule.hpp): the rule and its tile
decomposition as a stand-alone program under the sanitizers, the C structs against their ctypes mirrors, and the native region loop on the
CPU stand-in device -- which predates the entry point: the host's loop runs there and the text is the Python loop's."""
import ctypes as C
import io
import os
import subprocess

import pytest

from platypus_amd import _lib, caller, fastcaller as F, hostapi as H, synth
from platypus_amd.options import default_options
from platypus_amd.vcfrecords import VCF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fake():
    from tests import fakedev
    old = H._engine
    H._engine = fakedev.fake_engine()
    yield fakedev.fake_caller_lib()
    H._engine = old


def test_rule_and_tile_decomposition_under_the_sanitizers(tmp_path):
    """tests/refcov_driver.cpp: count_at against the naive loop of countReadsCoveringRegion, and tile_range + count_in on a copy of exactly
    the staged range (pos[iLo, iHi), end[iLo, iHi]) in exact-size heap blocks -- ordinary tables, odd ones (negative `longest`, reads at
    position 0, malformed reads, tiny tiles) and the ends of the number range."""
    exe = str(tmp_path / "refcov_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-I", os.path.join(ROOT, "platypus_amd", "csrc"), os.path.join(ROOT, "tests", "refcov_driver.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:verify_asan_link_order=0")     # (as tests/test_native_caller_cpu.py builds and runs its drivers)
    out = subprocess.run([exe], env=env, capture_output=True, text=True)
    assert out.returncode == 0, (out.stdout[-1000:], out.stderr[-2000:])
    lines = out.stdout.split("\n")
    fam = {ln.split()[0]: [int(x) for x in ln.split()[1:]] for ln in lines if len(ln.split()) == 3}
    assert fam["ordinary"][0] == 300 and fam["ordinary"][1] > 400000 and fam["odd"][0] == 300 and fam["odd"][1] > 100000 and fam["extremes"][1] > 1000
    assert out.stdout.strip().endswith("ok")


def test_header_is_c_and_structs_match_their_mirrors(tmp_path):
    F.build()
    src = tmp_path / "lay.c"
    src.write_text(r'''
#include <stdio.h>
#include <stddef.h>
#include "platypus_caller.h"
#include "platypus_mi355x.h"
int main(void){
  printf("%zu %zu %zu %zu %zu %zu\n", sizeof(plat_refcov_in), offsetof(plat_refcov_in, n_reads), offsetof(plat_refcov_in, read_pos), offsetof(plat_refcov_in, slice_longest),
         offsetof(plat_refcov_in, iv_count_off), offsetof(plat_refcov_in, iv_tile_first));
  printf("%zu %zu %zu\n", sizeof(plat_refcov_out), offsetof(plat_refcov_out, iv_min), offsetof(plat_refcov_out, counts));
  printf("%zu %zu %zu %zu\n", sizeof(plat_caller_stats), offsetof(plat_caller_stats, n_refcall_intervals_device), offsetof(plat_caller_stats, n_refcall_positions_device),
         offsetof(plat_caller_stats, n_refcall_intervals_host));
  printf("%d %d %d\n", PLAT_REFCOV_RAISES, PLAT_REFCOV_EMPTY, PLAT_REFCOV_TILE);
  { int (*fn)(plat_ctx*, const plat_refcov_in*, const plat_refcov_out*, void*) = plat_refcall_coverage_batch; printf("%d\n", fn(NULL, NULL, NULL, NULL)); }
  { int (*fn)(void) = plat_refcov_lds_reads; printf("%d\n", fn()); }
  return 0; }''')
    exe = tmp_path / "lay"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic-errors", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L" + os.path.dirname(F.LIB_PATH), "-lplat_caller", "-lplat_mi355x", "-Wl,-rpath," + os.path.dirname(F.LIB_PATH)])
    v = list(map(int, subprocess.check_output([str(exe)], text=True).split()))
    I, O, T = _lib.RefCovIn, _lib.RefCovOut, F.CallerStats
    assert v[0:6] == [C.sizeof(I), I.n_reads.offset, I.read_pos.offset, I.slice_longest.offset, I.iv_count_off.offset, I.iv_tile_first.offset]
    assert v[6:9] == [C.sizeof(O), O.iv_min.offset, O.counts.offset]
    assert v[9:13] == [C.sizeof(T), T.n_refcall_intervals_device.offset, T.n_refcall_positions_device.offset, T.n_refcall_intervals_host.offset]
    assert T.n_refcall_intervals_host.offset + 8 == C.sizeof(T)                  # (the new counters are the LAST fields)
    assert v[13:16] == [_lib.PLAT_REFCOV_RAISES, _lib.PLAT_REFCOV_EMPTY, _lib.PLAT_REFCOV_TILE]
    assert v[16] == -1 and 256 <= v[17] <= 1 << 15                               # (PLAT_ERR_INVALID for NULL arguments: the symbols link and run)
    assert "plat_refcall_coverage_batch" in _lib.SIGNATURES and hasattr(_lib.load(), "plat_refcall_coverage_batch")
    for name in ("plat_refcall_coverage_batch", "plat_refcov_lds_reads"):
        assert name in _lib.ADDED_LATER


@pytest.mark.parametrize("ns", [1, 2])
def test_stand_in_device_runs_the_hosts_loop(fake, ns):
    """outputRefCalls=1 on the CPU stand-in: no interval from the device, every REFCALL decision by the host's loop over refcov_rule.hpp, the
    text of the Python loop; without outputRefCalls none of the counters moves."""
    names = ["S%d" % (i + 1) for i in range(ns)]
    regs = [synth.config4_region(430 + i, n_samples=ns, region_len=2500, snp_rate=5e-3, indel_rate=1.5e-3, read_len=100, depth=[30, 6][i % 2]) for i in range(3)]
    fasta = H.FastaFile({r["chrom"]: r["ref"] for r in regs})
    work = [(r["chrom"], r["start"], r["end"], [H.bamReadBuffer([H.AlignedRead(x["seq"], x["qual"], x["pos"], x["mapq"], x["flag"], end=x["end"], cigarOps=x["cigar"])
                                                                 for x in reads], sample=names[i]) for i, reads in enumerate(r["samples"])]) for r in regs]
    for opt in (dict(outputRefCalls=1, refCallBlockSize=150), dict()):
        py = io.StringIO()
        caller.callVariantsInRegions(work, fasta, default_options(**opt), VCF(names), py)
        nc = F.NativeCaller(0, 2, 2, lib=fake)
        txt = nc.call_regions([F.RegionReads.from_buffers(c, s, e, fasta, b) for c, s, e, b in work], names, default_options(**opt))
        st = nc.stats
        nc.close()
        assert txt == py.getvalue() and txt.count("\n") > 10
        assert st["n_refcall_intervals_device"] == 0 and st["n_refcall_positions_device"] == 0
        if opt:
            assert st["n_refcall_records"] == txt.count("\tREFCALL\t") > 20 and st["n_refcall_intervals_host"] >= st["n_refcall_records"]
        else:
            assert st["n_refcall_intervals_host"] == 0 and st["n_refcall_records"] == 0
