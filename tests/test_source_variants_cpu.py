"""CPU tests of candidates from source VCF lines (include/platypus_caller_source.h, plat_source_variants_batch): the plain-Python
restatement (regionprep) and the host parser (libplat_caller's debug export) against the reference's own reader text
(tests/golden/source_cases.json.gz), the order of variantutils.py:161, the Python and the native region loop (on the CPU stand-in device:
the host parser) against the reference's region loop with that reader (source_region_cases.json.gz), the C header and its mirrors, the
setter's refusals, and that nothing changes for a call without source lines."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from platypus_amd import _lib, fastcaller as F, hostapi as H, regionprep as RP
from platypus_amd.options import default_options
from tests import region_golden as R
from tests import source_golden as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = S.load("source_cases.json.gz")
REGION_CASES = S.load("source_region_cases.json.gz")


@pytest.fixture(scope="module")
def fake():
    from tests import fakedev
    old = H._engine
    H._engine = fakedev.fake_engine()
    yield fakedev.fake_caller_lib()
    H._engine = old


def test_fixtures_cover_the_rule():
    """What the generator asserted when it wrote the files, checked again on the committed data."""
    text = "".join(c["text"] for c in CASES)
    assert len(CASES) >= 60 and sum(len(c["alleles"]) for c in CASES) >= 1500
    assert any(c["longHaps"] for c in CASES) and any(c["maxSize"] < 100 for c in CASES) and any(not c["text"].endswith("\n") for c in CASES)
    for needle in ("\t.\t", "\t*", "<DEL>", "\tA,\t", "\t,C", "\t0\t"):
        assert needle in text or needle.strip("\t") in text
    assert sum(len(c["ordered"]) < len(c["alleles"]) for c in CASES) >= 1            # duplicates collapsed by the set
    ties = 0
    for c in CASES:
        o = c["ordered"]
        ties += any(a[0] == b[0] and len(a[1]) == len(b[1]) and ((len(a[1]) == len(a[2]) == len(b[2]) == 1) or (len(a[1]) == 0 and a[2] and b[2]))
                    for a, b in zip(o, o[1:]))
    assert ties >= 10
    why = " ".join(c["why"] for c in REGION_CASES)
    opts = [c["options"] for c in REGION_CASES]
    assert any(o.get("getVariantsFromBAMs") == 0 for o in opts) and any(o.get("assemble") for o in opts) and any(o.get("longHaps") for o in opts)
    assert any(len(c["sample_names"]) == 2 for c in REGION_CASES) and any(len(c["regions"][0]["source"]) == 2 for c in REGION_CASES)
    lines = [ln for c in REGION_CASES for ln in c["lines"]]
    assert any("Source=File" in ln for ln in lines) and any("Platypus,File" in ln or "File,Platypus" in ln for ln in lines) and "no read" in why


@pytest.mark.parametrize("ci", range(len(CASES)))
def test_python_restatement_and_host_parser_equal_the_references_reader(fake, ci):
    c = CASES[ci]
    text = c["text"].encode()
    want = [(p, r.encode(), a.encode()) for p, r, a in c["alleles"]]
    got, stats, bad = RP.sourceTextAlleles(text, c["maxSize"], c["longHaps"])
    assert not bad and [(p, r, a) for p, r, a, _ in got] == want
    d = S.host_parse(fake, [text], [c["chrom"]], c["maxSize"], c["longHaps"])
    assert int(d["status"][0]) == 0 and int(d["status"][2]) == len(want) and int(d["status"][3]) == stats["lines"]
    assert S.alleles_of(d) == got                                                      # positions, bytes AND line numbers
    assert list(d["stats"][0]) == [stats["lines"], stats["skipped"], stats["invalid"], stats["oversize"]]
    assert list(d["hash"]) == S.python_parse([text], [c["chrom"]], c["maxSize"], c["longHaps"])[2]
    # the order of :161: the Python restatement and the host's replay
    ordered = [(p, r.encode(), a.encode()) for p, r, a in c["ordered"]]
    vs = RP.sourceVariants(c["chrom"], [text], c["maxSize"], c["longHaps"])
    assert [(v.refPos, v.removed, v.added) for v in vs] == ordered
    assert all(v.varSource == H.FILE_VAR and v.nSupportingReads == 0 for v in vs)
    alleles = S.alleles_of(d)
    assert [alleles[i][:3] for i in S.host_order(fake, d["text"], d, 0, len(alleles))] == ordered


def test_host_parser_refusals_capacity_and_offsets(fake):
    regions = [b"20\t5\t.\tA\tC,G\n20\t7\t.\tA\n20\t9\t.\tAT\tA\n", b"", b"#header\n\n20\tx1\t.\tA\tC\n20\t4294967297\t.\tA\tC\n20\t12\t.\tC\tT"]
    names = ["20", "20", "20"]
    d = S.host_parse(fake, regions, names)
    per, stats, hashes, bad = S.python_parse(regions, names)
    assert int(d["status"][0]) == -9 and int(d["status"][1]) == bad == 1                 # region 0, line 1: four columns
    assert [S.alleles_of(d, int(d["region_begin"][k]), int(d["region_begin"][k + 1])) for k in range(3)] == per
    assert (d["stats"] == stats).all() and list(d["stats"][2]) == [5, 2, 0, 0] and list(d["hash"]) == hashes
    ok = [b"20\t5\t.\tA\tC,G,T\n", b"20\t6\t.\tA\tAT\n"]
    d = S.host_parse(fake, ok, ["20", "20"], cap=2)
    assert list(d["status"]) == [-8, -1, 4, 2] and len(d["pos"]) == 2 and list(d["region_begin"]) == [0, 2, 2]
    d = S.host_parse(fake, ok, ["20", "20"], text_off=[0, 40, 30])
    assert int(d["status"][0]) == -1


@pytest.mark.parametrize("ci", range(len(REGION_CASES)))
def test_region_loops_write_the_references_records(fake, ci):
    case = REGION_CASES[ci]
    got, rlen = S.python_loop_text(case)
    assert got == case["lines"], R.diff(got, case["lines"])
    assert rlen == case["rlen_after"]
    got, rlen, st = S.native_loop_text(case, fake)
    assert got == case["lines"], R.diff(got, case["lines"])
    assert rlen == case["rlen_after"] and st["n_windows_failed"] == 0
    assert st["n_source_lines"] == sum(t.count("\n") for reg in case["regions"] for t in reg["source"]) and st["n_source_variants"] > 0
    assert st["n_regions_stage_b_device"] == 0


def test_without_source_lines_nothing_changes(fake):
    """An existing region case gives the text it gives today; source lines apply to ONE call; the setter and the call refuse what does not match."""
    base = R.load_cases()[0]
    want, rlen, failed = R.native_loop_text(base, fake)
    assert want == base["lines"]
    case = REGION_CASES[0]
    nc = F.NativeCaller(0, 2, 2, lib=fake)
    try:
        with_source, _, _ = S.native_loop_text(case, nc=nc)
        assert with_source == case["lines"]
        again, _, st = S.native_loop_text(case, nc=nc, source=False)           # the lines were cleared when the call returned
        assert again == base["lines"] == want and st["n_source_lines"] == 0 and st["n_source_variants"] == 0
        # a list of another length: the call is refused, and the lines are gone with it
        fasta, work, names = R.case_work(case)
        regs = [F.RegionReads.from_buffers(c, s, e, fasta, b) for c, s, e, b in work]
        with pytest.raises(_lib.PlatypusDeviceError) as e:
            nc.call_regions(regs, names, default_options(), source_lines=S.region_source(case) + [b""])
        assert e.value.code == -1 and "set_source_lines" in str(e.value)
        assert nc.call_regions(regs, names, default_options()).split("\n")[:-1] == want
        # no candidate source at all is still refused, with the message it had; with source lines set it is legal
        with pytest.raises(_lib.PlatypusDeviceError) as e:
            nc.call_regions(regs, names, default_options(getVariantsFromBAMs=0))
        assert e.value.code == -6 and "leaves no candidate source (source VCFs are not built)" in str(e.value)
        o = default_options(getVariantsFromBAMs=0, rlen=123)
        nc.call_regions(regs, names, o, source_lines=S.region_source(case))
        assert o.rlen == 123                                                   # rlen is left as it was
        # a line pysam would raise on ends the call, naming region and line
        with pytest.raises(_lib.PlatypusDeviceError) as e:
            nc.call_regions(regs, names, default_options(), source_lines=[b"20\t700\t.\tA\tC\n20\t701\tA\n"])
        assert e.value.code == -9 and "line 1" in str(e.value)
        # NULL arguments
        assert fake.plat_caller_set_source_lines(None, None, 0, 0) == -1 and fake.plat_caller_set_source_lines(nc.h, None, 1, 0) == -1
        # an empty list takes back lines set earlier: the next call is a call without source lines, refusal included
        keep = nc.set_source_lines(S.region_source(case))
        assert fake.plat_caller_set_source_lines(nc.h, None, 0, 0) == 0
        assert nc.call_regions(regs, names, default_options()).split("\n")[:-1] == want and nc.stats["n_source_lines"] == 0
        keep = nc.set_source_lines(S.region_source(case))
        assert fake.plat_caller_set_source_lines(nc.h, None, 0, 0) == 0
        with pytest.raises(_lib.PlatypusDeviceError) as e:
            nc.call_regions(regs, names, default_options(getVariantsFromBAMs=0))
        assert e.value.code == -6
        del keep
    finally:
        nc.close()


def test_stream_front_end_takes_the_lines_by_list_position(fake):
    """plat_call_regions_stream with source lines: regions loaded on demand get the lines of their place in the list (two regions, one per chunk)."""
    case = next(c for c in REGION_CASES if len(c["regions"]) == 2)
    fasta, work, names = R.case_work(case)
    regs = [F.RegionReads.from_buffers(c, s, e, fasta, b) for c, s, e, b in work]
    src = S.region_source(case)
    assert src[0] != src[1]
    for per_chunk in (1, 2):
        nc = F.NativeCaller(0, 2, per_chunk, lib=fake)
        try:
            def load(index, slot, out):
                regs[index].fill(out, len(names))
                return 0
            o = default_options(**case["options"])
            got = nc.call_stream(len(regs), load, None, names, o, n_slots=4, n_loaders=2, source_lines=src)
            assert got.split("\n")[:-1] == case["lines"] and o.rlen == case["rlen_after"]
            assert nc.stats["n_source_lines"] == sum(t.count(b"\n") for r in src for t in r) and nc.stats["n_source_chunks_device"] == 0
            swapped = nc.call_stream(len(regs), load, None, names, default_options(**case["options"]), n_slots=4, n_loaders=2, source_lines=src[::-1])
            assert swapped.split("\n")[:-1] != case["lines"]                  # (the place in the list is what assigns the lines)
            assert nc.call_stream(len(regs), load, None, names, default_options(**case["options"]), n_slots=4, n_loaders=2) == \
                nc.call_regions(regs, names, default_options(**case["options"]))
        finally:
            nc.close()


def test_cli_reads_plain_and_gzip_source_files(tmp_path):
    import gzip
    from platypus_amd.__main__ import read_source_lines
    from platypus_amd.options import build_parser
    body = b"##fileformat=VCFv4.1\n#CHROM\tPOS\n20\t5\t.\tA\tC\n\n20\t9\trs\tAT\tA\tq\r\n"
    (tmp_path / "a.vcf").write_bytes(body)
    with gzip.open(tmp_path / "a.vcf.gz", "wb") as f:
        f.write(body)
    want = [b"20\t5\t.\tA\tC", b"20\t9\trs\tAT\tA\tq"]
    assert read_source_lines(str(tmp_path / "a.vcf")) == want == read_source_lines(str(tmp_path / "a.vcf.gz"))
    o = build_parser().parse_args(["--source", "%s,%s" % (tmp_path / "a.vcf", tmp_path / "a.vcf.gz"), "--longHaps", "1", "--synthetic", "config4:2"])
    assert o.sourceFile == [str(tmp_path / "a.vcf"), str(tmp_path / "a.vcf.gz")] and o.longHaps == 1
    text = " ".join(build_parser().format_help().split())
    assert "STAND-IN for a tabix fetch" in text and "LEAVES IT OUT" in text
    # the stand-in leaves out what it cannot place; the same line inside a fetch handed over as text raises
    r = H.VariantCandidateReader([want + [b"20\t7\tA", b"20\tx\t.\tA\tC"]], o)
    assert [(v.refPos, v.removed, v.added) for v in r.Variants("20", 0, 100)] == [(4, b"A", b"C"), (8, b"AT", b"A")]      # (--longHaps=1: untrimmed)


def test_hostapi_reader_fetches_by_overlap():
    o = default_options()
    lines = b"##x\n20\t100\t.\tA\tC,G\n20\t150\t.\tATTT\tA\n21\t100\t.\tA\tT\n20\t5000\t.\tA\tT\n"
    r = H.VariantCandidateReader([lines], o)
    assert [(v.refPos, v.removed, v.added) for v in r.Variants("20", 0, 200)] == [(99, b"A", b"C"), (99, b"A", b"G"), (149, b"TTT", b"")]
    assert [v.refPos for v in r.Variants("20", 152, 153)] == [149]           # the record's span [149, 153) reaches into the region
    assert r.Variants("20", 153, 4999) == [] and [v.refPos for v in r.Variants("20", 4999, 5000)] == [4999]
    with pytest.raises(ValueError):
        H.VariantCandidateReader([{("20", 0, 10): b"20\t1\tA\n"}], o).Variants("20", 0, 10)


def test_source_header_is_c_and_structs_match_their_mirrors(tmp_path):
    F.build()
    src = tmp_path / "lay.c"
    src.write_text(r'''
#include <stdio.h>
#include <stddef.h>
#include "platypus_caller_source.h"
#include "platypus_mi355x.h"
int main(void){
  printf("%zu %zu\n", sizeof(plat_source_lines), offsetof(plat_source_lines, len));
  printf("%zu %zu %zu %zu\n", sizeof(plat_source_variants_in), offsetof(plat_source_variants_in, text), offsetof(plat_source_variants_in, text_off),
         offsetof(plat_source_variants_in, name_hash));
  printf("%zu %zu %zu %zu\n", sizeof(plat_source_variants_out), offsetof(plat_source_variants_out, region_begin), offsetof(plat_source_variants_out, line),
         offsetof(plat_source_variants_out, status));
  printf("%zu %zu %zu\n", sizeof(plat_caller_stats), offsetof(plat_caller_stats, n_source_lines), offsetof(plat_caller_stats, seconds_source));
  { int (*fn)(plat_caller*, const plat_source_lines*, int, int) = plat_caller_set_source_lines; printf("%d\n", fn(NULL, NULL, 0, 0)); }
  { int (*fn)(plat_ctx*, const plat_source_variants_in*, const plat_source_variants_out*, void*) = plat_source_variants_batch; printf("%d\n", fn(NULL, NULL, NULL, NULL)); }
  return 0; }''')
    exe = tmp_path / "lay"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic-errors", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L" + os.path.dirname(F.LIB_PATH), "-lplat_caller", "-lplat_mi355x", "-Wl,-rpath," + os.path.dirname(F.LIB_PATH)])
    v = list(map(int, subprocess.check_output([str(exe)], text=True).split()))
    L, I, O, T = F._SourceLines, _lib.SourceVariantsIn, _lib.SourceVariantsOut, F.CallerStats
    assert v[0:2] == [C.sizeof(L), L.len.offset]
    assert v[2:6] == [C.sizeof(I), I.text.offset, I.text_off.offset, I.name_hash.offset]
    assert v[6:10] == [C.sizeof(O), O.region_begin.offset, O.line.offset, O.status.offset]
    assert v[10:13] == [C.sizeof(T), T.n_source_lines.offset, T.seconds_source.offset]
    assert v[13:15] == [-1, -1]                                                # (PLAT_ERR_INVALID for NULL arguments: the symbols link and run)
    assert "plat_source_variants_batch" in _lib.SIGNATURES and hasattr(_lib.load(), "plat_source_variants_batch")


def test_host_parser_under_the_sanitizers(tmp_path):
    """tests/source_parse_driver.cpp: the host parser as a stand-alone program built with -fsanitize=address,undefined, fed the golden inputs
    and seeded random and truncated bytes."""
    exe = tmp_path / "source_parse_driver"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "source_parse_driver.cpp"), "-o", str(exe)])
    inp = tmp_path / "texts.bin"
    with open(inp, "wb") as f:
        for c in CASES:
            t = c["text"].encode()
            f.write(len(t).to_bytes(8, "little") + c["maxSize"].to_bytes(4, "little") + c["longHaps"].to_bytes(4, "little") + t)
    out = subprocess.check_output([str(exe), str(inp)], text=True)
    first = out.split("\n")[0].split()
    assert first[0] == "golden" and int(first[1]) == len(CASES) and int(first[2]) == sum(len(c["alleles"]) for c in CASES)
    assert "fuzz" in out and "truncated" in out and out.strip().endswith("ok")
