"""CPU tests of the indexed FASTA fetch (plat_fasta_fetch_batch, include/platypus_caller_fasta.h): the fixture
(tests/golden/fasta_cases.json.gz, README_fasta.md) pins the HOST TWIN (csrc/fasta_rule.hpp through tests/fasta_host_driver.cpp: the span
arithmetic, the byte map and the .fai parse the kernels read too) to what the reference's getRefs / getSequence / getCharacter return or
raise; the rule runs under the sanitizers as a stand-alone program.  Through the stand-in device: the caller library refuses cleanly
without plat_fasta_fetch_batch, and with PLAT_CALLER_HOST_FASTA=1 answers the fixture's queries and feeds the region goldens from a
FASTA file.  tests/test_gpu_fasta.py repeats it on the device."""
import ctypes as C
import os
import subprocess

import pytest

from platypus_amd import _lib, fastcaller as F
from platypus_amd.options import default_options
from tests import fasta_cases as FC, region_golden as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILES, BAD = FC.golden_files()


def test_fixture_covers_the_rule():
    qs = [q for f in FILES for q in f["queries"]]
    assert len(FILES) == 7 and len(qs) >= 500 and sum(len(f["chars"]) for f in FILES) >= 150
    assert sum(q["raises"] == "IndexError" for q in qs) >= 30 and sum(q["raises"] == "ZeroDivisionError" for q in qs) >= 20
    assert any(b"\r" in (q["seq"] or b"") for q in qs) and any(b">" in (q["seq"] or b"") for q in qs) and any(b"\x00" in (q["seq"] or b"") for q in qs)
    assert any(q["seq"] == b"" and q["beg"] != q["end"] for f in FILES if "lies" in f["label"] for q in f["queries"])      # wholly past the end of the file
    assert any(c["char"] == b"" for f in FILES for c in f["chars"]) and any(c["raises"] for f in FILES for c in f["chars"])
    assert any(f["refs0"].keys() != f["refs1"].keys() for f in FILES) and len(BAD) == 3


def test_rule_runs_clean_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "fasta_rule_driver")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DFASTA_DRIVER_MAIN",
                           "-I" + os.path.join(ROOT, "platypus_amd", "csrc"), os.path.join(ROOT, "tests", "fasta_host_driver.cpp"), "-o", exe])
    out = subprocess.check_output([exe], text=True)
    assert out.startswith("fasta rule driver OK")


@pytest.mark.parametrize("fi", range(len(FILES)))
def test_host_twin_equals_the_fixture(fi):
    f = FILES[fi]
    qs = [FC.entry_of(f["refs1"], q["name"]) + (q["beg"], q["end"], 0) for q in f["queries"]]
    seqs, status = FC.twin_fetch(f["fasta"], qs)
    for q, s, st in zip(f["queries"], seqs, status):
        assert FC.RAISES.get(st) == q["raises"], (f["label"], q)
        if q["raises"] is None:
            assert s == q["seq"], (f["label"], q["name"], q["beg"], q["end"])
    for c in f["chars"]:
        ch, st = FC.twin_char(f["fasta"], FC.entry_of(f["refs1"], c["name"]), c["pos"])
        assert FC.RAISES.get(st) == c["raises"] and (c["raises"] or ch == c["char"]), (f["label"], c)
    # the whole-contig mode: getSequence's bytes and the last base getSequence never returns (where the index tells the truth about its lines)
    if "ragged" not in f["label"] and "lies" not in f["label"]:
        for name, v in f["refs1"].items():
            whole, st = FC.twin_fetch(f["fasta"], [FC.entry_of(f["refs1"], name) + (5, 2, 1)])
            most, _ = FC.twin_fetch(f["fasta"], [FC.entry_of(f["refs1"], name) + (0, v[1], 0)])
            last, _ = FC.twin_char(f["fasta"], FC.entry_of(f["refs1"], name), v[1] - 1)
            assert st == [0] and whole[0] == most[0] + last and len(whole[0]) == v[1] + ((v[1] - 1) // v[3] if "CRLF" in f["label"] else 0)


@pytest.mark.parametrize("fi", range(len(FILES)))
def test_fai_parse_equals_getrefs(fi):
    f = FILES[fi]
    for ncbi, want in ((0, f["refs0"]), (1, f["refs1"])):
        got = FC.twin_refs(f["fai"], ncbi)
        assert got == {k: tuple(v[1:]) for k, v in want.items()}, (f["label"], ncbi)
    for b in BAD:
        rcs = [r[0] for r in FC.twin_parse(b["fai"].encode("latin-1"), 1)]
        assert b["raises"] == "IndexError" and any(rcs) and rcs.index(next(r for r in rcs if r)) + 1 == int(b["names"].split()[1])


def test_structs_match_their_ctypes_mirrors_and_the_symbols_are_declared(tmp_path):
    F.build()
    src = tmp_path / "lay.c"
    src.write_text(r'''
#include <stdio.h>
#include <stddef.h>
#include "platypus_mi355x.h"
#include "platypus_caller_fasta.h"
int main(void){
  printf("%zu %zu %zu %zu %zu %zu\n", sizeof(plat_fasta_fetch_in), sizeof(plat_fasta_fetch_out), offsetof(plat_fasta_fetch_in, n_queries), offsetof(plat_fasta_fetch_in, mode),
         offsetof(plat_fasta_fetch_out, out), sizeof(plat_fasta_info));
  printf("%d %d %d %d %d %d %d %d %d\n", PLAT_FASTA_STATUS_WORDS, PLAT_FASTA_OK, PLAT_FASTA_INDEX_ERROR, PLAT_FASTA_ZERO_LINE, PLAT_FASTA_BAD_INDEX, PLAT_FASTA_LEFT_OF_CUT,
         PLAT_FASTA_RIGHT_OF_CUT, PLAT_FASTA_MODE_SEQUENCE, PLAT_FASTA_MODE_CONTIG);
  { int (*fn)(plat_ctx*, const plat_fasta_fetch_in*, const plat_fasta_fetch_out*, void*) = plat_fasta_fetch_batch; printf("%d %d\n", fn(NULL, NULL, NULL, NULL), plat_fasta_tile_bytes()); }
  return 0; }''')
    exe = tmp_path / "lay"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L" + os.path.dirname(F.LIB_PATH), "-lplat_caller",
                           "-lplat_mi355x", "-Wl,-rpath," + os.path.dirname(F.LIB_PATH)])
    vals = list(map(int, subprocess.check_output([str(exe)], text=True).split()))
    I, O = _lib.FastaFetchIn, _lib.FastaFetchOut
    assert vals[:6] == [C.sizeof(I), C.sizeof(O), I.n_queries.offset, I.mode.offset, O.out.offset, C.sizeof(F.FastaInfo)]
    assert vals[6:15] == [_lib.FASTA_STATUS_WORDS, _lib.FASTA_OK, _lib.FASTA_INDEX_ERROR, _lib.FASTA_ZERO_LINE, _lib.FASTA_BAD_INDEX, _lib.FASTA_LEFT_OF_CUT,
                          _lib.FASTA_RIGHT_OF_CUT, _lib.FASTA_MODE_SEQUENCE, _lib.FASTA_MODE_CONTIG] == [4] + list(range(6)) + [0, 1]
    assert vals[15] == -1 and vals[16] == 1024
    assert (FC.OK, FC.INDEX_ERROR, FC.ZERO_LINE, FC.BAD_INDEX, FC.LEFT_OF_CUT, FC.RIGHT_OF_CUT) == tuple(range(6))
    for name in ("plat_fasta_fetch_batch", "plat_fasta_tile_bytes"):
        assert name in _lib.SIGNATURES and name in _lib.ADDED_LATER and hasattr(_lib.load(), name)
        assert name in open(os.path.join(ROOT, "bindings", "cplat.pxd")).read()
    assert "HOST_FASTA" in open(os.path.join(ROOT, "platypus_amd", "csrc", "host", "switches.hpp")).read()


@pytest.fixture(scope="module")
def fake():
    from platypus_amd import hostapi as H
    from tests import fakedev
    old = H._engine
    H._engine = fakedev.fake_engine()
    yield fakedev.fake_caller_lib()
    H._engine = old


def test_fake_device_refuses_the_fetch_and_stays_usable(fake, monkeypatch):
    """The CPU stand-in device has no plat_fasta_fetch_batch: PLAT_ERR_UNSUPPORTED naming the symbol, twice, from the three entry points;
    every refusal at open comes with its message and the line."""
    monkeypatch.delenv("PLAT_CALLER_HOST_FASTA", raising=False)
    nc = F.NativeCaller(0, 1, 1, lib=fake)
    try:
        f = FILES[0]
        fa = nc.open_fasta(f["fasta"], f["fai"], 1)
        assert [r[0] for r in fa.refs] == [b"chr1", b"chr2", b"chrM"] and fa.total_length == 150 + 61 + 1
        assert [fa.tid(n) for n in (b"chr1", b"chr2", b"chrM", b"chr", b"")] == [0, 1, 2, -1, -1]
        assert list(fa.refs[0][1:]) == f["refs1"][b"chr1"][1:] and fa.refs[0][3:] == (60, 61)
        for _ in range(2):
            for call in (lambda: fa.load(), lambda: fa.contig(1), lambda: fa.get_sequences([(0, 0, 10)])):
                with pytest.raises(_lib.PlatypusDeviceError) as e:
                    call()
                assert e.value.code == -6 and "plat_fasta_fetch_batch" in str(e.value)
        start = fa.refs[0][2]
        assert fa.get_character(0, 0) == f["fasta"][start:start + 1].upper() and fa.get_character(0, 150) == b"-"
        for label, fai, line in [(b["label"], b["fai"].encode("latin-1"), b["names"]) for b in BAD] + FC.LIMIT_INDEXES:
            with pytest.raises(_lib.PlatypusDeviceError) as e:
                nc.open_fasta(f["fasta"], fai, 1)
            assert e.value.code == -9 and "plat_fasta_open" in str(e.value) and line + " " in str(e.value), (label, str(e.value))
        fa.close()
        assert nc.call_regions([], ["S1"], default_options()) == ""
    finally:
        nc.close()


def test_fake_device_host_fasta_answers_the_fixture(fake, monkeypatch):
    monkeypatch.setenv("PLAT_CALLER_HOST_FASTA", "1")
    nc = F.NativeCaller(0, 1, 1, lib=fake)
    try:
        for f in FILES:
            for ncbi, want in ((0, f["refs0"]), (1, f["refs1"])):
                fa = nc.open_fasta(f["fasta"], f["fai"], ncbi)
                assert {r[0]: list(r[1:]) for r in fa.refs} == {k: v[1:] for k, v in want.items()} and fa.total_length == sum(v[1] for v in want.values())
                if ncbi == 0:
                    fa.close()
            got, info = fa.get_sequences([(fa.tid(q["name"]), q["beg"], q["end"]) for q in f["queries"]], info=True)
            assert info["device_calls"] == 0 and info["queries"] == len(got)
            for q, g in zip(f["queries"], got):
                assert (FC.RAISES[g] == q["raises"]) if isinstance(g, int) else (q["raises"] is None and g == q["seq"]), (f["label"], q)
            for c in f["chars"]:
                if c["raises"]:
                    with pytest.raises(_lib.PlatypusDeviceError) as e:
                        fa.get_character(fa.tid(c["name"]), c["pos"])
                    assert e.value.code == -9 and "LineLength 0" in str(e.value)
                else:
                    assert fa.get_character(fa.tid(c["name"]), c["pos"]) == c["char"]
            with pytest.raises(_lib.PlatypusDeviceError) as e:
                fa.get_sequences([(0, 0, 5), (len(f["refs1"]), 0, 5)])
            assert e.value.code == -1 and "query 1" in str(e.value)
            if "lies" in f["label"]:
                with pytest.raises(_lib.PlatypusDeviceError) as e:
                    fa.contig(fa.tid(b"zero"))
                assert e.value.code == -9 and "plat_fasta_contig" in str(e.value) and "zero" in str(e.value)
                arr, dev = fa.contig(fa.tid(b"long"))                      # the file ends early: what is there
                assert dev is None and arr.tobytes() == f["fasta"][3:].replace(b"\n", b"").upper()
            fa.close()
        assert nc.call_regions([], ["S1"], default_options()) == ""
    finally:
        nc.close()


def test_fake_device_region_goldens_from_a_fasta_file(fake, monkeypatch, tmp_path):
    monkeypatch.setenv("PLAT_CALLER_HOST_FASTA", "1")
    got, want = FC.region_lines_through_fasta(fake, tmp_path, R.load_cases())
    assert len(want) == 245 and got == want, R.diff(got, want)
