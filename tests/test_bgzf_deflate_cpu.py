"""CPU tests of the compressed VCF output (plat_bgzf_deflate_batch, include/platypus_caller_bgzfout.h): the HOST TWIN of the device encoder
(csrc/bgzf_deflate.hpp, built alone under AddressSanitizer and UBSan where libasan is installed) writes, for every case of
tests/bgzf_deflate_cases.py and both levels, the bytes the rule's Python restatement writes; gzip reads them back; every header field, BSIZE,
CRC32 and ISIZE is right; pieces begin on block boundaries; the inflate side (csrc/bgzf_inflate.hpp) accepts every block.  The structs
match their ctypes mirrors and the Cython declarations build.  The caller library linked against the CPU stand-in device refuses
plat_caller_compress_text cleanly, and with PLAT_CALLER_HOST_DEFLATE=1 compresses a golden region call's text region by region."""
import ctypes as C
import gzip
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from platypus_amd import _lib, fastcaller as F
from platypus_amd.options import default_options
from tests import bgzf_deflate_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    """(EOF block, {(case name, level): (bytes, piece_out_off, blocks, blocks the inflate side accepted)}) from the host driver."""
    d = tmp_path_factory.mktemp("bgzf_deflate_host")
    exe = str(d / "driver")
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I", os.path.join(ROOT, "platypus_amd", "csrc"),
            os.path.join(ROOT, "tests", "bgzf_deflate_host_driver.cpp"), "-o", exe]
    san = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan"], capture_output=True, text=True)
    if san.returncode != 0:
        subprocess.check_call(base)
    print("host driver built %s sanitizers" % ("with" if san.returncode == 0 else "WITHOUT"))
    cases = [(name, text, off, lv) for name, text, off in K.cases() for lv in (0, 1)]
    fin, fout = str(d / "cases.in"), str(d / "cases.out")
    with open(fin, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for _, text, off, lv in cases:
            f.write(struct.pack("<iiq", lv, len(off) - 1, len(text)) + text + struct.pack("<%dq" % len(off), *off))
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])           # 3: bytes behind the returned length; else a sanitizer report
    with open(fout, "rb") as f:
        raw = f.read()
    out, at = {}, 28
    for name, text, off, lv in cases:
        n = struct.unpack_from("<q", raw, at)[0]
        data = raw[at + 8:at + 8 + n]
        at += 8 + n
        poff = list(struct.unpack_from("<%dq" % len(off), raw, at))
        at += 8 * len(off)
        blocks, accepted = struct.unpack_from("<qq", raw, at)
        at += 16
        out[(name, lv)] = (data, poff, blocks, accepted)
    assert at == len(raw)
    return raw[:28], out


def test_case_list_is_the_issues():
    names = [name for name, _, _ in K.cases()]
    assert len(names) == len(set(names)) == 13
    by = {name: (text, off) for name, text, off in K.cases()}
    assert by["no pieces"] == (b"", [0])
    assert [b - a for a, b in zip(by["runs of one byte"][1], by["runs of one byte"][1][1:])] == [258, 259, 260, 263]
    assert len(by["exactly 0xff00 bytes"][0]) == 0xff00 and len(by["0xff00 + 1 bytes"][0]) == 0xff00 + 1
    assert len(by["1000 pieces of 0-300 bytes"][1]) == 1001 and len(by["the golden processes' record lines"][1]) == 42
    # the restatement itself: the stored fallback's size, and the four blocks around the threshold
    text, off = by["either side of the stored threshold"]
    sizes = K.compress(text, off, 1)[2]
    assert sizes == [18 + 4003 + 8, 18 + 4004 + 8, 18 + 4005 + 8, 18 + 4005 + 8]      # n + 3, n + 4 coded; n + 5 and n + 6 would be: stored
    assert K.compress(*by["0xff00 random bytes"], 1)[2] == [65311]


def test_host_twin_writes_the_restatements_bytes(twin):
    eof, got = twin
    assert eof == K.EOF_BLOCK and len(eof) == 28 and gzip.decompress(eof) == b""
    for name, text, off in K.cases():
        for lv in (0, 1):
            data, poff, blocks, accepted = got[(name, lv)]
            want, woff, sizes = K.compress(text, off, lv)
            assert data == want, (name, lv)
            assert poff == woff and blocks == len(sizes) == accepted, (name, lv)
            assert K.check_stream(data, poff, text, off) == blocks, (name, lv)
            assert gzip.decompress(data + eof) == text
    # level 0 stores everything; level 1 stores what it cannot shorten
    data = got[("0xff00 random bytes", 1)][0]
    assert len(data) == 65311 and data[18] == 1 and got[("0xff00 random bytes", 0)][0] == data
    assert got[("exactly 0xff00 bytes", 1)][0][18] & 7 == 3                            # BFINAL 1, BTYPE 01


def test_golden_lines_deflate_to_under_half(twin):
    """The 245 golden record lines joined with newlines: 69 132 bytes in two blocks.  Level 1 gives 28 961 bytes, 0.419 of the input (zlib
    level 1 on the same two blocks: 0.348; level 6: 0.277)."""
    lines = [ln for case in K.golden_lines() for ln in case]
    text = b"".join(ln + b"\n" for ln in lines)
    assert len(lines) == 245 and len(text) == 69132
    data, off, sizes = K.compress(text, [0, len(text)], 1)
    print("golden lines: %d -> %d bytes (%.3f), blocks %s" % (len(text), len(data), len(data) / len(text), sizes))
    assert len(sizes) == 2 and gzip.decompress(data) == text
    assert len(data) == 28961 and 2 * len(data) < len(text)
    # the pieces of the twin's run are the same lines process by process
    got = twin[1][("the golden processes' record lines", 1)]
    assert gzip.decompress(got[0]) == text


def test_deflate_structs_match_their_ctypes_mirrors(tmp_path):
    F.build()
    src = tmp_path / "lay.c"
    src.write_text(r'''
#include <stdio.h>
#include <stddef.h>
#include "platypus_caller_bgzfout.h"
#include "platypus_mi355x.h"
int main(void){
  printf("%zu %zu %zu %zu %zu\n", sizeof(plat_bgzf_deflate_in), offsetof(plat_bgzf_deflate_in, text_len), offsetof(plat_bgzf_deflate_in, n_pieces),
         offsetof(plat_bgzf_deflate_in, level), offsetof(plat_bgzf_deflate_in, piece_off));
  printf("%zu %zu %zu %zu\n", sizeof(plat_bgzf_deflate_out), offsetof(plat_bgzf_deflate_out, data), offsetof(plat_bgzf_deflate_out, piece_out_off),
         offsetof(plat_bgzf_deflate_out, status));
  { int (*fn)(plat_caller*, const char*, size_t, const int64_t*, int, int, int, uint8_t**, size_t*, int64_t*) = plat_caller_compress_text;
    printf("%d\n", fn(NULL, NULL, 0, NULL, 0, 1, 1, NULL, NULL, NULL)); }
  { int (*fn)(plat_ctx*, const plat_bgzf_deflate_in*, const plat_bgzf_deflate_out*, void*) = plat_bgzf_deflate_batch;
    printf("%d\n", fn(NULL, NULL, NULL, NULL)); }
  return 0; }''')
    exe = tmp_path / "lay"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic-errors", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L" + os.path.dirname(F.LIB_PATH), "-lplat_caller", "-lplat_mi355x", "-Wl,-rpath," + os.path.dirname(F.LIB_PATH)])
    v = list(map(int, subprocess.check_output([str(exe)], text=True).split()))
    I, O = _lib.BgzfDeflateIn, _lib.BgzfDeflateOut
    assert v[0:5] == [C.sizeof(I), I.text_len.offset, I.n_pieces.offset, I.level.offset, I.piece_off.offset]
    assert v[5:9] == [C.sizeof(O), O.data.offset, O.piece_out_off.offset, O.status.offset]
    assert v[9:11] == [-1, -1]                                            # (PLAT_ERR_INVALID for NULL arguments: both symbols link and run)
    lib = _lib.load()
    assert "plat_bgzf_deflate_batch" in _lib.SIGNATURES and hasattr(lib, "plat_bgzf_deflate_batch") and len(_lib.SIGNATURES["plat_bgzf_deflate_batch"][1]) == 4
    assert "plat_bgzf_deflate_batch" in _lib.ADDED_LATER


def test_cython_declarations_of_the_deflate_entry_point_build(tmp_path):
    pytest.importorskip("Cython")
    pyx = tmp_path / "deflate_check.pyx"
    pyx.write_text('''# cython: language_level=3
from libc.string cimport memset
cimport cplat

def sizes():
    cdef cplat.plat_bgzf_deflate_in i
    cdef cplat.plat_bgzf_deflate_out o
    memset(&i, 0, sizeof(i))
    memset(&o, 0, sizeof(o))
    return (sizeof(i), sizeof(o), cplat.plat_bgzf_deflate_batch(NULL, &i, &o, NULL))
''')
    c_file = tmp_path / "deflate_check.c"
    subprocess.check_call([sys.executable, "-m", "cython", "-3", "-I", os.path.join(ROOT, "bindings"), str(pyx), "-o", str(c_file)])
    import sysconfig
    subprocess.check_call(["gcc", "-c", "-fPIC", "-O0", "-I" + sysconfig.get_paths()["include"], "-I" + os.path.join(ROOT, "include"), str(c_file),
                           "-o", str(tmp_path / "deflate_check.o")])


@pytest.fixture()
def host_deflate():
    old = os.environ.get("PLAT_CALLER_HOST_DEFLATE")
    os.environ["PLAT_CALLER_HOST_DEFLATE"] = "1"
    yield
    if old is None:
        del os.environ["PLAT_CALLER_HOST_DEFLATE"]
    else:
        os.environ["PLAT_CALLER_HOST_DEFLATE"] = old


def test_fake_device_caller_library_refuses_compress_text_and_stays_usable():
    """The CPU stand-in device has no plat_bgzf_deflate_batch: PLAT_ERR_UNSUPPORTED with a message naming the symbol, twice, and the caller
    works afterwards.  Bad lengths are refused before that."""
    from tests.fakedev import fake_caller_lib
    assert os.environ.get("PLAT_CALLER_HOST_DEFLATE") is None
    nc = F.NativeCaller(0, 1, 1, lib=fake_caller_lib())
    try:
        for _ in range(2):
            with pytest.raises(_lib.PlatypusDeviceError) as e:
                nc.compress_text(b"chr20\t1\n", [8])
            assert e.value.code == -6 and "plat_bgzf_deflate_batch" in str(e.value)
        for lens in ([7], [9], [4, -4, 8], []):
            with pytest.raises(_lib.PlatypusDeviceError) as e:
                nc.compress_text(b"chr20\t1\n", lens)
            assert e.value.code == -1 and ("sum" in str(e.value) or "negative" in str(e.value))
        with pytest.raises(_lib.PlatypusDeviceError) as e:
            nc.compress_text(b"chr20\t1\n", [8], level=2)
        assert e.value.code == -1
        assert nc.call_regions([], ["S1"], default_options()) == ""
    finally:
        nc.close()


def test_fake_device_host_deflate_compresses_a_golden_call_region_by_region(host_deflate):
    """PLAT_CALLER_HOST_DEFLATE=1 on the stand-in device: a golden two-region call's text, compressed with its per-region lengths, is the
    restatement's bytes; region_out_len sums to the output less the EOF block; the per-region compressed blocks of two 'ranks' merged by
    BlockOrder.merge, plus the EOF block, decompress to the merged plain text."""
    from tests import region_golden as G
    from tests.fakedev import fake_caller_lib
    from platypus_amd import sharding
    lib = fake_caller_lib()
    case = next(c for c in G.load_cases() if sum(1 for r in c["regions"] if r["loaded"]) >= 2 and len(c["lines"]) >= 4)
    fasta, work, names = G.case_work(case)
    nc = F.NativeCaller(0, 2, 1, lib=lib)
    try:
        regions = [F.RegionReads.from_buffers(c, s, e, fasta, b) for c, s, e, b in work]
        text = nc.call_regions(regions, names, default_options(**case["options"])).encode("ascii")
        lens = nc.region_text_lengths(len(regions))
        assert int(lens.sum()) == len(text) and text.split(b"\n")[:-1] == [ln.encode() for ln in case["lines"]]
        off = [0] + list(np.cumsum(lens))
        for lv in (0, 1):
            packed, out_lens = nc.compress_text(text, lens, level=lv, eof=True)
            packed = bytes(packed)
            want, woff, _ = K.compress(text, [int(x) for x in off], lv)
            assert packed == want + K.EOF_BLOCK and list(np.cumsum(out_lens)) == woff[1:]
            assert int(out_lens.sum()) == len(packed) - 28 and gzip.decompress(packed) == text
            assert all((n > 0) == (m > 0) for n, m in zip(lens, out_lens))
        # two ranks, regions dealt round-robin: compressed pieces merge as plain ones do
        keys = [[(sharding.chrom_key(c), s, e) for c, s, e, _ in work[r::2]] for r in range(2)]
        plain, plens, packs, zlens = [], [], [], []
        for r in range(2):
            t = nc.call_regions(regions[r::2], names, default_options(**case["options"])).encode("ascii")
            ln = nc.region_text_lengths(len(regions[r::2]))
            z, zl = nc.compress_text(t, ln, eof=False)
            plain.append(t); plens.append(ln); packs.append(z); zlens.append(zl)
        plan = F.BlockOrder(keys)
        assert plan.ok
        merged_plain = F.text_bytes(plan.merge(plain, plens, lib=lib))
        merged_packed = F.text_bytes(plan.merge(packs, zlens, lib=lib))
        assert merged_plain == text and gzip.decompress(merged_packed + K.EOF_BLOCK) == merged_plain
        K.parse_blocks(merged_packed + K.EOF_BLOCK)
        # an empty text: nothing but the EOF block
        z, zl = nc.compress_text(b"", [0, 0], eof=True)
        assert bytes(z) == K.EOF_BLOCK and list(zl) == [0, 0]
    finally:
        nc.close()
