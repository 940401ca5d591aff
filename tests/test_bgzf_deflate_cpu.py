"""CPU tests of the compressed VCF output (plat_bgzf_deflate_batch, include/platypus_caller_bgzfout.h): the HOST TWIN of the device encoder
(csrc/bgzf_deflate.hpp, built alone under AddressSanitizer and UBSan where libasan is installed) writes, for every case of
tests/bgzf_deflate_cases.py and both levels, the bytes the rule's Python restatement writes; gzip reads them back; every header field, BSIZE,
CRC32 and ISIZE is right; pieces begin on block boundaries; the inflate side (csrc/bgzf_inflate.hpp) accepts every block.  The same for
the seam corpus (seam_blocks, seam_fuzz, batch_cases), whose every named case is first shown to reach its seam.  The structs
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
def driver(tmp_path_factory):
    """The stand-alone host driver, built once: run(cases) -> (EOF block, {(case name, level): (bytes, piece_out_off, blocks, blocks the
    inflate side accepted)}) for both levels of every case."""
    d = tmp_path_factory.mktemp("bgzf_deflate_host")
    exe = str(d / "driver")
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I", os.path.join(ROOT, "platypus_amd", "csrc"),
            os.path.join(ROOT, "tests", "bgzf_deflate_host_driver.cpp"), "-o", exe]
    san = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan"], capture_output=True, text=True)
    if san.returncode != 0:
        subprocess.check_call(base)
    print("host driver built %s sanitizers" % ("with" if san.returncode == 0 else "WITHOUT"))
    runs = [0]

    def run(case_list):
        cases = [(name, text, off, lv) for name, text, off in case_list for lv in (0, 1)]
        runs[0] += 1
        fin, fout = str(d / ("cases%d.in" % runs[0])), str(d / ("cases%d.out" % runs[0]))
        with open(fin, "wb") as f:
            f.write(struct.pack("<I", len(cases)))
            for _, text, off, lv in cases:
                f.write(struct.pack("<iiq", lv, len(off) - 1, len(text)) + text + struct.pack("<%dq" % len(off), *off))
        r = subprocess.run([exe, fin, fout], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
        assert r.returncode == 0, (r.returncode, r.stderr[-3000:])       # 3: bytes behind the returned length; else a sanitizer report
        with open(fout, "rb") as f:
            raw = f.read()
        os.remove(fin)
        os.remove(fout)
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
    return run


@pytest.fixture(scope="module")
def twin(driver):
    """(EOF block, {(case name, level): (bytes, piece_out_off, blocks, blocks the inflate side accepted)}) of the 13 cases from the host driver."""
    return driver(K.cases())


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


def _new_cases():
    return K.seam_blocks() + K.seam_fuzz() + K.batch_cases()


def test_every_seam_case_reaches_its_seam():
    """Conditions on the inputs, from the restatement alone (K.reach: hashes, candidates, tokens, chain positions, bit positions): a named
    case that misses the seam it is there for fails here, not silently on the device."""
    seams = K.seam_blocks()
    names = [name for name, _, _ in seams]
    assert len(names) == len(set(names)) == len(K.SEAM_REACH) and not set(names) & {name for name, _, _ in K.cases()}
    for name, text, off in seams:
        got = K.case_reach(text, off)
        assert K.SEAM_REACH[name], name
        for key in K.SEAM_REACH[name]:
            assert got[key] > 0, (name, key)
        want = K.SEAM_REACH[name]
        print("%-62s %s" % (name, "%s: %d" % (want[0], got[want[0]]) if len(want) == 1 else "%d keys, each %d..%d times" % (
            len(want), min(got[k] for k in want), max(got[k] for k in want))))
        assert len(text) <= 3 * K.PAYLOAD
    by = {name: (text, off) for name, text, off in seams}
    # what the keys cannot say
    for period in (1, 7, 112):
        text, off = by["20 000 bytes of period %d, then 3 000 of four letters" % period]
        toks = K.tokens(text)
        assert len(text) == 23000 and sum(1 for t in toks if not isinstance(t, int) and t == (258, period)) >= 70
    assert len(by["a full block of runs"][0]) == K.PAYLOAD and (K.PAYLOAD + K.SEG - 1) // K.SEG == 260
    assert K.case_reach(*by["a full block of runs"])["a segment without a chain position in front of more chain"] >= 3
    text, off = by["codes of 31 bits at every bit of a word"]
    assert len(off) == 2 and all(K.reach(text)["a code of 31 bits at bit %d" % k] for k in range(32))
    text, off = by["either side of the stored threshold at 15 to 4000 bytes"]
    for a, b in zip(off[:-1], off[1:]):
        coded, n = len(K.fixed_huffman(K.tokens(text[a:b]))), b - a
        assert (len(K.block(text[a:b], 1)) - 26 == n + 5 and text[a:b] in K.block(text[a:b], 1)) == (coded >= n + 5)
        if n in (5, 6, 7, 8):                                              # (n bytes code to (9 n + 17) >> 3 bytes at most: n + 4 needs n >= 15)
            assert coded == (9 * n + 17) >> 3 < n + 4
    assert (9 * 14 + 17) >> 3 < 14 + 4 and (9 * 22 + 17) >> 3 < 22 + 5        # ... and n + 5 needs n >= 23: 15 and 23 are the least
    # two keys of one hash cannot agree in three bytes: the fourth byte alone moves the top eight bits of the hash
    k = np.frombuffer(b"ABC", dtype=np.uint8)
    assert len({int(K.hashes(bytes(k) + bytes([b]))[0]) >> 7 for b in range(256)}) == 256


def test_reach_of_the_13_cases_and_of_the_new_corpus():
    """The tally the profile note quotes: per property the blocks, positions or tokens of the old 13 cases, the named seams and the fuzz
    that reach it.  What the issue says the 13 cases reach and miss is asserted; so is what the fuzz and the batch cases are there for."""
    import collections
    import time
    t0 = time.time()
    tally = []
    for group in (K.cases(), K.seam_blocks(), K.seam_fuzz()):
        c = collections.Counter()
        for _, text, off in group:
            c.update(K.case_reach(text, off))
        tally.append(c)
    old, seams, fuzz = tally
    sizes = ("n = ", "stored at n + 5", "coded at n + 4", "a match of ", "text offset", "a code of ")
    for key in sorted(set(old) | set(seams) | set(fuzz)):
        if not key.startswith(sizes) or key in ("a match of hash 0", "a match of hash 0x7fff", "a code of 31 bits at bit 31"):
            print("%-66s %7d %7d %7d" % (key, old[key], seams[key], fuzz[key]))
    for what, keys in (("match lengths 4..12, 255..258 at 16 alignments, two endings", [k for k in seams if k.startswith("a match of ") and "ended" in k]),
                       ("text offset & 3 against n = 1..9", ["text offset & 3 == %d, n = %d" % (o, n) for o in range(4) for n in range(1, 10)]),
                       ("codes of 28+ bits at bit 0..31", ["a code of 28+ bits at bit %d" % k for k in range(32)])):
        print("%-66s %7s %7s %7s" % (what, *["%d/%d" % (sum(1 for k in keys if c[k]), len(keys)) for c in tally]))
    # the 13: all 16 alignments, candidates near and far, matches across segment edges, threads of 64 and of none ...
    assert all(old["a match at (%d, %d)" % (p, q)] for p in range(4) for q in range(4))
    assert old["a candidate in the tile back"] and old["a candidate 1 tiles back"] and old["a candidate 4 tiles back"] and old["a candidate 6+ tiles back"]
    assert old["a match across a segment edge"] and old["a thread of 64 chain positions"] and old["a thread of no chain position"]
    # ... but no empty segment in front of more chain, three stored blocks of one residue, few staging pairs, no wide code on bit 31
    assert old["a segment without a chain position"] > 0 == old["a segment without a chain position in front of more chain"]
    assert [old["stored at level 1, body & 3 == %d" % r] for r in range(4)] == [0, 3, 0, 0]
    assert [n for n in range(1, 9) if old["text offset & 3 == 2, n = %d" % n]] == [3] and [n for n in range(1, 9) if old["text offset & 3 == 3, n = %d" % n]] == [2, 5, 8]
    assert not any(old["a code of 31 bits at bit %d" % k] for k in range(32)) and sum(1 for k in range(32) if old["a code of 28+ bits at bit %d" % k]) <= 2
    assert old["hash 0"] and old["hash 0x7fff"] and not old["a match of hash 0"] and not old["a match of hash 0x7fff"]
    assert old["3 positions of one hash in a tile, keys differ"] and not old["a thread whose chain is bits 0 and 63 alone"]
    assert not old["pieces of 3+ blocks"] and not old["a match at 0xff00 - 4"] and not old["distance 32767"]
    # the fuzz
    fz = K.seam_fuzz()
    assert K.seam_fuzz() is fz and K.seam_fuzz(7) is not fz and [c[1:] for c in K.seam_fuzz(7)] != [c[1:] for c in fz]
    lens = [len(text) for _, text, _ in fz]
    assert len(fz) == 300 and lens.count(K.PAYLOAD) == 4 and all(1 <= n <= 6000 for n in lens if n != K.PAYLOAD) and min(lens) < 20 and max(lens) == K.PAYLOAD
    assert all(1 <= len(off) - 1 <= 40 and off[0] == 0 and off[-1] == len(text) and off == sorted(off) for _, text, off in fz)
    assert {len(off) - 1 for _, _, off in fz} >= {1, 2, 39, 40} and fuzz["empty pieces"] > 50
    assert {name.split(", ")[1] for name, _, _ in fz} == {"2 letters", "4 letters", "20 letters", "256 letters"}
    assert fuzz["full blocks"] == 2 and all(fuzz["stored at level 1, body & 3 == %d" % r] and fuzz["coded, body & 3 == %d" % r] for r in range(4))
    assert all(fuzz["distance %d" % d] for d in (1, 2, 3, 4)) and fuzz["a run longer than 258"] and fuzz["a candidate 6+ tiles back"]
    assert any(b >= 144 for _, text, _ in fz[:20] for b in text) and any(b"chr20\t" in text for _, text, _ in fz)
    # the batch cases
    batch = {name: (text, np.asarray(off)) for name, text, off in K.batch_cases()}
    assert len(batch) == 5
    text, off = batch["1100 pieces, long ones of 3000-9000 bytes among short ones of 1-70"]
    n = np.diff(off)
    long, short = n >= K.LONG_PIECE, n <= 70
    assert len(n) == 1100 and (long | short).all() and n.min() == 1 and n.max() <= 9000 and 150 < long.sum() < 300
    for grid in range(1, 513):                                             # whatever the CU count: some workgroup takes a long block, then a short one
        assert (long[:-grid] & short[grid:]).any(), grid
    head = K.BATCH_HEAD
    for a, b in zip(off[:-1].tolist(), off[1:].tolist()):                  # a short piece is every long one's first bytes, and goes on as they do
        assert text[a:min(b, a + 128)] == head[:b - a]
    assert all(head[k] == head[k - 7] for k in range(7, 128))
    some = [text[a:b] for a, b in zip(off[:-1].tolist(), off[1:].tolist()) if 12 <= b - a <= 70][:20]
    assert some and all(K.tokens(d)[-1] == (len(d) - 7, 7) for d in some)      # (a match to the block's end, which the stale bytes behind it would lengthen)
    text, off = batch["pieces of 3 x 0xff00 + 17 and of 2 x 0xff00 bytes among 300 small ones"]
    n = np.diff(off).tolist()
    assert len(n) == 302 and n[100] == 3 * K.PAYLOAD + 17 and n[201] == 2 * K.PAYLOAD and max(n[:100] + n[101:201] + n[202:]) < 200 and min(n) > 0
    text, off = batch["empty pieces at the front, at the end and in runs of 5"]
    n = np.diff(off).tolist()
    assert [k > 0 for k in n] == [False] * 5 + [True, False, True] + [False] * 5 + [True, True] + [False] * 5 + [True] + [False] * 5
    text, off = batch["9000 pieces of 0-40 bytes"]
    n = np.diff(off)
    assert len(n) == 9000 and n.min() == 0 and n.max() == 40 and (n > 0).sum() > 4096 and (n[4096:] > 0).sum() > 4096 - 200
    text, off = batch["5000 pieces of one byte"]
    assert len(off) == 5001 and (np.diff(off) == 1).all()
    total = sum(len(text) for _, text, _ in _new_cases())
    took = time.time() - t0
    print("new corpus: %d cases, %d bytes of text; reach and generation %.1f s" % (len(_new_cases()), total, took))
    assert 2_500_000 < total < 3_500_000


def test_host_twin_writes_the_restatements_bytes_on_the_seam_corpus(driver):
    """Every new case at both levels through the sanitized stand-alone driver: the restatement's bytes, offsets and block counts; gzip and
    the block parser agree; the inflate side accepts every block."""
    import time
    t0 = time.time()
    eof, got = driver(_new_cases())
    t1 = time.time()
    blocks_seen = 0
    for name, text, off in _new_cases():
        for lv in (0, 1):
            data, poff, blocks, accepted = got[(name, lv)]
            want, woff, sizes = K.compress(text, off, lv)
            assert data == want, (name, lv)
            assert poff == woff and blocks == len(sizes) == accepted, (name, lv)
            assert K.check_stream(data, poff, text, off) == blocks, (name, lv)
            blocks_seen += blocks
    print("%d blocks; the driver %.1f s, the restatement and the stream checks %.1f s" % (blocks_seen, t1 - t0, time.time() - t1))
    assert blocks_seen > 2 * (9000 * 40 // 41 + 5000 + 1100)


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
