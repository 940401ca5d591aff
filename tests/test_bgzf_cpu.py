"""CPU tests of the BGZF front end (plat_bgzf_inflate_batch, plat_bam_find_records, include/platypus_caller_bgzf.h): the C structs match
their ctypes mirrors, the new header compiles as C, the Cython declarations build, the caller library linked against the CPU stand-in
device refuses the call cleanly, the BGZF writer (synth.bgzf_block / bgzf_stream) writes what the specification says, and the HOST BUILD
of csrc/bgzf_inflate.hpp -- the code that indexes memory from input data, the same text the device compiles -- inflates the whole grid as
zlib does, refuses the corrupt corpus without touching a guard band (under AddressSanitizer and UBSan where libasan is installed), gives
zlib's verdict on the streams of tests/deflate_writer.py that zlib's encoder never writes, and walks records -- the window-seam ladder
included -- by the rule restated in tests/bgzf_cases.py."""
import ctypes as C
import gzip
import os
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

from platypus_amd import _lib, fastcaller as F, hostapi as H, synth
from platypus_amd.options import default_options
from tests import bgzf_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bgzf_structs_match_their_ctypes_mirrors(tmp_path):
    F.build()
    src = tmp_path / "lay.c"
    src.write_text(r'''
#include <stdio.h>
#include <stddef.h>
#include "platypus_caller_bgzf.h"
#include "platypus_mi355x.h"
int main(void){
  printf("%zu %zu %zu %zu %zu %zu\n", sizeof(plat_bgzf_chunk), offsetof(plat_bgzf_chunk, data_len), offsetof(plat_bgzf_chunk, first_uoffset),
         offsetof(plat_bgzf_chunk, end_coffset), offsetof(plat_bgzf_chunk, end_uoffset), sizeof(plat_bgzf_sample));
  printf("%zu %zu\n", offsetof(plat_bgzf_sample, chunks), offsetof(plat_bgzf_sample, broken_mates));
  printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(plat_bgzf_region), offsetof(plat_bgzf_region, contig_seq), offsetof(plat_bgzf_region, dev_contig_seq),
         offsetof(plat_bgzf_region, tid), offsetof(plat_bgzf_region, itr_beg), offsetof(plat_bgzf_region, itr_end), offsetof(plat_bgzf_region, samples));
  printf("%zu %zu %zu %zu\n", sizeof(plat_bgzf_inflate_out), offsetof(plat_bgzf_inflate_out, data), offsetof(plat_bgzf_inflate_out, out_off),
         offsetof(plat_bgzf_inflate_out, status));
  printf("%zu %zu %zu %zu %zu %zu\n", sizeof(plat_bam_find_in), offsetof(plat_bam_find_in, n_blocks), offsetof(plat_bam_find_in, data),
         offsetof(plat_bam_find_in, stream_chunk_begin), offsetof(plat_bam_find_in, chunk_stop_blk), offsetof(plat_bam_find_in, end));
  printf("%zu %zu %zu %zu\n", sizeof(plat_bam_find_out), offsetof(plat_bam_find_out, rec_limit), offsetof(plat_bam_find_out, stream_begin),
         offsetof(plat_bam_find_out, status));
  { int (*fn)(plat_caller*, const plat_bgzf_region*, int, int, const char* const*, plat_caller_options*, const plat_caller_qc_options*, char**,
               size_t*, plat_fetched_region_info*, plat_caller_stats*) = plat_call_bgzf_regions;
    printf("%d\n", fn(NULL, NULL, 0, 0, NULL, NULL, NULL, NULL, NULL, NULL, NULL)); }
  return 0; }''')
    exe = tmp_path / "lay"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic-errors", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L" + os.path.dirname(F.LIB_PATH), "-lplat_caller", "-lplat_mi355x", "-Wl,-rpath," + os.path.dirname(F.LIB_PATH)])
    out = subprocess.check_output([str(exe)], text=True).split()
    v = list(map(int, out[:29]))
    Ch, S, G, I, FI, FO = F._BgzfChunk, F._BgzfSample, F._BgzfRegion, _lib.BgzfInflateOut, _lib.BamFindIn, _lib.BamFindOut
    assert v[0:6] == [C.sizeof(Ch), Ch.data_len.offset, Ch.first_uoffset.offset, Ch.end_coffset.offset, Ch.end_uoffset.offset, C.sizeof(S)]
    assert v[6:8] == [S.chunks.offset, S.broken_mates.offset]
    assert v[8:15] == [C.sizeof(G), G.contig_seq.offset, G.dev_contig_seq.offset, G.tid.offset, G.itr_beg.offset, G.itr_end.offset, G.samples.offset]
    assert v[15:19] == [C.sizeof(I), I.data.offset, I.out_off.offset, I.status.offset]
    assert v[19:25] == [C.sizeof(FI), FI.n_blocks.offset, FI.data.offset, FI.stream_chunk_begin.offset, FI.chunk_stop_blk.offset, FI.end.offset]
    assert v[25:29] == [C.sizeof(FO), FO.rec_limit.offset, FO.stream_begin.offset, FO.status.offset]
    assert int(out[29]) == -1                                # (PLAT_ERR_INVALID for a NULL caller: the symbol links and runs)
    lib = _lib.load()
    for name, n_args in (("plat_bgzf_inflate_batch", 8), ("plat_bam_find_records", 4)):
        assert name in _lib.SIGNATURES and hasattr(lib, name) and len(_lib.SIGNATURES[name][1]) == n_args
    # the BAM header's closing line points here
    with open(os.path.join(ROOT, "include", "platypus_caller_bam.h")) as f:
        assert "platypus_caller_bgzf.h" in f.read()


def test_cython_declarations_of_the_bgzf_entry_points_build(tmp_path):
    pytest.importorskip("Cython")
    pyx = tmp_path / "bgzf_check.pyx"
    pyx.write_text('''# cython: language_level=3
from libc.string cimport memset
cimport cplat

def sizes():
    cdef cplat.plat_bgzf_region r
    cdef cplat.plat_bgzf_inflate_out o
    cdef cplat.plat_bam_find_in fi
    cdef cplat.plat_bam_find_out fo
    memset(&r, 0, sizeof(r))
    memset(&o, 0, sizeof(o))
    memset(&fi, 0, sizeof(fi))
    memset(&fo, 0, sizeof(fo))
    return (sizeof(cplat.plat_bgzf_chunk), sizeof(cplat.plat_bgzf_sample), sizeof(r), sizeof(o),
            cplat.plat_bgzf_inflate_batch(NULL, 0, NULL, 0, NULL, NULL, &o, NULL), cplat.plat_bam_find_records(NULL, &fi, &fo, NULL),
            cplat.plat_call_bgzf_regions(NULL, &r, 0, 0, NULL, NULL, NULL, NULL, NULL, NULL, NULL))
''')
    c_file = tmp_path / "bgzf_check.c"
    subprocess.check_call([sys.executable, "-m", "cython", "-3", "-I", os.path.join(ROOT, "bindings"), str(pyx), "-o", str(c_file)])
    import sysconfig
    subprocess.check_call(["gcc", "-c", "-fPIC", "-O0", "-I" + sysconfig.get_paths()["include"], "-I" + os.path.join(ROOT, "include"), str(c_file),
                           "-o", str(tmp_path / "bgzf_check.o")])


def _tiny_region():
    ref = b"ACGT" * 100
    fasta = H.FastaFile({"20": ref})
    reads = [H.AlignedRead(ref[p:p + 50], bytes([30] * 50), p, bitFlag=3) for p in (110, 120)]
    return F.BgzfRegion.from_reads("20", 100, 300, fasta, [(reads, [])])


def test_fake_device_caller_library_refuses_the_bgzf_call_and_stays_usable():
    """The CPU stand-in device has no plat_bgzf_inflate_batch: the caller library still loads, returns PLAT_ERR_UNSUPPORTED with a message
    naming the symbol, twice, and works afterwards."""
    from tests.fakedev import fake_caller_lib
    lib = fake_caller_lib()
    nc = F.NativeCaller(0, 1, 1, lib=lib)
    try:
        for _ in range(2):
            with pytest.raises(_lib.PlatypusDeviceError) as e:
                nc.call_bgzf_regions([_tiny_region()], ["S1"], default_options())
            assert e.value.code == -6 and "plat_bgzf_inflate_batch" in str(e.value)
        assert nc.call_regions([], ["S1"], default_options()) == ""
    finally:
        nc.close()


def test_writer_writes_the_specified_bytes():
    rng = np.random.default_rng(3)
    data = rng.integers(0, 256, size=200000, dtype=np.uint8).tobytes() + bytes(100000) + b"ACGT" * 30000
    stream, off = synth.bgzf_stream(data)
    assert gzip.decompress(stream) == data
    assert len(off) == -(-len(data) // 0xff00) + 1 and stream[int(off[-1]):] == synth.BGZF_EOF
    for lv, st, bp in ((0, 0, 1000), (1, zlib.Z_RLE, 0xff00), (9, zlib.Z_FIXED, 777)):
        s2, o2 = synth.bgzf_stream(data[:150000], block_payload=bp, level=lv, strategy=st)
        assert gzip.decompress(s2) == data[:150000] and len(o2) == -(-150000 // bp) + 1
        assert all(s2[int(o):int(o) + 4] == b"\x1f\x8b\x08\x04" for o in o2)
    # by hand: a stored block of "ACGT" (level 0: BFINAL 1, BTYPE 0, LEN 4, NLEN ~4, the bytes) -- CRC32("ACGT") = 0xa30e9ff2
    assert synth.bgzf_block(b"ACGT", level=0).hex() == (
        "1f8b0804" "00000000" "00" "ff" "0600" "4243" "0200" "2200" "01" "0400" "fbff" "41434754" "f29f0ea3" "04000000")
    # the EOF block of the SAM specification (4.1.2), verbatim
    eof = "1f8b08040000000000ff0600424302001b0003000000000000000000"
    assert synth.bgzf_block(b"").hex() == eof and synth.BGZF_EOF.hex() == eof and len(synth.BGZF_EOF) == 28
    # another subfield goes in front of BC; BSIZE counts it
    b = synth.bgzf_block(b"ACGT", level=0, extra_subfields=b"XY\x03\x00abc")
    assert b[10:12] == (13).to_bytes(2, "little") and b[12:19] == b"XY\x03\x00abc" and b[19:23] == b"BC\x02\x00"
    assert struct.unpack_from("<H", b, 23)[0] == len(b) - 1 and gzip.decompress(b) == b"ACGT"
    with pytest.raises(ValueError):
        synth.bgzf_block(bytes(65537))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """tests/bgzf_host_driver.cpp + csrc/bgzf_inflate.hpp built with g++, with -fsanitize=address,undefined when that links here."""
    d = tmp_path_factory.mktemp("bgzf_host")
    exe = str(d / "driver")
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I", os.path.join(ROOT, "platypus_amd", "csrc"), os.path.join(ROOT, "tests", "bgzf_host_driver.cpp"),
            "-o", exe]
    san = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan"], capture_output=True, text=True)
    sanitized = san.returncode == 0
    if not sanitized:
        subprocess.check_call(base)
    print("host driver built %s sanitizers" % ("with" if sanitized else "WITHOUT"))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:verify_asan_link_order=0")     # (a library loaded in front of ASan's runtime is no error)

    def run(mode, cases, tag):
        fin, fout = str(d / (tag + ".in")), str(d / (tag + ".out"))
        with open(fin, "wb") as f:
            f.write(struct.pack("<I", len(cases)))
            for c in cases:
                blob, rest = (c, b"") if isinstance(c, bytes) else c
                f.write(struct.pack("<I", len(blob)) + blob + rest)
        r = subprocess.run([exe, mode, fin, fout], capture_output=True, text=True, env=env)
        assert r.returncode == 0, (r.returncode, r.stderr[-3000:])       # 3: a guard band was written; else a sanitizer report or an abort
        with open(fout, "rb") as f:
            raw = f.read()
        out, at = [], 0
        for _ in cases:
            rc = struct.unpack_from("<q", raw, at)[0]
            at += 8
            if mode == "inflate":
                out.append(raw[at:at + rc] if rc >= 0 else None)
                at += max(rc, 0)
            else:
                nk, walked = struct.unpack_from("<qq", raw, at)
                at += 16
                out.append((rc, list(struct.unpack_from("<%dq" % nk, raw, at)), walked))
                at += 8 * nk
        assert at == len(raw)
        return out
    return run


def test_host_build_inflates_the_grid_as_zlib_does(driver):
    grid = K.inflate_grid()
    assert len(grid) == 7 * 4 * 4
    # every block fits BSIZE -- the writer dropped no case -- and the largest is the 65 280-byte payload's
    sizes = [len(b) for _, _, b in grid]
    assert max(sizes) == 65352 and max(sizes) == max(len(b) for n, p, b in grid if len(p) == 65280)
    got = driver("inflate", [b for _, _, b in grid], "grid")
    for (name, payload, block), out in zip(grid, got):
        xlen = struct.unpack_from("<H", block, 10)[0]
        want = zlib.decompress(block[12 + xlen:-8], -15)
        assert want == payload
        assert out is not None, name
        assert out == want and zlib.crc32(out) == struct.unpack_from("<I", block, len(block) - 8)[0], name
    # all three block types and several deflate blocks per BGZF block took part
    first_types = {(b[12 + 6] >> 1) & 3 for _, _, b in grid}
    assert first_types == {0, 1, 2}
    assert any(len(p) > 40000 and (b[18] & 1) == 0 for _, p, b in grid)                  # (BFINAL clear on a first deflate block)
    # BC behind another subfield, and the EOF block
    got = driver("inflate", [synth.bgzf_block(b"behind", extra_subfields=b"XY\x03\x00abc" + b"BC\x01\x00z"), synth.BGZF_EOF], "extra")
    assert got == [b"behind", b""]


def test_host_build_refuses_the_corrupt_corpus(driver):
    bad = K.corrupt_blocks()
    assert len(bad) >= 25
    for why, block in bad.items():
        assert K.reference_verdict(block) is None, why                # (the reference reader refuses each too)
    got = driver("inflate", list(bad.values()), "corrupt")
    assert [why for why, out in zip(bad, got) if out is not None] == []
    # every truncation of a valid block: inside the header, the payload and the trailer
    text = b"truncate me, " * 30
    for lv in (0, 6):
        block = synth.bgzf_block(text, lv)
        cuts = [block[:k] for k in range(len(block))]
        assert driver("inflate", cuts, "cuts%d" % lv) == [None] * len(cuts)
        assert driver("inflate", [block], "whole%d" % lv) == [text]
    # ... and with BSIZE rewritten to the shorter length, so that the header is consistent and the deflate data or the trailer is what is short
    block = synth.bgzf_block(text, 6)
    short = []
    for k in range(26, len(block)):
        b = bytearray(block[:k])
        struct.pack_into("<H", b, 16, k - 1)
        short.append(bytes(b))
    got = driver("inflate", short, "short")
    assert [k for k, out in enumerate(got) if out is not None and K.reference_verdict(short[k]) is None] == []


def test_host_build_agrees_with_zlib_on_2000_bit_flips(driver):
    """One random bit flipped in each of 2 000 blocks: every one ends in a refusal or in bytes whose CRC still matches (a flip in MTIME, XFL,
    OS or behind the last deflate block), and zlib says which -- what zlib inflates to the right CRC inflates here too, to the same bytes."""
    rng = np.random.default_rng(2024)
    sources = []
    recs = K.synthetic_record_bytes(6000)
    for p in (recs, b"a periodic text, " * 200, rng.integers(0, 256, size=500, dtype=np.uint8).tobytes(), bytes(3000)):
        for lv, st in ((6, 0), (1, 0), (9, zlib.Z_FIXED), (6, zlib.Z_HUFFMAN_ONLY), (0, 0)):
            sources.append(synth.bgzf_block(p, lv, st))
    flipped = []
    for k in range(2000):
        b = bytearray(sources[k % len(sources)])
        bit = int(rng.integers(0, 8 * len(b)))
        b[bit >> 3] ^= 1 << (bit & 7)
        flipped.append(bytes(b))
    got = driver("inflate", flipped, "flips")
    want = [K.reference_verdict(b) for b in flipped]
    assert [k for k in range(2000) if got[k] != want[k]] == []
    accepted = sum(1 for w in want if w is not None)
    print("bit flips: %d refused, %d harmless" % (2000 - accepted, accepted))
    assert 0 < accepted < 200


def _walk_case_bytes(data, first, stop, tid, beg, end, block_payload):
    """The driver's case for one walk: the bytes as a BGZF stream of block_payload-byte blocks, `stop` as (block, offset in block)."""
    stream, off = synth.bgzf_stream(data, block_payload=block_payload, eof=False)
    if stop is None:
        sb, su = -1, 0
    else:
        sb, su = (stop // block_payload, stop % block_payload) if stop < len(data) else (-1, 0)
        assert stop <= len(data)
    return stream, struct.pack("<iiiiii", first, sb, su, tid, beg, end), len(off)


def test_host_build_walks_records_by_the_rule(driver):
    cases = K.walk_cases()
    n_err = spans = 0
    for bp in (65536, 100, 37):                                        # whole, and in blocks shorter than a record: records span blocks
        packed, want = [], []
        for name, data, first, stop, tid, beg, end in cases:
            stream, tail, n_blk = _walk_case_bytes(data, first, stop, tid, beg, end, bp)
            packed.append((stream, tail))
            want.append(K.rule_walk(data, first, stop, tid, beg, end))
            spans += n_blk > 1
        got = driver("walk", packed, "walk%d" % bp)
        for (name, *_), (rc, kept, walked), (w_rc, w_kept, w_walked, _) in zip(cases, got, want):
            assert rc == w_rc, (name, bp)
            if rc == 0:
                assert kept == w_kept and walked == w_walked, (name, bp)
            n_err += rc != 0
    assert n_err == 3 * 5 and spans > 20
    # what the rule gives on the edge cases, by hand: of the twelve records of "the window's edges" ten are walked and six kept, in this order
    name, data, first, stop, tid, beg, end = cases[0]
    rc, kept, walked, ended = K.rule_walk(data, first, stop, tid, beg, end)
    pos = [struct.unpack_from("<i", data, k + 4)[0] for k in kept]
    assert (rc, pos, walked, ended) == (0, [960, 990, 1200, 1300, 1400, 1999], 10, True)
    # a stop exactly at a block boundary: the position at the end of a block's data is offset 0 of the next block
    three = b"".join(K.record(3, 1100 + 10 * k, [(0, 20)]) for k in range(4))
    one = len(three) // 4
    stream, off = synth.bgzf_stream(three, block_payload=2 * one, eof=False)
    assert len(off) == 2
    got = driver("walk", [(stream, struct.pack("<iiiiii", 0, 1, 0, 3, 1000, 2000))], "boundary")
    assert got == [(0, [4, 4 + one], 2)]


def test_host_build_gives_zlibs_verdict_on_streams_zlib_never_writes(driver):
    """tests/deflate_writer.py's streams (tests/test_deflate_writer_cpu.py says what they reach): the slow canonical walk at every depth,
    the headers' full ranges, every length and distance symbol, the overlap ladder, the dependence chains at the batch border -- which the
    driver replays in the device's order too --, the far edges, the block sequences, the refusals, 400 seeded streams and of each a copy
    with bits of its first header flipped.  zlib decides every verdict and every payload."""
    named = [(n, b) for n, _, b in K.foreign_blocks()]
    fuzz, _ = K.foreign_fuzz()
    cases = named + [(n, b) for n, _, b, _ in fuzz] + [(n + ", flipped", f) for n, _, _, f in fuzz]
    got = driver("inflate", [b for _, b in cases], "foreign")
    want = [K.reference_verdict(b) for _, b in cases]
    assert [n for (n, _), g, w in zip(cases, got, want) if g != w] == []
    n_ok = sum(1 for w in want if w is not None)
    assert n_ok >= 630 and len(want) - n_ok >= 300


def test_host_build_walks_the_window_seam_ladder_by_the_rule(driver):
    """The host build has no windows: this pins the cases themselves (every stream walks to its end by walk_step as by rule_walk) before
    the device sees them, which is where the windows are."""
    cases, _ = K.walk_seam_cases()
    for bp in (65536, 37):
        packed = [_walk_case_bytes(data, first, stop, tid, beg, end, bp)[:2] for _, data, first, stop, tid, beg, end in cases]
        got = driver("walk", packed, "seam%d" % bp)
        for (name, data, first, stop, tid, beg, end), (rc, kept, walked) in zip(cases, got):
            w_rc, w_kept, w_walked, _ = K.rule_walk(data, first, stop, tid, beg, end)
            assert (rc, kept, walked) == (0, w_kept, w_walked) and w_rc == 0, (name, bp)
