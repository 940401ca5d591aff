"""CPU tests of source VCFs taken as the BGZF blocks of their tabix fetches (plat_tabix_fetch_batch, include/platypus_caller_tabix.h): the
plain-Python mirror of the rule (tests/tabix_cases.py) and tabixindex's choice of chunks against what the reference's own tabix returned
(tests/golden/tabix_cases.json.gz); the HOST BUILD of csrc/tabix_rule.hpp over csrc/bgzf_inflate.hpp -- the text the device compiles -- as a
stand-alone program under AddressSanitizer and UBSan against the mirror on goldens and hand-made edge streams; the C structs and their
ctypes mirrors, the header as C99, the Cython declarations; and the caller library linked against the CPU stand-in device: the refusal
without the device entry point, and with PLAT_CALLER_HOST_TABIX=1 the region loop over blocks against the same loop over lines."""
import ctypes as C
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from platypus_amd import _lib, fastcaller as F, hostapi as H, synth, tabixindex
from platypus_amd.options import default_options
from tests import region_golden as R
from tests import source_golden as S
from tests import tabix_cases as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAYLOADS = (65536, 100, 37)


@pytest.fixture(scope="module")
def fake():
    from tests import fakedev
    old = H._engine
    H._engine = fakedev.fake_engine()
    yield fakedev.fake_caller_lib()
    H._engine = old


def test_goldens_cover_the_corners():
    files = T.golden_files()
    assert sorted(f["payload"] for f in files) == [37, 100, 65280]
    for f in files:
        assert f["names"] == [b"2", b"20", b"20_alt"]
        text = b"".join(synth_inflate(f["vcf_gz"]))
        lines = text.split(b"\n")
        assert any(ln.startswith(b"#") for ln in lines[4:]) and b"\t\tC\t" in text                       # meta lines inside the data, an empty REF
        for needle in (b"\tEND=70900", b"SVEND=7", b"CIEND=1;END=7", b"\tEND=40000;DP=3", b"20\t0\t", b"20\t010\t", b"20\t0x10\t", b"20\t 12\t"):
            assert needle in text, needle
        assert any(not q["lines"] for q in f["queries"]) and any(len(q["lines"]) > 3 for q in f["queries"])
    big = next(f for f in files if f["payload"] == 65280)
    assert max(len(ln) for q in big["queries"] for ln in q["lines"]) > 65536
    assert any(1024 < len(ln) < 65536 for f in files if f["payload"] == 100 for q in f["queries"] for ln in q["lines"])
    assert not b"".join(synth_inflate(next(f for f in files if f["payload"] == 37)["vcf_gz"])).endswith(b"\n")
    # lines that end exactly on block ends, and lines that span blocks
    small = next(f for f in files if f["payload"] == 37)
    text = b"".join(synth_inflate(small["vcf_gz"]))
    ends = [i + 1 for i, c in enumerate(text) if c == 10]
    assert sum(e % 37 == 0 for e in ends) >= 2 and any(e // 37 - s // 37 >= 2 for s, e in zip(ends, ends[1:]))
    assert sum(len(s[3]) > 1 for _, s, _ in T.golden_streams()) >= 10                                     # queries that cross chunk gaps


def synth_inflate(data):
    """The payloads of a BGZF file's blocks."""
    import zlib
    out = []
    for at, n, isize in T.blocks_of(data):
        xlen, = struct.unpack_from("<H", data, at + 10)
        out.append(zlib.decompress(data[at + 12 + xlen:at + n - 8], -15))
    return out


def test_mirror_and_chunk_selection_return_the_references_lines():
    """On every golden query, the mirror over the chunks tabixindex derives from the committed .tbi returns what ti_read returned."""
    got = T.golden_streams()
    assert len(got) >= 90
    for label, stream, lines in got:
        m = T.mirror([stream])
        assert m["status"][0] == 0 and m["text"] == b"".join(x + b"\n" for x in lines), label
        assert m["counts"][1] == len(lines) and m["counts"][0] >= len(lines)


def test_reg2bins_and_index_fields():
    assert tabixindex.reg2bins(0, 1) == [0, 1, 9, 73, 585, 4681] and tabixindex.reg2bins(5, 5) == []
    assert tabixindex.reg2bins(16383, 16385)[-2:] == [4681, 4682] and len(tabixindex.reg2bins(0, 1 << 29)) == 37449
    f = T.golden_files()[0]
    idx = tabixindex.TabixIndex(f["tbi"])
    assert (idx.preset & 0xffff, idx.col_seq, idx.col_beg, idx.meta) == (2, 1, 2, ord("#")) and idx.tid("20_alt") == 2 and idx.tid(b"21") == -1
    assert idx.query(1, 10, 5) is None and idx.query(1, 1 << 28, 1 << 29) == []
    tf = tabixindex.TabixFile(f["vcf_gz"], idx)
    assert tf.fetch_blocks("21", 0, 10) is None and tf.fetch_blocks("20", -5, 10)[:3] == (b"20", 0, 10)
    with pytest.raises(ValueError):
        tabixindex.TabixIndex(f["vcf_gz"])


def test_mirror_on_the_edge_streams():
    """The hand-made streams say what their labels promise (the mirror is the yardstick of the host driver and the kernels)."""
    for payload in PAYLOADS:
        got = {label: T.mirror([s]) for label, s in T.edge_streams(payload)}
        assert got["stop with kept-looking lines and a whole chunk behind it"]["counts"] == [2, 2]
        assert got["overshoot past a non-last chunk's end"]["status"][:2] == [T.PLAT_ERR_BAD_INPUT, 0]
        assert got["overshoot past the last chunk's end"]["status"][0] == 0 and got["overshoot past the last chunk's end"]["counts"] == [2, 2]
        for label in ("an empty line", "a one-column line", "END=-5"):
            assert got[label]["counts"] == [1, 1] and got[label]["status"][0] == 0
        assert got["a POS beyond int32"]["status"][0] == T.PLAT_ERR_BAD_INPUT and got["an END beyond int32"]["counts"] == [0, 0]
        assert got["a NUL inside a line"]["counts"] == [4, 4] and b"\x00" in got["a NUL inside a line"]["text"]
        assert got["adjacent and non-adjacent chunks"]["counts"] == [8, 5]
        assert got["a stop exactly on a block boundary"]["counts"] == [1, 1] and got["a chunk that ends on a block boundary and goes on"]["counts"] == [3, 3]
        assert got["white space, signs and bases in POS and END"]["counts"] == [14, 13] and b"\r\t" in got["white space, signs and bases in POS and END"]["text"]
        assert not got["a last line without its newline, and no chunks"]["text"][:-1].endswith(b"\n")


def test_strtol_restatement():
    for s, want in ((b"12", 12), (b" \t+12x", 12), (b"-7", -7), (b"010", 8), (b"019", 1), (b"0x10", 16), (b"0X1fg", 31), (b"0x", 0), (b"0xg", 0), (b"", 0), (b"+", 0),
                    (b"- 5", 0), (b"2147483647", 2 ** 31 - 1)):
        assert T.strtol0(s) == (want, False), s
    assert T.strtol0(b"2147483648")[1] and T.strtol0(b"-2147483648")[1] and T.strtol0(b"0x80000000")[1] and T.strtol0(b"9" * 40)[1]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """tests/tabix_host_driver.cpp + csrc/tabix_rule.hpp + csrc/bgzf_inflate.hpp built with g++, with -fsanitize=address,undefined when that links here."""
    d = tmp_path_factory.mktemp("tabix_host")
    exe = str(d / "driver")
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I", os.path.join(ROOT, "platypus_amd", "csrc"), os.path.join(ROOT, "tests", "tabix_host_driver.cpp"),
            "-o", exe]
    san = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan"], capture_output=True, text=True)
    sanitized = san.returncode == 0
    if not sanitized:
        subprocess.check_call(base)
    print("host driver built %s sanitizers" % ("with" if sanitized else "WITHOUT"))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:verify_asan_link_order=0")     # (a library loaded in front of ASan's runtime is no error)

    def run(batches, tag):
        fin, fout = str(d / (tag + ".in")), str(d / (tag + ".out"))
        with open(fin, "wb") as f:
            f.write(struct.pack("<I", len(batches)))
            for streams in batches:
                f.write(struct.pack("<I", len(streams)))
                for name, beg, end, chunks in streams:
                    f.write(struct.pack("<I", len(name)) + name + struct.pack("<iiI", beg, end, len(chunks)))
                    for data, first_u, end_c, end_u in chunks:
                        data = bytes(data)
                        f.write(struct.pack("<I", len(data)) + data + struct.pack("<iqi", first_u, end_c, end_u))
        r = subprocess.run([exe, fin, fout], capture_output=True, text=True, env=env)
        assert r.returncode == 0, (r.returncode, r.stderr[-3000:])       # 3: a guard band was written; else a sanitizer report or an abort
        with open(fout, "rb") as f:
            raw = f.read()
        out, at = [], 0
        for streams in batches:
            n = len(streams)
            v = struct.unpack_from("<%dq" % (5 + 3 * n), raw, at)
            at += 8 * (5 + 3 * n)
            out.append({"status": list(v[:4]), "off": list(v[4:5 + n]), "counts": list(v[5 + n:]), "text": raw[at:at + v[3]]})
            at += v[3]
        assert at == len(raw)
        return out
    return run


def test_host_rule_under_the_sanitizers_equals_the_mirror(driver):
    """Goldens and edge streams, one stream per batch and all of them in one batch, at the three block payloads."""
    golden = [s for _, s, _ in T.golden_streams()]
    batches = [[s] for s in golden] + [golden]
    for payload in PAYLOADS:
        edges = [s for _, s in T.edge_streams(payload)]
        batches += [[s] for s in edges] + [edges]
    got = driver(batches, "all")
    for i, (streams, g) in enumerate(zip(batches, got)):
        assert g == T.mirror(streams), i
    assert sum(g["status"][0] == T.PLAT_ERR_BAD_INPUT for g in got) >= 3 * 3 + 3 and sum(g["status"][2] for g in got) > 300


def test_headers_are_c_and_structs_match_their_mirrors(tmp_path):
    F.build()
    src = tmp_path / "lay.c"
    src.write_text(r'''
#include <stdio.h>
#include <stddef.h>
#include "platypus_caller_tabix.h"
#include "platypus_mi355x.h"
#define O(t, f) printf("%zu\n", offsetof(t, f))
int main(void){
  printf("%zu\n", sizeof(plat_tabix_fetch)); O(plat_tabix_fetch, itr_beg); O(plat_tabix_fetch, itr_end); O(plat_tabix_fetch, n_chunks); O(plat_tabix_fetch, chunks);
  printf("%zu\n", sizeof(plat_source_blocks)); O(plat_source_blocks, fetches);
  printf("%zu\n", sizeof(plat_source_blocks_info)); O(plat_source_blocks_info, compressed_bytes); O(plat_source_blocks_info, kept_bytes); O(plat_source_blocks_info, seconds);
  printf("%zu\n", sizeof(plat_tabix_fetch_in)); O(plat_tabix_fetch_in, n_blocks); O(plat_tabix_fetch_in, data); O(plat_tabix_fetch_in, data_len); O(plat_tabix_fetch_in, out_off);
  O(plat_tabix_fetch_in, stream_chunk_begin); O(plat_tabix_fetch_in, chunk_stop_uoffset); O(plat_tabix_fetch_in, names); O(plat_tabix_fetch_in, name_off); O(plat_tabix_fetch_in, end);
  printf("%zu\n", sizeof(plat_tabix_fetch_out)); O(plat_tabix_fetch_out, text); O(plat_tabix_fetch_out, stream_text_off); O(plat_tabix_fetch_out, stream_counts); O(plat_tabix_fetch_out, status);
  { int (*fn)(plat_caller*, const plat_source_blocks*, int, int, plat_source_blocks_info*) = plat_caller_set_source_blocks; printf("%d\n", fn(NULL, NULL, 0, 0, NULL)); }
  { int (*fn)(plat_ctx*, const plat_tabix_fetch_in*, const plat_tabix_fetch_out*, void*) = plat_tabix_fetch_batch; printf("%d\n", fn(NULL, NULL, NULL, NULL)); }
  printf("%d\n", PLAT_ABI_VERSION);
  return 0; }''')
    exe = tmp_path / "lay"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic-errors", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L" + os.path.dirname(F.LIB_PATH), "-lplat_caller", "-lplat_mi355x", "-Wl,-rpath," + os.path.dirname(F.LIB_PATH)])
    v = list(map(int, subprocess.check_output([str(exe)], text=True).split()))
    TF, SB, SI, I, O = F._TabixFetch, F._SourceBlocks, F.SourceBlocksInfo, _lib.TabixFetchIn, _lib.TabixFetchOut
    assert v[0:5] == [C.sizeof(TF), TF.itr_beg.offset, TF.itr_end.offset, TF.n_chunks.offset, TF.chunks.offset]
    assert v[5:7] == [C.sizeof(SB), SB.fetches.offset]
    assert v[7:11] == [C.sizeof(SI), SI.compressed_bytes.offset, SI.kept_bytes.offset, SI.seconds.offset]
    assert v[11:21] == [C.sizeof(I), I.n_blocks.offset, I.data.offset, I.data_len.offset, I.out_off.offset, I.stream_chunk_begin.offset,
                        I.chunk_stop_uoffset.offset, I.names.offset, I.name_off.offset, I.end.offset]
    assert v[21:26] == [C.sizeof(O), O.text.offset, O.stream_text_off.offset, O.stream_counts.offset, O.status.offset]
    assert v[26:29] == [-1, -1, 1]                                              # (PLAT_ERR_INVALID for NULL arguments: the symbols link and run; the ABI version stays)
    assert "plat_tabix_fetch_batch" in _lib.SIGNATURES and hasattr(_lib.load(), "plat_tabix_fetch_batch")


def test_cython_declarations_build(tmp_path):
    pytest.importorskip("Cython")
    pyx = tmp_path / "tabix_check.pyx"
    pyx.write_text('''
cimport cplat
def sizes():
    cdef cplat.plat_tabix_fetch_in fi
    cdef cplat.plat_tabix_fetch_out fo
    cdef cplat.plat_tabix_fetch ft
    cdef cplat.plat_source_blocks sb
    cdef cplat.plat_source_blocks_info info
    fi.n_streams = 0
    fi.data_len = 0
    fo.cap_text = 0
    ft.n_chunks = 0
    sb.n_fetches = 0
    info.seconds = 0
    return (sizeof(fi), sizeof(fo), cplat.plat_tabix_fetch_batch(NULL, &fi, &fo, NULL), cplat.plat_caller_set_source_blocks(NULL, &sb, 0, 0, &info))
''')
    c_file = tmp_path / "tabix_check.c"
    subprocess.check_call([sys.executable, "-m", "cython", "-3", "-I", os.path.join(ROOT, "bindings"), str(pyx), "-o", str(c_file)])
    import sysconfig
    subprocess.check_call(["gcc", "-c", "-fPIC", "-O0", "-I" + sysconfig.get_paths()["include"], "-I" + os.path.join(ROOT, "include"), str(c_file),
                           "-o", str(tmp_path / "tabix_check.o")])


def region_blocks(case, payload=65536, window=(0, 1 << 29)):
    """The source texts of a region case, each bgzipped and handed over as one chunk of blocks: per loaded region a list of fetches."""
    return [[(reg["chrom"].encode(), window[0], window[1], T.cut(t.encode(), payload, [(0, None)])) for t in reg["source"]]
            for reg in case["regions"] if reg["loaded"]]


REGION_CASES = S.load("source_region_cases.json.gz")


def test_stand_in_device_refuses_and_the_caller_works_afterwards(fake, monkeypatch):
    monkeypatch.delenv("PLAT_CALLER_HOST_TABIX", raising=False)
    case = REGION_CASES[0]
    fasta, work, names = R.case_work(case)
    regs = [F.RegionReads.from_buffers(c, s, e, fasta, b) for c, s, e, b in work]
    nc = F.NativeCaller(0, 2, 2, lib=fake)
    try:
        for _ in range(2):
            with pytest.raises(_lib.PlatypusDeviceError) as e:
                nc.set_source_blocks(region_blocks(case))
            assert e.value.code == -6 and "plat_tabix_fetch_batch" in str(e.value)
        assert nc.call_regions(regs, names, default_options(**case["options"]), source_lines=S.region_source(case)).split("\n")[:-1] == case["lines"]
        assert fake.plat_caller_set_source_blocks(None, None, 0, 0, None) == -1 and fake.plat_caller_set_source_blocks(nc.h, None, 1, 0, None) == -1
        assert fake.plat_caller_set_source_blocks(nc.h, None, 0, 0, None) == 0
    finally:
        nc.close()


@pytest.mark.parametrize("ci", range(len(REGION_CASES)))
def test_host_path_over_blocks_writes_what_lines_write(fake, monkeypatch, ci):
    monkeypatch.setenv("PLAT_CALLER_HOST_TABIX", "1")
    case = REGION_CASES[ci]
    fasta, work, names = R.case_work(case)
    regs = [F.RegionReads.from_buffers(c, s, e, fasta, b) for c, s, e, b in work]
    nc = F.NativeCaller(0, 2, 2, lib=fake)
    try:
        want = nc.call_regions(regs, names, default_options(**case["options"]), source_lines=S.region_source(case))
        assert want.split("\n")[:-1] == case["lines"]
        lines_stats = nc.stats
        for payload in (65536, 37):
            o = default_options(**case["options"])
            got = nc.call_regions(regs, names, o, source_blocks=region_blocks(case, payload))
            assert got == want and o.rlen == case["rlen_after"]
            assert nc.stats["n_source_lines"] == lines_stats["n_source_lines"] and nc.stats["n_source_variants"] == lines_stats["n_source_variants"]
            info = nc.source_blocks_info
            src = [t for r in S.region_source(case) for t in r]
            assert info["inflated_bytes"] == sum(len(t) for t in src) and info["lines_kept"] == info["lines_walked"] == sum(t.count(b"\n") for t in src)
            assert info["kept_bytes"] == info["inflated_bytes"] and info["compressed_bytes"] > 0 and info["n_blocks"] >= len(src) and info["seconds"] > 0
        # the blocks applied to ONE call
        o = default_options(**case["options"])
        if o.getVariantsFromBAMs or o.assemble:
            nc.call_regions(regs, names, o)
            assert nc.stats["n_source_lines"] == 0
        else:                                                                      # (the source was the call's only candidates)
            with pytest.raises(_lib.PlatypusDeviceError) as e:
                nc.call_regions(regs, names, o)
            assert e.value.code == -6
    finally:
        nc.close()


def test_host_path_fetches_by_the_window_and_replaces_and_takes_back(fake, monkeypatch):
    """A window that keeps only some lines gives the text those lines give; a second set replaces the first; an empty one takes it back."""
    monkeypatch.setenv("PLAT_CALLER_HOST_TABIX", "1")
    case = REGION_CASES[0]
    fasta, work, names = R.case_work(case)
    regs = [F.RegionReads.from_buffers(c, s, e, fasta, b) for c, s, e, b in work]
    nc = F.NativeCaller(0, 2, 2, lib=fake)
    try:
        blocks = region_blocks(case, 100, window=(0, 1 << 29))
        first_pos = [[int(t.split(b"\t")[1]) if t else 1 for t in r] for r in S.region_source(case)]      # each fetch's window: its first line's base alone
        narrow = [[(n, first_pos[k][j] - 1, first_pos[k][j], ch) for j, (n, _, _, ch) in enumerate(fetches)] for k, fetches in enumerate(blocks)]
        kept = [T.mirror(fetches) for fetches in narrow]
        assert any(0 < m["status"][2] for m in kept) and sum(m["status"][3] for m in kept) < sum(len(t) for r in S.region_source(case) for t in r)
        want = nc.call_regions(regs, names, default_options(**case["options"]), source_lines=[m["text"] for m in kept])
        assert nc.call_regions(regs, names, default_options(**case["options"]), source_blocks=narrow) == want
        assert nc.source_blocks_info["kept_bytes"] == sum(m["status"][3] for m in kept) and nc.source_blocks_info["lines_kept"] == sum(m["status"][2] for m in kept)
        nc.set_source_blocks(blocks)
        nc.set_source_blocks(narrow)                                               # replaces the first
        assert nc.call_regions(regs, names, default_options(**case["options"])) == want
        nc.set_source_blocks(narrow)
        nc.set_source_blocks([])                                                   # takes it back
        plain = nc.call_regions(regs, names, default_options(**case["options"]))
        assert nc.stats["n_source_lines"] == 0 and plain == nc.call_regions(regs, names, default_options(**case["options"]))
        with pytest.raises(ValueError):
            nc.call_regions(regs, names, default_options(), source_lines=[b""] * len(regs), source_blocks=narrow)
    finally:
        nc.close()


def test_refusals_name_their_place_and_leave_the_caller_usable(fake, monkeypatch):
    monkeypatch.setenv("PLAT_CALLER_HOST_TABIX", "1")
    case = REGION_CASES[0]
    fasta, work, names = R.case_work(case)
    regs = [F.RegionReads.from_buffers(c, s, e, fasta, b) for c, s, e, b in work]
    good = region_blocks(case, 100)
    name, beg, end, chunks = good[-1][-1]
    data = bytes(chunks[0][0])
    blocks = T.blocks_of(data)
    assert len(blocks) >= 3

    def with_data(d, **kw):
        bad = [list(f) for f in good]
        bad[-1][-1] = (name, beg, end, [(np.frombuffer(d, dtype=np.uint8), kw.get("first", 0), kw.get("end_c", -1), kw.get("end_u", 0))])
        return bad
    where = "region %d, file %d, chunk 0" % (len(good) - 1, len(good[-1]) - 1)
    at1, n1, _ = blocks[1]
    nc = F.NativeCaller(0, 2, 2, lib=fake)
    try:
        cases = [
            (data[:at1] + synth.BGZF_EOF + data[at1:], "block 1 of " + where + " is empty"),                       # an empty block with data behind it
            (data[:at1 + 16] + bytes([data[at1 + 16] ^ 0x40]) + data[at1 + 17:], "do not chain"),                # BSIZE's low byte
            (data[:at1 + n1 - 8] + bytes([data[at1 + n1 - 8] ^ 1]) + data[at1 + n1 - 7:], "block 1 of " + where + " cannot be inflated"),      # the CRC32
        ]
        for d, message in cases:
            with pytest.raises(_lib.PlatypusDeviceError) as e:
                nc.set_source_blocks(with_data(d))
            assert e.value.code == -9 and message in str(e.value) and where in str(e.value), str(e.value)
        with pytest.raises(_lib.PlatypusDeviceError) as e:
            nc.set_source_blocks(with_data(data, end_c=at1 + 1))
        assert e.value.code == -9 and "not a block boundary" in str(e.value)
        # a stream the walk refuses: named with "line walk"
        refused = [list(f) for f in good]
        refused[0][0] = (name, 0, 1 << 29, T.cut(b"%s\t99999999999\t.\tA\tC\n" % name, 100, [(0, None)]))
        with pytest.raises(_lib.PlatypusDeviceError) as e:
            nc.set_source_blocks(refused)
        assert e.value.code == -9 and "line walk of region 0, file 0" in str(e.value)
        # the EOF blocks at the end of a chunk's data are welcome, and nothing of the refused sets is left
        assert nc.call_regions(regs, names, default_options(**case["options"])) == nc.call_regions(regs, names, default_options(**case["options"]))
        assert nc.stats["n_source_lines"] == 0
        got = nc.call_regions(regs, names, default_options(**case["options"]), source_blocks=with_data(data + synth.BGZF_EOF))
        assert got.split("\n")[:-1] == case["lines"]
    finally:
        nc.close()
