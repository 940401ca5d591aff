"""CPU tests of the tabix index of the compressed output (plat_tabix_index_batch, include/platypus_caller_tbi.h): the rule's Python mirror
(tests/tabix_index_cases.py) and the HOST TWIN (csrc/tabix_index.hpp: built alone under AddressSanitizer and UBSan where libasan is
installed, and run through PLAT_CALLER_HOST_TBI=1 on the stand-in device) give, parsed with tabixindex.TabixIndex, the names, bins with
their chunk lists and linear indexes the reference's ti_index_build wrote for every committed bgzipped VCF, and refuse what it refused,
naming the line; twin and mirror leave the same intermediate and the same index bytes on hand-made corner files and seeded random ones.
The structs match their ctypes mirrors; the caller library on the stand-in device refuses the call cleanly without the switch."""
import ctypes as C
import gzip
import os
import struct
import subprocess

import pytest

from platypus_amd import _lib, fastcaller as F, tabixindex
from platypus_amd.options import default_options
from tests import tabix_index_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def all_files():
    """[(label, vcf_gz)]: everything the twin and the mirror are compared on."""
    out = [(label, z) for label, z, _ in K.committed_pairs()] + [(c["label"], c["vcf_gz"]) for c in K.golden_cases()]
    out += [(label, z) for label, z, _, _ in K.hand_files()] + [(label, z) for label, z in K.random_files()[:4] + K.random_files()[6:]]
    return out


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    """{label: (status, intermediate dict, index bytes or None)} from the host driver over all_files()."""
    d = tmp_path_factory.mktemp("tabix_index_host")
    exe = str(d / "driver")
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I", os.path.join(ROOT, "platypus_amd", "csrc"),
            os.path.join(ROOT, "tests", "tabix_index_host_driver.cpp"), "-o", exe]
    san = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan"], capture_output=True, text=True)
    if san.returncode != 0:
        subprocess.check_call(base)
    print("host driver built %s sanitizers" % ("with" if san.returncode == 0 else "WITHOUT"))
    files = all_files()
    fin, fout = str(d / "cases.in"), str(d / "cases.out")
    with open(fin, "wb") as f:
        f.write(struct.pack("<I", len(files)))
        for _, z in files:
            f.write(struct.pack("<q", len(z)) + z)
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    with open(fout, "rb") as f:
        raw = f.read()
    out, at = {}, 0

    def take(fmt, n=1):
        nonlocal at
        v = struct.unpack_from("<%d%s" % (n, fmt), raw, at)
        at += struct.calcsize("<%d%s" % (n, fmt))
        return list(v)

    for label, _ in files:
        st = take("q", K.ST_WORDS)
        n, = take("q")
        tid, b, u = take("i", n), take("i", n), take("q", n)
        r_, = take("q")
        off, ln, first = take("q", r_), take("i", r_), take("q", r_ + 1)
        w, = take("q")
        lin = take("q", w)
        size, = take("q")
        tbi = None if size < 0 else raw[at:at + size]
        at += max(size, 0)
        out[label] = (st, {"runs": list(zip(tid, b, u)), "names": list(zip(off, ln)), "lin_first": first, "lin": lin, "status": st}, tbi)
    assert at == len(raw)
    return out


def test_the_mirror_reproduces_the_references_indexes():
    """Every committed pair: names, every bin's chunk list and every linear index as ti_index_build wrote them."""
    pairs = K.committed_pairs() + [(c["label"], c["vcf_gz"], c["tbi"]) for c in K.golden_cases() if c["tbi"]]
    assert len(pairs) >= 4
    for label, z, tbi in pairs:
        st, raw = K.index_of(z)
        assert st[K.ST_VERDICT] == 0, label
        want, got = tabixindex.TabixIndex(tbi), tabixindex.TabixIndex(gzip.compress(raw))
        assert K.parsed(got) == K.parsed(want), label
        assert st[K.ST_CONTIGS] == len(want.names) and st[K.ST_WINDOWS] == sum(len(l) for l in want.linear)


def test_the_mirror_refuses_what_the_reference_refused():
    for c in K.golden_cases():
        st, raw = K.index_of(c["vcf_gz"])
        assert (st[K.ST_VERDICT] != 0) == bool(c["refused"]), c["label"]
    for label, z, line, kind in K.hand_files():
        st, raw = K.index_of(z)
        if line is None:
            assert st[K.ST_VERDICT] == 0 and raw is not None, label
        else:
            assert (st[K.ST_VERDICT], st[K.ST_LINE], st[K.ST_KIND]) == (K.ERR_BAD_INPUT, line, kind) and raw is None, label


def test_the_first_record_quirk_and_the_odd_ends():
    """What the issue states of the corners, on the mirror: [0, X, Y] for a first record at offset 0; END=0 and END below POS are indexed."""
    by = {label: text for label, text, _, _ in K.hand_texts()}
    z = K.synth.bgzf_stream(by["no header, first record at offset 0"], 65280)[0]
    idx = tabixindex.TabixIndex(gzip.compress(K.index_of(z)[1]))
    lin = idx.linear[0]
    second = len(K.L(b"20", 100)) + 1
    assert lin[0] == 0 and lin[1] == second and lin[2] > lin[1] and len(lin) == 3           # (a minimum taking 0 as a value gives [0, 0, Y])
    for label in ("END=0", "END below POS"):
        st, raw = K.index_of(K.synth.bgzf_stream(by[label], 100)[0])
        assert st[K.ST_VERDICT] == 0 and st[K.ST_RECORDS] == 3
    st, raw = K.index_of(K.synth.bgzf_stream(by["END=0"], 100)[0])
    assert K.reg2bin(119, 0) == 0 and 0 in tabixindex.TabixIndex(gzip.compress(raw)).bins[0]


def test_host_twin_leaves_the_mirrors_intermediate_and_bytes(twin):
    for label, z in all_files():
        data, out_off, addr = K.inflate_file(z)
        want = K.build(data, out_off, addr)
        st, got, tbi = twin[label]
        assert st == want["status"], label
        if st[K.ST_VERDICT] != 0:
            assert tbi is None
            continue
        assert got == want, label
        assert tbi == K.finish(want, data), label


def test_host_twin_reproduces_the_references_indexes(twin):
    for label, z, tbi in K.committed_pairs():
        assert K.parsed(tabixindex.TabixIndex(gzip.compress(twin[label][2]))) == K.parsed(tabixindex.TabixIndex(tbi)), label


def test_index_structs_match_their_ctypes_mirrors(tmp_path):
    F.build()
    src = tmp_path / "lay.c"
    src.write_text(r'''
#include <stdio.h>
#include <stddef.h>
#include "platypus_mi355x.h"
#include "platypus_caller_tbi.h"
int main(void){
  printf("%zu %zu %zu %zu %zu\n", sizeof(plat_tabix_index_in), sizeof(plat_tabix_index_out), offsetof(plat_tabix_index_in, blk_addr),
         offsetof(plat_tabix_index_out, run_tid), offsetof(plat_tabix_index_out, status));
  printf("%zu %zu %d %d\n", sizeof(plat_tbi_info), offsetof(plat_tbi_info, seconds), PLAT_TBI_STATUS_WORDS, PLAT_TBI_MAX_REF);
  { int (*fn)(plat_caller*, const uint8_t*, size_t, uint8_t**, size_t*, plat_tbi_info*) = plat_caller_index_bgzf; (void)fn; }
  return 0; }''')
    exe = tmp_path / "lay"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L" + os.path.dirname(F.LIB_PATH), "-lplat_caller",
                           "-lplat_mi355x", "-Wl,-rpath," + os.path.dirname(F.LIB_PATH)])
    vals = list(map(int, subprocess.check_output([str(exe)], text=True).split()))
    I, O = _lib.TabixIndexIn, _lib.TabixIndexOut
    assert vals[:5] == [C.sizeof(I), C.sizeof(O), I.blk_addr.offset, O.run_tid.offset, O.status.offset]
    assert vals[5:] == [C.sizeof(F.TbiInfo), F.TbiInfo.seconds.offset, _lib.TBI_STATUS_WORDS, _lib.TBI_MAX_REF]
    assert _lib.TBI_STATUS_WORDS == K.ST_WORDS
    assert "plat_tabix_index_batch" in _lib.SIGNATURES and "plat_tabix_index_batch" in _lib.ADDED_LATER and hasattr(_lib.load(), "plat_tabix_index_batch")
    assert "HOST_TBI" in open(os.path.join(ROOT, "platypus_amd", "csrc", "host", "switches.hpp")).read()


def test_fake_device_caller_library_refuses_index_bgzf_and_stays_usable(monkeypatch):
    """The CPU stand-in device has no plat_tabix_index_batch: PLAT_ERR_UNSUPPORTED with a message naming the symbol, twice, and the caller
    works afterwards."""
    from tests.fakedev import fake_caller_lib
    monkeypatch.delenv("PLAT_CALLER_HOST_TBI", raising=False)
    nc = F.NativeCaller(0, 1, 1, lib=fake_caller_lib())
    try:
        z = K.committed_pairs()[0][1]
        for _ in range(2):
            with pytest.raises(_lib.PlatypusDeviceError) as e:
                nc.index_bgzf(z)
            assert e.value.code == -6 and "plat_tabix_index_batch" in str(e.value)
        assert nc.call_regions([], ["S1"], default_options()) == ""
    finally:
        nc.close()


def test_fake_device_host_tbi_indexes_every_file_and_names_the_refused_line(monkeypatch):
    """PLAT_CALLER_HOST_TBI=1 on the stand-in device: the reference's index for every committed pair and golden; the mirror's bytes,
    BGZF-compressed with the EOF block behind them; a refused file is a data error naming the line, and the next call is clean."""
    from tests.fakedev import fake_caller_lib
    from tests import bgzf_deflate_cases as D
    monkeypatch.setenv("PLAT_CALLER_HOST_TBI", "1")
    nc = F.NativeCaller(0, 1, 1, lib=fake_caller_lib())
    try:
        for label, z, tbi in K.committed_pairs() + [(c["label"], c["vcf_gz"], c["tbi"]) for c in K.golden_cases() if c["tbi"]]:
            got, info = nc.index_bgzf(z, info=True)
            assert K.parsed(tabixindex.TabixIndex(got)) == K.parsed(tabixindex.TabixIndex(tbi)), label
            st, raw = K.index_of(z)
            assert got.endswith(D.EOF_BLOCK) and gzip.decompress(got) == raw
            assert D.parse_blocks(got) and info.device_calls == 0
            assert (info.lines, info.records, info.runs, info.contigs, info.windows) == tuple(st[k] for k in (K.ST_LINES, K.ST_RECORDS, K.ST_RUNS, K.ST_CONTIGS, K.ST_WINDOWS))
        refused = [(c["label"], c["vcf_gz"]) for c in K.golden_cases() if c["refused"]] + [(label, z) for label, z, line, _ in K.hand_files() if line is not None]
        assert len(refused) >= 7
        for label, z in refused:
            st, _ = K.index_of(z)
            with pytest.raises(_lib.PlatypusDeviceError) as e:
                nc.index_bgzf(z)
            assert e.value.code == K.ERR_BAD_INPUT and ("line %d " % st[K.ST_LINE]) in str(e.value), (label, str(e.value))
            assert nc.index_bgzf(K.committed_pairs()[0][1]) == nc.index_bgzf(K.committed_pairs()[0][1])
        for label, z, line, _ in K.hand_files():
            if line is None:
                assert gzip.decompress(nc.index_bgzf(z)) == K.index_of(z)[1], label
        # a file that is no BGZF, and one with an empty block in front of data
        with pytest.raises(_lib.PlatypusDeviceError) as e:
            nc.index_bgzf(b"chr20\t1\n")
        assert e.value.code == K.ERR_BAD_INPUT and "chain" in str(e.value)
        a, b = K.synth.bgzf_stream(K.HEADER, eof=True)[0], K.synth.bgzf_stream(K.L(b"1", 5) + b"\n")[0]
        with pytest.raises(_lib.PlatypusDeviceError) as e:
            nc.index_bgzf(a + b)
        assert e.value.code == K.ERR_BAD_INPUT and "empty" in str(e.value)
        assert nc.call_regions([], ["S1"], default_options()) == ""
    finally:
        nc.close()
