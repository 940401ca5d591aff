"""GPU tests of the tabix index built on the device: plat_tabix_index_batch's intermediate (runs, names, windows, status) against the rule's
mirror, which tests/test_tabix_index_cpu.py pins to the host twin and to the reference's own indexes, on every golden and hand-made file
and on seeded random sorted VCFs sized to where the kernels can go wrong (tests/tabix_index_cases.py); the capacity contract; the refused
kinds; plat_caller_index_bgzf on a synthetic call's compressed text against PLAT_CALLER_HOST_TBI=1 and through the existing tabix fetch;
and the command line's --outputIndex."""
import gzip
import os

import numpy as np
import pytest

from platypus_amd import _lib, fastcaller as F, hostapi as H, synth, tabixindex
from platypus_amd.options import default_options
from tests import tabix_cases as T, tabix_index_cases as K

pytestmark = pytest.mark.gpu


def device_index(eng, vcf_gz, **caps):
    """(the device's intermediate, the mirror's, the inflated bytes) of one bgzipped file."""
    data, out_off, addr = K.inflate_file(vcf_gz)
    blocks = T.blocks_of(vcf_gz)[:len(out_off) - 1]
    inflated = eng.bgzf_inflate(vcf_gz, np.array([b[0] for b in blocks], dtype=np.int64), keep_device=True)
    assert inflated["data"].tobytes() == data and inflated["out_off"].tolist() == out_off
    want = K.build(data, out_off, addr)
    return eng.tabix_index(inflated, addr, **caps), dict(want, name_bytes=b"".join(data[o:o + n] for o, n in want["names"])), data


def same(got, want, label):
    assert got["guard_intact"], label
    if want["status"][K.ST_VERDICT] != 0:
        assert got["status"][:3] == want["status"][:3], label             # (of a refused file only the verdict, the line and the kind are defined)
        return
    assert got["status"] == want["status"], label
    assert got["runs"] == want["runs"] and got["names"] == want["names"], label
    assert got["lin_first"] == want["lin_first"] and got["lin"] == want["lin"], label
    assert got["name_bytes"] == want["name_bytes"], label


def test_device_intermediate_on_goldens_and_hand_files():
    eng = H.get_engine()
    files = [(label, z) for label, z, _ in K.committed_pairs()] + [(c["label"], c["vcf_gz"]) for c in K.golden_cases()] + [(label, z) for label, z, _, _ in K.hand_files()]
    refused = 0
    for label, z in files:
        got, want, _ = device_index(eng, z)
        same(got, want, label)
        refused += want["status"][K.ST_VERDICT] != 0
    assert refused >= 7 * 3
    # the next call on the same context after a refusal is clean, and a second call gives the same
    got, want, _ = device_index(eng, files[0][1])
    same(got, want, files[0][0])


@pytest.mark.parametrize("index", range(9))
def test_device_intermediate_on_seeded_files(index):
    eng = H.get_engine()
    label, z = K.random_files()[index]
    got, want, data = device_index(eng, z)
    st = want["status"]
    assert st[K.ST_VERDICT] == 0 and st[K.ST_RECORDS] > (100 if index < 7 else 3) and st[K.ST_RUNS] >= 2, label
    same(got, want, label)
    if index in (4, 5):
        assert len(data) > 1024 * 1000                                  # a few thousand tiles: several workgroups take part
    if index == 6:
        assert max(data[k * 1024:(k + 1) * 1024].count(b"\n") for k in range(2)) > 64      # more than one 64-lane round in a tile


def test_capacities_overflow_once_each_then_fit():
    eng = H.get_engine()
    by = {label: z for label, z, _, _ in K.hand_files()}
    z = by["one record with 2000 windows @100"]
    full, want, _ = device_index(eng, z)
    same(full, want, "full")
    st = want["status"]
    assert st[K.ST_RUNS] >= 4 and st[K.ST_CONTIGS] == 2 and st[K.ST_WINDOWS] > 2000
    for caps in (dict(cap_runs=st[K.ST_RUNS] - 1), dict(cap_names=1), dict(cap_windows=st[K.ST_WINDOWS] - 1), dict(cap_name_bytes=1),
                 dict(cap_runs=0, cap_names=0, cap_windows=0, cap_name_bytes=0)):
        got, _, _ = device_index(eng, z, **caps)
        assert got["status"] == [K.ERR_OVERFLOW] + st[1:] and got["guard_intact"], caps         # the full counts, nothing behind a capacity
        assert got["runs"] == want["runs"][:caps.get("cap_runs", 1 << 30)] and got["names"] == want["names"][:caps.get("cap_names", 1 << 30)]
        assert got["lin"] == ([] if "cap_windows" in caps else want["lin"])
        assert got["name_bytes"] == (b"" if "cap_name_bytes" in caps else b"12")
        again, _, _ = device_index(eng, z, cap_runs=got["status"][K.ST_RUNS], cap_names=got["status"][K.ST_CONTIGS], cap_windows=got["status"][K.ST_WINDOWS],
                                   cap_name_bytes=got["status"][K.ST_NAME_BYTES])
        same(again, want, caps)


def test_refused_kinds_are_verdicts_with_the_lowest_line():
    eng = H.get_engine()
    seen = set()
    for label, z, line, kind in K.hand_files((100,)):
        if line is None:
            continue
        got, want, _ = device_index(eng, z)
        assert got["status"][:3] == [K.ERR_BAD_INPUT, line, kind] and got["guard_intact"], label
        seen.add(kind)
        clean, want, _ = device_index(eng, K.committed_pairs()[0][1])
        same(clean, want, "after " + label)
    assert seen == {K.KIND_COLUMNS, K.KIND_WIDE, K.KIND_NEGATIVE_END, K.KIND_ORDER, K.KIND_NAME_AGAIN}
    # a refused line far behind the first tiles, and two refusals in different workgroups: the lowest wins
    text = K.random_text(11, 30000)
    lines = text.split(b"\n")
    lines[20000], lines[9000] = b"", lines[8000]
    bad = b"\n".join(lines)
    got, want, _ = device_index(eng, synth.bgzf_stream(bad, 65280, level=1)[0])
    assert want["status"][K.ST_VERDICT] == K.ERR_BAD_INPUT and want["status"][K.ST_LINE] <= 9001
    assert got["status"][:3] == want["status"][:3]


def test_caller_indexes_a_synthetic_call_and_the_fetch_reads_it_back(monkeypatch):
    monkeypatch.delenv("PLAT_CALLER_HOST_TBI", raising=False)
    regs = [synth.config4_region_arrays(i, region_len=4000, n_samples=1, read_len=100) for i in range(4)]
    nc = F.NativeCaller(0, 2, 2)
    try:
        opts = default_options(rlen=100)
        opts.originalMaxHaplotypes = opts.maxHaplotypes
        text = nc.call_regions([F.region_from_arrays(r) for r in regs], ["S1"], opts).encode("ascii")
        lens = [int(x) for x in nc.region_text_lengths(4)]
        packed, _ = nc.compress_text(K.HEADER + text, [len(K.HEADER)] + lens)
        packed = bytes(packed)
        tbi, info = nc.index_bgzf(packed, info=True)
        records = [ln for ln in text.split(b"\n") if ln]
        assert info.records == len(records) > 10 and info.lines == len(records) + 2 and info.device_calls >= 1 and info.contigs >= 1
        st, raw = K.index_of(packed)
        assert gzip.decompress(tbi) == raw
        monkeypatch.setenv("PLAT_CALLER_HOST_TBI", "1")
        assert nc.index_bgzf(packed) == tbi
        monkeypatch.delenv("PLAT_CALLER_HOST_TBI")
        tf = tabixindex.TabixFile(packed, tbi)
        eng = H.get_engine()
        first = lambda ln: (ln.split(b"\t")[0], int(ln.split(b"\t")[1]) - 1, int(ln.split(b"\t")[1]) - 1 + len(ln.split(b"\t")[3]))
        got_any = 0
        for r in regs:
            for k in range(3):
                beg, end = r["start"] + 1300 * k, r["start"] + 1300 * (k + 1) + 37
                stream = tf.fetch_blocks(r["chrom"], beg, end)
                assert stream is not None
                want = [ln + b"\n" for ln in records if first(ln)[0] == stream[0] and first(ln)[2] > beg and end > first(ln)[1]]
                assert T.mirror([stream])["text"] == b"".join(want), (r["chrom"], beg, end)
                got_any += len(want)
        assert got_any > 10
        # a refused file is a data error naming the line, and the caller goes on
        bad = synth.bgzf_stream(K.HEADER + b"20\t5\t.\tA\tC\n20\t4\t.\tA\tC\n")[0]
        with pytest.raises(_lib.PlatypusDeviceError) as e:
            nc.index_bgzf(bad)
        assert e.value.code == K.ERR_BAD_INPUT and "line 4 " in str(e.value)
        assert nc.index_bgzf(packed) == tbi
    finally:
        nc.close()


def test_cli_writes_an_index_the_next_run_opens(tmp_path):
    from platypus_amd.__main__ import call_variants
    out = tmp_path / "x.vcf.gz"
    base = ["--synthetic", "config4:4", "--bufferSize", "4000"]
    call_variants(base + ["--output", str(out), "--outputIndex", "1"])
    tbi = tmp_path / "x.vcf.gz.tbi"
    assert tbi.exists()
    idx = tabixindex.TabixIndex(tbi.read_bytes())
    assert idx.names and sum(len(c) for bins in idx.bins for c in bins.values()) >= 1
    st, raw = K.index_of(out.read_bytes())
    assert gzip.decompress(tbi.read_bytes()) == raw
    plain = tmp_path / "y.vcf"
    call_variants(base + ["--output", str(plain), "--source", str(out)])
    assert sum(1 for ln in plain.read_text().split("\n") if ln and not ln.startswith("#")) > 10
    assert not (tmp_path / "y.vcf.tbi").exists()
