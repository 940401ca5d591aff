"""GPU tests of source VCFs taken as the BGZF blocks of their tabix fetches: plat_tabix_fetch_batch directly over plat_bgzf_inflate_batch's
output against the plain-Python mirror (tests/tabix_cases.py) on the goldens (what the reference's own tabix returned), the hand-made edge
streams and a seeded fuzz; degenerate batches, the capacity, a refusal next to good streams; the region loop through source_blocks=
against the same loop through source_lines=, on the device and with PLAT_CALLER_HOST_TABIX=1; and the command line with a .tbi."""
import random

import numpy as np
import pytest

from platypus_amd import fastcaller as F, hostapi as H, tabixindex
from platypus_amd.options import default_options
from tests import region_golden as R
from tests import source_golden as S
from tests import tabix_cases as T

pytestmark = pytest.mark.gpu

PAYLOADS = (65536, 100, 37)


@pytest.fixture(scope="module")
def eng():
    return H.get_engine()


def fetch(eng, streams, cap_text=None):
    """inflate + fetch on the device; the fetch's dict."""
    a = T.batch_arrays(streams)
    inf = eng.bgzf_inflate(a["blob"], a["blk_off"], blk_limit=a["blk_limit"], keep_device=True)
    assert inf["guard_intact"] and int(inf["status"][2]) == a["inflated"]
    return eng.tabix_fetch(inf, a, cap_text)


def same(got, want):
    assert got["guard_intact"]
    assert got["status"] == want["status"] and got["off"] == want["off"] and got["counts"] == want["counts"]
    assert got["text"] == want["text"]


def test_goldens_on_the_device(eng):
    """Every golden query alone in a batch would be ninety launches of seven kernels: the files' queries go file by file, and all at once."""
    golden = T.golden_streams()
    by_file = {}
    for label, stream, lines in golden:
        by_file.setdefault(label.split(" ")[1], []).append((stream, lines))
    assert len(by_file) == 3
    for group in by_file.values():
        got = fetch(eng, [s for s, _ in group])
        same(got, T.mirror([s for s, _ in group]))
        for k, (_, lines) in enumerate(group):                        # ... which is what the reference returned
            assert got["text"][got["off"][k]:got["off"][k + 1]] == b"".join(x + b"\n" for x in lines)
    everything = [s for _, s, _ in golden]
    same(fetch(eng, everything), T.mirror(everything))
    # one query alone, with a line longer than a 64 KiB block: the whole line comes back
    label, stream, lines = max(golden, key=lambda g: max([len(x) for x in g[2]] + [0]))
    assert max(len(x) for x in lines) > 65536
    same(fetch(eng, [stream]), T.mirror([stream]))


@pytest.mark.parametrize("payload", PAYLOADS)
def test_edge_streams_on_the_device(eng, payload):
    """Each stream alone, and all of them in one batch: a refused stream leaves the other streams' output intact."""
    edges = T.edge_streams(payload)
    for label, s in edges:
        got = fetch(eng, [s])
        want = T.mirror([s])
        assert got["status"] == want["status"] and got["counts"] == want["counts"] and got["text"] == want["text"] and got["guard_intact"], label
    streams = [s for _, s in edges]
    want = T.mirror(streams)
    assert want["status"][0] == T.PLAT_ERR_BAD_INPUT and want["status"][1] == 1 and want["status"][2] > 30
    same(fetch(eng, streams), want)


def many_streams(n):
    """n streams of one to four lines in blocks of 1 to 50 bytes; every third fetches behind its lines."""
    line = b"20\t100\t.\tA\tC\t.\t.\tDP=1\n"
    return [(b"20", 0 if k % 3 else 100, 1000, T.cut(line * (1 + k % 4), 1 + k % 50, [(0, None)])) for k in range(n)]


def test_degenerate_batches(eng):
    same(fetch(eng, []), {"text": b"", "off": [0], "counts": [], "status": [0, -1, 0, 0]})
    empty = (b"20", 0, 100, [])
    same(fetch(eng, [empty, empty, empty]), T.mirror([empty] * 3))
    many = many_streams(700)
    want = T.mirror(many)
    assert want["status"][2] == sum(1 + k % 4 for k in range(700) if k % 3)
    same(fetch(eng, many), want)


def test_scans_take_a_second_round(eng):
    """One round of the workgroup scan is 4096 elements.  One stream of more tiles (1024 bytes) than that, with kept and skipped lines that
    start in the tiles of the second round; then more streams than that."""
    ROUND, TILE = 4096, 1024
    wide = lambda pos: b"20\t%d\t.\tA\tC\t.\t.\tDP=1\tGT" % pos + b"\t0/1" * 17499 + b"\n"
    front = b"".join(wide(10 if k % 3 == 2 else 100) for k in range(59))                  # every third lies in front of the fetch: skipped
    short = b"20\t100\t.\tA\tC\t.\t.\tDP=1\t\n"
    filler = short[:-1] + b"x" * (ROUND * TILE + 5 - len(front) - len(short)) + b"\n"    # ends five bytes into tile 4096
    behind = [b"20\t101\t.\tG\tT\t.\t.\tDP=2\n", b"20\t11\t.\tG\tT\t.\t.\tDP=3\n", b"20\t102\t.\tGA\tG\t.\t.\tDP=4\n",
              b"20\t103\t.\tA\tT\t.\t.\tDP=5\t" + b"x" * 1100 + b"\n"]
    text = front + filler + b"".join(behind)
    assert len(front) + len(filler) == ROUND * TILE + 5 and (ROUND + 1) * TILE < len(text) < (ROUND + 2) * TILE
    stream = (b"20", 50, 1000, T.cut(text, 65536, [(0, None)]))
    want = T.mirror([stream])
    assert want["counts"] == [64, 44] and want["status"][0] == 0 and want["text"].endswith(filler + behind[0] + behind[2] + behind[3])
    same(fetch(eng, [stream]), want)
    many = many_streams(ROUND + 4)
    want = T.mirror(many)
    assert want["status"][2] == sum(1 + k % 4 for k in range(ROUND + 4) if k % 3)
    same(fetch(eng, many), want)


def test_capacity(eng):
    streams = [s for _, s, _ in T.golden_streams() if s[0] == b"20"][:12]
    want = T.mirror(streams)
    full = want["status"][3]
    assert full > 5000
    for cap in (full - 1, full // 2, 0):
        got = fetch(eng, streams, cap_text=cap)
        assert got["guard_intact"] and got["status"] == [T.PLAT_ERR_OVERFLOW, -1, want["status"][2], full]
        assert got["text"] == want["text"][:cap] and got["off"] == [min(o, cap) for o in want["off"]] and got["counts"] == want["counts"]
    same(fetch(eng, streams, cap_text=full), want)                     # the repeated call, with room
    # a refusal wins over an overflow
    bad = streams + [(b"20", 0, 100, T.cut(b"20\t99999999999\n", 100, [(0, None)]))]
    got = fetch(eng, bad, cap_text=10)
    assert got["status"][:2] == [T.PLAT_ERR_BAD_INPUT, len(streams)] and got["guard_intact"]


def fuzz_stream(rng):
    """One short stream: 1-40 lines of random columns, a random block payload down to 1 byte, random chunk cuts on line boundaries."""
    name = rng.choice([b"20", b"2", b"chr1", b"20_alt"])
    def pos(at):
        form = rng.random()
        return (b"%d" % at if form < 0.85 else b"0%o" % at if form < 0.89 else b"0x%x" % at if form < 0.93 else b" %d" % at if form < 0.97 else
                rng.choice([b"", b"-3", b"x", b"+%d" % at, b"99999999999", b"%d\r" % at]))
    def info(at):
        form = rng.random()
        return (b"DP=%d" % rng.randrange(99) if form < 0.65 else b"END=%d" % (at + rng.randrange(300)) if form < 0.75 else b"SVEND=%d" % rng.randrange(50) if form < 0.8 else
                b"CIEND=1;END=%d" % (at + rng.randrange(300)) if form < 0.93 else rng.choice([b"END=-5", b"END=", b"XEND=3;END=", b".", b"END=0x20", b";END=12", b"END=99999999999"]))
    lines, at = [], rng.randrange(1, 200)
    for _ in range(rng.randrange(1, 41)):
        at += rng.randrange(0, 30)
        kind = rng.random()
        if kind < 0.86:
            cols = [name, pos(at), b".", b"ACGT"[:rng.randrange(0, 5)], b"C", b"9", b".", info(at)][:rng.choice([8, 8, 8, 8, 8, 2, 3, 4, 5, 7])]
            if len(cols) == 8 and rng.random() < 0.7:
                cols += [b"GT", b"\t".join([b"0/1"] * rng.randrange(1, 30))]
            ln = b"\t".join(cols)
            if rng.random() < 0.03:
                ln = ln.replace(b"\t", b"\x00", 1)
        elif kind < 0.93:
            ln = b"#" + bytes(rng.randrange(32, 127) for _ in range(rng.randrange(0, 40)))
        elif kind < 0.95:
            ln = rng.choice([name + b"x", name[:-1], b"", name, name.upper() + b"\t5"]) + rng.choice([b"", b"\t%d\t.\tA\tC" % at])
        else:
            ln = b"\t".join([name, b"%d" % at, b".", b"A" * rng.randrange(1, 400), b"C"])
        lines.append(ln)
    text = b"".join(x + b"\n" for x in lines)
    if rng.random() < 0.2:
        text = text[:-1]
    ends = [i + 1 for i, c in enumerate(text) if c == 10]
    cuts = sorted(set(rng.sample(ends, min(len(ends), rng.randrange(0, 4))))) if ends else []
    marks = [0] + [c for c in cuts if c < len(text)]
    spans = []
    for k, a in enumerate(marks):
        last = k + 1 == len(marks)
        if rng.random() < 0.25 and not last:
            continue                                                   # a gap: the chunks are not adjacent
        spans.append((a, None if last and rng.random() < 0.5 else (marks[k + 1] if not last else len(text))))
    payload = rng.choice([1, 2, 3, 7, 16, 37, 100, 1000, 65536])
    beg = rng.randrange(0, 400)
    return (name, beg, beg + rng.randrange(0, 600), T.cut(text, payload, spans, extra_blocks=rng.randrange(0, 3)))


@pytest.mark.parametrize("seed", (20, 21, 22))
def test_seeded_fuzz(eng, seed):
    """A hundred and fifty short streams per seed in one call: EVERY stream is compared with the mirror."""
    rng = random.Random(seed)
    streams = [fuzz_stream(rng) for _ in range(150)]
    want = T.mirror(streams)
    alone = [T.mirror([s]) for s in streams]
    assert sum(m["status"][0] != 0 for m in alone) >= 3 and sum(m["counts"][1] > 0 for m in alone) >= 75 and sum(m["counts"][0] > m["counts"][1] for m in alone) >= 30
    got = fetch(eng, streams)
    for k, m in enumerate(alone):
        assert got["counts"][2 * k:2 * k + 2] == m["counts"] and got["text"][got["off"][k]:got["off"][k + 1]] == m["text"], (seed, k)
    same(got, want)


# ---- the region loop -------------------------------------------------------------------------------------------------------------------
def region_blocks(case, payload, regions=None):
    return [[(reg["chrom"].encode(), 0, 1 << 29, T.cut(t.encode(), payload, [(0, None)])) for t in reg["source"]]
            for reg in (regions if regions is not None else [r for r in case["regions"] if r["loaded"]])]


def test_region_loop_through_blocks(monkeypatch):
    monkeypatch.delenv("PLAT_CALLER_HOST_TABIX", raising=False)
    cases = S.load("source_region_cases.json.gz")
    nc = F.NativeCaller(0, 2, 2)
    try:
        for ci, case in enumerate(cases):
            fasta, work, names = R.case_work(case)
            regs = [F.RegionReads.from_buffers(c, s, e, fasta, b) for c, s, e, b in work]
            want = nc.call_regions(regs, names, default_options(**case["options"]), source_lines=S.region_source(case))
            assert want.split("\n")[:-1] == case["lines"]
            n_lines = nc.stats["n_source_lines"]
            src = [t for r in S.region_source(case) for t in r]
            for host in (False, True):
                if host:
                    monkeypatch.setenv("PLAT_CALLER_HOST_TABIX", "1")
                else:
                    monkeypatch.delenv("PLAT_CALLER_HOST_TABIX", raising=False)
                o = default_options(**case["options"])
                got = nc.call_regions(regs, names, o, source_blocks=region_blocks(case, (37, 100, 65536)[ci % 3]))
                assert got == want and o.rlen == case["rlen_after"] and nc.stats["n_source_lines"] == n_lines
                info = nc.source_blocks_info
                assert info["inflated_bytes"] == info["kept_bytes"] == sum(len(t) for t in src) and info["lines_kept"] == info["lines_walked"] == n_lines
                assert info["compressed_bytes"] > 0 and info["n_blocks"] >= len(src) and info["seconds"] > 0
        monkeypatch.delenv("PLAT_CALLER_HOST_TABIX", raising=False)
        # a refusal names its place and leaves the caller usable; the blocks applied to one call
        case = cases[0]
        fasta, work, names = R.case_work(case)
        regs = [F.RegionReads.from_buffers(c, s, e, fasta, b) for c, s, e, b in work]
        bad = region_blocks(case, 100)
        bad[0][0] = (b"20", 0, 1 << 29, T.cut(b"20\t99999999999\t.\tA\tC\n", 100, [(0, None)]))
        with pytest.raises(F._lib.PlatypusDeviceError) as e:
            nc.set_source_blocks(bad)
        assert e.value.code == -9 and "line walk of region 0, file 0" in str(e.value)
        d = bytes(region_blocks(case, 100)[0][0][3][0][0])
        at, n, _ = T.blocks_of(d)[1]
        broken = region_blocks(case, 100)
        broken[0][0] = (b"20", 0, 1 << 29, [(np.frombuffer(d[:at + n - 8] + bytes([d[at + n - 8] ^ 1]) + d[at + n - 7:], dtype=np.uint8), 0, -1, 0)])
        with pytest.raises(F._lib.PlatypusDeviceError) as e:
            nc.set_source_blocks(broken)
        assert e.value.code == -9 and "block 1 of region 0, file 0, chunk 0 cannot be inflated" in str(e.value)
        got = nc.call_regions(regs, names, default_options(**case["options"]), source_blocks=region_blocks(case, 100))
        assert got.split("\n")[:-1] == case["lines"]
    finally:
        nc.close()


def test_bgzf_front_end_through_blocks():
    """plat_call_bgzf_regions with source_blocks= gives what it gives with source_lines=."""
    case = next(c for c in S.load("source_region_cases.json.gz") if len(c["regions"]) == 2)
    fc = S.load("region_fetched_cases.json.gz")[case["base_case"]]
    fasta = H.FastaFile({"20": fc["ref"].encode()})
    mk = lambda lst: [H.AlignedRead(x["seq"].encode(), bytes(ord(c) - 33 for c in x["qual"]), x["pos"], x["mapq"], x["flag"], end=x["end"],
                                    cigarOps=[tuple(c) for c in x["cigar"]], chromID=x["chromID"], mateChromID=x["mateChromID"], insertSize=x["insertSize"],
                                    matePos=x["matePos"]) for x in lst]
    regs = lambda: [F.BgzfRegion.from_reads(r["chrom"], r["start"], r["end"], fasta, [(mk(s["fetched"]), []) for s in r["samples"]]) for r in fc["regions"]]
    names = fc["sample_names"]
    src = S.region_source(case)
    nc = F.NativeCaller(0, 2, 2)
    try:
        want = nc.call_bgzf_regions(regs(), names, default_options(**case["options"]), source_lines=src)
        n_lines = nc.stats["n_source_lines"]
        assert want.count("\n") > 0 and "File" in want and n_lines == sum(t.count(b"\n") for r in src for t in r)
        got = nc.call_bgzf_regions(regs(), names, default_options(**case["options"]), source_blocks=region_blocks(case, 37, case["regions"]))
        assert got == want and nc.stats["n_source_lines"] == n_lines and nc.loaded == [1, 1]
        assert nc.call_bgzf_regions(regs(), names, default_options(**case["options"])) != want and nc.stats["n_source_lines"] == 0
    finally:
        nc.close()


def test_cli_config4_with_an_indexed_source_file(tmp_path, capsys):
    """`callVariants --synthetic=config4:N --source=known.vcf.gz` with a .tbi next to it (written by the reference's indexer when the goldens
    were made) gives the records the plain known.vcf gives through the CLI's stand-in."""
    from platypus_amd.__main__ import call_variants
    cli = T.golden_cli()
    (tmp_path / "known.vcf").write_bytes(cli["vcf"])
    (tmp_path / "known.vcf.gz").write_bytes(cli["vcf_gz"])
    (tmp_path / "known.vcf.gz.tbi").write_bytes(cli["tbi"])
    assert tabixindex.TabixFile.open(str(tmp_path / "known.vcf.gz")).index.names == [b"r0", b"r1"]
    args = ["--synthetic", "config4:2", "--bufferSize", "4000", "--nCPU", "1"]
    call_variants(args + ["--source", str(tmp_path / "known.vcf"), "--output", str(tmp_path / "plain.vcf")])
    call_variants(args + ["--source", str(tmp_path / "known.vcf.gz"), "--output", str(tmp_path / "indexed.vcf")])
    want = [ln for ln in open(tmp_path / "plain.vcf") if not ln.startswith("#")]
    got = [ln for ln in open(tmp_path / "indexed.vcf") if not ln.startswith("#")]
    assert got == want and sum("File" in ln.split("Source=")[1].split(";")[0] for ln in got if "Source=" in ln) >= 4
    capsys.readouterr()
