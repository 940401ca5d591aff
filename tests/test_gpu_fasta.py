"""GPU tests of the indexed FASTA fetch on the device: plat_fasta_fetch_batch against the fixture (tests/golden/fasta_cases.json.gz) and
against the host twin (csrc/fasta_rule.hpp through tests/fasta_host_driver.cpp, which tests/test_fasta_cpu.py pins to the fixture) on
files sized to where the kernels change path -- T = plat_fasta_tile_bytes(): spans around a tile and two, every residue of a span's start
and of the output's address modulo 16, newlines on both sides of a tile's edge, cuts of the file, a capacity one byte short, a mixed
batch --, then the caller library, hostapi.IndexedFastaFile and the CLI end to end."""
import json
import os
import random
import subprocess
import sys

import pytest

from platypus_amd import _lib, fastcaller as F, hostapi as H
from tests import fasta_cases as FC, region_golden as R

pytestmark = pytest.mark.gpu
FILES, _BAD = FC.golden_files()
NO_LINES = 1 << 40                                                          # a LineLength no position reaches: offset = StartPos + pos


@pytest.fixture(scope="module")
def eng():
    return H.get_engine()


@pytest.fixture(scope="module")
def T(eng):
    t = eng.lib.plat_fasta_tile_bytes()
    assert t == 1024
    return t


def expect(eng, cut, queries, file_base=0, file_size=None, **kw):
    """The device's answer equals the twin's: bytes, status, offsets, totals; nothing written outside what the totals name."""
    want, status = FC.twin_fetch(cut, queries, file_base, file_size)
    got = eng.fasta_fetch(cut, queries, file_base=file_base, file_size=file_size, cap_bytes=sum(len(w) for w in want) + 7, **kw)
    assert got["status"] == status and got["guard_intact"]
    assert got["seqs"] == want, [k for k in range(len(want)) if got["seqs"][k] != want[k]][:5]
    assert got["off"] == [sum(len(w) for w in want[:k]) for k in range(len(want) + 1)]
    assert got["totals"][0] == 0 and got["totals"][1] == got["off"][-1] and got["totals"][3] == sum(s != 0 for s in status)
    return got


def seeded_file(seed, n, line_len, eol=b"\n", last_newline=True):
    rng = random.Random(seed)
    seq = bytes(rng.choice(b"ACGTacgtNnRYKM") for _ in range(n))
    data, fai = FC.write_fasta([(b"h%d some words" % seed, seq)], line_len, eol, last_newline)
    name, n_, start, L, full = fai.split(b"\t")
    return data, (int(start), int(L), int(full), int(n_)), seq


@pytest.mark.parametrize("fi", range(len(FILES)))
def test_device_equals_the_fixture(eng, fi):
    f = FILES[fi]
    qs = [FC.entry_of(f["refs1"], q["name"]) + (q["beg"], q["end"], 0) for q in f["queries"]]
    got = expect(eng, f["fasta"], qs)
    for q, s, st in zip(f["queries"], got["seqs"], got["status"]):
        assert FC.RAISES.get(st) == q["raises"] and (q["raises"] or s == q["seq"]), (f["label"], q)
    # whole contigs: the last base getSequence never returns is there (the twin, pinned by the CPU test); beg and end are not read
    whole = expect(eng, f["fasta"], [FC.entry_of(f["refs1"], n) + (9, 3, 1) for n in f["refs1"]])
    if "ragged" not in f["label"] and "lies" not in f["label"]:
        for (name, v), s in zip(f["refs1"].items(), whole["seqs"]):
            most = next(q["seq"] for q in f["queries"] if q["name"] == name and (q["beg"], q["end"]) == (0, v[1]))
            assert s[:len(most)] == most and len(s) == len(most) + 1


def test_span_seams_and_every_residue(eng, T):
    rng = random.Random(5)
    cut = bytes(rng.choice(b"acgtACGTn") for _ in range(4 * T + 300))
    qs = []
    for size in (T - 1, T, T + 1, 2 * T + 1):
        for r in range(16):                                                 # the span [48 + r, 48 + r + size) of the file: one long line
            qs.append((48 + r, NO_LINES, NO_LINES, 4 * T, 0, size, 0))
    qs += [(0, NO_LINES, NO_LINES, T + 1, 0, 0, 1), (16, NO_LINES, NO_LINES, 3 * T, 0, 0, 1), (5, NO_LINES, NO_LINES, 2 * T + 11, 0, 0, 1)]
    expect(eng, cut, qs)
    for r in range(1, 16, 3):                                               # the blob itself at other residues of its address
        expect(eng, cut, qs[r::7], guard=64 + r)
    # a newline as the last byte of a tile and as the first of the next, for spans that begin in the tile's first word and later
    for at in (T - 1, T, 2 * T - 1, 2 * T):
        b = bytearray(cut)
        b[at] = 0x0A
        b[at + 17] = 0x0A
        expect(eng, bytes(b), [(0, NO_LINES, NO_LINES, 4 * T, 0, 3 * T, 0), (3, NO_LINES, NO_LINES, 4 * T, 0, 3 * T, 0), (0, NO_LINES, NO_LINES, 4 * T, at - 1, at + 2, 0),
                               (0, NO_LINES, NO_LINES, 4 * T, at, at + 1, 0), (0, NO_LINES, NO_LINES, 4 * T, at + 1, at + 40, 0)])


@pytest.mark.parametrize("line_len, eol, n", [(1, b"\n", 2600), (60, b"\n", 7000), (70, b"\r\n", 7000), (3 * 1024 + 77, b"\n", 5 * 1024)])
def test_line_lengths(eng, T, line_len, eol, n):
    for last_newline in (True, False):                                      # (False: a last line without a newline, the cut's last word short)
        data, e, seq = seeded_file(line_len, n, line_len, eol, last_newline)
        rng = random.Random(n)
        qs = [e + (0, 0, 1), e + (0, n, 0), e + (0, n - 1, 0), e + (n - 1, n + 3, 0)]
        for _ in range(60):
            b = rng.randrange(-3, n)
            qs.append(e + (b, b + rng.randrange(0, 2 * T + 50), 0))
        qs += [e + (line_len - 1, line_len, 0), e + (line_len, line_len + 1, 0), e + (0, line_len, 0), e + (2 * line_len, 2 * line_len, 0), e + (9, 2, 0)]
        got = expect(eng, data, qs)
        want = seq.upper() if eol == b"\n" else None
        if want is not None:
            assert got["seqs"][0] == want and got["seqs"][1] == want[:n - 1] and got["status"][-1] == FC.INDEX_ERROR


def test_file_and_index_edges(eng, T):
    data, e, seq = seeded_file(11, 3 * T, 60, last_newline=False)
    size = len(data)
    long_ = (e[0], e[1], e[2], 10 * T)                                      # an index that claims more than the file holds
    far = (size + 500, 60, 61, 100)
    qs = [long_ + (0, 10 * T, 0), long_ + (0, 0, 1), long_ + (4 * T, 5 * T, 0), far + (0, 50, 0), far + (0, 0, 1), (e[0], 0, 1, e[3], 0, 10, 0), (e[0], 0, 1, e[3], 0, 0, 1),
          (-4, 60, 61, 100, 0, 10, 0), (e[0], 60, 59, 100, 0, 10, 0), (e[0], -60, 61, 100, 0, 10, 0), (1 << 62, 1 << 61, 1 << 62, 1 << 62, 1 << 61, 1 << 62, 0)]
    got = expect(eng, data, qs)
    assert got["status"] == [0, 0, 0, 0, 0, FC.ZERO_LINE, FC.ZERO_LINE, FC.BAD_INDEX, FC.BAD_INDEX, FC.BAD_INDEX, FC.BAD_INDEX]       # (the last one's offsets leave 63 bits)
    assert got["seqs"][0] == seq.upper() and got["seqs"][2] == got["seqs"][3] == got["seqs"][4] == b"" and got["seqs"][-1] == b""


def test_cuts_of_the_file(eng, T):
    data, e, seq = seeded_file(12, 6 * T, 60)
    for base, end in ((1000, 1000 + 3 * T + 5), (32, len(data) - 3), (2 * T + 7, 2 * T + 7 + 333)):
        cut = data[base:end]
        inside_b = (base - e[0]) * 60 // 61 + 70                            # a base whose offset lies well inside the cut
        qs = [e + (inside_b, inside_b + 100, 0), e + (0, inside_b, 0), e + (inside_b, 6 * T, 0), e + (0, 0, 1), e + (inside_b + 5, inside_b + 5, 0),
              e + (inside_b, inside_b + 200, 0), e + (3, 1, 0)]
        got = expect(eng, cut, qs, file_base=base, file_size=len(data))
        assert got["status"] == [0, FC.LEFT_OF_CUT, FC.RIGHT_OF_CUT, FC.LEFT_OF_CUT, 0, 0, FC.INDEX_ERROR]
        assert got["seqs"][0] == seq.upper()[inside_b:inside_b + 100] and got["seqs"][1] == got["seqs"][2] == b""


def test_capacity_one_short_then_enough(eng, T):
    data, e, seq = seeded_file(13, 2 * T + 100, 60)
    qs = [e + (5, 900, 0), e + (0, 0, 1), e + (7, 7, 0), e + (T, 2 * T, 0)]
    want, status = FC.twin_fetch(data, qs)
    need = sum(len(w) for w in want)
    short = eng.fasta_fetch(data, qs, cap_bytes=need - 1)
    assert short["totals"][:2] == [-8, need] and short["seqs"] == [None] * 4 and short["guard_intact"] and short["status"] == status
    assert short["off"] == [sum(len(w) for w in want[:k]) for k in range(5)]
    exact = eng.fasta_fetch(data, qs, cap_bytes=need)
    assert exact["totals"][:2] == [0, need] and exact["seqs"] == want and exact["guard_intact"]
    none = eng.fasta_fetch(data, qs, cap_bytes=0)
    assert none["totals"][:2] == [-8, need] and none["guard_intact"]


def test_mixed_batch_and_no_queries(eng, T):
    rng = random.Random(14)
    contigs = [(b"c%d" % k, bytes(rng.choice(b"ACGTacgtn") for _ in range(n))) for k, n in enumerate((310000, 5000, 777))]
    data, fai = FC.write_fasta(contigs, 60)
    refs = FC.twin_refs(fai, 0)
    ent = [(v[1], v[2], v[3], v[0]) for v in (refs[b"c0"], refs[b"c1"], refs[b"c2"])]
    qs = []
    for k in range(1000):
        e = ent[rng.randrange(3)]
        b = rng.randrange(-5, e[3])
        qs.append(e + (b, b + rng.randrange(0, 201), 0))
        if k == 500:
            qs.append(ent[0] + (700, 700 + 300 * 1024, 0))                  # one of 300 KB among them
    got = expect(eng, data, qs)
    assert got["seqs"][501] == contigs[0][1].upper()[700:700 + 300 * 1024] and got["totals"][2] > 300
    got = expect(eng, data, [ent[0] + (0, 0, 1), ent[1] + (0, 0, 1), ent[2] + (0, 0, 1)])
    assert got["seqs"] == [c[1].upper() for c in contigs]
    empty = eng.fasta_fetch(data, [])
    assert empty["totals"] == [0, 0, 0, 0] and empty["off"] == [0] and empty["guard_intact"]
    assert eng.fasta_fetch(b"", [ent[2] + (0, 5, 0)], file_size=0)["seqs"] == [b""]


def test_caller_library_equals_the_fixture_and_the_twin(monkeypatch):
    monkeypatch.delenv("PLAT_CALLER_HOST_FASTA", raising=False)
    nc = F.NativeCaller(0, 1, 1)
    try:
        for f in FILES:
            fa = nc.open_fasta(f["fasta"], f["fai"], 1)
            ask = [(fa.tid(q["name"]), q["beg"], q["end"]) for q in f["queries"]]
            got, info = fa.get_sequences(ask, info=True)
            assert info["device_calls"] == 1 and 0 < info["file_bytes"] <= len(f["fasta"]) + 16
            for q, g in zip(f["queries"], got):
                assert (FC.RAISES[g] == q["raises"]) if isinstance(g, int) else (q["raises"] is None and g == q["seq"]), (f["label"], q)
            assert fa.get_sequences([]) == []
            monkeypatch.setenv("PLAT_CALLER_HOST_FASTA", "1")
            assert fa.get_sequences(ask) == got
            monkeypatch.delenv("PLAT_CALLER_HOST_FASTA")
            tids = [t for t, r in enumerate(fa.refs) if r[3] != 0]
            fa.load(tids[1:])                                              # some now, the rest when they are asked for
            for t in tids:
                arr, dev = fa.contig(t)
                e = fa.refs[t]
                assert dev and arr.tobytes() == FC.twin_fetch(f["fasta"], [(e[2], e[3], e[4], e[1], 0, 0, 1)])[0][0]
            fa.close()
    finally:
        nc.close()


def test_region_goldens_from_a_fasta_file_on_the_device(monkeypatch, tmp_path):
    monkeypatch.delenv("PLAT_CALLER_HOST_FASTA", raising=False)
    got, want = FC.region_lines_through_fasta(None, tmp_path, R.load_cases())
    assert len(want) == 245 and got == want, R.diff(got, want)


def test_indexed_fasta_file_equals_the_fixture(tmp_path):
    nc = F.NativeCaller(0, 1, 1)
    try:
        for k, f in enumerate(FILES):
            path = str(tmp_path / ("f%d.fa" % k))
            with open(path, "wb") as out, open(path + ".fai", "wb") as fai:
                out.write(f["fasta"])
                fai.write(f["fai"])
            ff = H.IndexedFastaFile(path, path + ".fai", parseNCBI=True, caller=nc)
            name = lambda b: b.decode("latin-1")
            assert {n: (r.SeqLength, r.StartPos, r.LineLength, r.FullLineLength) for n, r in ff.refs.items()} == {name(n): tuple(v[1:]) for n, v in f["refs1"].items()}
            assert ff.getTotalSequenceLength() == sum(v[1] for v in f["refs1"].values())
            for q in f["queries"][::2]:
                if q["raises"]:
                    with pytest.raises({"IndexError": IndexError, "ZeroDivisionError": ZeroDivisionError}[q["raises"]]):
                        ff.getSequence(name(q["name"]), q["beg"], q["end"])
                else:
                    assert ff.getSequence(name(q["name"]), q["beg"], q["end"]) == q["seq"]
            for c in f["chars"]:
                if c["raises"]:
                    with pytest.raises(ZeroDivisionError):
                        ff.getCharacter(name(c["name"]), c["pos"])
                else:
                    assert ff.getCharacter(name(c["name"]), c["pos"]) == c["char"]
            # the cache: set once, answered by slices where the reference's test lets it
            first = name(next(iter(f["refs1"])))
            if f["refs1"][next(iter(f["refs1"]))][3] > 0:
                ff.setCacheSequence(first, 0, 40)
                assert ff.getSequence(first, 2, 9) == ff.cache[2:9] and ff.cacheStartPos == 0
            with pytest.raises(Exception, match="Invalid contig name nope"):
                ff.setCacheSequence("nope", 0, 1)
            ff.close()
    finally:
        nc.close()


@pytest.mark.parametrize("python_loop", [False, True])
def test_cli_ref_file_equals_the_generator(tmp_path, python_loop):
    """--synthetic=config4:4 with the regions' contigs taken from a FASTA file through the new path: the same record lines as without."""
    from platypus_amd import synth
    size = 3000
    ref = str(tmp_path / "config4.fa")
    assert synth.write_config4_fasta(ref, 4, size, arrays=not python_loop) == ["r0", "r1", "r2", "r3"]
    env = dict(os.environ, PLAT_PYTHON_CALLER="1" if python_loop else "0")
    env.pop("PLAT_CALLER_HOST_FASTA", None)
    base = [sys.executable, "-m", "platypus_amd", "callVariants", "--synthetic", "config4:4", "--bufferSize", str(size)]
    texts = []
    for extra in ([], ["--refFile", ref]):
        out = tmp_path / ("with.vcf" if extra else "without.vcf")
        r = subprocess.run(base + extra + ["--output", str(out)], capture_output=True, text=True, env=env)
        assert r.returncode == 0, r.stderr[-1500:]
        assert json.loads(r.stdout.strip().splitlines()[-1])["records"] > 5
        texts.append([ln for ln in out.read_text().split("\n") if not ln.startswith("##")])
    assert texts[0] == texts[1]
    # a region whose contig the index lacks ends the run with the reference's message
    with open(ref + ".fai") as f:
        lines = f.read().split("\n")
    with open(ref + ".fai", "w") as f:
        f.write("\n".join(lines[:2] + lines[3:]))
    r = subprocess.run(base + ["--refFile", ref, "--output", str(tmp_path / "no.vcf")], capture_output=True, text=True, env=env)
    assert r.returncode != 0 and "Invalid contig name r2. Make sure your FASTA reference file and query regions have the same naming convention" in r.stderr
