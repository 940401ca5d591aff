"""Helper of the FASTA fetch tests (not a test module): the fixture (tests/golden/fasta_cases.json.gz: small FASTA files with their .fai
texts, queries, and per query what the reference's FastaIndex.getRefs / FastaFile.getSequence / getCharacter return or raise --
gen_golden_fasta.py writes it from the files made here, README_fasta.md says how), the writer of FASTA files with a chosen line layout,
the HOST TWIN of the device call as a ctypes library (tests/fasta_host_driver.cpp over csrc/fasta_rule.hpp: what the caller library runs
under PLAT_CALLER_HOST_FASTA=1), which tests/test_fasta_cpu.py pins to the fixture and the GPU tests then take their expectations from,
and the seeded cases beyond the fixture."""
import ctypes as C
import gzip
import json
import os
import random
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden", "fasta_cases.json.gz")
OK, INDEX_ERROR, ZERO_LINE, BAD_INDEX, LEFT_OF_CUT, RIGHT_OF_CUT = range(6)
RAISES = {INDEX_ERROR: "IndexError", ZERO_LINE: "ZeroDivisionError"}


def write_fasta(contigs, line_len=60, eol=b"\n", last_newline=True):
    """contigs: [(header bytes behind '>', sequence bytes)] -> (the file's bytes, its .fai's bytes as `samtools faidx` writes one: name,
    SeqLength, StartPos, LineLength, FullLineLength)."""
    out, fai = bytearray(), bytearray()
    for k, (head, seq) in enumerate(contigs):
        out += b">" + head + eol
        fai += b"%s\t%d\t%d\t%d\t%d\n" % (head.split()[0], len(seq), len(out), line_len, line_len + len(eol))
        for at in range(0, len(seq), line_len):
            out += seq[at:at + line_len]
            if at + line_len < len(seq) or last_newline or k + 1 < len(contigs):
                out += eol
    return bytes(out), bytes(fai)


def seeded_seq(rng, n, alphabet=b"ACGTacgtNn"):
    return bytes(rng.choice(alphabet) for _ in range(n))


def edge_queries(name, seq_len, line_len):
    """The positions the rule turns on, for one contig: column 0, the last column, one past a newline, empty, reversed, negative, past the
    end, the last base."""
    L = max(line_len, 1)
    qs = [(0, seq_len), (0, seq_len - 1), (0, seq_len + 5), (-3, 4), (0, 0), (5, 5), (7, 3), (seq_len - 1, seq_len), (seq_len, seq_len + 2),
          (seq_len - 2, seq_len - 1), (0, 1), (L - 1, L), (L, L + 1), (L - 1, L + 1), (L, 2 * L), (1, 2 * L + 1), (L + 1, 3 * L - 1), (-10, -2)]
    return [(name, b, e) for b, e in qs]


def fixture_files():
    """The files of the fixture, as dicts {label, fasta, fai, queries [(name, beg, end)], chars [(name, pos)]}: names are the index's keys
    under parseNCBI = 1."""
    rng = random.Random(20260214)
    files = []

    def add(label, fasta, fai, contigs, extra=()):
        qs, cs = list(extra), []
        for name, n, L in contigs:
            qs += edge_queries(name, n, L)
            for _ in range(12):
                b = rng.randrange(-2, n + 2)
                qs.append((name, b, b + rng.randrange(0, 3 * max(L, 1) + 2)))
            cs += [(name, p) for p in (-1, 0, 1, L - 1, L, n - 2, n - 1, n, n + 3)]
        files.append(dict(label=label, fasta=fasta, fai=fai, queries=qs, chars=cs))

    c60 = [(b"chr1 the first", seeded_seq(rng, 150)), (b"chr2", seeded_seq(rng, 61, b"ACGTRYKMSWBDHVNacgtrykmswbdhvn")), (b"chrM", b"g")]
    add("60/61, mixed case and IUPAC codes, no newline at the end", *write_fasta(c60, 60, last_newline=False), [(b"chr1", 150, 60), (b"chr2", 61, 60), (b"chrM", 1, 60)])
    c70 = [(b"a", seeded_seq(rng, 211)), (b"b", seeded_seq(rng, 140))]
    add("70/72 CRLF", *write_fasta(c70, 70, eol=b"\r\n"), [(b"a", 211, 70), (b"b", 140, 70)])
    add("1/2: every other byte a newline", *write_fasta([(b"x", seeded_seq(rng, 33)), (b"y", seeded_seq(rng, 8))], 1), [(b"x", 33, 1), (b"y", 8, 1)])
    # a ragged middle line: the index (written for 20/21) is wrong behind it, and the second contig's header leaks into the first's tail
    rag = b">r1\n" + seeded_seq(rng, 20) + b"\n" + seeded_seq(rng, 11) + b"\n" + seeded_seq(rng, 20) + b"\n" + seeded_seq(rng, 9) + b"\n>r2 next\n" + seeded_seq(rng, 30) + b"\n"
    add("a ragged middle line: header bytes leak", rag, b"r1\t70\t4\t20\t21\nr2\t30\t77\t20\t21\n", [(b"r1", 70, 20), (b"r2", 30, 20)])
    odd = bytes([0, 0x80, 0xFF, 0xE9, ord("a"), ord("z"), ord("{"), ord("`"), ord("@"), ord("["), 0x0D, 0x7F, 0xB5, ord("m"), 0xC4, 0x9A])
    body = odd * 3 + seeded_seq(rng, 12, bytes(range(1, 256)).replace(b"\n", b"").replace(b">", b""))
    add("NUL, bytes above 0x7f, the neighbours of a and z", *write_fasta([(b"odd", body)], 16), [(b"odd", len(body), 16)])
    # an index that claims more than the file holds: spans cut at the end of the file and wholly past it; LineLength 0; a later duplicate line
    short, _ = write_fasta([(b"s", seeded_seq(rng, 50))], 25, last_newline=False)
    lying = b"s\t50\t3\t25\t26\nlong\t500\t3\t25\t26\nfar\t40\t900\t25\t26\nzero\t50\t3\t0\t1\ns\t45\t3\t25\t26\n"
    add("an index that lies about the file's end, LineLength 0, a repeated name", short, lying, [(b"s", 45, 25), (b"long", 500, 25), (b"far", 40, 25), (b"zero", 50, 0)])
    # names: spaces, NCBI, junk behind numbers (atoll), a CRLF index
    n1, n2 = seeded_seq(rng, 30), seeded_seq(rng, 25)
    h1, h2, h3 = b">gi|568336023|ref|NC_000001.11| Homo\n", b">gi|1|gb|X| other\n", b">gi|2|ref\n"
    fa = h1 + n1 + b"\n" + h2 + n2 + b"\n" + h3 + n2 + b"\n"
    s1 = len(h1)
    s2 = s1 + 31 + len(h2)
    s3 = s2 + 26 + len(h3)
    fai = (b"gi|568336023|ref|NC_000001.11| Homo sapiens\t30junk\t %d\t30 \t31\tignored\textra\r\n" % s1 +
           b"  gi|1|gb|X|  other words\t25\t+%dx\t25\t26\r\n" % s2 + b"gi|2|ref\t25\t%d\t25\t26\r\n" % s3)
    add("names with spaces, NCBI names, junk behind numbers, a CRLF index", fa, fai, [(b"NC_000001.11", 30, 30), (b"gi|1|gb|X|", 25, 25), (b"gi|2|ref", 25, 25)])
    return files


# index texts the reference raises on (FastaIndex.getRefs): (label, fai, what the message names)
BAD_INDEXES = [
    ("four fields", b"a\t10\t3\t10\t11\nb\t10\t20\t10\n", "line 2"),
    ("a blank line", b"a\t10\t3\t10\t11\n\nb\t10\t20\t10\t11\n", "line 2"),
    ("a name field of blanks", b"a\t10\t3\t10\t11\nb\t10\t20\t10\t11\n \t \t10\t30\t10\t11\n", "line 3"),
]
# ... and the stated limits: lines the library refuses where the reference would seek to a negative offset
LIMIT_INDEXES = [
    ("a negative StartPos", b"a\t10\t-3\t10\t11\n", "line 1"),
    ("FullLineLength < LineLength", b"a\t10\t3\t10\t11\nb\t10\t20\t11\t10\n", "line 2"),
    ("a negative LineLength", b"a\t10\t3\t-10\t11\n", "line 1"),
]


def golden_files():
    """The fixture: per file a dict {label, fasta, fai (bytes), refs0 / refs1 (getRefs with parseNCBI 0 / 1: {name: [field 0, SeqLength,
    StartPos, LineLength, FullLineLength]}), queries [{name, beg, end, seq | raises}], chars [{name, pos, char | raises}]}, and the index texts getRefs raises on."""
    with gzip.open(GOLDEN, "rt") as f:
        raw = json.load(f)
    b = lambda s: s.encode("latin-1")
    out = []
    for f in raw["files"]:
        out.append(dict(label=f["label"], fasta=b(f["fasta"]), fai=b(f["fai"]),
                        refs0={b(k): [b(v[0])] + v[1:] for k, v in f["refs0"].items()}, refs1={b(k): [b(v[0])] + v[1:] for k, v in f["refs1"].items()},
                        queries=[dict(name=b(q["name"]), beg=q["beg"], end=q["end"], seq=b(q["seq"]) if "seq" in q else None, raises=q.get("raises")) for q in f["queries"]],
                        chars=[dict(name=b(c["name"]), pos=c["pos"], char=b(c["char"]) if "char" in c else None, raises=c.get("raises")) for c in f["chars"]]))
    return out, raw["bad_indexes"]


# ---- the host twin (csrc/fasta_rule.hpp through tests/fasta_host_driver.cpp) as a ctypes library ---------------------------------------
_twin = None


def twin_lib():
    global _twin
    if _twin is None:
        src, out = os.path.join(HERE, "fasta_host_driver.cpp"), os.path.join(HERE, "libfasta_host_driver.so")
        rule = os.path.join(ROOT, "platypus_amd", "csrc", "fasta_rule.hpp")
        if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(src), os.path.getmtime(rule)):
            subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-I" + os.path.dirname(rule), src, "-o", out])
        _twin = C.CDLL(out)
        _twin.fasta_twin_fetch.restype = C.c_int64
        _twin.fasta_twin_fetch.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]
        _twin.fasta_twin_parse.restype = C.c_int64
        _twin.fasta_twin_parse.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_int64, C.c_void_p]
        _twin.fasta_twin_char.restype = C.c_int
        _twin.fasta_twin_char.argtypes = [C.c_void_p, C.c_int64] + [C.c_int64] * 5
    return _twin


def twin_fetch(cut, queries, file_base=0, file_size=None):
    """The host twin of plat_fasta_fetch_batch: queries [(StartPos, LineLength, FullLineLength, SeqLength, beg, end, mode)] over the cut.
    Returns ([bytes per query], [status])."""
    cut = bytes(cut)
    n = len(queries)
    size = file_base + len(cut) if file_size is None else file_size
    q = np.ascontiguousarray(np.asarray([[int(x) for x in t] for t in queries], dtype=np.int64).reshape(n, 7))
    off, status, out = np.zeros(n + 1, dtype=np.int64), np.zeros(max(n, 1), dtype=np.int32), np.zeros(len(cut) * max(n, 1) + 1, dtype=np.uint8)
    total = twin_lib().fasta_twin_fetch(cut, len(cut), file_base, size, n, q.ctypes.data, off.ctypes.data, status.ctypes.data, out.ctypes.data, len(out))
    assert 0 <= total <= len(out)
    blob = out[:total].tobytes()
    return [blob[off[k]:off[k + 1]] for k in range(n)], status[:n].tolist()


def twin_parse(fai, parseNCBI):
    """The rule's .fai parse, line by line: [(rc, name bytes, SeqLength, StartPos, LineLength, FullLineLength)] (rc 0, 1: few fields, 2: no name)."""
    fai = bytes(fai)
    cap = fai.count(b"\n") + 2
    rows = np.zeros((cap, 7), dtype=np.int64)
    n = twin_lib().fasta_twin_parse(fai, len(fai), int(parseNCBI), cap, rows.ctypes.data)
    return [(int(r[0]), fai[r[1]:r[1] + r[2]] if r[0] == 0 else b"", int(r[3]), int(r[4]), int(r[5]), int(r[6])) for r in rows[:n]]


def twin_refs(fai, parseNCBI):
    """... as the dict getRefs returns: {name: (SeqLength, StartPos, LineLength, FullLineLength)}, a later line replacing an earlier one."""
    d = {}
    for rc, name, *nums in twin_parse(fai, parseNCBI):
        assert rc == 0
        d[name] = tuple(nums)
    return d


def twin_char(data, entry, pos):
    """getCharacter by the rule: (the byte, or b"" where the file ends in front of it; status)."""
    data = bytes(data)
    r = twin_lib().fasta_twin_char(data, len(data), *[int(x) for x in entry], int(pos))
    return (b"" if r & 0x100 else bytes([r & 0xff])), r >> 12


def entry_of(refs, name):
    """(StartPos, LineLength, FullLineLength, SeqLength) of a getRefs value [field 0, SeqLength, StartPos, LineLength, FullLineLength]."""
    v = refs[name]
    return (v[2], v[3], v[4], v[1])


def write_region_fasta(path, contigs, line_len, eol=b"\n"):
    """{name: sequence} to path and path + '.fai'."""
    data, fai = write_fasta([(k.encode() if isinstance(k, str) else k, bytes(v)) for k, v in contigs.items()], line_len, eol)
    with open(path, "wb") as f:
        f.write(data)
    with open(path + ".fai", "wb") as f:
        f.write(fai)
    return data, fai


def region_lines_through_fasta(lib, tmp_path, cases):
    """Every region golden with its contig written to a FASTA file: at 60/61 the contigs plat_fasta_contig hands over feed the native loop;
    at 7/9 CRLF they hold the '\\r' of every line and differ -- only that is asserted.  Returns (lines, the goldens' lines)."""
    from platypus_amd import fastcaller as F
    from platypus_amd.options import default_options
    from tests import region_golden as R
    got, want = [], []
    for ci, case in enumerate(cases):
        fasta, work, names = R.case_work(case)
        ref = case["ref"].encode()
        nc = F.NativeCaller(0, 2, 2, lib=lib) if lib is not None else F.NativeCaller(0, 2, 2)
        try:
            data, fai = write_region_fasta(str(tmp_path / ("c%d_crlf.fa" % ci)), {"20": ref}, 7, b"\r\n")
            crlf = nc.open_fasta(data, fai)
            arr, _ = crlf.contig(0)
            assert len(ref) > 7 and arr.tobytes() != ref.upper()
            crlf.close()
            data, fai = write_region_fasta(str(tmp_path / ("c%d.fa" % ci)), {"20": ref}, 60)
            fa = nc.open_fasta(np.frombuffer(data, dtype=np.uint8), fai)
            fa.load()
            arr, dev = fa.contig(fa.tid("20"))
            assert arr.tobytes() == ref.upper() and (dev is not None) == (lib is None)
            opts = default_options(**case["options"])
            regions = [F.FastaContigRegion(F.RegionReads.from_buffers(c, s, e, fasta, b), fa, fa.tid(c)) for c, s, e, b in work]
            txt = nc.call_regions(regions, names, opts)
            assert nc.stats["n_windows_failed"] == 0
            fa.close()
        finally:
            nc.close()
        got += txt.split("\n")[:-1]
        want += case["lines"]
    return got, want
