"""Generate tests/golden/fasta_cases.json.gz: what the reference's FastaIndex.getRefs, FastaFile.getSequence and FastaFile.getCharacter
(src/cython/fastafile.pyx:64-82, 173-207, 120-139) return or raise over the small files tests/fasta_cases.py makes (fixture_files,
BAD_INDEXES).

The reference's module cannot be compiled for Python 3 with build-level adaptations alone (README_fasta.md says what was tried and where it
stops), so the expectations come from THIS file's restatement of those statements over real Python file objects opened 'rb' -- iterate
the index's lines, strip, split, libc's atoll; seek, read, replace(b"\\n", b""), upper() -- which is a weaker pin than the reference's own
code and is named as such.  Nothing is compiled from the reference and none of its text is kept.

Usage:  python tests/golden/gen_golden_fasta.py [--scratch DIR]"""
import argparse
import ctypes
import gzip
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import fasta_cases as FC  # noqa: E402

libc = ctypes.CDLL(None)
libc.atoll.restype = ctypes.c_longlong
libc.atoll.argtypes = [ctypes.c_char_p]


def get_refs(index_path, parse_ncbi):
    """getRefs: the dict of name -> [field 0, SeqLength, StartPos, LineLength, FullLineLength]; raises what the statements raise."""
    d = {}
    with open(index_path, "rb") as f:
        for the_line in f:
            line = the_line.strip().split(b"\t")
            name = line[0].split()[0]
            if name.startswith(b"gi|") and parse_ncbi:
                ids = name.split(b"|")
                if len(ids) >= 4 and ids[2] == b"ref":
                    name = ids[3]
            d[name] = [line[0], libc.atoll(line[1]), libc.atoll(line[2]), libc.atoll(line[3]), libc.atoll(line[4])]
    return d


def offset(t, pos):
    return t[2] + pos + (t[4] - t[3]) * int(float(pos) / t[3])            # (division by a zero LineLength raises, as the module's does without cdivision)


def get_sequence(f, refs, name, beg, end):
    t = refs[name]
    beg, end = max(0, beg), min(t[1] - 1, end)
    lo, hi = offset(t, beg), offset(t, end)
    if end < beg:
        raise IndexError("Cannot have beginPos = %s, endPos = %s" % (beg, end))
    f.seek(lo)
    return f.read(hi - lo).replace(b"\n", b"").upper()


def get_character(f, refs, name, pos):
    t = refs[name]
    if pos >= t[1] or pos < 0:
        return b"-"
    f.seek(offset(t, pos))
    return f.read(1).upper()                                              # (nothing where the file ends in front of the offset)


def outcome(fn, *a):
    try:
        return dict(seq=fn(*a).decode("latin-1"))
    except (IndexError, ZeroDivisionError) as e:
        return dict(raises=type(e).__name__)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scratch", default=None)
    a = ap.parse_args()
    scratch = a.scratch or tempfile.mkdtemp(prefix="fasta_golden_")
    os.makedirs(scratch, exist_ok=True)
    s = lambda b: b.decode("latin-1")
    files = []
    for k, fx in enumerate(FC.fixture_files()):
        fa, fai = os.path.join(scratch, "f%d.fa" % k), os.path.join(scratch, "f%d.fa.fai" % k)
        with open(fa, "wb") as f:
            f.write(fx["fasta"])
        with open(fai, "wb") as f:
            f.write(fx["fai"])
        refs0, refs1 = get_refs(fai, 0), get_refs(fai, 1)
        out = dict(label=fx["label"], fasta=s(fx["fasta"]), fai=s(fx["fai"]),
                   refs0={s(n): [s(v[0])] + v[1:] for n, v in refs0.items()}, refs1={s(n): [s(v[0])] + v[1:] for n, v in refs1.items()}, queries=[], chars=[])
        with open(fa, "rb") as f:
            for name, beg, end in fx["queries"]:
                out["queries"].append(dict(name=s(name), beg=beg, end=end, **outcome(get_sequence, f, refs1, name, beg, end)))
            for name, pos in fx["chars"]:
                r = outcome(get_character, f, refs1, name, pos)
                out["chars"].append(dict(name=s(name), pos=pos, **({"char": r["seq"]} if "seq" in r else r)))
        files.append(out)
    bad = []
    for k, (label, fai_text, names) in enumerate(FC.BAD_INDEXES):
        path = os.path.join(scratch, "bad%d.fai" % k)
        with open(path, "wb") as f:
            f.write(fai_text)
        try:
            get_refs(path, 1)
            raise SystemExit("the statements accept index %r" % label)
        except IndexError as e:
            bad.append(dict(label=label, fai=s(fai_text), raises=type(e).__name__, names=names))
    with gzip.GzipFile(FC.GOLDEN, "wb", mtime=0) as f:
        f.write(json.dumps(dict(files=files, bad_indexes=bad), sort_keys=True).encode())
    print("wrote %s: %d files, %d queries, %d characters, %d refused indexes, %d bytes" % (
        FC.GOLDEN, len(files), sum(len(f["queries"]) for f in files), sum(len(f["chars"]) for f in files), len(bad), os.path.getsize(FC.GOLDEN)))


if __name__ == "__main__":
    main()
