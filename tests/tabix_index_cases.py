"""Helper of the tabix index tests (not a test module): a plain-Python mirror of the rule plat_tabix_index_batch states
(include/platypus_mi355x.h; the reference: ti_index_core with ti_conf_vcf, src/tabix/index.c.pysam.c:320-393) with its finishing stage
(csrc/tabix_index.hpp: runs grouped by contig and bin, merge_chunks, fill_missing, the first-record quirk, the serialisation), the goldens
(the four bgzipped VCFs of tests/golden/tabix_cases.json.gz with the .tbi the reference wrote for each, and tests/golden/
tabix_index_cases.json.gz where it exists), files made by hand for the corners of the rule, and seeded random sorted VCFs sized to where
the device kernels can go wrong."""
import base64
import bisect
import functools
import gzip
import json
import os
import random
import re
import struct
import zlib

from platypus_amd import synth
from tests import tabix_cases as T

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tabix_index_cases.json.gz")
ST_VERDICT, ST_LINE, ST_KIND, ST_RECORDS, ST_RUNS, ST_CONTIGS, ST_WINDOWS, ST_END, ST_FIRST0, ST_FIRST_BEG, ST_FIRST_END, ST_LINES, ST_NAME_BYTES, ST_WORDS = range(14)
KIND_COLUMNS, KIND_WIDE, KIND_NEGATIVE_END, KIND_ORDER, KIND_NAME_AGAIN = 1, 2, 3, 4, 5
ERR_BAD_INPUT, ERR_OVERFLOW = -9, -8
INT_LIMIT = 2 ** 31 - 1


# ---- the rule ------------------------------------------------------------------------------------------------------------------------
def parse_record(line):
    """(name, beg, end, kind) of a record line without its newline; kind 0 or why the indexer refuses it."""
    cols = re.split(b"[\t\x00]", line)
    if len(cols) < 2:
        return cols[0], 0, 0, KIND_COLUMNS
    v, wide = T.strtol0(T.c_string(line, len(cols[0]) + 1))
    if wide:
        v = (INT_LIMIT + 1) * (1 if v > 0 else -1)
    b, e = max(v - 1, 0), max(v, 1)
    if len(cols) >= 4 and cols[3]:
        e = b + len(cols[3])
    if len(cols) >= 8:
        info = cols[7]
        at = info.find(b"END=")
        if at == 0:
            at = 4
        elif at > 0:
            at = info.find(b";END=")
            at = at + 5 if at >= 0 else -1
        if at >= 0:
            e, w = T.strtol0(info[at:])
            wide = wide or w
    if wide or e > INT_LIMIT:
        return cols[0], 0, 0, KIND_WIDE
    return cols[0], b, e, (KIND_NEGATIVE_END if e < 0 else 0)


def reg2bin(beg, end):
    """ti_reg2bin in unsigned 32-bit arithmetic."""
    beg, end = beg & 0xffffffff, (end - 1) & 0xffffffff
    for first, shift in ((4681, 14), (585, 17), (73, 20), (9, 23), (1, 26)):
        if beg >> shift == end >> shift:
            return first + (beg >> shift)
    return 0


def inflate_file(data):
    """A bgzipped file as plat_bgzf_inflate_batch leaves it, for the index call: (inflated bytes, out_off [n + 1], blk_addr [n + 1]) over
    the blocks up to the last that holds data; the last address is the one behind that block."""
    data = bytes(data)
    blocks = T.blocks_of(data)
    n = len(blocks)
    while n and blocks[n - 1][2] == 0:
        n -= 1
    out, out_off, addr = b"", [0], []
    for at, ln, isize in blocks[:n]:
        xlen, = struct.unpack_from("<H", data, at + 10)
        out += zlib.decompress(data[at + 12 + xlen:at + ln - 8], -15)
        out_off.append(len(out))
        addr.append(at)
    addr.append(blocks[n][0] if n < len(blocks) else len(data))
    return out, out_off, addr


def build(data, out_off, blk_addr):
    """The intermediate the device call and the host twin leave: {"runs": [(tid, bin, u)], "names": [(off, len)], "lin_first", "lin",
    "status" [13]}.  A refused file: the status alone."""
    st = [0] * ST_WORDS
    st[ST_LINE] = -1
    total, n_blocks = out_off[-1], len(out_off) - 1

    def refuse(line, kind):
        return {"runs": [], "names": [], "lin_first": [0], "lin": [], "status": [ERR_BAD_INPUT, line, kind] + [0] * (ST_WORDS - 3)}

    def voffset(t):
        b = min(bisect.bisect_right(out_off, t) - 1, n_blocks - 1)      # the last block with out_off[b] <= t
        return blk_addr[b] << 16 | (t - out_off[b])

    runs, names, lin, seen = [], [], [], {}
    p, lines, records, prev = 0, 0, 0, None
    while p < total:
        e = data.find(b"\n", p)
        e = total if e < 0 else e
        s, p = p, (e + 1 if e < total else e)
        lines += 1
        if data[s:s + 1] == b"#":
            continue
        name, beg, end, kind = parse_record(data[s:e])
        if kind:
            return refuse(lines, kind)
        change = prev is None or prev[0] != name
        if change:
            if name in seen:
                return refuse(lines, KIND_NAME_AGAIN)
            seen[name] = len(names)
            names.append((s, len(name)))
            lin.append([])
        elif prev[1] > beg:
            return refuse(lines, KIND_ORDER)
        tid, u, b = len(names) - 1, voffset(s), reg2bin(beg, end)
        if change or b != prev[2]:
            runs.append((tid, b, u))
        w0, w1 = beg >> 14, (end - 1) >> 14
        L = lin[tid]
        if w1 + 1 > len(L):
            L.extend([0] * (w1 + 1 - len(L)))
        for w in range(w0, w1 + 1):
            if L[w] == 0:
                L[w] = u
        if records == 0 and u == 0:
            st[ST_FIRST0], st[ST_FIRST_BEG], st[ST_FIRST_END] = 1, w0, w1
        records += 1
        prev = (name, beg, b)
    lin_first = [0]
    for L in lin:
        lin_first.append(lin_first[-1] + len(L))
    st[ST_NAME_BYTES] = sum(n for _, n in names)
    st[ST_RECORDS], st[ST_RUNS], st[ST_CONTIGS], st[ST_WINDOWS], st[ST_END], st[ST_LINES] = records, len(runs), len(names), lin_first[-1], blk_addr[-1] << 16, lines
    return {"runs": runs, "names": names, "lin_first": lin_first, "lin": [x for L in lin for x in L], "status": st}


def finish(inter, data):
    """The finishing stage: the intermediate of an accepted file to the index's bytes before BGZF (bins ascending)."""
    st, runs = inter["status"], inter["runs"]
    names = [bytes(data[o:o + n]) for o, n in inter["names"]]
    out = b"TBI\x01" + struct.pack("<8i", len(names), 2, 1, 2, 0, ord("#"), 0, sum(len(n) + 1 for n in names)) + b"".join(n + b"\x00" for n in names)
    for tid in range(len(names)):
        bins = {}
        for k, (t, b, u) in enumerate(runs):
            if t != tid:
                continue
            v = runs[k + 1][2] if k + 1 < len(runs) else st[ST_END]
            chunks = bins.setdefault(b, [])
            if chunks and chunks[-1][1] >> 16 == u >> 16:               # merge_chunks
                chunks[-1][1] = v
            else:
                chunks.append([u, v])
        out += struct.pack("<i", len(bins))
        for b in sorted(bins):
            out += struct.pack("<Ii", b, len(bins[b])) + b"".join(struct.pack("<QQ", u, v) for u, v in bins[b])
        L = list(inter["lin"][inter["lin_first"][tid]:inter["lin_first"][tid + 1]])
        for j in range(1, len(L)):                                     # fill_missing
            if L[j] == 0:
                L[j] = L[j - 1]
        if tid == 0 and st[ST_FIRST0]:                                 # the first record at offset 0
            for j in range(max(st[ST_FIRST_BEG], 0), min(st[ST_FIRST_END] + 1, len(L))):
                L[j] = 0
        out += struct.pack("<i", len(L)) + struct.pack("<%dQ" % len(L), *L)
    return out


def index_of(vcf_gz):
    """(status, the index's bytes before BGZF or None where the file is refused) by the mirror."""
    data, out_off, addr = inflate_file(vcf_gz)
    inter = build(data, out_off, addr)
    return inter["status"], (finish(inter, data) if inter["status"][ST_VERDICT] == 0 else None)


def parsed(index):
    """What a test compares of a tabixindex.TabixIndex: names, bins with their chunk lists, linear indexes."""
    return index.names, [{b: list(c) for b, c in sorted(bins.items())} for bins in index.bins], [list(l) for l in index.linear]


# ---- files made by hand -----------------------------------------------------------------------------------------------------------------
def L(chrom, pos, ref=b"A", alt=b"C", info=b".", tail=b"\tGT\t0/1"):
    return b"\t".join([chrom, b"%d" % pos if isinstance(pos, int) else pos, b".", ref, alt, b"50", b"PASS", info]) + tail


def _lines(*lines):
    return b"".join(x + b"\n" for x in lines)


HEADER = _lines(b"##fileformat=VCFv4.1", b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS1")


def hand_texts():
    """[(label, text, the line the file is refused at or None, its kind)]: the corners the issue lists, as plain text."""
    out = []
    out.append(("no header, first record at offset 0", _lines(L(b"20", 100), L(b"20", 200), L(b"20", 2 * 16384 + 5)), None, 0))
    out.append(("END=0", HEADER + _lines(L(b"20", 100), L(b"20", 120, info=b"END=0"), L(b"20", 150)), None, 0))
    out.append(("END below POS", HEADER + _lines(L(b"20", 40000), L(b"20", 50000, info=b"DP=3;END=20000"), L(b"20", 50010)), None, 0))
    out.append(("END over windows and bin levels", HEADER + _lines(L(b"20", 100), L(b"20", 16000, info=b"END=5000000"), L(b"20", 16001), L(b"20", 9000000)), None, 0))
    out.append(("a bin in two runs", HEADER + _lines(L(b"20", 100), L(b"20", 110), L(b"20", 120, info=b"END=40000"), L(b"20", 130), L(b"20", 140)), None, 0))
    out.append(("a contig change where the bin repeats", HEADER + _lines(L(b"20", 100), L(b"20", 110), L(b"21", 100), L(b"21", 120), L(b"2", 100), L(b"200", 100)), None, 0))
    out.append(("meta lines between records, CR, no last newline", HEADER + _lines(L(b"20", 100), b"#x", L(b"20", 110), b"##y", L(b"21\r", 5), L(b"21\r", b"7\r"))[:-1], None, 0))
    out.append(("only a header", HEADER, None, 0))
    out.append(("an empty file", b"", None, 0))
    out.append(("one record with 2000 windows", HEADER + _lines(L(b"1", 5), L(b"1", 70000, info=b"END=%d" % (70000 + 2000 * 16384)), L(b"1", 70001), L(b"2", 9)), None, 0))
    out.append(("refused: an empty line", HEADER + _lines(L(b"20", 100), b"", L(b"20", 150)), 4, KIND_COLUMNS))
    out.append(("refused: a one-column line", HEADER + _lines(L(b"20", 100), L(b"20", 150), b"20"), 5, KIND_COLUMNS))
    out.append(("refused: END=-5", HEADER + _lines(L(b"20", 100), L(b"20", 120, info=b"END=-5")), 4, KIND_NEGATIVE_END))
    out.append(("refused: out of order", HEADER + _lines(L(b"20", 100), L(b"20", 150), L(b"20", 149), L(b"20", 10)), 5, KIND_ORDER))
    out.append(("refused: a contig again", HEADER + _lines(L(b"20", 100), L(b"21", 150), b"#z", L(b"20", 200), L(b"21", 1)), 6, KIND_NAME_AGAIN))
    out.append(("refused: a POS beyond int32", _lines(L(b"20", 100), L(b"20", b"2147483648")), 2, KIND_WIDE))
    out.append(("refused: two kinds, the lowest line", HEADER + _lines(L(b"20", 100), L(b"21", 5), L(b"21", 4), L(b"20", 7), b""), 5, KIND_ORDER))
    return out


@functools.lru_cache(maxsize=None)
def hand_files(payloads=(37, 100, 65280)):
    """[(label, vcf_gz bytes, refused line or None, kind)]: every hand text bgzipped at each payload."""
    return [("%s @%d" % (label, p), synth.bgzf_stream(text, p)[0], line, kind) for label, text, line, kind in hand_texts() for p in payloads]


# ---- seeded random sorted VCFs --------------------------------------------------------------------------------------------------------
def random_text(seed, n_lines=400, long_line=0, header=True):
    """A sorted VCF text: contigs whose names are prefixes of each other, short and long lines, '#' lines between records, positions that
    repeat, cross windows and bin levels; long_line: the INFO bytes of one record longer than a tile or a block."""
    rng = random.Random(seed)
    contigs = [b"1", b"10", b"100", b"1_alt", b"2", b"20", b"X"][:rng.randint(2, 7)]
    out = [HEADER] if header else []
    per = max(1, n_lines // len(contigs))
    for ci, chrom in enumerate(contigs):
        pos = rng.randint(1, 40000)
        for k in range(per):
            r = rng.random()
            pos += 0 if r < 0.1 else rng.randint(1, 30) if r < 0.8 else rng.randint(2000, 40000)
            kind = rng.random()
            info = b"DP=%d" % rng.randint(1, 99)
            ref = b"ACGT"[rng.randint(0, 3):][:1] * rng.randint(1, 1 if kind < 0.8 else 40)
            if kind > 0.95:
                info = b"SVTYPE=DEL;END=%d" % (pos + rng.randint(0, 300000))
            if long_line and ci == 0 and k == per // 2:
                info += b";X=" + b"z" * long_line
            if kind < 0.5:
                out.append(b"%s\t%d\t.\t%s\n" % (chrom, pos, ref))                   # ten-odd bytes a line
            else:
                out.append(L(chrom, pos, ref=ref, info=info) + b"\n")
            if rng.random() < 0.05:
                out.append(b"#" + b"c" * rng.randint(0, 60) + b"\n")
    return b"".join(out)


@functools.lru_cache(maxsize=None)
def random_files():
    """[(label, vcf_gz bytes)]: the shapes the issue lists for the GPU test, bgzipped at payloads 37, 100, 1024 and 65280."""
    out = []
    for seed, (payload, n_lines, long_line) in enumerate([(37, 300, 0), (100, 600, 1500), (1024, 3000, 70000), (65280, 3000, 70000), (1024, 40000, 0), (65280, 60000, 0)]):
        out.append(("seed %d payload %d lines %d" % (seed, payload, n_lines), synth.bgzf_stream(random_text(seed, n_lines, long_line, header=seed != 0), payload, level=1)[0]))
    # about a hundred ten-byte lines in one tile; a line start on a tile's and a block's first byte; a run, a contig change and a '#'
    # line each across a tile edge
    short = b"".join(b"7\t%d\tA\n" % (100000 + 200 * k) for k in range(300))      # (eleven bytes a line: some ninety to a tile)
    out.append(("ten-byte lines", synth.bgzf_stream(short, 1024, level=1)[0]))
    pad = lambda text, to: text + b"#" + b"p" * (to - len(text) - 2) + b"\n"
    edge = pad(HEADER, 1024) + L(b"1", 5) + b"\n"
    edge = pad(edge, 2048 - 3) + b"#ab\n" + L(b"1", 6) + b"\n"                          # (a '#' line across the tile edge)
    edge += L(b"1", 7, info=b"X=" + b"q" * (3072 - len(edge) - len(L(b"1", 7, info=b"X=")) - 1)) + b"\n" + L(b"2", 7) + b"\n"   # (a contig change on a tile's first byte)
    assert edge.find(L(b"2", 7)) == 3072
    out.append(("tile edges", synth.bgzf_stream(edge, 1024, level=1)[0]))
    out.append(("tile edges, odd blocks", synth.bgzf_stream(edge, 100, level=1)[0]))
    return out


# ---- goldens ---------------------------------------------------------------------------------------------------------------------------
def committed_pairs():
    """[(label, vcf_gz, tbi)]: the four files of tabix_cases.json.gz (and its command-line file) with the reference's index of each."""
    out = [(f["label"], f["vcf_gz"], f["tbi"]) for f in T.golden_files()]
    cli = T.golden_cli()
    out.append(("cli", cli["vcf_gz"], cli["tbi"]))
    return out


def golden_cases():
    """[{"label", "vcf_gz", "tbi" or None, "refused": bool}] of tests/golden/tabix_index_cases.json.gz; [] where it is not there."""
    if not os.path.exists(GOLDEN):
        return []
    with gzip.open(GOLDEN, "rt") as f:
        raw = json.load(f)
    return [dict(c, vcf_gz=base64.b64decode(c["vcf_gz"]), tbi=base64.b64decode(c["tbi"]) if c.get("tbi") else None) for c in raw["cases"]]
