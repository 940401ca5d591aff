"""Helper of the tabix tests (not a test module): a plain-Python mirror of the rule plat_tabix_fetch_batch states (include/platypus_mi355x.h;
the reference: ti_iter_read, ti_readline, ti_get_intv's VCF preset, src/tabix/index.c.pysam.c), the goldens of tests/golden/
tabix_cases.json.gz (what the reference's own ti_queryi / ti_read returned), hand-made edge streams its indexer would not produce, and the
arrays of a batch of streams as the device entry points take them.

A stream here is (name bytes, beg, end, chunks); a chunk is (block bytes, first_uoffset, end_coffset, end_uoffset), as plat_bgzf_chunk."""
import base64
import gzip
import json
import os
import re
import struct
import zlib

import numpy as np

from platypus_amd import synth, tabixindex

KEEP, SKIP, STOP, REFUSE = 0, 1, 2, 3
INT_LIMIT = 2 ** 31 - 1
PLAT_ERR_BAD_INPUT, PLAT_ERR_OVERFLOW = -9, -8
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tabix_cases.json.gz")


# ---- the rule ------------------------------------------------------------------------------------------------------------------------
def strtol0(s):
    """strtol(s, NULL, 0) of the C string s (bytes without a NUL): (value, outside +-(2^31 - 1))."""
    i, n = 0, len(s)
    while i < n and s[i] in b" \t\n\v\f\r":
        i += 1
    neg = False
    if i < n and s[i] in b"+-":
        neg = s[i] == 0x2d
        i += 1
    base = 10
    if i < n and s[i] == 0x30:
        if i + 2 < n and s[i + 1] in b"xX" and s[i + 2] in b"0123456789abcdefABCDEF":
            base, i = 16, i + 2
        else:
            base = 8
    digits = b"0123456789abcdefABCDEF"[:base if base <= 10 else 22]
    j = i
    while j < n and s[j] in digits:
        j += 1
    v = int(s[i:j], base) if j > i else 0
    return (-v if neg else v), v > INT_LIMIT


def c_string(s, at):
    """The C string that starts at s[at]: up to the first NUL."""
    e = s.find(b"\x00", at)
    return s[at:e if e >= 0 else len(s)]


def line_verdict(line, name, beg, end):
    """KEEP / SKIP / STOP / REFUSE for one line (without its newline) of the fetch of `name` over [beg, end)."""
    if line[:1] == b"#":
        return SKIP
    cols = re.split(b"[\t\x00]", line)
    if len(cols) < 2:
        return STOP
    v, wide = strtol0(c_string(line, len(cols[0]) + 1))       # (the reference's strtol runs on from column 2's start: a tab is white space)
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
            e, w = strtol0(info[at:])
            wide = wide or w
    if wide or e > INT_LIMIT:
        return REFUSE
    if e < 0 or cols[0] != name or b >= end:
        return STOP
    return KEEP if e > beg and end > b else SKIP


def walk_stream(chunks, name, beg, end):
    """chunks: [(the chunk's inflated bytes, first offset, stop offset or -1)].  {"lines": kept lines each with its '\\n' (None: refused),
    "walked": lines ahead of the stop or refusal}."""
    kept, walked = [], 0
    for q, (data, p, stop) in enumerate(chunks):
        hi = len(data)
        stop = hi if stop < 0 else min(stop, hi)
        while p < stop and p < hi:
            e = data.find(b"\n", p)
            e = hi if e < 0 else e
            v = line_verdict(data[p:e], name, beg, end)
            if v == REFUSE:
                return {"lines": None, "walked": walked}
            if v == STOP:
                return {"lines": kept, "walked": walked}
            walked += 1
            if v == KEEP:
                kept.append(data[p:e] + b"\n")
            p = e + 1 if e < hi else e
        if q + 1 < len(chunks) and p > stop:
            return {"lines": None, "walked": walked}
    return {"lines": kept, "walked": walked}


# ---- blocks --------------------------------------------------------------------------------------------------------------------------
def blocks_of(data):
    """[(offset, length, ISIZE)] of the BGZF blocks that chain through data."""
    data = bytes(data)
    out, at = [], 0
    while at < len(data):
        n = tabixindex.block_length(data, at)
        out.append((at, n, struct.unpack_from("<I", data, at + n - 4)[0]))
        at += n
    return out


def inflate_chunk(chunk):
    """(inflated bytes, first, stop) of a chunk (block bytes, first_uoffset, end_coffset, end_uoffset), for walk_stream."""
    data, first_u, end_c, end_u = chunk
    data = bytes(data)
    out, stop = b"", -1
    for at, n, isize in blocks_of(data):
        if at == end_c:
            stop = len(out) + end_u
        xlen, = struct.unpack_from("<H", data, at + 10)
        out += zlib.decompress(data[at + 12 + xlen:at + n - 8], -15)
    if end_c == len(data) and end_u == 0:
        stop = -1
    assert end_c < 0 or stop >= 0 or (end_c == len(data) and end_u == 0), "end_coffset is no block boundary"
    return out, first_u, stop


def mirror(streams):
    """What plat_tabix_fetch_batch leaves for these streams: {"text", "off" [n + 1], "counts" [2 n], "status" [4]} (no capacity limit)."""
    text, off, counts, refused, kept = b"", [0], [], -1, 0
    for s, (name, beg, end, chunks) in enumerate(streams):
        r = walk_stream([inflate_chunk(c) for c in chunks], name, beg, end)
        if r["lines"] is None:
            refused = s if refused < 0 else refused
            counts += [r["walked"], 0]
        else:
            text += b"".join(r["lines"])
            counts += [r["walked"], len(r["lines"])]
            kept += len(r["lines"])
        off.append(len(text))
    return {"text": text, "off": off, "counts": counts, "status": [PLAT_ERR_BAD_INPUT if refused >= 0 else 0, refused, kept, len(text)]}


def batch_arrays(streams):
    """The streams' blocks in one blob and their geometry: a dict of numpy arrays named as plat_bgzf_inflate_batch and plat_tabix_fetch_in
    name them (blob, blk_off, blk_limit, stream_chunk_begin, chunk_*, names, name_off, beg, end) and "inflated" (the ISIZEs' sum)."""
    blob, blk_off, blk_limit, inflated = b"", [], [], 0
    scb, cf, ce, cfu, csb, csu, names, name_off, beg, end = [0], [], [], [], [], [], b"", [0], [], []
    for name, b, e, chunks in streams:
        for data, first_u, end_c, end_u in chunks:
            data = bytes(data)
            cf.append(len(blk_off))
            stop_blk = -1
            for at, n, isize in blocks_of(data):
                if at == end_c and not (end_c == len(data) and end_u == 0):
                    stop_blk = len(blk_off)
                blk_off.append(len(blob) + at)
                blk_limit.append(len(blob) + len(data))
                inflated += isize
            ce.append(len(blk_off))
            cfu.append(first_u)
            csb.append(stop_blk)
            csu.append(end_u if stop_blk >= 0 else 0)
            blob += data
        scb.append(len(cf))
        names += name
        name_off.append(len(names))
        beg.append(b)
        end.append(e)
    i32, i64 = (lambda v: np.array(v, dtype=np.int32)), (lambda v: np.array(v, dtype=np.int64))
    return {"blob": np.frombuffer(blob, dtype=np.uint8), "blk_off": i64(blk_off), "blk_limit": i64(blk_limit), "inflated": inflated,
            "stream_chunk_begin": i32(scb), "chunk_blk_first": i32(cf), "chunk_blk_end": i32(ce), "chunk_first_uoffset": i32(cfu),
            "chunk_stop_blk": i32(csb), "chunk_stop_uoffset": i32(csu), "names": np.frombuffer(names, dtype=np.uint8), "name_off": i32(name_off),
            "beg": i32(beg), "end": i32(end)}


# ---- streams made by hand --------------------------------------------------------------------------------------------------------------
def cut(text, payload, spans, extra_blocks=0):
    """`text` bgzipped in blocks of `payload` bytes, and the chunks whose inflated bytes are text[a:e] for (a, e) in spans (e None: to
    the end of the chunk's data), cut as an index lookup cuts them; extra_blocks: further blocks of the file behind the chunk's end."""
    data, off = synth.bgzf_stream(text, payload)
    off = [int(x) for x in off] + [len(data)]
    chunks = []
    for a, e in spans:
        b0 = a // payload
        if e is None:
            chunks.append((np.frombuffer(data, dtype=np.uint8)[off[b0]:], a % payload, -1, 0))
            continue
        b1, u1 = e // payload, e % payload                     # (an end at a block's end IS offset 0 of the next block)
        last = min(b1 + (1 if u1 else 0) + extra_blocks, len(off) - 1)
        chunks.append((np.frombuffer(data, dtype=np.uint8)[off[b0]:off[last]], a % payload, off[b1] - off[b0], u1))
    return chunks


def _lines(*lines):
    return b"".join(x + b"\n" for x in lines)


def edge_streams(payload):
    """[(label, stream)] -- each a stream the indexer would not produce, or one that meets a corner of the walk -- at one block payload."""
    L = lambda chrom, pos, ref=b"A", alt=b"C", info=b".", tail=b"\tGT\t0/1": b"\t".join([chrom, pos, b".", ref, alt, b"50", b"PASS", info]) + tail
    out = []
    body = _lines(L(b"20", b"100"), L(b"20", b"150"), L(b"21", b"10"), L(b"20", b"160"), L(b"20", b"170"))
    n3 = len(_lines(L(b"20", b"100"), L(b"20", b"150"), L(b"21", b"10")))
    out.append(("stop with kept-looking lines and a whole chunk behind it", (b"20", 0, 1000, cut(body, payload, [(0, n3), (n3, None)]))))
    two = _lines(L(b"20", b"100"), L(b"20", b"150"), L(b"20", b"160"))
    n1 = len(_lines(L(b"20", b"100")))
    out.append(("overshoot past a non-last chunk's end", (b"20", 0, 1000, cut(two, payload, [(0, n1 + 5), (len(two) - n1, None)], extra_blocks=4))))
    out.append(("overshoot past the last chunk's end", (b"20", 0, 1000, cut(two, payload, [(0, n1), (n1, n1 + 5)], extra_blocks=4))))
    out.append(("an empty line", (b"20", 0, 1000, cut(_lines(L(b"20", b"100"), b"", L(b"20", b"150")), payload, [(0, None)]))))
    out.append(("a one-column line", (b"20", 0, 1000, cut(_lines(L(b"20", b"100"), b"20", L(b"20", b"150")), payload, [(0, None)]))))
    out.append(("END=-5", (b"20", 0, 1000, cut(_lines(L(b"20", b"100"), L(b"20", b"120", info=b"END=-5"), L(b"20", b"150")), payload, [(0, None)]))))
    out.append(("a POS beyond int32", (b"20", 0, 1000, cut(_lines(L(b"20", b"100"), L(b"20", b"2147483648"), L(b"20", b"150")), payload, [(0, None)]))))
    out.append(("an END beyond int32", (b"20", 0, 1000, cut(_lines(L(b"20", b"100", info=b"DP=1;END=99999999999"), L(b"20", b"150")), payload, [(0, None)]))))
    out.append(("a NUL inside a line", (b"20", 0, 1000, cut(_lines(L(b"20", b"100"), b"20\x00150\t.\tA\x00C\t.\t.\tEND=7", L(b"20\x00", b"150"), L(b"20", b"160")),
                                                       payload, [(0, None)]))))
    many = _lines(*[L(b"20", b"%d" % (100 + 10 * i), ref=b"A" * (1 + i % 5)) for i in range(12)])
    ends = [m.end() for m in re.finditer(b"\n", many)]
    out.append(("adjacent and non-adjacent chunks", (b"20", 125, 190, cut(many, payload, [(0, ends[2]), (ends[2], ends[4]), (ends[6], ends[9]), (ends[10], None)]))))
    out.append(("first_uoffset in mid-block, the window's end stops the stream", (b"20", 0, 175, cut(many, payload, [(ends[1], ends[5]), (ends[5], None)]))))
    # a stop exactly on a block boundary: the first line padded so that the second one starts a block
    first = L(b"20", b"100", info=b"X=" + b"y" * ((-len(L(b"20", b"100", info=b"X=")) - 1) % payload))
    edge = _lines(first, L(b"22", b"1"), L(b"20", b"150"))
    assert (len(first) + 1) % payload == 0
    out.append(("a stop exactly on a block boundary", (b"20", 0, 1000, cut(edge, payload, [(0, len(first) + 1), (len(first) + 1, None)]))))
    out.append(("a chunk that ends on a block boundary and goes on", (b"20", 0, 1000, cut(_lines(first, L(b"20", b"150"), L(b"20", b"160")), payload,
                                                                                        [(0, len(first) + 1), (len(first) + 1, None)]))))
    out.append(("white space, signs and bases in POS and END", (b"20", 0, 1000, cut(_lines(
        L(b"20", b" +12"), L(b"20", b"\t14"), L(b"20", b"0x1G"), L(b"20", b"0x"), L(b"20", b"019"), L(b"20", b"-7"), L(b"20", b"", ref=b""),
        L(b"20", b"30", info=b"SVEND=7"), L(b"20", b"31", info=b"CIEND=1;END=7"), L(b"20", b"32", info=b"END= 0x30;END=2"), L(b"20", b"33", info=b"AEND=1;END=+;END=9"),
        L(b"20", b"40\r", alt=b"C\r"), b"20\t50", b"20\t60\t.\tACGT"), payload, [(0, None)]))))
    out.append(("a last line without its newline, and no chunks", (b"20", 0, 1000, cut(_lines(L(b"20", b"100"))[:-1], payload, [(0, None)]))))
    out.append(("a stream without chunks", (b"20", 0, 1000, [])))
    return out


# ---- goldens ---------------------------------------------------------------------------------------------------------------------------
_golden = None


def golden_files():
    """[{"label", "payload", "vcf_gz" bytes, "tbi" bytes, "names" [bytes], "queries": [{"tid", "beg", "end", "lines": [bytes]}]}]"""
    global _golden
    if _golden is None:
        with gzip.open(GOLDEN, "rt") as f:
            raw = json.load(f)
        _golden = [dict(f, vcf_gz=base64.b64decode(f["vcf_gz"]), tbi=base64.b64decode(f["tbi"]), names=[n.encode("latin-1") for n in f["names"]],
                        queries=[dict(q, lines=[x.encode("latin-1") for x in q["lines"]]) for q in f["queries"]]) for f in raw["files"]]
    return _golden


def golden_cli():
    """{"vcf": the text, "vcf_gz", "tbi": bytes}: a source VCF for `--synthetic=config4:2 --bufferSize 4000` and the index the reference wrote."""
    with gzip.open(GOLDEN, "rt") as f:
        cli = json.load(f)["cli"]
    return {"vcf": cli["vcf"].encode(), "vcf_gz": base64.b64decode(cli["vcf_gz"]), "tbi": base64.b64decode(cli["tbi"])}


def golden_streams():
    """[(label, stream, the reference's lines)] for every golden query, the stream's chunks chosen by tabixindex from the committed .tbi."""
    out = []
    for f in golden_files():
        tf = tabixindex.TabixFile(f["vcf_gz"], f["tbi"])
        assert tf.index.names == f["names"]
        for q in f["queries"]:
            chunks = tf.index.query(q["tid"], q["beg"], q["end"])
            stream = (f["names"][q["tid"]], max(q["beg"], 0), q["end"], tabixindex.cut_chunks(tf.data, chunks or []))
            out.append(("%s %d:%d-%d" % (f["label"], q["tid"], q["beg"], q["end"]), stream, q["lines"]))
    return out
