"""Cases shared by tests/test_bgzf_cpu.py (the host build of csrc/bgzf_inflate.hpp) and tests/test_gpu_bgzf.py (the device): the inflate
grid, the corrupt blocks -- each a valid block with bytes edited, or a deflate stream written bit by bit here inside a valid frame --, the
reference verdict on a block (Python's zlib behind a restatement of the header rules), the record walk's rule restated, the streams that
zlib's encoder never writes (foreign_blocks, foreign_fuzz: written by tests/deflate_writer.py) and the record walk's window-seam ladder
(walk_seam_cases).  Nothing here calls the code under test."""
import struct
import zlib

import numpy as np

from platypus_amd import hostapi as H, synth

LEVELS = (0, 1, 6, 9)
STRATEGIES = (zlib.Z_DEFAULT_STRATEGY, zlib.Z_FIXED, zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE)


def synthetic_record_bytes(n_bytes, seed=5):
    """Real synthetic records (config-4 reads as BAM records behind their block_size words), cut to n_bytes."""
    reg, samples = synth.config4_fetched_region(seed, region_len=4000)
    data, _ = synth.bam_records(samples[0], block_size=True)
    return data.tobytes()[:n_bytes]


def payloads():
    rng = np.random.default_rng(11)
    text = (b"the quick brown fox jumps over the lazy dog; " * 1500)
    return [("random", rng.integers(0, 256, size=30000, dtype=np.uint8).tobytes()), ("zeros", bytes(40000)), ("periodic text", text[:50001]),
            ("records", synthetic_record_bytes(60000)), ("empty", b""), ("one byte", b"\x5a"),
            ("65280 random", rng.integers(0, 256, size=65280, dtype=np.uint8).tobytes())]


def inflate_grid():
    """[(name, payload, block)] for payloads x levels x strategies."""
    out = []
    for name, p in payloads():
        for lv in LEVELS:
            for st in STRATEGIES:
                out.append(("%s level %d strategy %d" % (name, lv, st), p, synth.bgzf_block(p, lv, st)))
    return out


# ---- blocks written by hand ----------------------------------------------------------------------------------------------------------
class BitWriter:
    """Deflate's bit order: fields LSB first, Huffman codes MSB first."""

    def __init__(self):
        self.bits = []

    def field(self, value, n):
        self.bits += [(value >> k) & 1 for k in range(n)]
        return self

    def code(self, text):
        self.bits += [int(c) for c in text]
        return self

    def bytes(self):
        b = self.bits + [0] * (-len(self.bits) % 8)
        return bytes(sum(b[i + k] << k for k in range(8)) for i in range(0, len(b), 8))


def frame(cdata, payload=b"", extra=b"", crc=None, isize=None, bsize=None, magic=b"\x1f\x8b\x08", flg=4, bc=b"BC", slen=2):
    """A BGZF block around a deflate stream; every header and trailer field can be set wrong."""
    xlen = len(extra) + 6
    total = 12 + xlen + len(cdata) + 8
    return (magic + bytes([flg]) + b"\0\0\0\0\0\xff" + struct.pack("<H", xlen) + extra + bc + struct.pack("<HH", slen, (total - 1) if bsize is None else bsize) +
            cdata + struct.pack("<II", zlib.crc32(payload) if crc is None else crc, len(payload) if isize is None else isize))


def raw_deflate(payload, level=6, strategy=0):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    return c.compress(payload) + c.flush()


FIXED_A = "01110001"                                          # the literal 'A' (0x41) in the fixed code: 0x30 + 0x41, 8 bits


def corrupt_blocks():
    """{why: block} -- every refusal of plat_bgzf_inflate_batch's list that can be told from the block's own bytes."""
    text = b"GATTACA, said the sequencer, and GATTACA said the aligner: " * 40
    good = raw_deflate(text)
    assert len(good) > 40
    out = {}
    out["magic byte 0"] = frame(good, text, magic=b"\x1e\x8b\x08")
    out["magic byte 1"] = frame(good, text, magic=b"\x1f\x8a\x08")
    out["compression method 7"] = frame(good, text, magic=b"\x1f\x8b\x07")
    out["FLG without FEXTRA"] = frame(good, text, flg=0)
    out["FLG with FNAME"] = frame(good, text, flg=4 | 8)
    out["FLG with FHCRC"] = frame(good, text, flg=4 | 2)
    out["no BC subfield"] = frame(good, text, bc=b"BD")
    out["BC with SLEN 3"] = frame(good, text, slen=3)
    out["only another subfield"] = frame(good, text, extra=b"XY\x02\x00ab", bc=b"ZZ")
    out["BSIZE too small for header and trailer"] = frame(b"", b"", bsize=12 + 6 + 8 - 2)
    out["BSIZE past the block's bytes"] = frame(good, text, bsize=12 + 6 + len(good) + 8)
    out["ISIZE 65537"] = frame(good, text, isize=65537)
    out["block type 3"] = frame(BitWriter().field(1, 1).field(3, 2).bytes())
    out["stored LEN / NLEN mismatch"] = frame(b"\x01\x04\x00\xfa\xffACGT", b"ACGT")
    # dynamic headers: BFINAL 1, BTYPE 2, HLIT, HDIST, HCLEN, then the code-length code's lengths in the order 16 17 18 0 8 7 ...
    dyn = lambda hlit, hdist, hclen: BitWriter().field(1, 1).field(2, 2).field(hlit, 5).field(hdist, 5).field(hclen, 4)
    w = dyn(0, 0, 0)
    for v in (1, 1, 1, 0):
        w.field(v, 3)                                                     # three one-bit codes
    out["over-subscribed code-length set"] = frame(w.bytes() + bytes(8))
    w = dyn(0, 0, 0)
    for v in (1, 0, 0, 1):
        w.field(v, 3)                                                     # 16 -> "1", 0 -> "0"
    out["repeat code with nothing to repeat"] = frame(w.code("1").field(0, 2).bytes() + bytes(8))
    w = dyn(0, 0, 0)
    for v in (0, 0, 1, 1):
        w.field(v, 3)                                                     # 18 -> "1", 0 -> "0"; 258 lengths wanted, 2 x 138 given
    out["more code lengths than HLIT + HDIST"] = frame(w.code("1").field(127, 7).code("1").field(127, 7).bytes() + bytes(8))
    # a distance set without any code, then a length symbol: lit/len 256 -> "0", 257 -> "1"; the code-length code 0 -> "0", 1 -> "10", 18 -> "11"
    w = dyn(1, 0, 14)
    cl = [0] * 18
    cl[2], cl[3], cl[17] = 2, 1, 2
    for v in cl:
        w.field(v, 3)
    w.code("11").field(127, 7).code("11").field(118 - 11, 7).code("10").code("10").code("0")
    out["a symbol with no code"] = frame(w.code("1").bytes() + bytes(8))
    fixed = lambda: BitWriter().field(1, 1).field(1, 2)
    out["length symbol 286"] = frame(fixed().code("11000110").bytes() + bytes(4))
    out["distance symbol 30"] = frame(fixed().code(FIXED_A).code("0000001").code("11110").bytes() + bytes(4), b"AAAA")
    out["a distance before the block's output"] = frame(fixed().code(FIXED_A).code("0000001").code("00001").code("0000000").bytes(), b"AAAA")
    out["input exhausted before the end-of-block symbol"] = frame(good[:-3], text)
    out["more output than ISIZE"] = frame(good, text, isize=len(text) - 1)
    out["less output than ISIZE"] = frame(good, text, isize=len(text) + 1)
    out["CRC32 mismatch"] = frame(good, text, crc=zlib.crc32(text) ^ 0x00010000)
    return out


def reference_verdict(block):
    """What a BGZF reader built on zlib says of one block lying alone in `block`: the payload, or None when it is refused.  The header
    rules are those of include/platypus_mi355x.h, restated; inflate and CRC32 are zlib's."""
    n = len(block)
    if n < 26 or block[:3] != b"\x1f\x8b\x08" or block[3] != 4:
        return None
    xlen = struct.unpack_from("<H", block, 10)[0]
    if 12 + xlen + 8 > n:
        return None
    x, bsize = 0, None
    while x + 4 <= xlen:
        si, slen = block[12 + x:14 + x], struct.unpack_from("<H", block, 14 + x)[0]
        if x + 4 + slen > xlen:
            return None
        if si == b"BC" and slen == 2 and bsize is None:
            bsize = struct.unpack_from("<H", block, 16 + x)[0]
        x += 4 + slen
    if x != xlen or bsize is None:
        return None
    total = bsize + 1
    if total < 12 + xlen + 8 or total > n:
        return None
    crc, isize = struct.unpack_from("<II", block, total - 8)
    if isize > 65536:
        return None
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(block[12 + xlen:total - 8])
    except zlib.error:
        return None
    if not d.eof or len(out) != isize or zlib.crc32(out) != crc:
        return None
    return out


# ---- the record walk -----------------------------------------------------------------------------------------------------------------
def rule_walk(data, first, stop, tid, beg, end):
    """sam_itr_next as plat_bam_find_records states it, over the contiguous inflated bytes of one chunk: (0 or -9, offsets of the kept
    records' refID, records walked, whether the walk ended on a record outside the window)."""
    hi, pos, kept, walked = len(data), first, [], 0
    stop = hi if stop is None else stop
    while pos < stop and pos < hi:
        if hi - pos < 4:
            return -9, kept, walked, False
        bs = struct.unpack_from("<i", data, pos)[0]
        if bs < 32 or pos + 4 + bs > hi:
            return -9, kept, walked, False
        t, b = struct.unpack_from("<ii", data, pos + 4)
        if t != tid or b >= end:
            return 0, kept, walked, True
        n_cig, l_name = struct.unpack_from("<H", data, pos + 16)[0], data[pos + 12]
        if 36 + l_name + 4 * n_cig > 4 + bs:
            return -9, kept, walked, False
        e = b + 1
        if n_cig:
            words = struct.unpack_from("<%dI" % n_cig, data, pos + 36 + l_name)
            e = b + sum(w >> 4 for w in words if (w & 15) in (0, 2, 3, 7, 8))
        walked += 1
        if e > beg and end > b:
            kept.append(pos + 4)
        pos += 4 + bs
    return 0, kept, walked, False


def record(tid, pos, cigar, n_bases=20, name=b"r\0", flag=3, aux=b""):
    """block_size + one alignment record, field by field (SAM/BAM specification 4.2)."""
    rec = (struct.pack("<iiBBHHHiiii", tid, pos, len(name), 60, 0, len(cigar), flag, n_bases, tid, pos + 100, 120) + name +
           b"".join(struct.pack("<I", (ln << 4) | op) for op, ln in cigar) + bytes([0x12] * ((n_bases + 1) // 2)) + bytes([30] * n_bases) + aux)
    return struct.pack("<i", len(rec)) + rec


def walk_cases():
    """[(name, inflated bytes, first, stop or None, tid, beg, end)]: window 1000-2000 on tid 3 unless said otherwise."""
    M = lambda n: [(0, n)]
    out = []
    body = b"".join([record(3, 100, M(50)),                       # before the window
                     record(3, 960, M(50)),                       # overlapping its start
                     record(3, 950, M(50)),                       # touching it: e == beg
                     record(3, 990, [(4, 10), (0, 10), (2, 5)]),  # M + D reach 1005
                     record(3, 1000, [(4, 20)]),                  # reference length 0 with b == beg: e == b == beg, not kept
                     record(3, 1200, [(4, 10), (1, 10)]),         # reference length 0 with b > beg: kept
                     record(3, 1300, []),                         # no CIGAR: e = b + 1
                     record(3, 999, []),                          # no CIGAR, e == beg: not kept
                     record(3, 1400, M(20), flag=4),              # flag 4 plays no part
                     record(3, 1999, M(20), name=b"n" * 254 + b"\0", aux=b"XYZ" * 40),
                     record(3, 2000, M(20)),                      # pos >= end: the walk ends
                     record(3, 1500, M(20))])                     # ... with a kept-looking record behind it
    out.append(("the window's edges", body, 0, None, 3, 1000, 2000))
    out.append(("another tid first", record(2, 1500, M(20)) + body, 0, None, 3, 1000, 2000))
    out.append(("another tid after", record(3, 1500, M(20)) + record(4, 1500, M(20)) + record(3, 1600, M(20)), 0, None, 3, 1000, 2000))
    out.append(("a first offset inside the bytes", b"\xff" * 37 + body, 37, None, 3, 1000, 2000))
    three = [record(3, 1100 + 10 * k, M(20)) for k in range(6)]
    out.append(("stop before the window's end", b"".join(three), 0, sum(len(r) for r in three[:4]), 3, 1000, 2000))
    out.append(("stop inside a record: it is still read", b"".join(three), 0, sum(len(r) for r in three[:4]) + 1, 3, 1000, 2000))
    out.append(("stop at the first offset", b"".join(three), len(three[0]), len(three[0]), 3, 1000, 2000))
    out.append(("block_size 31", three[0] + struct.pack("<i", 31) + three[1][4:], 0, None, 3, 1000, 2000))
    out.append(("a negative block_size", three[0] + struct.pack("<i", -40) + three[1][4:], 0, None, 3, 1000, 2000))
    out.append(("a record running past the stream", b"".join(three)[:-1], 0, None, 3, 1000, 2000))
    out.append(("three bytes of a block_size", b"".join(three) + b"\x40\0\0", 0, None, 3, 1000, 2000))
    short = bytearray(three[1])
    struct.pack_into("<H", short, 16, 40)                         # n_cigar_op: 40 words do not fit the record's bytes
    out.append(("a CIGAR running past its record", three[0] + bytes(short) + three[2], 0, None, 3, 1000, 2000))
    long_cigar = record(3, 1000, [(0, 1), (1, 1)] * 3000, n_bases=3000)       # 24 kB of CIGAR: more than one staging window
    out.append(("a CIGAR longer than a staging window", three[0] + long_cigar + three[1], 0, None, 3, 1000, 9000))
    many = b"".join(record(3, 1000 + k, M(30 + k % 7), name=b"q" * (1 + k % 40) + b"\0") for k in range(900))
    out.append(("many records", many, 0, None, 3, 1200, 1700))
    out.append(("an empty stream", b"", 0, None, 3, 1000, 2000))
    return out


def aligned(x, end=None):
    """A fixture read (tests/golden/region_fetched_cases.json.gz) as hostapi.AlignedRead."""
    return H.AlignedRead(x["seq"].encode(), bytes(ord(c) - 33 for c in x["qual"]), x["pos"], x["mapq"], x["flag"],
                         end=x["end"] if end is None else end, cigarOps=[tuple(c) for c in x["cigar"]], chromID=x.get("chromID", 0),
                         mateChromID=x.get("mateChromID", 0), insertSize=x.get("insertSize", 0), matePos=x["matePos"])


# ---- streams zlib never writes (tests/deflate_writer.py) ------------------------------------------------------------------------------
BGZF_MAX_CDATA = 65536 - 26                                # BSIZE is 16 bits: a block is at most 65536 bytes, 26 of them header and trailer


def zlib_message(block):
    """zlib's own words for refusing the block's deflate stream ('' when it inflates it to the end; 'incomplete' when the input ends
    first): the reach checks read these, not the decoder under test."""
    xlen = struct.unpack_from("<H", block, 10)[0]
    d = zlib.decompressobj(-15)
    try:
        d.decompress(block[12 + xlen:len(block) - 8])
    except zlib.error as e:
        return str(e)
    return "" if d.eof else "incomplete"


def _text(seed, n, alphabet=b"ACGT"):
    rng = np.random.default_rng(seed)
    return bytes(alphabet[int(k)] for k in rng.integers(0, len(alphabet), size=n))


OVERLAP_DISTS = (1, 2, 3, 4, 5, 7, 63, 64, 65, 127, 128, 129, 257, 258)
OVERLAP_LENS = (3, 4, 63, 64, 65, 128, 129, 257, 258)
_foreign_cache = {}


def _foreign():
    if "blocks" in _foreign_cache:
        return _foreign_cache["blocks"], _foreign_cache["records"]
    from tests import deflate_writer as D
    out, recs = [], D.Records()
    rng = np.random.default_rng(1951)
    noise = lambda n: rng.integers(0, 256, size=n, dtype=np.uint8).tobytes()

    def add(name, w, valid=True, pad=0, **kw):
        """valid=False: the hand-written claim that zlib refuses the block (the CPU test checks every claim against zlib)."""
        payload = bytes(w.out)
        cdata = w.finish(pad)
        assert len(cdata) <= BGZF_MAX_CDATA and len(payload) <= 65536 + 2, name
        if "isize" in kw:
            kw.setdefault("crc", zlib.crc32(payload[:kw["isize"]]))
        out.append((name, payload if valid else None, frame(cdata, payload, **kw)))
        recs.merge(w.rec)

    def flat(tokens, extra_lit=(), extra_dist=()):
        ls, ds = D.used_symbols(tokens)
        ls, ds = sorted(set(ls) | set(extra_lit)), sorted(set(ds) | set(extra_dist))
        lit = D.flat_lengths(ls, 288) if len(ls) > 1 else D.single_lengths(256, 288)
        dist = D.flat_lengths(ds, 32) if len(ds) > 1 else D.single_lengths(ds[0], 32) if ds else [0] * 32
        return lit, dist

    def dyn(tokens, final=True, **kw):
        lit, dist = flat(tokens)
        return D.DeflateWriter().dynamic(tokens, lit, dist, final=final, **kw)

    # -- long codes
    order = [65, 67, 71, 84, 78, 97, 99, 103, 116, 110, 257, 46, 285, 42, 256, 61]
    for name, entries in (("256 at 15 bits", order), ("256 at 1 bit", order[::-1])):
        lit = D.ladder_lengths(entries, 288)
        assert sorted(set(lit)) == list(range(16))
        toks = [s for s in entries if s < 256] * 2 + [(3, 1), (258, 2), 61, (258, 1), 65, 42, 46, 110, (3, 2)]
        w = D.DeflateWriter().dynamic(toks, lit, D.flat_lengths([0, 1], 32), final=True)
        assert w.rec.lit_lens == set(range(1, 16))
        add("literal/length codes of 1..15 bits, " + name, w)
    dorder = [3, 0, 7, 1, 10, 2, 12, 4, 14, 5, 16, 6, 18, 8, 20, 9]
    dist = D.ladder_lengths(dorder, 32)
    toks = list(_text(7, 1600, b"ACGTNacgtn"))
    for k in dorder + dorder[::-1]:
        toks += [(257 + k % 5, 0, k, 0), (258, 0, k, (1 << D.DEXT[k]) - 1), 36 + k]
    lit, _ = flat(toks)
    w = D.DeflateWriter().dynamic(toks, lit, dist, final=True)
    assert w.rec.dist_lens == set(range(1, 16))
    add("distance codes of 1..15 bits", w)
    lit = [0] * 288
    lit[65:73], lit[256], lit[257], lit[258] = [4] * 8, 2, 3, 3
    toks = list(b"ABCDEFGH") + [(3, 1), (4, 1), 72, 65]
    w = D.DeflateWriter().dynamic(toks, lit, D.single_lengths(0, 32), final=True, cl_lens=D.ladder_lengths([18, 4, 0, 3, 2, 17, 1, 16], 19, maxlen=7))
    assert 7 in w.rec.cl_lens
    add("a code-length code of 1..7 bits", w)

    # -- every length symbol and every distance symbol, extra bits all zero and all one
    toks = [97, 98]
    for k in range(29):
        toks += [(257 + k, 0, k % 2, 0), 99 + k, (257 + k, (1 << D.LEXT[k]) - 1, k % 2, 0)]
    add("all length symbols, fixed", D.DeflateWriter().fixed(toks, final=True))
    add("all length symbols, dynamic", dyn(toks))
    add("length 258 as symbol 284 + 31", D.DeflateWriter().fixed([97, 98, (284, 31, 1, 0), 99], final=True))
    far = noise(32768)
    toks = []
    for k in range(30):
        toks += [(257 + k % 7, 0, k, 0), 48 + k, (258 + k % 3, 0, k, (1 << D.DEXT[k]) - 1)]
    for how in ("fixed", "dynamic"):
        w = D.DeflateWriter().stored(far)
        lit, dist = flat(toks)
        w.fixed(toks, final=True) if how == "fixed" else w.dynamic(toks, lit, dist, final=True)
        add("all distance symbols, " + how, w)

    # -- header extremes
    lits = list(b"header extremes")
    add("HLIT 29, HDIST 29, HCLEN 15", D.DeflateWriter().dynamic(lits + [(5, 3)], *flat(lits + [(5, 3)]), final=True, hlit=29, hdist=29, hclen=15))
    add("HLIT 0, HDIST 0", D.DeflateWriter().dynamic(lits, *flat(lits), final=True, hlit=0, hdist=0))
    all8 = D.flat_lengths(list(range(255)) + [256], 288)                       # 256 codes of 8 bits: the lengths need 8, 0 and 18 only
    assert set(all8) == {0, 8}
    cl = [0] * 19
    cl[8], cl[0], cl[18] = 1, 2, 2
    add("HCLEN 1: the least a valid block can have", D.DeflateWriter().dynamic(list(range(0, 255, 5)), all8, [0] * 32, final=True, cl_lens=cl, hclen=1, rle="none"))
    cl = [0] * 19
    cl[0], cl[18], cl[17] = 1, 2, 2
    add("HCLEN 0: no code for a length but 0", D.DeflateWriter().dynamic([], [0] * 288, [0] * 32, final=True, cl_lens=cl, hclen=0, check=False, end=False).raw("0" * 64), valid=False)
    for mode in ("none", "greedy"):
        add("header run-length mode " + mode, dyn(lits + [(4, 2), (9, 7)], rle=mode))
    lit = [0] * 288
    lit[97], lit[98], lit[256], lit[257], lit[258] = 3, 3, 2, 2, 2
    d4 = [2, 2, 2, 2]
    seq = lit[:259] + d4
    head = D.rle_greedy(seq[:256])
    toks = [97, 98, 97, (3, 1), (4, 2), (3, 3), (4, 4)]
    w = D.DeflateWriter().dynamic(toks, lit, d4, final=True, rle=head + [(2, 1), (2, 1), (16, 5)])
    assert w.rec.cross16 == 1 and w.rec.rle_modes == {"explicit"}
    add("a 16 from the last literal length into the distance lengths", w)
    add("a 16 at the first distance length", D.DeflateWriter().dynamic(toks, lit, d4, final=True, rle=head + [(2, 1)] * 3 + [(16, 4)]))
    lit, _ = flat(lits)
    d14 = [0] * 12 + [1, 1]
    head = D.rle_greedy(lit[:257])
    w = D.DeflateWriter().dynamic(lits, lit, d14, final=True, hlit=10, rle=head + [(18, 22), (1, 1), (1, 1)])
    assert w.rec.cross18 == 1
    add("an 18 from the literal lengths into the distance lengths", w)
    toks = list(_text(3, 70)) + [(3, 65), (4, 70)]                            # distance symbols 12 and 13, behind twelve lengths of zero
    lit, _ = flat(toks)
    w = D.DeflateWriter().dynamic(toks, lit, d14, final=True, hlit=10, rle=D.rle_greedy(lit[:259]) + [(18, 20), (1, 1), (1, 1)])
    assert w.rec.cross18 == 1
    add("an 18 across the boundary, the distances used", w)
    d10 = [1, 1] + [0] * 8
    toks = lits + [(3, 1), (3, 2)]
    lit, _ = flat(toks)
    w = D.DeflateWriter().dynamic(toks, lit, d10, final=True, hdist=9, rle=D.rle_greedy(lit[:258] + [1, 1]) + [(17, 8)])
    add("a 17 that ends on the last length", w)

    # -- small sets
    lit, _ = flat([97, (3, 1)])
    add("a distance set of one code, used", D.DeflateWriter().dynamic([97, (3, 1), 97], lit, D.single_lengths(0, 32), final=True))
    toks = list(b"abcdefgh") + [(3, 7), (5, 8)]
    add("a distance set of one code, at symbol 5", D.DeflateWriter().dynamic(toks, flat(toks)[0], D.single_lengths(5, 32), final=True))
    add("a distance set of one code, the unused code met", D.DeflateWriter().dynamic([97, D.canonical(lit)[257] + "1"], lit, D.single_lengths(0, 32), final=True), valid=False)
    add("no distance code under literals only", D.DeflateWriter().dynamic(lits, flat(lits)[0], [0] * 32, final=True))
    add("a literal/length set of 256 alone", D.DeflateWriter().dynamic([], D.single_lengths(256, 288), [0] * 32, final=True))
    add("a literal/length set of 256 alone, twice, then data", D.DeflateWriter().dynamic([], D.single_lengths(256, 288), [0] * 32).dynamic([], D.single_lengths(256, 288), [0], rle="none").fixed(lits, final=True))
    add("the unused code of a literal/length set of one", D.DeflateWriter().dynamic(["1"], D.single_lengths(256, 288), [0] * 32, final=True, end=False).raw("0" * 40), valid=False)

    # -- overlap ladder: dist literals (no two neighbours alike), then one match of len at dist
    for i, dist in enumerate(OVERLAP_DISTS):
        for j, ln in enumerate(OVERLAP_LENS):
            toks = [(k * 7 + 3 + dist) % 251 for k in range(dist)] + [(ln, dist), 255]
            add("overlap dist %d len %d" % (dist, ln), D.DeflateWriter().fixed(toks, final=True) if (i + j) % 2 else dyn(toks))

    # -- dependence chains: every match reads what the one before wrote
    chain = [(3, 3), (6, 6), (12, 12), (24, 24), (48, 48), (96, 96), (192, 192), (258, 258)]
    add("chain", D.DeflateWriter().fixed(list(b"abc") + chain, final=True))
    between = list(b"abc")
    at = 3
    for k, (ln, _) in enumerate(chain):
        between += [(ln, at), 65 + k]                                           # (the distance grows by the literal: still the whole output so far)
        at += ln + 1
    add("chain with literals between", dyn(between))
    for shift in range(67):                                                    # every link once on command slots 62..65 of a batch
        toks = [(33 + 5 * k) % 256 for k in range(shift)] + list(b"abc") + chain + [36]
        add("chain behind %d literals" % shift, D.DeflateWriter().fixed(toks, final=True) if shift % 2 else dyn(toks))

    # -- far edges
    add("distance 32768, length 258, at output 32768", D.DeflateWriter().stored(far).fixed([(258, 32768), 33], final=True))
    fill = lambda n, dist: [(258, dist)] * (n // 258) + ([(n % 258, dist)] if n % 258 >= 3 else [0x33] * (n % 258))
    base = noise(30000)
    rest = 65536 - 30000
    assert rest % 258 == 190
    add("a match ending on byte 65535 of 65536", D.DeflateWriter().stored(base).fixed(fill(rest, 30000), final=True))
    add("a literal as byte 65535 of 65536", D.DeflateWriter().stored(base).fixed(fill(rest - 1, 29999) + [0x5a], final=True))
    add("a match with dist == out", dyn([(k * 11 + 1) % 256 for k in range(300)] + [(258, 300), 1]))
    add("a match of 258 at distance 1 as the first match", D.DeflateWriter().fixed([7, (258, 1), (258, 1), 8], final=True))

    # -- block sequences
    w = D.DeflateWriter()
    for k in range(300):
        if k % 3 == 0:
            w.stored(b"", pad=k & 31)
        elif k % 3 == 1:
            w.fixed([])
        else:
            w.dynamic([], D.single_lengths(256, 288), [0] * 32, rle=("greedy", "none")[k % 2])
    add("300 empty blocks, then data", w.fixed(lits, final=True))
    rec = synthetic_record_bytes(3000)
    toks = D.match_tokens(rec, cuts=(500, 1000, 1700, 2200))
    p = D.split_tokens(toks, (500, 1000, 1700, 2200))
    w = D.DeflateWriter().stored(rec[:500])
    w.dynamic(p[1], *flat(p[1])).stored(rec[1000:1700], pad=0x55).fixed(p[3]).dynamic(p[4], *flat(p[4]), final=True, rle="none")
    assert bytes(w.out) == rec and w.rec.blocks == ["stored", "dynamic", "stored", "fixed", "dynamic"]
    add("stored, dynamic, stored, fixed, dynamic", w, pad=0x7f)
    add("a stored block of LEN 0 as the final block", D.DeflateWriter().fixed(lits).stored(b"", final=True, pad=0xff))
    big = noise(BGZF_MAX_CDATA - 10)                                           # (65535 + 1 does not fit BSIZE: the most two stored blocks can hold)
    add("65500 bytes as stored 65499 + stored 1", D.DeflateWriter().stored(big[:-1]).stored(big[-1:], final=True))
    for j in range(8):                                                         # 3 + 8 x 3 + 9 j + 7 bits: the fixed block ends on bit (2 + j) % 8
        w = D.DeflateWriter().fixed([65, 67, 71] + [200 + j] * j).stored(b"behind phase %d" % j, final=j % 2 == 0, pad=(0, 0xff)[j % 2])
        if j % 2:
            w.fixed([33], final=True)
        assert w.rec.stored_phases == [(2 + j) % 8]
        add("a stored block behind a coded block that ends on bit %d" % ((2 + j) % 8), w, pad=0xff * (j % 2))
    add("non-zero padding bits", D.DeflateWriter().fixed(lits).stored(b"padded", pad=0x15).fixed([1, 2, 3], final=True), pad=0x7f)

    # -- refused
    bad = lambda toks, lit, dist, **kw: D.DeflateWriter().dynamic(toks, lit, dist, final=True, check=False, **kw).raw("0" * 32)
    lit = [0] * 288
    lit[97] = lit[98] = 1
    add("no code for 256", bad([97, 98], lit, [0] * 32, end=False), valid=False)
    lit = [0] * 288
    lit[97] = lit[256] = 2
    add("an incomplete literal/length set of two codes", bad([97], lit, [0] * 32), valid=False)
    lit, _ = flat(lits + [(3, 1)])
    add("an over-subscribed distance set", bad(lits, lit, [1, 1, 1]), valid=False)
    add("an over-subscribed literal/length set", bad([], [1] * 3 + [0] * 253 + [1], [0] * 32, end=False), valid=False)
    for h in (30, 31):
        add("HLIT %d" % h, bad(lits, lit, [1, 1], hlit=h), valid=False)
        add("HDIST %d" % h, bad(lits, lit, [1, 1], hdist=h), valid=False)
    for isize, before, ln in ((65536, 65534, 3), (65535, 65533, 3), (65536, 65535, 3), (65536, 65279, 258)):
        w = D.DeflateWriter().stored(base).fixed(fill(before - 30000, 30000) + [(ln, 2)], final=True)
        assert len(w.out) == before + ln > isize
        add("a match from %d to %d under ISIZE %d" % (before, before + ln, isize), w, valid=False, isize=isize)
    add("a literal past ISIZE 65536", D.DeflateWriter().stored(base).fixed(fill(rest, 30000) + [1], final=True), valid=False, isize=65536)
    add("a stored block whose LEN runs past ISIZE", D.DeflateWriter().fixed(lits).stored(bytes(100), final=True), valid=False, isize=len(lits) + 99)
    add("output one byte short of ISIZE", D.DeflateWriter().fixed(lits, final=True), valid=False, isize=len(lits) + 1)
    # ... and one stream for each of zlib's refusals that the list above does not reach
    add("block type 3", D.DeflateWriter().fixed(lits).raw("011" + "0" * 40), valid=False)
    add("stored NLEN not the complement", D.DeflateWriter().fixed(lits).stored(b"ACGT", final=True, nlen=0xfffa), valid=False)
    assert set(lit) == {0, 3, 4}
    for name, n in (("over-subscribed", 1), ("incomplete", 2)):
        cl = [0] * 19
        cl[0] = cl[3] = cl[4] = n
        add("an %s code-length set" % name, bad(lits, lit, [0], cl_lens=cl, rle="none"), valid=False)
    cl = D.flat_lengths([0, 1, 2, 3, 16], 19)
    add("a 16 with no length in front of it", bad([], [0] * 288, [0], cl_lens=cl, rle=[(16, 3), (1, 1)], end=False), valid=False)
    lit2 = [0] * 256 + [1, 1]
    add("a 16 running past HLIT + HDIST", bad([], lit2, [0], rle=D.rle_greedy(lit2[:256]) + [(1, 1), (1, 1), (16, 3)], end=False), valid=False)
    add("an 18 running past HLIT + HDIST", bad([], [0] * 256 + [1], [0], rle=[(18, 138), (18, 121)], cl_lens=D.flat_lengths([1, 18], 19), end=False), valid=False)
    add("a distance one byte too far back", D.DeflateWriter().fixed([1, 2, 3, D.token_bits((3, 4))], final=True), valid=False)
    add("distance 32768 at output 32767", D.DeflateWriter().stored(far[:-1]).fixed([D.token_bits((3, 32768))], final=True), valid=False)
    _foreign_cache["blocks"], _foreign_cache["records"] = out, recs
    return out, recs


def foreign_blocks():
    """[(name, payload or None, block)]: BGZF blocks around deflate streams written by tests/deflate_writer.py, valid ones that zlib's
    encoder never writes and invalid ones.  `None` is a hand-written claim that zlib refuses the block: the verdict of every case is
    reference_verdict(block), and tests/test_deflate_writer_cpu.py checks every claim against it."""
    return list(_foreign()[0])


def foreign_records():
    """What the writer recorded while it wrote foreign_blocks() (deflate_writer.Records, merged)."""
    return _foreign()[1]


def _fuzz_stream(D, rng, payload):
    """One stream over `payload` with every choice of the writer drawn from rng: (DeflateWriter, final padding)."""
    n = len(payload)
    cuts = sorted({int(c) for c in rng.integers(0, n + 1, size=int(rng.integers(0, 4)))} - {0, n}) if n else []
    toks = D.match_tokens(payload, max_dist=int(2 ** rng.uniform(0, 15)), min_len=int(rng.choice([3, 3, 4, 8, 30])), cuts=cuts)
    parts = D.split_tokens(toks, cuts)
    edges = [0] + cuts + [n]
    w = D.DeflateWriter()

    def empty():
        kind = int(rng.integers(3))
        if kind == 0:
            w.stored(b"", pad=int(rng.integers(32)))
        elif kind == 1:
            w.fixed([])
        else:
            w.dynamic([], D.single_lengths(256, 288), [0] * 32, rle=("none", "greedy")[int(rng.integers(2))])

    for k, part in enumerate(parts):
        while rng.random() < 0.15:
            empty()
        final = k == len(parts) - 1
        kind = int(rng.integers(4))
        if kind == 0 and edges[k + 1] - edges[k] <= 65535:
            w.stored(payload[edges[k]:edges[k + 1]], final=final, pad=int(rng.integers(32)))
        elif kind == 1:
            w.fixed(part, final=final)
        else:
            ls, ds = D.used_symbols(part)
            ls = sorted(set(ls) | {int(s) for s in rng.integers(0, 286, size=int(rng.integers(0, 12)))})
            ds = sorted(set(ds) | {int(s) for s in rng.integers(0, 30, size=int(rng.integers(0, 4)))})
            deep = float(rng.choice([0.0, 0.5, 0.9, 1.0]))
            lit = D.random_lengths(rng, ls, 288, deep=deep) if len(ls) > 1 else D.single_lengths(256, 288)
            dist = D.random_lengths(rng, ds, 32, deep=deep) if len(ds) > 1 else D.single_lengths(ds[0], 32) if ds else [0] * 32
            nl, nd = max(257, max(ls) + 1), max([1] + [d + 1 for d in ds])
            nl, nd = (nl, nd) if rng.random() < 0.5 else (int(rng.integers(nl, 287)), int(rng.integers(nd, 31)))
            seq = (lit + [0] * 288)[:nl] + (dist + [0] * 32)[:nd]
            mode = ("none", "greedy", "explicit")[int(rng.integers(3))]
            ops = D.rle_none(seq) if mode == "none" else D.rle_greedy(seq) if mode == "greedy" else D.rle_random(seq, rng)
            cs = sorted({s for s, _ in ops} | {int(s) for s in rng.integers(0, 19, size=int(rng.integers(0, 3)))})
            cs = cs if len(cs) > 1 else cs + [(cs[0] + 1) % 19]
            cl = D.random_lengths(rng, cs, 19, maxlen=7, deep=float(rng.choice([0.0, 0.6, 1.0])))
            need = max(4, max(i + 1 for i, s in enumerate(D.CL_ORDER) if cl[s]))
            w.dynamic(part, lit, dist, final=final, hlit=nl - 257, hdist=nd - 1, hclen=(need if rng.random() < 0.5 else int(rng.integers(need, 20))) - 4,
                      cl_lens=cl, rle=mode if mode != "explicit" else ops)
    return w, int(rng.integers(256)) if rng.random() < 0.5 else 0


_fuzz_cache = {}


def foreign_fuzz(seed=1952, n=400):
    """([(name, payload, block, flipped block)], Records): n streams from the writer with every choice drawn at random -- payloads of
    0..65536 bytes (most of them short: every one costs the suite time) of synthetic BAM records, a four-letter alphabet or random bytes
    -- and of each a copy with 1-3 bits flipped inside the first deflate block's header and code lengths.  Every verdict is zlib's
    (reference_verdict): a stream the writer calls valid and zlib refuses is a bug of the writer, and no stream is left out.  A draw that
    does not fit BSIZE is drawn again at half the size, which is part of the generation and not a choice made after a verdict."""
    if (seed, n) in _fuzz_cache:
        return _fuzz_cache[(seed, n)]
    from tests import deflate_writer as D
    rng = np.random.default_rng(seed)
    recs_src = synthetic_record_bytes(65536)
    out, recs = [], D.Records()
    for k in range(n):
        src = ("records", "four letters", "random")[k % 3]
        u = rng.random()
        size = (0, 65536)[int(rng.integers(2))] if k % 50 == 7 else int(rng.integers(0, 300) if u < 0.5 else rng.integers(300, 3000) if u < 0.85 else
                                                                          rng.integers(3000, 20000) if u < 0.97 else rng.integers(20000, 65537))
        while True:
            if src == "records":
                a = int(rng.integers(0, len(recs_src) - size + 1))
                payload = recs_src[a:a + size]
            elif src == "four letters":
                payload = bytes(b"ACGT"[int(c)] for c in rng.integers(0, 4, size=size))
            else:
                payload = rng.integers(0, 256, size=size, dtype=np.uint8).tobytes()
            w, pad = _fuzz_stream(D, rng, payload)
            assert bytes(w.out) == payload
            cdata = w.finish(pad)
            if len(cdata) <= BGZF_MAX_CDATA:
                break
            size //= 2
        flipped = bytearray(cdata)
        for bit in rng.integers(0, w.rec.first_head_bits, size=int(rng.integers(1, 4))):
            flipped[int(bit) >> 3] ^= 1 << (int(bit) & 7)
        recs.merge(w.rec)
        out.append(("fuzz %d: %d bytes of %s in %s" % (k, len(payload), src, "+".join(w.rec.blocks)), payload, frame(cdata, payload), frame(bytes(flipped), payload)))
    _fuzz_cache[(seed, n)] = (out, recs)
    return out, recs


# ---- the record walk's window seam -----------------------------------------------------------------------------------------------------
FIND_WINDOW = 16384                                        # plat_bgzf.hip, restated: k_bam_find stages the inflated bytes in windows of this size,
window_base = lambda pos: pos & ~3                         # each starting at the first record that did not fit the one before, rounded down to a dword


def record_need(rec):
    """The bytes of a record (block_size word included) that the walk reads: the 36 fixed ones, the name, the CIGAR."""
    return 36 + rec[12] + 4 * struct.unpack_from("<H", rec, 16)[0]


def window_bases(starts, needs, hi):
    """The window bases k_bam_find goes through over records at `starts` (what the walk reads of each: `needs`), by the rule its header
    comment states: a window ends at base + FIND_WINDOW or the stream's end; the first record whose read bytes pass that end starts the
    next window, unless it is the window's own first record (which is then read where it lies)."""
    bases, i = [], 0
    while i < len(starts):
        base = window_base(starts[i])
        bases.append(base)
        w_end, j = min(base + FIND_WINDOW, hi), i
        while j < len(starts) and (starts[j] + needs[j] <= w_end or j == i or w_end >= hi):
            j += 1
        i = j
    return bases


def sized_record(size, pos, name=b"r\0", n_cigar=1):
    """A record of exactly `size` bytes (block_size word included) on tid 3; aux bytes make up the size."""
    cigar = [(0, 7)] * n_cigar
    least = len(record(3, pos, cigar, 8, name))
    assert size >= least, (size, least)
    return record(3, pos, cigar, 8, name, aux=b"\x41" * (size - least))


def _seam_stream(first, d, probe_shape=None, end_extra=None, seed=0):
    """(bytes, probe's start): `first` junk bytes, then records such that the probe begins d bytes before the end of the SECOND window;
    probe_shape: (name length, CIGAR count).  end_extra: the stream ends that many bytes behind the second window's end instead (the
    probe is its last record); otherwise the length is a multiple of 4, so that such streams laid side by side keep their window bases."""
    rng = np.random.default_rng(1000 + seed)
    parts, at, pos = [b"\xff" * first], first, 100
    starts, needs = [], []

    def put(rec):
        nonlocal at, pos
        starts.append(at)
        needs.append(record_need(rec))
        parts.append(rec)
        at += len(rec)
        pos += 3

    def filler():
        l_name, n_cig = int(rng.integers(1, 30)), int(rng.integers(0, 5))
        put(sized_record(48 + l_name + 4 * n_cig + int(rng.integers(0, 300)), pos, name=b"q" * (l_name - 1) + b"\0", n_cigar=n_cig))

    while at < first + FIND_WINDOW + 400:
        filler()
    bases = window_bases(starts, needs, 1 << 30)
    assert len(bases) == 2 and bases[0] == window_base(first)
    w2_end = bases[1] + FIND_WINDOW
    target = w2_end - d
    while at < target - 900:
        filler()
    gap = target - at
    put(sized_record(gap // 2, pos))
    put(sized_record(gap - gap // 2, pos))
    assert at == target
    l_name, n_cig = probe_shape if probe_shape is not None else (2 + d % 7, d % 3)
    name = b"p" * (l_name - 1) + b"\0"
    least = 48 + l_name + 4 * n_cig
    if end_extra is not None:
        put(sized_record(d + end_extra, pos, name, n_cig))
        assert at == w2_end + end_extra
    else:
        put(sized_record(least + 40 + d, pos, name, n_cig))
        for k in range(3):
            put(sized_record(100 + 9 * k, pos))
        put(sized_record(120 + (-(at + 120) % 4), pos))
    return b"".join(parts), target


_seam_cache = {}


def walk_seam_cases():
    """([(name, inflated bytes, first, stop or None, tid, beg, end)], probes): the format of walk_cases(); every record lies in the window,
    so rule_walk's kept offsets are ALL the records' starts and a record the device skips or reads at a wrong place shows.  probes:
    {case index: (d, probe's start)} for the ladder -- a probe record that begins d bytes before the end of the second 16 KiB window, d in
    0..44 (its block_size word, the name-length byte at +12, the n_cigar field at +16 straddle the window's end in turn), and for each d
    that allows it name lengths and CIGAR counts such that the last CIGAR word ends at the window's end -4, -1, 0, +1, +4."""
    if _seam_cache:
        return _seam_cache["cases"], _seam_cache["probes"]
    out, probes = [], {}
    T = (3, 0, 1 << 30)
    for d in range(45):
        shapes = [None]
        for delta in (-4, -1, 0, 1, 4):
            rest = d - 36 + delta                         # name length + 4 x CIGAR count
            if rest >= 1:
                n_cig = min((rest - 1) // 4, (d + delta) % 3)
                shapes.append((rest - 4 * n_cig, n_cig))
        for k, shape in enumerate(shapes):
            data, probe = _seam_stream((d + k) % 4, d, shape, seed=d)
            probes[len(out)] = (d, probe)
            out.append(("probe %d bytes before the window's end, shape %s" % (d, shape), data, (d + k) % 4, None) + T)
    for e in range(41):
        data, _ = _seam_stream(e % 4, 70 + e % 9, end_extra=e, seed=100 + e)
        out.append(("the stream ends %d bytes behind a window's end" % e, data, e % 4, None) + T)
    # a record whose CIGAR alone is longer than a window, and one whose bases are, each at a window's start, then records again
    M = [(0, 7)]
    small = lambda k0, n: b"".join(sized_record(90 + (7 * k) % 50, 1000 + k0 + k, n_cigar=k % 4) for k in range(n))
    huge_cigar = record(3, 5000, [(0, 1), (1, 1)] * 2200, n_bases=2200)
    huge_bases = record(3, 5001, M, n_bases=12000)
    assert record_need(huge_cigar) > FIND_WINDOW and len(huge_bases) > FIND_WINDOW > record_need(huge_bases)
    for first in (0, 3):
        data = b"\xff" * first + small(0, 150) + huge_cigar + small(200, 40) + huge_bases + small(300, 60)
        out.append(("records longer than a window at a window's start, first %d" % first, data, first, None) + T)
    _seam_cache["cases"], _seam_cache["probes"] = out, probes
    return out, probes
