"""Cases shared by tests/test_bgzf_cpu.py (the host build of csrc/bgzf_inflate.hpp) and tests/test_gpu_bgzf.py (the device): the inflate
grid, the corrupt blocks -- each a valid block with bytes edited, or a deflate stream written bit by bit here inside a valid frame --, the
reference verdict on a block (Python's zlib behind a restatement of the header rules) and the record walk's rule restated.  Nothing here
calls the code under test."""
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
