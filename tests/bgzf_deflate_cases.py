"""Cases shared by tests/test_bgzf_deflate_cpu.py (the host twin, csrc/bgzf_deflate.hpp) and tests/test_gpu_bgzf_deflate.py (the device,
plat_bgzf_deflate_batch), and a restatement in Python of the encoding rule include/platypus_mi355x.h states: pieces cut into blocks of 0xff00
bytes, level 0 stored, level 1 one-candidate LZ77 (15-bit multiplicative hash of four bytes, nearest earlier position with the same hash, every
position inserted, greedy parse) coded with the fixed Huffman codes of RFC 1951, stored instead when that is no shorter.  The restatement
looks codes up in the RFC's tables; the C++ computes them."""
import gzip
import json
import os
import struct
import zlib

import numpy as np

PAYLOAD = 0xff00
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEXT = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DEXT = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "region_cases.json.gz")


def hashes(data):
    """h(p) for p <= n - 4."""
    a = np.frombuffer(data, dtype=np.uint8).astype(np.uint64)
    if len(a) < 4:
        return np.zeros(0, dtype=np.int64)
    le = a[:-3] | (a[1:-2] << np.uint64(8)) | (a[2:-1] << np.uint64(16)) | (a[3:] << np.uint64(24))
    return (((le * np.uint64(2654435761)) & np.uint64(0xffffffff)) >> np.uint64(17)).astype(np.int64)


def tokens(data):
    """The greedy parse of one block: an int per literal, (length, distance) per match."""
    n, h = len(data), hashes(data).tolist()
    cand, head = [-1] * n, {}
    for p, k in enumerate(h):
        cand[p] = head.get(k, -1)
        head[k] = p
    out, p = [], 0
    while p < n:
        q = cand[p]
        if q >= 0 and p - q <= 32768:
            cap, ln = min(258, n - p), 0
            while ln < cap and data[q + ln] == data[p + ln]:
                ln += 1
            if ln >= 4:
                out.append((ln, p - q))
                p += ln
                continue
        out.append(data[p])
        p += 1
    return out


class _Bits:
    def __init__(self):
        self.out, self.acc, self.n, self.total = bytearray(), 0, 0, 0

    def put(self, value, nbits):                                         # least significant bit first
        self.acc |= value << self.n
        self.n += nbits
        self.total += nbits
        while self.n >= 8:
            self.out.append(self.acc & 0xff)
            self.acc >>= 8
            self.n -= 8

    def huff(self, code, nbits):                                         # a Huffman code goes in from its most significant bit
        self.put(int(format(code, "0%db" % nbits)[::-1], 2), nbits)

    def symbol(self, s):
        if s < 144:
            self.huff(0x30 + s, 8)
        elif s < 256:
            self.huff(0x190 + s - 144, 9)
        elif s < 280:
            self.huff(s - 256, 7)
        else:
            self.huff(0xc0 + s - 280, 8)

    def done(self):
        if self.n:
            self.out.append(self.acc & 0xff)
        return bytes(self.out)


def fixed_huffman(toks):
    b = _Bits()
    b.put(1, 1)
    b.put(1, 2)
    for t in toks:
        if isinstance(t, int):
            b.symbol(t)
            continue
        ln, dist = t
        i = max(k for k in range(29) if LBASE[k] <= ln)
        b.symbol(257 + i)
        b.put(ln - LBASE[i], LEXT[i])
        j = max(k for k in range(30) if DBASE[k] <= dist)
        b.huff(j, 5)
        b.put(dist - DBASE[j], DEXT[j])
    b.symbol(256)
    return b.done()


def block(data, level):
    n = len(data)
    assert 0 < n <= PAYLOAD
    stored = b"\x01" + struct.pack("<HH", n, n ^ 0xffff) + data
    body = stored
    if level > 0:
        coded = fixed_huffman(tokens(data))
        if len(coded) < n + 5:
            body = coded
    total = 18 + len(body) + 8
    return (b"\x1f\x8b\x08\x04" + bytes(4) + b"\x00\xff" + struct.pack("<H", 6) + b"BC" + struct.pack("<HH", 2, total - 1) + body +
            struct.pack("<II", zlib.crc32(data), n))


_memo = {}


def compress(text, piece_off, level):
    """(bytes, piece_out_off, block sizes) of a text cut into pieces."""
    out, off, sizes = bytearray(), [], []
    for a, b in zip(piece_off[:-1], piece_off[1:]):
        off.append(len(out))
        for at in range(a, b, PAYLOAD):
            key = (bytes(text[at:min(b, at + PAYLOAD)]), level)
            if key not in _memo:
                _memo[key] = block(key[0], level)
            out += _memo[key]
            sizes.append(len(_memo[key]))
    off.append(len(out))
    return bytes(out), off, sizes


def golden_lines():
    with gzip.open(GOLDEN) as f:
        return [[ln.encode() for ln in c["lines"]] for c in json.load(f)]


def _pieces(parts):
    off = [0]
    for p in parts:
        off.append(off[-1] + len(p))
    return b"".join(parts), off


def _distance_case(dist, rng):
    """Four-letter filler around a 40-byte marker that comes back `dist` bytes later."""
    marker = bytes(rng.integers(33, 127, size=40, dtype=np.uint8))
    fill = lambda k: bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=k))
    return fill(700) + marker + fill(dist - 40) + marker + fill(900)


def _same_bucket_keys():
    """Two different 4-byte keys whose hashes agree."""
    seen = {}
    for v in range(1 << 20):
        k = struct.pack("<I", 0x41424300 + v * 7)
        h = int(hashes(k)[0])
        if h in seen and seen[h] != k:
            return seen[h], k
        seen[h] = k
    raise AssertionError("no two keys share a bucket")


def _near_threshold(rng, want):
    """A block whose fixed-Huffman size is n + 5 + want: bytes >= 144 cost 9 bits, bytes < 144 cost 8; all distinct enough not to match."""
    n = 4000
    n_high = 8 * (5 + want) - 10                                         # 3 + 8 n + n_high + 7 bits
    d = np.concatenate([rng.integers(144, 256, size=n_high, dtype=np.uint8), rng.integers(0, 144, size=n - n_high, dtype=np.uint8)])
    data = bytes(rng.permutation(d))
    assert len(fixed_huffman(tokens(data))) == n + 5 + want
    return data


_cases = None


def cases():
    """[(name, text, piece_off)]"""
    global _cases
    if _cases is not None:
        return _cases
    rng = np.random.default_rng(20260)
    out = [("no pieces", b"", [0])]
    out.append(("an empty piece between full ones",) + _pieces([b"first piece, first piece\n", b"", b"second piece second piece\n"]))
    out.append(("1, 3 and 4 bytes",) + _pieces([b"a", b"abc", b"abcd", b"aaaa", b"aaaaa"]))
    out.append(("runs of one byte",) + _pieces([b"x" * k for k in (258, 259, 260, 263)]))
    text = (b"chr20\t%d\t.\tA\tG\t30\tPASS\tDP=%d\n" * 4000) % tuple(range(8000))
    out.append(("exactly 0xff00 bytes",) + _pieces([text[:PAYLOAD]]))
    out.append(("0xff00 + 1 bytes",) + _pieces([text[:PAYLOAD + 1]]))
    out.append(("bytes 144-255 repeated",) + _pieces([bytes(range(144, 256)) * 40]))
    near, far = _distance_case(32768, rng), _distance_case(32769, rng)
    toks = tokens(near)
    assert any(not isinstance(t, int) and t[1] == 32768 and t[0] >= 40 for t in toks) and all(isinstance(t, int) or t[1] <= 32768 for t in toks)
    assert all(isinstance(t, int) or t[1] <= 32768 for t in tokens(far))
    out.append(("a marker at distance 32768 and one at 32769",) + _pieces([near, far]))
    k1, k2 = _same_bucket_keys()
    clash = k1 + b"...." + k2 + b"____" + k1 + b"~~~~" + k2
    assert int(hashes(k1)[0]) == int(hashes(k2)[0]) and all(isinstance(t, int) for t in tokens(clash))     # (each key's candidate is the other key)
    out.append(("two keys in one bucket",) + _pieces([clash]))
    noise = bytes(rng.integers(0, 256, size=PAYLOAD, dtype=np.uint8))
    assert len(block(noise, 1)) == 65311
    out.append(("0xff00 random bytes",) + _pieces([noise]))
    out.append(("either side of the stored threshold",) + _pieces([_near_threshold(rng, w) for w in (-2, -1, 0, 1)]))
    sizes = rng.integers(0, 301, size=1000)
    words = [b"0/1:", b"1/1:", b"0/0:", b"chr1\t", b"PASS\t", b"GT:GL:GQ:NR:NV\t", b".\t", b"\n"]
    many = [b"".join(words[i] for i in rng.integers(0, len(words), size=80))[:int(k)] for k in sizes]
    out.append(("1000 pieces of 0-300 bytes",) + _pieces(many))
    out.append(("the golden processes' record lines",) + _pieces([b"".join(ln + b"\n" for ln in lines) for lines in golden_lines()]))
    _cases = out
    return out


def parse_blocks(data):
    """[(offset, block length, ISIZE, CRC32)] of a BGZF byte string, every header field checked."""
    out, at = [], 0
    while at < len(data):
        assert data[at:at + 4] == b"\x1f\x8b\x08\x04" and data[at + 4:at + 10] == b"\x00\x00\x00\x00\x00\xff", at
        assert data[at + 10:at + 16] == b"\x06\x00BC\x02\x00", at
        total = struct.unpack_from("<H", data, at + 16)[0] + 1
        assert at + total <= len(data) and total >= 28
        crc, isize = struct.unpack_from("<II", data, at + total - 8)
        assert data[at + 18] & 1 == 1                                      # BFINAL on the one deflate block
        out.append((at, total, isize, crc))
        at += total
    return out


def check_stream(data, piece_out_off, text, piece_off):
    """What every producer's output must satisfy, whatever its bytes: gzip reads the text back, the blocks' fields are right, every piece
    begins at a block boundary and piece_out_off is the scan of the block sizes."""
    assert gzip.decompress(data) == text if data else text == b""
    blocks = parse_blocks(data)
    starts = [a for a, _, _, _ in blocks] + [len(data)]
    at = 0
    for i in range(len(piece_off) - 1):
        a, b = piece_off[i], piece_off[i + 1]
        assert piece_out_off[i] == starts[at], (i, piece_out_off[i], starts[at])
        for k in range(a, b, PAYLOAD):
            payload = text[k:min(b, k + PAYLOAD)]
            off, total, isize, crc = blocks[at]
            assert isize == len(payload) and crc == zlib.crc32(payload) and total <= len(payload) + 31
            assert zlib.decompress(data[off + 18:off + total - 8], -15) == payload
            at += 1
    assert at == len(blocks) and piece_out_off[-1] == len(data)
    return len(blocks)
