"""Cases shared by tests/test_bgzf_deflate_cpu.py (the host twin, csrc/bgzf_deflate.hpp) and tests/test_gpu_bgzf_deflate.py (the device,
plat_bgzf_deflate_batch), and a restatement in Python of the encoding rule include/platypus_mi355x.h states: pieces cut into blocks of 0xff00
bytes, level 0 stored, level 1 one-candidate LZ77 (15-bit multiplicative hash of four bytes, nearest earlier position with the same hash, every
position inserted, greedy parse) coded with the fixed Huffman codes of RFC 1951, stored instead when that is no shorter.  The restatement
looks codes up in the RFC's tables; the C++ computes them.  Behind the 13 cases of cases() come the seams of the device's block kernel:
reach() says from the restatement alone what a block puts in front of each phase, seam_blocks() holds a named case per seam, seam_fuzz()
seeded blocks, batch_cases() calls for the kernels around the block kernel (tests/test_gpu_bgzf_deflate_seams.py runs them on the device)."""
import bisect
import collections
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


def parse(data):
    """The greedy parse of one block with what led to it: (the hash of every position that has one, per position the candidate or -1, the
    tokens -- an int per literal, (length, distance) per match --, the tokens' positions)."""
    n, h = len(data), hashes(data).tolist()
    cand, head = [-1] * n, {}
    for p, k in enumerate(h):
        cand[p] = head.get(k, -1)
        head[k] = p
    out, pos, p = [], [], 0
    while p < n:
        pos.append(p)
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
    return h, cand, out, pos


def tokens(data):
    """The greedy parse of one block: an int per literal, (length, distance) per match."""
    return parse(data)[2]


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


def _same_bucket_keys(count=2):
    """`count` different 4-byte keys whose hashes agree."""
    seen = {}
    for v in range(1 << 20):
        k = struct.pack("<I", 0x41424300 + v * 7)
        group = seen.setdefault(int(hashes(k)[0]), [])
        group.append(k)
        if len(group) == count:
            return tuple(group)
    raise AssertionError("no %d keys share a bucket" % count)


def _near_threshold(rng, want, n=4000, least=False):
    """A block whose fixed-Huffman size is n + 5 + want: bytes >= 144 cost 9 bits, bytes < 144 cost 8; all distinct enough not to match.
    `least`: with the fewest bytes >= 144 that give that size (n + 4 needs 15 of them, n + 5 needs 23), else the most."""
    n_high = 8 * (5 + want) - (17 if least else 10)                     # 3 + 8 n + n_high + 7 bits
    assert 0 <= n_high <= n
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


# ---- the seams of the device's block kernel (plat_bgzfout.hip): what a block reaches, from the restatement alone, and the cases built to reach it

TILE, SEG = 64, 252                                                      # positions per sort tile and per thread of phase C; per chain segment
EDGE_LENGTHS = tuple(range(4, 13)) + (255, 256, 257, 258)
_LSYM_BITS = [7 if 257 + i < 280 else 8 for i in range(29)]


def code_bits(t):
    """Bits of a token's fixed-Huffman code, from the RFC's tables."""
    if isinstance(t, int):
        return 8 if t < 144 else 9
    i, j = bisect.bisect_right(LBASE, t[0]) - 1, bisect.bisect_right(DBASE, t[1]) - 1
    return _LSYM_BITS[i] + LEXT[i] + 5 + DEXT[j]


_reach = {}


def reach(data):
    """A Counter of what the block `data` puts in front of the device kernel's phases (keys in words, as the seam cases and the tally name them), memoised per block."""
    data = bytes(data)
    if data in _reach:
        return _reach[data]
    n = len(data)
    h, cand, toks, pos = parse(data)
    c = collections.Counter()
    first = {}                                                           # per hash its first position
    for t0 in range(0, len(h), TILE):
        group = {}
        for p in range(t0, min(len(h), t0 + TILE)):
            group.setdefault(h[p], []).append(p)
            first.setdefault(h[p], p)
        for ps in group.values():
            if len(ps) >= 3:
                same = len({data[p:p + 4] for p in ps}) == 1
                for m in range(3, min(len(ps), 4) + 1):
                    c["%d positions of one hash in a tile, %s" % (m, "one key" if same else "keys differ")] += 1
    if 0 in first:
        c["hash 0"] += 1
    if 0x7fff in first:
        c["hash 0x7fff"] += 1
    at = 3
    for t, p in zip(toks, pos):
        nb = code_bits(t)
        if nb >= 28:
            c["a code of 28+ bits at bit %d" % (at & 31)] += 1
            c["a code of %d bits at bit %d" % (nb, at & 31)] += 1
        at += nb
        if p % SEG == SEG - 1:
            c["a chain position on a segment's last position"] += 1
        q = cand[p]
        if isinstance(t, int):
            if q >= 0 and n - p >= 4:
                same = 0
                while same < 4 and data[q + same] == data[p + same]:
                    same += 1
                if p - q <= 32768 and same < 4:
                    c["a candidate of another key that agrees in %d bytes" % same] += 1
                if p - q == 32769 and same == 4:
                    c["a candidate at distance 32769 refused"] += 1
            continue
        ln, dist = t
        assert q == p - dist
        back = p // TILE - q // TILE
        c["a candidate %s back" % ("in the tile" if back == 0 else "%d tiles" % back if back < 6 else "6+ tiles")] += 1
        if back == 0 and first[h[p]] < p - p % TILE:
            c["a candidate in the tile, an older one in the table"] += 1
        if back == 1 and q % TILE == TILE - 1 and p % TILE == 0:
            c["a candidate on lane 63, its next on lane 0"] += 1
        if h[p] in (0, 0x7fff):
            c["a match of hash %s" % ("0" if h[p] == 0 else "0x7fff")] += 1
        end = p + ln == n
        if ln in EDGE_LENGTHS:
            c["a match of %d at (%d, %d) ended by %s" % (ln, p & 3, q & 3, "the block" if end else "a byte")] += 1
        c["a match at (%d, %d)" % (p & 3, q & 3)] += 1
        if end and ln <= 7:
            c["a cap of %d" % ln] += 1
        if ln == 258 and p + 258 < n and data[q + 258] == data[p + 258]:
            c["a run longer than 258"] += 1
        if q == 0:
            c["a candidate at position 0"] += 1
        if p == PAYLOAD - 4:
            c["a match at 0xff00 - 4"] += 1
        if dist in (1, 2, 3, 4, 32767, 32768):
            c["distance %d" % dist] += 1
        if p // SEG != (p + ln) // SEG:
            c["a match across a segment edge"] += 1
        if (p + ln) % SEG == 0 and p + ln < n:
            c["a match whose next position is a segment's first"] += 1
        if p % SEG == SEG - 1:
            c["a match on a segment's last position"] += 1
    have = {p // SEG for p in pos}
    c["a segment without a chain position in front of more chain"] += sum(1 for s in range(max(have)) if s not in have)
    c["a segment without a chain position"] += (n + SEG - 1) // SEG - len(have)
    per = collections.Counter(p // TILE for p in pos)
    threads = (n + TILE - 1) // TILE
    literals = collections.Counter(p // TILE for t, p in zip(toks, pos) if isinstance(t, int))
    for t in range(threads):
        if per[t] == TILE and ((t > 0 and per[t - 1] == 0) or (t + 1 < threads and per[t + 1] == 0)):
            c["a thread of 64 chain positions next to one of none"] += 1
            c["a thread of 64 literals next to one of none"] += literals[t] == TILE
        c["a thread of 64 chain positions"] += per[t] == TILE
        c["a thread of no chain position"] += per[t] == 0
    chain = set(pos)
    for t in (t for t, k in per.items() if k == 2):
        if TILE * t in chain and TILE * t + TILE - 1 in chain:
            c["a thread whose chain is bits 0 and 63 alone"] += 1
    coded = (at + 7 + 7) >> 3
    assert coded == len(fixed_huffman(toks))
    if coded >= n + 5:
        c["stored at level 1, body & 3 == %d" % ((n + 5) & 3)] += 1
        if coded == n + 5:
            c["stored at n + 5, n = %d" % n] += 1
    else:
        c["coded, body & 3 == %d" % (coded & 3)] += 1
        if coded == n + 4:
            c["coded at n + 4, n = %d" % n] += 1
    c["full blocks"] += n == PAYLOAD
    _reach[data] = +c
    return _reach[data]


def case_reach(text, piece_off):
    """reach() summed over the blocks of a case, and what depends on where a block lies: its length and its text offset's low bits."""
    c = collections.Counter()
    for a, b in zip(piece_off[:-1], piece_off[1:]):
        c["empty pieces"] += a == b
        c["pieces of 3+ blocks"] += b - a > 2 * PAYLOAD
        for at in range(a, b, PAYLOAD):
            d = text[at:min(b, at + PAYLOAD)]
            c.update(reach(d))
            if len(d) <= 9 or len(d) == 5000:
                c["text offset & 3 == %d, n = %d" % (at & 3, len(d))] += 1
            if len(d) <= 600:
                c["n = %d" % len(d)] += 1
    c["pieces"] += len(piece_off) - 1
    return c


def _fill(rng, k, hi=144):
    """k random bytes that cost 8 bits each as literals (a block of them is coded, not stored) and hardly ever match."""
    return bytes(rng.integers(0, hi, size=k, dtype=np.uint8))


def _letters(rng, k, alphabet=b"ACGT"):
    return bytes(rng.choice(np.frombuffer(alphabet, dtype=np.uint8), size=k))


def _key_with_hash(want):
    le = np.arange(0x30313233, 0x30313233 + (1 << 22), dtype=np.uint64)
    hv = ((le * np.uint64(2654435761)) & np.uint64(0xffffffff)) >> np.uint64(17)
    k = struct.pack("<I", int(le[np.flatnonzero(hv == want)[0]]))
    assert int(hashes(k)[0]) == want
    return k


def _prefix2_keys():
    """Two keys of one hash that agree in their first two bytes.  (Three cannot: the fourth byte alone moves the hash's top eight bits, the
    multiplier being odd.)"""
    for prefix in range(0x4142, 0x4142 + 4096):
        seen = {}
        for b23 in range(65536):
            k = struct.pack("<I", prefix | (b23 << 16))
            hv = int(hashes(k)[0])
            if hv in seen:
                return seen[hv], k
            seen[hv] = k
    raise AssertionError("no such keys")


def _at(rng, placed, n):
    """Filler of n bytes with the strings of `placed` {position: bytes} written over it."""
    d = bytearray(_fill(rng, n))
    for p, s in placed.items():
        assert p + len(s) <= n
        d[p:p + len(s)] = s
    return bytes(d)


def _edge_unit(rng, have, pp, qq, ln, to_end):
    """Bytes to append to a block of `have` bytes: a string of ln bytes at a position q with q & 3 == qq, and again at p, p & 3 == pp,
    followed by another byte than the first time, or by nothing."""
    m = bytes(rng.integers(160, 256, size=ln, dtype=np.uint8))            # (filler is < 144: nothing else matches it)
    out = _fill(rng, 3 + (qq - have - 4) % 4) + b"\x92" + m + b"\x90"                          # (0x92, 0x93: the match does not begin a byte early)
    out += _fill(rng, 7 + (pp - have - len(out) - 8) % 4) + b"\x93" + m
    return out if to_end else out + b"\x91"


SEAM_REACH = {}                                                          # case name -> the reach keys it is there for
_seam_blocks = None


def seam_blocks():
    """[(name, text, piece_off)]: one seam of the block kernel each; SEAM_REACH says which."""
    global _seam_blocks
    if _seam_blocks is not None:
        return _seam_blocks
    out = []

    def add(name, parts, *keys):
        assert name not in SEAM_REACH
        SEAM_REACH[name] = list(keys)
        out.append((name,) + _pieces(parts))
    rng = np.random.default_rng(20261)
    # -- tiles (A1, A2)
    keys4 = _same_bucket_keys(4)
    for m in (3, 4):
        add("%d positions of one key in one tile" % m, [_at(rng, {64 + 2 + 15 * j: keys4[0] for j in range(m)}, 200)],
            "%d positions of one hash in a tile, one key" % m)
        add("%d positions of two keys of one hash in one tile" % m, [_at(rng, {64 + 2 + 15 * j: keys4[j & 1] for j in range(m)}, 200)],
            "%d positions of one hash in a tile, keys differ" % m)
    add("4 positions of four keys of one hash in one tile", [_at(rng, {64 + 2 + 15 * j: keys4[j] for j in range(4)}, 200)],
        "4 positions of one hash in a tile, keys differ")
    for hv, word in ((0, "0"), (0x7fff, "0x7fff")):
        k = _key_with_hash(hv)
        add("a key of hash " + word, [_at(rng, {30: k, 100: k, 300: k}, 400)], "hash " + word, "a match of hash " + word)
    add("a key on lane 63 and on lane 0 of the next tile", [_at(rng, {127: b"\xa5" * 5}, 300)], "a candidate on lane 63, its next on lane 0", "distance 1")
    mark = bytes(range(200, 208))
    for back in (1, 3, 4, 5):
        add("a candidate %d tiles back" % back, [_at(rng, {64 * 2 + 50: mark, 64 * (2 + back) + 3: mark}, 64 * (4 + back))],
            "a candidate %d tiles back" % back)
    add("a candidate in the tile and an older one in the table", [_at(rng, {10: mark, 64 * 3 + 5: mark, 64 * 3 + 40: mark}, 400)],
        "a candidate in the tile, an older one in the table", "a candidate 3 tiles back")
    sizes = [64 * k + r for k in (0, 1, 4, 5) for r in (1, 3, 4, 5, 63, 64)]
    add("blocks of 64 k + {1, 3, 4, 5, 63, 64} bytes", [_letters(rng, k) for k in sizes], *["n = %d" % k for k in sizes])
    # -- the match compare (A3)
    for pp in range(4):
        for qq in range(4):
            text = b""
            for ln in EDGE_LENGTHS:
                text += _edge_unit(rng, len(text), pp, qq, ln, False)
            add("matches at (%d, %d) ended by a byte" % (pp, qq), [text],
                *["a match of %d at (%d, %d) ended by a byte" % (ln, pp, qq) for ln in EDGE_LENGTHS])
            add("matches at (%d, %d) ended by the block" % (pp, qq), [_edge_unit(rng, 0, pp, qq, ln, True) for ln in EDGE_LENGTHS],
                *(["a match of %d at (%d, %d) ended by the block" % (ln, pp, qq) for ln in EDGE_LENGTHS] + ["a cap of %d" % c for c in (4, 5, 6, 7)]))
    long_mark = bytes(rng.integers(160, 256, size=300, dtype=np.uint8))
    add("a run longer than 258", [_at(rng, {20: long_mark, 400: long_mark}, 800)], "a run longer than 258")
    k1, k2 = _prefix2_keys()
    assert k1[:2] == k2[:2] and k1 != k2 and int(hashes(k1)[0]) == int(hashes(k2)[0])
    add("two keys of one hash that share two bytes", [_at(rng, {20: k1, 90: k2, 130: k1, 170: k2}, 300)], "a candidate of another key that agrees in 2 bytes")
    add("a candidate at position 0", [_at(rng, {0: mark, 150: mark}, 300)], "a candidate at position 0")
    add("a candidate for the last hashed position of a full block", [_at(rng, {PAYLOAD - 1000: mark[:4], PAYLOAD - 4: mark[:4]}, PAYLOAD)],
        "a match at 0xff00 - 4", "a cap of 4", "full blocks")
    add("runs of period 1, 2, 3, 4", [_fill(rng, 30) + bytes(range(170, 170 + k)) * 100 + _fill(rng, 30) for k in (1, 2, 3, 4)],
        *["distance %d" % k for k in (1, 2, 3, 4)])
    add("markers at distance 32767, 32768, 32769", [_distance_case(d, rng) for d in (32767, 32768, 32769)],
        "distance 32767", "distance 32768", "a candidate at distance 32769 refused")
    # -- the chain (B)
    gap = "a segment without a chain position in front of more chain"
    for period in (1, 7, 112):
        unit = bytes(rng.permutation(np.arange(100, 100 + period, dtype=np.uint8)))
        add("20 000 bytes of period %d, then 3 000 of four letters" % period, [(unit * 20000)[:20000] + _letters(rng, 3000)], gap)
    m20 = bytes(range(180, 200))
    add("a match whose next position is a segment's first", [_at(rng, {30: m20, 2 * SEG - 20: m20}, 700)], "a match whose next position is a segment's first")
    add("a match on a segment's last position", [_at(rng, {30: m20, 2 * SEG - 1: m20}, 700)],
        "a match on a segment's last position", "a chain position on a segment's last position", "a match across a segment edge")
    add("blocks of 251, 252, 253, 504, 505 bytes", [_letters(rng, k) for k in (251, 252, 253, 504, 505)], *["n = %d" % k for k in (251, 252, 253, 504, 505)])
    runs = b"".join((bytes(rng.permutation(np.arange(100, 100 + period, dtype=np.uint8))) * 20000)[:20000] for period in (1, 7, 112))
    add("a full block of runs", [runs + _letters(rng, PAYLOAD - len(runs))], gap, "full blocks")
    # -- the packing (C)
    # 40 matches of 140 bytes (8 + 5 bits) at distances past 16384 (5 + 13 bits) one behind the other: each begins one bit earlier in its word
    # than the one before.  A match begins where the key's hash has no later position in front of it.
    src = _fill(rng, 9000)
    wide, s = src + _fill(rng, 16500), 0
    for _ in range(40):
        hv = hashes(wide).tolist()
        last = {k: p for p, k in enumerate(hv)}
        while last[hv[s]] != s:
            s += 1
        wide += src[s:s + 140]
        s += 150
    add("codes of 31 bits at every bit of a word", [wide], "a code of 31 bits at bit 31", *["a code of 28+ bits at bit %d" % k for k in range(32)])
    m70 = bytes(rng.integers(160, 256, size=70, dtype=np.uint8))
    add("a thread of 63 literals and a match next to a thread of none", [_at(rng, {10: m70, 64 * 4 - 1: m70}, 500)], "a thread of 64 chain positions next to one of none")
    add("a thread of none in front of a thread of 64 literals", [_at(rng, {10: m70 + b"\x90", 64 * 4 - 70: m70 + b"\x91"}, 500)],
        "a thread of 64 literals next to one of none")
    add("a thread whose chain is bits 0 and 63", [_at(rng, {10: m70[:63] + b"\x90", 64 * 3: m70[:63] + b"\x91"}, 500)], "a thread whose chain is bits 0 and 63 alone")
    parts, keys = [], []
    for n, wants in ((15, (-1,)), (23, (-1, 0)), (24, (-1, 0)), (64, (-1, 0)), (4000, (-1, 0))):
        for w in wants:
            parts.append(_near_threshold(rng, w, n, least=n < 64))
            keys.append(("coded at n + 4, n = %d" if w < 0 else "stored at n + 5, n = %d") % n)
    parts += [bytes(rng.integers(144, 256, size=n, dtype=np.uint8)) for n in (5, 6, 7, 8, 23, 24, 25, 26)]      # 9 bits a byte: the longest code n bytes can have
    parts += [bytes(rng.integers(0, 256, size=n, dtype=np.uint8)) for n in (300, 301, 302, 303)]
    parts += [_fill(rng, n) for n in (30, 31, 32, 33)]
    add("either side of the stored threshold at 15 to 4000 bytes", parts,
        *(keys + ["stored at level 1, body & 3 == %d" % r for r in range(4)] + ["coded, body & 3 == %d" % r for r in range(4)]))
    # -- the staging
    parts, at = [], 0
    for n in range(1, 10):
        for o in range(4):
            if (o - at) & 3:
                parts.append(_fill(rng, (o - at) & 3, 256))
                at += len(parts[-1])
            parts.append(_fill(rng, n, 256) if n < 8 else _letters(rng, 4) * 2 + _fill(rng, n - 8))
            at += n
    add("1 to 9 bytes at every text offset & 3", parts, *["text offset & 3 == %d, n = %d" % (o, n) for n in range(1, 10) for o in range(4)])
    parts = []
    for o in range(4):
        parts += [_fill(rng, 1 if o else 4, 256), _letters(rng, 5000, b"ACGT\t\n01/:.")]
    add("5 000 bytes at every text offset & 3", parts, *["text offset & 3 == %d, n = 5000" % o for o in range(4)])
    _seam_blocks = out
    return out


_seam_fuzz = {}


def seam_fuzz(seed=20262):
    """[(name, text, piece_off)]: about 300 seeded blocks of 1..6000 bytes and a few of 0xff00 -- alphabets of 2, 4, 20 and 256 letters, planted
    repeats of 3..600 bytes at distances 1..40 000, runs, VCF-like lines and bytes >= 144 mixed in --, each cut into 1..40 pieces."""
    if seed in _seam_fuzz:
        return _seam_fuzz[seed]
    rng = np.random.default_rng(seed)
    words = [b"0/1:", b"1/1:", b"chr20\t", b"PASS\t", b"GT:GL:GQ:NR:NV\t", b".\t", b"\n", b"-12.5,-3.01,0:", b"DP=", b"99"]
    out = []
    for i in range(300):
        full = i % 75 == 7
        n = PAYLOAD if full else int(rng.integers(1, 6001)) if i % 3 else int(rng.integers(1, 400))
        letters = (2, 4, 20, 256)[int(rng.integers(0, 4))]
        d = bytearray(rng.integers(0, letters, size=n, dtype=np.uint8) + (0 if letters == 256 else 65))
        for _ in range(int(rng.integers(0, 4 + n // 150))):
            kind, p = int(rng.integers(0, 10)), int(rng.integers(0, n))
            ln = min(n - p, int(rng.integers(3, 601)) if kind == 0 else int(rng.integers(3, 40)))
            if kind <= 5 and p > 0:                                          # a repeat (one that overlaps itself is a run of that period)
                dist = min(p, int(rng.integers(1, 40001)) if kind < 3 else int(rng.integers(1, 300)))
                for k in range(ln):
                    d[p + k] = d[p + k - dist]
            elif kind == 6:
                d[p:p + ln] = bytes([int(rng.integers(0, 256))]) * ln
            elif kind == 7:
                d[p:p + ln] = b"".join(words[j] for j in rng.integers(0, len(words), size=12))[:ln]
            else:
                d[p:p + ln] = bytes(rng.integers(144, 256, size=ln, dtype=np.uint8))
        pieces = 1 if full and i < 150 else int(rng.integers(1, 41))
        off = [0] + sorted(int(x) for x in rng.integers(0, n + 1, size=pieces - 1)) + [n]
        out.append(("fuzz %d: %d bytes, %d letters, %d pieces" % (i, n, letters, pieces), bytes(d), off))
    _seam_fuzz[seed] = out
    return out


BATCH_HEAD = (b"GATTACA" * 19)[:128]
LONG_PIECE = 3000                                                        # a piece of batch_cases()' first case is this long at least, or 70 bytes at most
_batch_cases = None


def batch_cases():
    """[(name, text, piece_off)]: calls that exercise the kernels around the block kernel (the plan, the grid-stride loop and its bisection,
    the scan, the copy)."""
    global _batch_cases
    if _batch_cases is not None:
        return _batch_cases
    rng = np.random.default_rng(20263)
    words = [b"0/1:", b"1/1:", b"0/0:", b"chr1\t", b"PASS\t", b"GT:GL:GQ:NR:NV\t", b".\t", b"\n"]
    line = lambda k: b"".join(words[i] for i in rng.integers(0, len(words), size=k))
    # every piece begins with the same 128 bytes of period 7: a short piece is what a long one goes on with behind the short one's length
    start = BATCH_HEAD
    parts = []
    for i in range(1100):
        if rng.integers(0, 5) == 0:
            unit = line(int(rng.integers(20, 60)))
            k = int(rng.integers(LONG_PIECE, 9001))
            parts.append((start + unit * (k // len(unit) + 1))[:k])
        else:
            parts.append(start[:int(rng.integers(1, 71))])
    out = [("1100 pieces, long ones of 3000-9000 bytes among short ones of 1-70",) + _pieces(parts)]
    small = lambda: line(20)[:int(rng.integers(1, 200))]
    parts = [small() for _ in range(300)]
    unit = line(400)
    parts[100:100] = [(unit * 500)[:3 * PAYLOAD + 17]]
    parts[201:201] = [(unit[::-1] * 400)[:2 * PAYLOAD]]
    out.append(("pieces of 3 x 0xff00 + 17 and of 2 x 0xff00 bytes among 300 small ones",) + _pieces(parts))
    parts = [b""] * 5 + [small(), b"", small()] + [b""] * 5 + [small(), small()] + [b""] * 5 + [small()] + [b""] * 5
    out.append(("empty pieces at the front, at the end and in runs of 5",) + _pieces(parts))
    pool = line(2000)
    parts = [pool[a:a + k] for a, k in zip(rng.integers(0, len(pool) - 40, size=9000).tolist(), rng.integers(0, 41, size=9000).tolist())]
    out.append(("9000 pieces of 0-40 bytes",) + _pieces(parts))
    out.append(("5000 pieces of one byte",) + _pieces([bytes([b]) for b in rng.integers(0, 256, size=5000).tolist()]))
    _batch_cases = out
    return out
