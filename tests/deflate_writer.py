"""An RFC 1951 ENCODER for tests whose every choice is a parameter: the tokens, the code lengths, the header's counts and the run-length
coding of the lengths, the sequence of blocks and the padding bits.  It writes the valid streams zlib's own encoder never writes (codes
of 15 bits on small alphabets, runs across the literal/distance boundary, empty blocks, stored blocks at every bit phase) and, with
check=False, the invalid ones.  It builds on BitWriter of tests/bgzf_cases.py and calls nothing under test: what a stream means is
decided by zlib (bgzf_cases.reference_verdict), never here.

As it writes, the writer RECORDS what it emitted (Records): the reach checks of tests/test_deflate_writer_cpu.py read these records,
not the decoder."""
from tests.bgzf_cases import BitWriter

import numpy as np

# RFC 1951, 3.2.5, restated
LBASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEXT = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DBASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577)
DEXT = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32


def length_symbol(length):
    """(symbol, extra) of a match length 3..258; 258 is symbol 285."""
    assert 3 <= length <= 258
    k = 28 if length == 258 else max(i for i in range(28) if LBASE[i] <= length)
    return 257 + k, length - LBASE[k]


def dist_symbol(dist):
    assert 1 <= dist <= 32768
    k = max(i for i in range(30) if DBASE[i] <= dist)
    return k, dist - DBASE[k]


_LSYM = [None] * 3 + [length_symbol(n) for n in range(3, 259)]


# ---- tokens ------------------------------------------------------------------------------------------------------------------------
# A token is a literal (an int), a match (length, distance), a match by its symbols (length symbol, extra, distance symbol, extra) -- for
# the encodings a matcher never chooses, such as 284 + 31 -- or a str of '0' / '1': bits written as they are (invalid streams only).
def token_span(t):
    if isinstance(t, int):
        return 1, 0
    if isinstance(t, str):
        return 0, 0
    if len(t) == 2:
        return t
    return LBASE[t[0] - 257] + t[1], DBASE[t[2]] + t[3]


def replay(tokens, out=None):
    """The bytes the tokens stand for (RFC 1951's copy rule, a byte at a time), appended to `out`."""
    out = bytearray() if out is None else out
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
            continue
        n, d = token_span(t)
        assert n == 0 or 1 <= d <= len(out), "a distance before the output's start"
        for _ in range(n):
            out.append(out[-d])
    return out


def match_tokens(data, max_dist=32768, min_len=3, max_len=258, cuts=()):
    """A small greedy matcher: the last position of every 3-byte key is the one candidate.  No match spans a position in `cuts` (where
    the caller starts another block).  replay(result) == data."""
    assert 1 <= max_dist <= 32768 and 3 <= min_len <= max_len <= 258
    data, n = bytes(data), len(data)
    cuts = sorted(set(cuts) | {n})
    table, tokens, i, ci = {}, [], 0, 0
    while i < n:
        while cuts[ci] <= i:
            ci += 1
        best, lim = 0, min(max_len, cuts[ci] - i)
        if i + 3 <= n:
            key = data[i:i + 3]
            cand = table.get(key)
            if cand is not None and i - cand <= max_dist and lim >= 3:
                ln = 3
                while ln < lim and data[cand + ln] == data[i + ln]:
                    ln += 1
                if ln >= min_len:
                    best, dist = ln, i - cand
            table[key] = i
        if best:
            tokens.append((best, dist))
            for k in range(i + 1, min(i + best, n - 2), 3):
                table[data[k:k + 3]] = k
            i += best
        else:
            tokens.append(data[i])
            i += 1
    return tokens


def split_tokens(tokens, cuts):
    """The token list cut where the output reaches each position of `cuts` (which match_tokens was given)."""
    parts, cur, at, cuts = [], [], 0, sorted(cuts)
    for t in tokens:
        while cuts and at >= cuts[0]:
            parts.append(cur)
            cur = []
            cuts.pop(0)
        cur.append(t)
        at += token_span(t)[0]
    parts.append(cur)
    parts += [[] for _ in cuts]
    return parts


# ---- codes -------------------------------------------------------------------------------------------------------------------------
def kraft(lengths, maxlen=15):
    """The code space the lengths take, in units of 2**-maxlen: 2**maxlen is a complete code."""
    return sum(1 << (maxlen - l) for l in lengths if l)


def check_code(lengths, kind):
    """A complete prefix code, or one of the incomplete ones RFC 1951 and zlib permit: a single one-bit code (literal/length and distance
    sets), no code at all (distance set)."""
    maxlen = 7 if kind == "cl" else 15
    used = [l for l in lengths if l]
    assert all(1 <= l <= maxlen for l in used), (kind, "a length outside 1..%d" % maxlen)
    if kraft(used, maxlen) == 1 << maxlen:
        return
    assert kind != "cl", "an incomplete code-length code"
    assert used == [1] or (kind == "dist" and not used), (kind, "neither complete nor a permitted incomplete code")


def canonical(lengths):
    """{symbol: code as a str of bits, first bit first} by RFC 1951, 3.2.2."""
    count = [0] * 17
    for l in lengths:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for bits in range(1, 17):
        code = (code + count[bits - 1]) << 1
        nxt[bits] = code
    out = {}
    for s, l in enumerate(lengths):
        if l:
            out[s] = format(nxt[l] & ((1 << l) - 1), "0%db" % l)
            nxt[l] += 1
    return out


def ladder_lengths(entries, size, maxlen=15):
    """A skewed code: the lengths Huffman's construction gives a Fibonacci-like frequency ladder (F(k), ..., 3, 2, 1, 1), that is
    1, 2, ..., k - 1, k - 1 for k entries, most frequent first; with maxlen + 1 entries every length 1..maxlen occurs.  An entry is a
    symbol, or a list of 2**m symbols that share its leaf as a flat subtree (m bits longer)."""
    k = len(entries)
    assert 2 <= k <= maxlen + 1
    lens = [0] * size
    for e, l in zip(entries, list(range(1, k)) + [k - 1]):
        group = list(e) if isinstance(e, (list, tuple)) else [e]
        m = len(group).bit_length() - 1
        assert len(group) == 1 << m and l + m <= maxlen
        for s in group:
            assert lens[s] == 0
            lens[s] = l + m
    return lens


def flat_lengths(symbols, size):
    """A flat code over `symbols` (two or more): lengths k and k + 1 only."""
    symbols = list(symbols)
    n = len(symbols)
    assert n >= 2
    k = n.bit_length() - 1
    short = (2 << k) - n                                   # this many codes of k bits, the others k + 1 (n a power of two: all k)
    lens = [0] * size
    for i, s in enumerate(symbols):
        lens[s] = k if i < short else k + 1
    return lens


def single_lengths(symbol, size):
    lens = [0] * size
    lens[symbol] = 1
    return lens


def random_lengths(rng, symbols, size, maxlen=15, deep=0.5):
    """A random complete code over `symbols` (two or more): a tree grown by splitting a leaf, the deepest one with probability `deep`."""
    symbols = list(symbols)
    assert 2 <= len(symbols) <= 1 << maxlen
    leaves = [1, 1]
    while len(leaves) < len(symbols):
        open_ = [i for i, d in enumerate(leaves) if d < maxlen]
        i = max(open_, key=lambda j: leaves[j]) if rng.random() < deep else open_[int(rng.integers(len(open_)))]
        leaves[i] += 1
        leaves.append(leaves[i])
    order = rng.permutation(len(symbols))
    lens = [0] * size
    for k, d in zip(order, leaves):
        lens[symbols[int(k)]] = d
    return lens


# ---- the header's run-length coding ------------------------------------------------------------------------------------------------
def rle_none(seq):
    return [(v, 1) for v in seq]


def rle_greedy(seq):
    """Maximal use of 18 / 17 for zeros and of 16 behind a first explicit length; runs do not stop at the literal/distance boundary."""
    ops, i = [], 0
    while i < len(seq):
        v, j = seq[i], i
        while j < len(seq) and seq[j] == v:
            j += 1
        run = j - i
        if v == 0:
            while run >= 11:
                r = min(run, 138)
                ops.append((18, r))
                run -= r
            if run >= 3:
                ops.append((17, run))
                run = 0
        else:
            ops.append((v, 1))
            run -= 1
            while run >= 3:
                r = min(run, 6)
                ops.append((16, r))
                run -= r
        ops += [(v, 1)] * run
        i = j
    return ops


def rle_random(seq, rng):
    """Every run coded by a random mix of explicit lengths and repeats of random size: an explicit list of (symbol, repeat)."""
    ops, i = [], 0
    while i < len(seq):
        v, j = seq[i], i
        while j < len(seq) and seq[j] == v:
            j += 1
        run = j - i
        if v and (i == 0 or seq[i - 1] != v):
            ops.append((v, 1))
            run -= 1
        while run:
            kinds = [(v, 1, 1)]
            if v == 0 and run >= 3:
                kinds.append((17, 3, min(run, 10)))
            if v == 0 and run >= 11:
                kinds.append((18, 11, min(run, 138)))
            if v and run >= 3:
                kinds.append((16, 3, min(run, 6)))
            s, lo, hi = kinds[int(rng.integers(len(kinds)))]
            r = int(rng.integers(lo, hi + 1))
            ops.append((s, r))
            run -= r
        i = j
    return ops


def rle_expand(ops):
    out = []
    for s, r in ops:
        if s < 16:
            out.append(s)
        elif s == 16:
            out += [out[-1]] * r
        else:
            out += [0] * r
    return out


# ---- what was written --------------------------------------------------------------------------------------------------------------
class Records:
    def __init__(self):
        self.lit_lens, self.dist_lens, self.cl_lens = set(), set(), set()        # code lengths of the symbols emitted
        self.len_syms, self.dist_syms = {}, {}                                    # symbol -> {"zero", "one"}: extra bits all zero / all one
        self.blocks = []                                                          # "stored" / "fixed" / "dynamic", in order
        self.stored_phases = []                                                   # bits written (mod 8) in front of each stored block's header
        self.rle_modes = set()                                                    # "none" / "greedy" / "explicit"
        self.cross16 = self.cross18 = 0                                           # repeats that start in the literal lengths and end in the distance lengths
        self.first_head_bits = None                                               # the first block's header (and code lengths): this many bits

    def merge(self, other):
        for name in ("lit_lens", "dist_lens", "cl_lens", "rle_modes"):
            getattr(self, name).update(getattr(other, name))
        for name in ("len_syms", "dist_syms"):
            for s, v in getattr(other, name).items():
                getattr(self, name).setdefault(s, set()).update(v)
        self.blocks += other.blocks
        self.stored_phases += other.stored_phases
        self.cross16 += other.cross16
        self.cross18 += other.cross18
        return self


def _extremes(extra, nbits):
    return ({"zero"} if extra == 0 else set()) | ({"one"} if extra == (1 << nbits) - 1 else set())


class DeflateWriter:
    """One deflate stream: any sequence of stored(), fixed() and dynamic() blocks, the last with final=True, then finish()."""

    def __init__(self):
        self.w = BitWriter()
        self.rec = Records()
        self.out = bytearray()                                                    # the payload, by replay()

    def _begin(self, kind, final):
        self.rec.blocks.append(kind)
        self.w.field(1 if final else 0, 1).field({"stored": 0, "fixed": 1, "dynamic": 2}[kind], 2)

    def _end_head(self):
        if self.rec.first_head_bits is None:
            self.rec.first_head_bits = len(self.w.bits)

    def raw(self, bits):
        self.w.code(bits)
        return self

    def stored(self, data, final=False, pad=0, length=None, nlen=None):
        """pad: the padding bits up to the byte boundary, as a number (LSB first); length / nlen: LEN and NLEN written wrong."""
        data = bytes(data)
        assert len(data) <= 65535
        self.rec.stored_phases.append(len(self.w.bits) % 8)
        self._begin("stored", final)
        self.w.field(pad, -len(self.w.bits) % 8)
        ln = len(data) if length is None else length
        self.w.field(ln, 16).field(ln ^ 0xffff if nlen is None else nlen, 16)
        self._end_head()
        self.w.bits += np.unpackbits(np.frombuffer(data, dtype=np.uint8), bitorder="little").tolist()
        self.out += data
        return self

    def _tokens(self, tokens, lit_lens, dist_lens, end):
        lc, dc, rec, bits = canonical(lit_lens), canonical(dist_lens), self.rec, self.w.bits
        for t in list(tokens) + ([256] if end else []):
            if isinstance(t, str):
                self.w.code(t)
            elif isinstance(t, int):
                bits += map(int, lc[t])
                rec.lit_lens.add(lit_lens[t])
            else:
                ls, le, ds, de = t if len(t) == 4 else _LSYM[t[0]] + dist_symbol(t[1])
                assert 0 <= le < 1 << LEXT[ls - 257] and 0 <= de < 1 << DEXT[ds]
                bits += map(int, lc[ls])
                self.w.field(le, LEXT[ls - 257])
                bits += map(int, dc[ds])
                self.w.field(de, DEXT[ds])
                rec.lit_lens.add(lit_lens[ls])
                rec.dist_lens.add(dist_lens[ds])
                rec.len_syms.setdefault(ls, set()).update(_extremes(le, LEXT[ls - 257]))
                rec.dist_syms.setdefault(ds, set()).update(_extremes(de, DEXT[ds]))
        replay([t for t in tokens if not isinstance(t, str)], self.out)

    def fixed(self, tokens, final=False, end=True):
        self._begin("fixed", final)
        self._end_head()
        self._tokens(tokens, FIXED_LIT, FIXED_DIST, end)
        return self

    def dynamic(self, tokens, lit_lens, dist_lens, final=False, hlit=None, hdist=None, hclen=None, cl_lens=None, rle="greedy", check=True, end=True):
        """lit_lens / dist_lens: code lengths by symbol (trailing zeros may be left out).  hlit / hdist / hclen: the header's counts
        (default: the smallest that hold the lengths), padded with zero lengths.  cl_lens: the code-length code's 19 lengths (default: a
        flat code over the symbols the run-length coding uses).  rle: "none", "greedy" or a list of (symbol, repeat) -- a length 0..15
        (repeat 1), 16 (3..6), 17 (3..10) or 18 (11..138).  check=False writes what it is told, valid or not."""
        lit, dist = list(lit_lens), list(dist_lens)
        top = lambda a, least: max([least] + [i + 1 for i, l in enumerate(a) if l])
        nl = top(lit, 257) if hlit is None else hlit + 257
        nd = top(dist, 1) if hdist is None else hdist + 1
        if check:
            assert 257 <= nl <= 286 and 1 <= nd <= 30 and nl >= top(lit, 257) and nd >= top(dist, 1)
            check_code(lit, "lit")
            check_code(dist, "dist")
            assert lit[256] if len(lit) > 256 else False, "no code for 256"
        lit, dist = (lit + [0] * 288)[:max(nl, 288)], (dist + [0] * 32)[:max(nd, 32)]
        seq = lit[:nl] + dist[:nd]
        ops = rle_none(seq) if rle == "none" else rle_greedy(seq) if rle == "greedy" else list(rle)
        self.rec.rle_modes.add(rle if isinstance(rle, str) else "explicit")
        if check:
            assert rle_expand(ops) == seq, "the run-length coding does not give the lengths"
            assert all(r == 1 if s < 16 else 3 <= r <= 6 if s == 16 else 3 <= r <= 10 if s == 17 else 11 <= r <= 138 for s, r in ops)
        if cl_lens is None:
            used = sorted({s for s, _ in ops})
            cl_lens = flat_lengths(used if len(used) > 1 else used + [(used[0] + 1) % 19], 19)
        cl_lens = list(cl_lens)
        need = max([4] + [i + 1 for i, s in enumerate(CL_ORDER) if cl_lens[s]])
        n_cl = need if hclen is None else hclen + 4
        if check:
            check_code(cl_lens, "cl")
            assert need <= n_cl <= 19
        self._begin("dynamic", final)
        self.w.field(nl - 257, 5).field(nd - 1, 5).field(n_cl - 4, 4)
        for s in CL_ORDER[:n_cl]:
            self.w.field(cl_lens[s], 3)
        cc, at = canonical(cl_lens), 0
        for s, r in ops:
            self.w.code(cc[s])
            self.rec.cl_lens.add(cl_lens[s])
            if s >= 16:
                self.w.field(r - (11 if s == 18 else 3), 7 if s == 18 else 3 if s == 17 else 2)
                if at < nl < at + r:
                    self.rec.cross16 += s == 16
                    self.rec.cross18 += s == 18
            at += 1 if s < 16 else r
        self._end_head()
        self._tokens(tokens, lit, dist, end)
        return self

    def finish(self, pad=0):
        """The stream's bytes; pad: the bits behind the last block up to the byte boundary, as a number."""
        self.w.field(pad, -len(self.w.bits) % 8)
        return self.w.bytes()


def token_bits(t, lit_lens=FIXED_LIT, dist_lens=FIXED_DIST):
    """A token's bits as a str in stream order, for what replay() refuses to write: a match that reaches before the output's start."""
    w = DeflateWriter()
    w.out += bytes(32768)
    w._tokens([t], list(lit_lens), list(dist_lens), False)
    return "".join(map(str, w.w.bits))


def used_symbols(tokens):
    """(literal/length symbols, distance symbols) the tokens need, 256 included."""
    ls, ds = {256}, set()
    for t in tokens:
        if isinstance(t, int):
            ls.add(t)
        elif not isinstance(t, str):
            a, _, d, _ = t if len(t) == 4 else _LSYM[t[0]] + dist_symbol(t[1])
            ls.add(a)
            ds.add(d)
    return sorted(ls), sorted(ds)
