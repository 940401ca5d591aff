"""Helper of the index query tests (not a test module): the fixture (tests/golden/index_query_cases.json.gz: .tbi files the reference's
indexer wrote, queries and the chunk lists its ti_iter_query returned -- gen_golden_index_query.py writes it from the texts made here),
the flat tables of an index as csrc/index_query.hpp makes them (flat_of, a plain-Python mirror of its flatten), hand-made indexes for the
corners the reference's indexer never writes, serialised to .tbi and .bai bytes, and a BAI built from synthetic records.  The oracle of
the hand-made cases is platypus_amd.tabixindex.TabixIndex.query, which the fixture pins to the reference first."""
import base64
import gzip
import json
import os
import random
import struct

from platypus_amd import tabixindex

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "index_query_cases.json.gz")
MAX_CHUNKS = 2048                                         # PLAT_IDXQ_MAX_CHUNKS
PSEUDO_BIN = 37450
HEADER = b"##fileformat=VCFv4.1\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n"


# ---- the fixture's inputs -----------------------------------------------------------------------------------------------------------
def vcf_line(chrom, pos, end=None):
    return b"\t".join([chrom, b"%d" % pos, b".", b"A", b"<DEL>" if end else b"C", b".", b".", b"END=%d" % end if end else b"."]) + b"\n"


def fixture_texts():
    """[(label, payload, text)]: VCFs whose indexes have many chunks per bin and full parent bins.  Block payloads of a few lines, so that
    the indexer's merge of chunks that meet in one block joins little."""
    out = []
    # "wide": a record every 20 kb over 24 Mb, a long END= record (100 kb .. 3 Mb: levels 4 .. 2) behind every fourth, so that parent bins
    # hold many separate chunks; the whole contig gathers about 1500 chunks.  Then a short second contig and a third with one record.
    t, rng = HEADER, random.Random(5)
    for i in range(1200):
        pos = 1000 + 20000 * i
        t += vcf_line(b"1", pos)
        if i % 4 == 3:
            t += vcf_line(b"1", pos + 7, end=pos + rng.choice((100000, 130000, 1000000, 3000000)))
    for i in range(40):
        t += vcf_line(b"2", 500 + 3000 * i)
    t += vcf_line(b"3", 70000)
    out.append(("wide", 120, t))
    # "dense": a record every 700 bases over 1.2 Mb with an END= record of 20 .. 150 kb behind every third: a 100 kb window touches about 13
    # bins and gathers 10 .. 30 chunks, one of 450 kb gathers 60 .. 70
    t, rng = HEADER, random.Random(6)
    for i in range(1700):
        pos = 200 + 700 * i
        t += vcf_line(b"chrD", pos)
        if i % 3 == 2:
            t += vcf_line(b"chrD", pos + 1, end=pos + rng.choice((20000, 60000, 150000)))
    out.append(("dense", 2000, t))
    return out


def fixture_queries(label, index):
    """[(tid, beg, end)] for one fixture file: the corners the issue lists."""
    q = []
    if label == "wide":
        n_lin = len(index.linear[0])
        q += [(0, 0, 500), (0, 5000, 5000), (0, 5000, 4000), (0, -100, 30000), (0, 23000000, (1 << 29) + 5), (0, 0, (1 << 30)),
              (0, (n_lin - 1) << 14, (n_lin << 14) + 10), (0, n_lin << 14, (n_lin << 14) + 100000), (0, (n_lin + 50) << 14, 1 << 29),
              (0, 16384 * 100, 16384 * 101), (0, 16384 * 100 + 5, 16384 * 100 + 6), (0, 2000000, 2100000), (0, 2000000, 2100001), (0, 7000000, 8500000),
              (0, 0, 1 << 29), (1, 0, 1 << 29), (2, 0, 1 << 29), (1, 200000, 300000), (2, 69999, 70000), (2, 70000, 70001), (1, 0, 1)]
    else:
        q += [(0, 0, 100), (0, 300000, 400000), (0, 311111, 411111), (0, 500000, 950000), (0, 100000, 560000), (0, 0, 1 << 29), (0, 1189000, 1300000),
              (0, 1 << 28, 1 << 29), (0, 600000, 616384), (0, 16384 * 30, 16384 * 31)]
    return q


_golden = None


def golden_files():
    """[{"label", "tbi" bytes, "queries": [{"tid", "beg", "end", "chunks": [(u, v)] or None}]}] of the fixture."""
    global _golden
    if _golden is None:
        with gzip.open(GOLDEN) as f:
            raw = json.loads(f.read().decode())
        _golden = [dict(f, tbi=base64.b64decode(f["tbi"]),
                        queries=[dict(q, chunks=None if q["chunks"] is None else [tuple(c) for c in q["chunks"]]) for q in f["queries"]]) for f in raw["files"]]
    return _golden


# ---- flat tables ----------------------------------------------------------------------------------------------------------------------
def flat_of(index):
    """The flat tables of a TabixIndex / BamIndex / Hand (csrc/index_query.hpp, flatten): bins ascending within a reference, chunks in
    file order within a bin, the linear index with every zero replaced by the last non-zero entry below it."""
    f = dict(ref_bin_first=[0], bin_id=[], bin_chunk_first=[0], chunk_u=[], chunk_v=[], ref_lin_first=[0], lin_fill=[])
    for bins, lin in zip(index.bins, index.linear):
        for b in sorted(bins):
            f["bin_id"].append(b)
            for u, v in bins[b]:
                f["chunk_u"].append(u)
                f["chunk_v"].append(v)
            f["bin_chunk_first"].append(len(f["chunk_u"]))
        f["ref_bin_first"].append(len(f["bin_id"]))
        last = 0
        for x in lin:
            last = x or last
            f["lin_fill"].append(last)
        f["ref_lin_first"].append(len(f["lin_fill"]))
    return f


def gathered_of(index, tid, beg, end):
    """How many chunks the query gathers (those with v > min_off in the listed bins): what the device's limit is about."""
    beg = max(beg, 0)
    if end < beg:
        return 0
    lin = flat_of_lin(index.linear[tid])
    min_off = lin[min(beg >> 14, len(lin) - 1)] if lin else 0
    return sum(1 for b in tabixindex.reg2bins(beg, end) for c in index.bins[tid].get(b, ()) if c[1] > min_off)


def flat_of_lin(lin):
    out, last = [], 0
    for x in lin:
        last = x or last
        out.append(last)
    return out


# ---- hand-made indexes ----------------------------------------------------------------------------------------------------------------
class Hand:
    """An index made by hand: bins [per reference {bin: [(u, v)]}], linear [per reference [offset]], names; pseudo: references that also
    carry the metadata pseudo-bin; order: the bins are serialised in this order (default: as given).  query is TabixIndex's."""

    def __init__(self, bins, linear, names=None, pseudo=(), n_no_coor=None):
        self.bins, self.linear = bins, linear
        self.names = names if names is not None else [b"r%d" % t for t in range(len(bins))]
        self.pseudo, self.n_no_coor = set(pseudo), n_no_coor

    query = tabixindex.TabixIndex.query

    def _body(self):
        out = b""
        for t, (bins, lin) in enumerate(zip(self.bins, self.linear)):
            keys = list(bins)[::-1]                                          # (descending: the flatten has to sort)
            out += struct.pack("<i", len(keys) + (t in self.pseudo))
            for k, b in enumerate(keys):
                if t in self.pseudo and k == len(keys) // 2:
                    out += struct.pack("<Ii4Q", PSEUDO_BIN, 2, 1, 2, 3, 4)
                out += struct.pack("<Ii", b, len(bins[b])) + b"".join(struct.pack("<QQ", u, v) for u, v in bins[b])
            if t in self.pseudo and not keys:
                out += struct.pack("<Ii4Q", PSEUDO_BIN, 2, 1, 2, 3, 4)
            out += struct.pack("<i", len(lin)) + struct.pack("<%dQ" % len(lin), *lin)
        return out

    def tbi_raw(self):
        names = b"".join(n + b"\x00" for n in self.names)
        return b"TBI\x01" + struct.pack("<8i", len(self.bins), 2, 1, 2, 0, ord("#"), 0, len(names)) + names + self._body()

    def tbi(self):
        return bgzf(self.tbi_raw())

    def bai(self):
        return b"BAI\x01" + struct.pack("<i", len(self.bins)) + self._body() + (struct.pack("<Q", self.n_no_coor) if self.n_no_coor is not None else b"")


def bgzf(raw):
    """raw as a BGZF stream with its EOF block (what plat_index_open takes for a .tbi)."""
    from platypus_amd import synth
    return synth.bgzf_stream(raw, 65280, eof=True)[0]


def vo(block, within=0):
    return (block << 16) | within


def spaced(n, first_block=10, step=3, length=1):
    """n chunks that neither touch nor share a block: none is dropped, cut or merged."""
    return [(vo(first_block + step * i), vo(first_block + step * i + length, 7)) for i in range(n)]


def leaf(pos):
    return 4681 + (pos >> 14)


def hand_cases():
    """[(label, Hand, [(tid, beg, end)])]: what the reference's indexer never writes, and the sizes at which the kernels change path."""
    cases = []
    W = 16384

    def one_bin(label, chunks, lin=(1,), extra=()):
        # every chunk in the leaf bin of window 3; lin small so that nothing is filtered unless the case says so
        h = Hand([{leaf(3 * W): list(chunks)}], [list(lin)])
        cases.append((label, h, [(0, 3 * W, 3 * W + 10), (0, 0, 1 << 29)] + list(extra)))

    for n in (0, 1, 63, 64, 65, 200, MAX_CHUNKS - 1):
        one_bin("%d gathered chunks" % n, spaced(n))
    # exactly the limit and one more, spread over two levels so that the gather crosses a level range
    for n in (MAX_CHUNKS, MAX_CHUNKS + 1):
        c = spaced(n)
        cases.append(("%d gathered chunks over two levels" % n, Hand([{leaf(3 * W): c[:n // 2], 585: c[n // 2:]}], [[1]]), [(0, 3 * W, 3 * W + 10)]))
    # a chunk that contains the 100 (and the 700) behind it: the prefix maximum has to carry across lanes and tiles
    for n in (100, 700):
        c = spaced(n, first_block=20)
        big = (vo(5), vo(20 + 3 * (n - 30), 9))
        one_bin("a container %d places in front" % n, [big] + c)
        one_bin("a container %d places in front, unsorted in the bin" % n, c[::-1] + [big])
    # merge runs: chunks that meet in one block, run after run; one run crossing a 64 boundary; one covering the whole list
    run = [(vo(10 + i, 5), vo(11 + i, 5)) for i in range(40)]               # each ends in the block the next begins in
    one_bin("a merge run over the whole list (40)", run)
    one_bin("a merge run over the whole list (300)", [(vo(10 + i, 5), vo(11 + i, 5)) for i in range(300)])
    one_bin("a merge run crossing place 64", spaced(50, first_block=10) + [(vo(500 + i, 5), vo(501 + i, 5)) for i in range(30)] + spaced(20, first_block=900))
    one_bin("merge runs of 3 among 130", [(vo(10 + 4 * (i // 3) + i % 3, 5), vo(11 + 4 * (i // 3) + i % 3, 5)) for i in range(130)])
    # overlaps that are cut, then meet in one block
    one_bin("overlapping chunks", [(vo(10), vo(14)), (vo(12), vo(18)), (vo(13, 5), vo(15)), (vo(30), vo(31))])
    # v == min_off exactly is dropped, one above is kept
    m = vo(100)
    one_bin("v equal to min_off", [(vo(90), m), (vo(95), m + 1), (vo(101), vo(103))], lin=[0, 0, 0, m], extra=[(0, 3 * W + 1, 3 * W + 2)])
    # linear indexes: none; a zero with non-zero entries below it; all zeros; a query beyond its end
    cases.append(("an empty linear index", Hand([{leaf(3 * W): spaced(5)}], [[]]), [(0, 3 * W, 4 * W)]))
    c = [(vo(10), vo(12)), (vo(50), vo(52)), (vo(90), vo(92))]
    cases.append(("a zero linear entry above non-zero ones", Hand([{leaf(3 * W): c, leaf(9 * W): c}], [[0, vo(11), 0, 0, vo(60), 0, 0, 0, 0, 0]]),
                  [(0, 3 * W, 4 * W), (0, 0, W), (0, 9 * W, 10 * W), (0, 2 * W, 10 * W), (0, 50 * W, 51 * W)]))
    cases.append(("a linear index of zeros", Hand([{leaf(3 * W): c}], [[0, 0, 0, 0, 0]]), [(0, 3 * W, 4 * W), (0, 100 * W, 101 * W)]))
    # ties in u (v ascending here), zero-length chunks
    one_bin("ties in u", [(vo(10), vo(30)), (vo(10), vo(20)), (vo(10), vo(20)), (vo(40), vo(41)), (vo(40), vo(45)), (vo(70), vo(71))])
    one_bin("ties in u among 90", spaced(44) + [(vo(300), vo(310)), (vo(300), vo(305))] + spaced(44, first_block=400))
    one_bin("zero-length chunks", [(vo(10), vo(10)), (vo(20, 5), vo(20, 5)), (vo(20, 5), vo(22)), (vo(30), vo(31)), (vo(31), vo(31))])
    # a reference without bins between two with; the pseudo-bin present; tid out of range is asked by the tests themselves
    cases.append(("a reference without bins", Hand([{leaf(0): spaced(3)}, {}, {0: spaced(2, 100)}], [[1], [], [1]], pseudo=(0, 1)),
                  [(0, 0, 10), (1, 0, 1 << 29), (1, 5, 5), (2, 0, 10), (2, 10, 5)]))
    # about 5000 bins: every leaf bin of 64 Mb and every level-4 bin above them, one chunk each
    bins = {leaf(w * W): [(vo(10 + 2 * w), vo(11 + 2 * w, 1))] for w in range(4096)}
    bins.update({585 + k: [(vo(20000 + 2 * k), vo(20001 + 2 * k, 1))] for k in range(512)})
    bins.update({73 + k: [(vo(30000 + 2 * k), vo(30001 + 2 * k, 1))] for k in range(64)})
    bins[0] = [(vo(40000), vo(40001))]
    cases.append(("a reference with 4673 bins", Hand([bins], [[1] * 4096]),
                  [(0, 1000 * W, 1000 * W + 1), (0, 1000 * W, 1013 * W), (0, 0, 1 << 29), (0, 4095 * W, 5000 * W), (0, 1 << 27, 1 << 28)]))
    return cases


def synthetic_bai(seed=3, n=400, ref_len=3000000):
    """(BamIndex-like Hand, records): a BAI built from synthetic records the way an indexer does, ONE CHUNK PER RECORD (no merging): record
    i lies at virtual offsets [rec[i].u, rec[i].v); bin = reg2bin(beg, end); the linear index holds the first record's offset per window."""
    rng = random.Random(seed)
    recs, at = [], vo(3, 100)
    pos = 0
    for i in range(n):
        pos += rng.randrange(0, 2 * ref_len // n)
        length = rng.choice((50, 150, 150, 150, 5000, 20000, 200000)) if i % 7 else 150
        beg, end = pos, min(pos + length, ref_len)
        size = rng.randrange(200, 400)
        block, within = at >> 16, (at & 0xffff) + size
        nxt = vo(block + within // 60000, within % 60000)                   # (blocks of 60000 inflated bytes; block numbers stand for addresses)
        recs.append((beg, end, at, nxt))
        at = nxt
        if pos >= ref_len - 1:
            break
    bins, lin = {}, [0] * ((ref_len >> 14) + 1)
    for beg, end, u, v in recs:
        if end <= beg:
            continue
        b = reg2bin(beg, end)
        bins.setdefault(b, []).append((u, v))
        for w in range(beg >> 14, ((end - 1) >> 14) + 1):
            if lin[w] == 0:
                lin[w] = u
    return Hand([bins], [lin], pseudo=(0,), n_no_coor=17), [r for r in recs if r[1] > r[0]]


def reg2bin(beg, end):
    end -= 1
    for shift, first in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return first + (beg >> shift)
    return 0


def random_lists(seed, n_lists):
    """Seeded random chunk lists sorted by (u, v), ties and zero-length chunks included: what the three loops are compared on."""
    rng = random.Random(seed)
    out = []
    for _ in range(n_lists):
        n = rng.choice((0, 1, 2, 3, 5, 8, 13, 40))
        span = rng.choice((1 << 17, 1 << 18, 1 << 20))
        c = []
        for _ in range(n):
            u = rng.randrange(span)
            c.append((u, u + rng.choice((0, 0, 1, rng.randrange(1 << 16), rng.randrange(span)))))
        out.append(sorted(c))
    return out
