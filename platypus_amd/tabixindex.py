"""A tabix index (.tbi) read in plain Python, and a query's chunks cut out of the bgzipped file as BGZF blocks -- what an integrator's
loader does in front of plat_caller_set_source_blocks (include/platypus_caller_tabix.h).  The C library reads an index itself
(include/platypus_caller_index.h: opened once, queried in device batches); this module is the plain-Python statement of the same rule and
serves the tests, and TabixFile.fetch_blocks_batch hands a list of fetches to the library's index.

The layout is the public one (the tabix format description: magic TBI\\1, n_ref, format, col_seq, col_beg, col_end, meta, skip, l_nm, the
names, then per sequence the bins with their chunks and the linear index), gzip-compressed.  The chunk list of a query is chosen as
ti_iter_query chooses it (src/tabix/index.c.pysam.c:799-870): reg2bins, the linear index's minimum offset, sort, drop contained chunks,
cut overlaps, merge chunks that meet in one block.  Only the VCF preset is handled; CSI indexes are not."""
import gzip
import struct

import numpy as np

TBI_MAGIC = b"TBI\x01"
TI_PRESET_VCF = 2
LIDX_SHIFT = 14


def reg2bins(beg, end):
    """The bins that may hold an interval overlapping [beg, end) (index.c.pysam.c:776-789)."""
    if beg >= end:
        return []
    end = min(end, 1 << 29) - 1
    bins = [0]
    for first, shift in ((1, 26), (9, 23), (73, 20), (585, 17), (4681, 14)):
        bins.extend(range(first + (beg >> shift), first + (end >> shift) + 1))
    return bins


class TabixIndex:
    """names: the sequence names in tid order (bytes); bins[tid]: {bin: [(beg, end) virtual offsets]}; linear[tid]: [offset]."""

    def __init__(self, raw):
        data = gzip.decompress(bytes(raw))
        if data[:4] != TBI_MAGIC:
            raise ValueError("not a tabix index (no TBI\\1 magic)")
        n_ref, self.preset, self.col_seq, self.col_beg, self.col_end, self.meta, self.skip, l_nm = struct.unpack_from("<8i", data, 4)
        if (self.preset & 0xffff) != TI_PRESET_VCF:
            raise ValueError("only the VCF preset of tabix is handled (format %d)" % self.preset)
        at = 36
        self.names = data[at:at + l_nm].split(b"\x00")[:n_ref]
        at += l_nm
        self.bins, self.linear = [], []
        for _ in range(n_ref):
            n_bin, = struct.unpack_from("<i", data, at)
            at += 4
            bins = {}
            for _ in range(n_bin):
                b, n_chunk = struct.unpack_from("<Ii", data, at)
                at += 8
                v = struct.unpack_from("<%dQ" % (2 * n_chunk), data, at)
                at += 16 * n_chunk
                bins[b] = list(zip(v[0::2], v[1::2]))
            n_intv, = struct.unpack_from("<i", data, at)
            at += 4
            self.linear.append(list(struct.unpack_from("<%dQ" % n_intv, data, at)))
            at += 8 * n_intv
            self.bins.append(bins)

    def tid(self, name):
        name = name if isinstance(name, bytes) else name.encode()
        return self.names.index(name) if name in self.names else -1

    def query(self, tid, beg, end):
        """ti_iter_query's chunk list for [beg, end) of sequence tid: [(u, v)] virtual offsets in order; None where it returns no iterator."""
        beg = max(beg, 0)
        if end < beg:
            return None
        lin = self.linear[tid]
        min_off = 0
        if lin:
            k = beg >> LIDX_SHIFT
            min_off = lin[-1] if k >= len(lin) else lin[k]
            if min_off == 0:                                        # (index files of tabix before 0.1.4)
                for i in range(min(k, len(lin)) - 1, -1, -1):
                    if lin[i] != 0:
                        min_off = lin[i]
                        break
        off = [c for b in reg2bins(beg, end) for c in self.bins[tid].get(b, ()) if c[1] > min_off]
        if not off:
            return []
        off.sort(key=lambda c: c[0])
        kept = [list(off[0])]
        for u, v in off[1:]:                                        # completely contained chunks
            if kept[-1][1] < v:
                kept.append([u, v])
        for i in range(1, len(kept)):                               # overlaps (the merge at indexing may leave some)
            if kept[i - 1][1] >= kept[i][0]:
                kept[i - 1][1] = kept[i][0]
        out = [kept[0]]
        for u, v in kept[1:]:                                       # chunks that meet in one block
            if out[-1][1] >> 16 == u >> 16:
                out[-1][1] = v
            else:
                out.append([u, v])
        return [tuple(c) for c in out]


BAI_MAGIC = b"BAI\x01"
PSEUDO_BIN = 37450


class BamIndex:
    """A BAM index (.bai, uncompressed): the same bins, chunks and linear index per reference, no names; the metadata pseudo-bin 37450 is
    left out of bins and kept in pseudo[tid]; n_no_coor is the trailing count, None when the file has none.  query is TabixIndex's."""

    def __init__(self, raw):
        data = bytes(raw)
        if data[:4] != BAI_MAGIC:
            raise ValueError("not a BAM index (no BAI\\1 magic)")
        n_ref, = struct.unpack_from("<i", data, 4)
        at = 8
        self.bins, self.linear, self.pseudo = [], [], []
        for _ in range(n_ref):
            n_bin, = struct.unpack_from("<i", data, at)
            at += 4
            bins, pseudo = {}, None
            for _ in range(n_bin):
                b, n_chunk = struct.unpack_from("<Ii", data, at)
                at += 8
                v = struct.unpack_from("<%dQ" % (2 * n_chunk), data, at)
                at += 16 * n_chunk
                if b == PSEUDO_BIN:
                    pseudo = list(zip(v[0::2], v[1::2]))
                else:
                    bins[b] = list(zip(v[0::2], v[1::2]))
            n_intv, = struct.unpack_from("<i", data, at)
            at += 4
            self.linear.append(list(struct.unpack_from("<%dQ" % n_intv, data, at)))
            at += 8 * n_intv
            self.bins.append(bins)
            self.pseudo.append(pseudo)
        self.n_no_coor = struct.unpack_from("<Q", data, at)[0] if len(data) - at >= 8 else None
        self.names = []

    query = TabixIndex.query


def block_length(data, at):
    """The length of the BGZF block at data[at] (its BSIZE + 1), the BC subfield looked for among the extra subfields."""
    if data[at:at + 4] != b"\x1f\x8b\x08\x04":
        raise ValueError("no BGZF block at offset %d" % at)
    xlen, = struct.unpack_from("<H", data, at + 10)
    x = at + 12
    while x + 4 <= at + 12 + xlen:
        slen, = struct.unpack_from("<H", data, x + 2)
        if data[x:x + 2] == b"BC" and slen == 2:
            return struct.unpack_from("<H", data, x + 4)[0] + 1
        x += 4 + slen
    raise ValueError("the block at offset %d has no BC subfield" % at)


def cut_chunks(data, chunks):
    """The chunks [(u, v)] of a query as plat_bgzf_chunk takes them: [(block bytes uint8 array, first_uoffset, end_coffset, end_uoffset)].
    A chunk's bytes run from the block of u through the block of v (a valid index ends chunks on line boundaries: no line runs on)."""
    out = []
    for u, v in chunks:
        c0, c1 = u >> 16, v >> 16
        stop = c1 + block_length(data, c1) if v & 0xffff else c1
        out.append((np.frombuffer(data, dtype=np.uint8, count=stop - c0, offset=c0), u & 0xffff, c1 - c0, v & 0xffff))
    return out


class TabixFile:
    """A bgzipped VCF and its index, both in memory."""

    def __init__(self, data, index):
        self.data = bytes(data)
        self.raw_index = None if isinstance(index, TabixIndex) else bytes(index)
        self.index = index if isinstance(index, TabixIndex) else TabixIndex(index)

    @classmethod
    def open(cls, path, index_path=None):
        with open(path, "rb") as f, open(index_path or path + ".tbi", "rb") as g:
            return cls(f.read(), g.read())

    def fetch_blocks(self, name, beg, end):
        """The fetch of name:[beg, end) (0-based half-open, as pysam's fetch(chrom, start, end)) as NativeCaller.set_source_blocks takes
        it: (seq_name, beg, end, chunks); None where the reference's fetch raises (a name the index does not hold, end < beg)."""
        tid = self.index.tid(name)
        chunks = self.index.query(tid, beg, end) if tid >= 0 else None
        if chunks is None:
            return None
        return (self.index.names[tid], max(beg, 0), end, cut_chunks(self.data, chunks))

    def fetch_blocks_batch(self, queries, caller, native_index=None):
        """fetch_blocks for a list of (name, beg, end), the chunk lists chosen by the library in one device batch (NativeCaller.query_index
        over this file's index, opened on `caller` unless native_index is one already).  Needs the index's bytes (TabixFile(data, raw))."""
        opened = native_index is None
        idx = caller.open_index(self.raw_index, "tbi") if opened else native_index
        try:
            tids = [idx.tid(name) for name, _, _ in queries]
            asked = [(t, b, e) for t, (_, b, e) in zip(tids, queries) if t >= 0]
            lists = iter(caller.query_index(idx, asked))
            out = []
            for t, (_, beg, end) in zip(tids, queries):
                chunks = next(lists) if t >= 0 else None
                out.append(None if chunks is None else (self.index.names[t], max(beg, 0), end, cut_chunks(self.data, chunks)))
            return out
        finally:
            if opened:
                idx.close()
