"""ctypes binding of libplat_caller.so (include/platypus_caller.h, include/platypus_caller_fetched.h): the native region loop.

    reads of a region in host memory (structure-of-arrays)  ->  VCF record lines

`ReadTable` / `RegionReads` are the array form of ReadArray / bamReadBuffer (cwindow.pyx:92-236,485-513);
`NativeCaller.call_regions` is callVariantsInRegion (variantcaller.pyx:535-615) for a list of regions and writes the
text platypus_amd.caller.callVariantsInRegions writes (tests/test_native_caller_*.py compare the two).  The library
is host code on top of libplat_mi355x.so; like the rest of the package it has no CPU fallback.
`FetchedRegion` / `NativeCaller.call_fetched_regions` take the reads as a BAM fetch returns them instead (the loader's
addReadToBuffer QC and split run on the device, cwindow.pyx:560-595); `BamRegion` / `NativeCaller.call_bam_regions` take the raw BAM
alignment records (include/platypus_caller_bam.h: ReadIterator.get, htslibWrapper.pyx:328-406, runs on the device too);
`BamFileRegion` / `BgzfFileRegion` with `NativeCaller.call_bam_regions_rg` / `call_bgzf_regions_rg` take the fetches of merged FILES and a
read-group table (include/platypus_caller_rg.h: the records are split by sample on the device)."""
import ctypes as C
import os
import subprocess

import numpy as np

from . import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libplat_caller.so")
HOST_SRC = os.path.join(HERE, "csrc", "host")


READS_ASCII, READS_PACKED = 0, 1


class _ReadTable(C.Structure):
    _fields_ = [("n_reads", C.c_int32), ("encoding", C.c_int32)] + [(k, C.c_void_p) for k in (
        "seq", "qual", "off", "pos", "end", "mapq", "flags", "mate_pos", "cigar", "cig_off")] + \
               [("n_exceptions", C.c_int64), ("exc_index", C.c_void_p), ("exc_base", C.c_void_p), ("exc_qual", C.c_void_p),
                ("dev_seq", C.c_void_p), ("dev_qual", C.c_void_p)] + [(k, C.c_void_p) for k in (
                    "dev_off", "dev_pos", "dev_end", "dev_mapq", "dev_flags", "dev_cigar", "dev_cig_off")] + \
               [("longest_read", C.c_int32), ("most_bases", C.c_int32)]       # optional: the loader's own figures (0 = not known)


class _SampleReads(C.Structure):
    _fields_ = [("reads", _ReadTable), ("bad_reads", _ReadTable), ("broken_mates", _ReadTable)]


class _Region(C.Structure):
    _fields_ = [("chrom", C.c_char_p), ("start", C.c_int32), ("end", C.c_int32), ("contig_seq", C.c_void_p),
                ("contig_len", C.c_int64), ("samples", C.POINTER(_SampleReads)), ("dev_contig_seq", C.c_void_p)]


_OPT_FIELDS = [("rlen", C.c_int32), ("minReads", C.c_int32), ("maxReads", C.c_double), ("maxSize", C.c_int32), ("largeWindows", C.c_int32),
               ("maxVariants", C.c_int32), ("coverageSamplingLevel", C.c_int32), ("maxHaplotypes", C.c_int32),
               ("originalMaxHaplotypes", C.c_int32), ("skipDifficultWindows", C.c_int32), ("getVariantsFromBAMs", C.c_int32),
               ("genSNPs", C.c_int32), ("genIndels", C.c_int32), ("mergeClusteredVariants", C.c_int32), ("minFlank", C.c_int32),
               ("filterVarsByCoverage", C.c_int32), ("filteredReadsFrac", C.c_double), ("maxVarDist", C.c_int32), ("minVarDist", C.c_int32),
               ("useEMLikelihoods", C.c_int32), ("countOnlyExactIndelMatches", C.c_int32), ("calculateFlankScore", C.c_int32),
               ("assemble", C.c_int32), ("outputRefCalls", C.c_int32), ("minMapQual", C.c_int32), ("minBaseQual", C.c_int32),
               ("minPosterior", C.c_int32), ("sbThreshold", C.c_double), ("scThreshold", C.c_double), ("abThreshold", C.c_double),
               ("minVarFreq", C.c_double), ("badReadsWindow", C.c_int32), ("badReadsThreshold", C.c_int32), ("rmsmqThreshold", C.c_int32),
               ("qdThreshold", C.c_int32), ("hapScoreThreshold", C.c_int32), ("refCallBlockSize", C.c_int32),
               ("assemblyRegionSize", C.c_int32), ("assembleAll", C.c_int32), ("assembleBadReads", C.c_int32), ("assembleBrokenPairs", C.c_int32),
               ("assemblerKmerSize", C.c_int32), ("noCycles", C.c_int32)]


class CallerOptions(C.Structure):
    _fields_ = _OPT_FIELDS

    @classmethod
    def from_options(cls, options):
        """From the reference's options object (platypus_amd.options.default_options())."""
        o = cls()
        for name, typ in _OPT_FIELDS:
            if name != "_pad":
                setattr(o, name, (float if typ is C.c_double else int)(getattr(options, name)))
        return o


class CallerStats(C.Structure):
    _fields_ = [(k, C.c_int64) for k in ("n_regions", "n_reads", "n_candidate_records", "n_variants", "n_windows", "n_windows_called",
                                         "n_records", "n_windows_greedy", "n_windows_failed")] + \
               [(k, C.c_double) for k in ("seconds_total", "seconds_host", "seconds_device_wait")] + [("seconds_stage", C.c_double * 8)] + \
               [("seconds_load", C.c_double), ("seconds_source_wait", C.c_double), ("input_bytes", C.c_int64), ("n_assembly_tiles", C.c_int64),
                ("n_assembler_variants", C.c_int64), ("n_refcall_records", C.c_int64), ("seconds_assemble", C.c_double), ("n_pairs", C.c_int64),
                ("n_dp_reference", C.c_int64), ("cells_reference", C.c_int64), ("n_dp_launched", C.c_int64), ("cells_launched", C.c_int64),
                ("n_align_batches", C.c_int64), ("align_hap_bytes", C.c_int64), ("align_read_bytes", C.c_int64), ("align_reads", C.c_int64),
                ("align_dp_bytes", C.c_int64), ("seconds_kernel_seed", C.c_double), ("seconds_kernel_dp", C.c_double),
                ("seconds_kernel_sweep", C.c_double), ("seconds_kernel_pairs", C.c_double), ("n_regions_stage_b_device", C.c_int64),
                ("n_regions_stage_b_host", C.c_int64), ("n_windows_stage_b_host", C.c_int64), ("n_regions_dict_replay_device", C.c_int64),
                ("seconds_worker_cpu", C.c_double), ("seconds_kernel_unpack", C.c_double), ("seconds_kernel_candidates", C.c_double),
                ("unpack_bytes", C.c_int64), ("candidates_bytes", C.c_int64), ("n_unpack_launches", C.c_int64), ("n_candidates_launches", C.c_int64),
                ("kernel_ms", C.c_double * 32), ("kernel_launches", C.c_int64 * 32),
                ("n_source_lines", C.c_int64), ("n_source_variants", C.c_int64), ("seconds_source", C.c_double),
                ("n_source_chunks_device", C.c_int64), ("n_source_retries", C.c_int64),
                ("n_refcall_intervals_device", C.c_int64), ("n_refcall_positions_device", C.c_int64), ("n_refcall_intervals_host", C.c_int64)]

    STAGES = ("upload", "candidate_scan", "variants_windows_haplotypes", "greedy_rounds", "window_batch", "posteriors", "read_stats_calls", "text")

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_ if k not in ("seconds_stage", "kernel_ms", "kernel_launches")}
        d["seconds_stage"] = dict(zip(self.STAGES, list(self.seconds_stage)))
        d["kernel_ms"], d["kernel_launches"] = list(self.kernel_ms), list(self.kernel_launches)
        return d


class _SourceLines(C.Structure):
    """plat_source_lines (include/platypus_caller_source.h)."""
    _fields_ = [("text", C.c_void_p), ("len", C.c_int64)]


class _TabixFetch(C.Structure):
    """plat_tabix_fetch (include/platypus_caller_tabix.h)."""
    _fields_ = [("seq_name", C.c_char_p), ("itr_beg", C.c_int32), ("itr_end", C.c_int32), ("n_chunks", C.c_int32), ("chunks", C.c_void_p)]


class _SourceBlocks(C.Structure):
    _fields_ = [("n_fetches", C.c_int32), ("fetches", C.c_void_p)]


class SourceBlocksInfo(C.Structure):
    """plat_source_blocks_info."""
    _fields_ = [(k, C.c_int64) for k in ("n_blocks", "compressed_bytes", "inflated_bytes", "lines_walked", "lines_kept", "kept_bytes")] + [("seconds", C.c_double)]


class IndexQueryInfo(C.Structure):
    """plat_index_query_info (include/platypus_caller_index.h)."""
    _fields_ = [(k, C.c_int64) for k in ("queries", "handed_over", "chunks", "device_calls")] + [("seconds", C.c_double)]


class _SourceFile(C.Structure):
    """plat_source_file."""
    _fields_ = [("data", C.c_void_p), ("data_len", C.c_int64), ("index", C.c_void_p)]


class _SourceRegion(C.Structure):
    """plat_source_region."""
    _fields_ = [("chrom", C.c_char_p), ("start", C.c_int32), ("end", C.c_int32)]


INDEX_KINDS = {"tbi": 0, "bai": 1}


class FastaInfo(C.Structure):
    """plat_fasta_info (include/platypus_caller_fasta.h)."""
    _fields_ = [(k, C.c_int64) for k in ("queries", "file_bytes", "out_bytes", "device_calls")] + [("seconds", C.c_double)]


class _FetchedReads(C.Structure):
    _fields_ = [("fetched", _ReadTable), ("broken_mates", _ReadTable), ("chrom_id", C.c_void_p), ("mate_chrom_id", C.c_void_p),
                ("insert_size", C.c_void_p)]


class _FetchedRegion(C.Structure):
    _fields_ = [("chrom", C.c_char_p), ("start", C.c_int32), ("end", C.c_int32), ("contig_seq", C.c_void_p),
                ("contig_len", C.c_int64), ("samples", C.POINTER(_FetchedReads)), ("dev_contig_seq", C.c_void_p)]


_QC_FIELDS = ("minGoodQualBases", "minMapQual", "minBaseQual", "trimOverlapping", "trimAdapter", "trimReadFlank", "trimSoftClipped",
              "filterDuplicates", "filterReadsWithUnmappedMates", "filterReadsWithDistantMates", "filterReadPairsWithSmallInserts")


class CallerQCOptions(C.Structure):
    """plat_caller_qc_options: the options bamReadBuffer's constructor reads (cwindow.pyx:490-526)."""
    _fields_ = [(k, C.c_int32) for k in _QC_FIELDS]

    @classmethod
    def from_options(cls, options):
        o = cls()
        for k in _QC_FIELDS:
            setattr(o, k, int(getattr(options, k)))
        return o


class _FetchedRegionInfo(C.Structure):
    _fields_ = [("loaded", C.c_int32), ("sample_counts", C.c_void_p)]


class _BamRecords(C.Structure):
    _fields_ = [("n_records", C.c_int32), ("data", C.c_void_p), ("data_len", C.c_int64), ("rec_off", C.c_void_p)]


class _BamSample(C.Structure):
    _fields_ = [("fetched", _BamRecords), ("broken_mates", _BamRecords)]


class _BamRegion(C.Structure):
    _fields_ = [("chrom", C.c_char_p), ("start", C.c_int32), ("end", C.c_int32), ("contig_seq", C.c_void_p),
                ("contig_len", C.c_int64), ("samples", C.POINTER(_BamSample)), ("dev_contig_seq", C.c_void_p)]


class _BgzfChunk(C.Structure):
    _fields_ = [("data", C.c_void_p), ("data_len", C.c_int64), ("first_uoffset", C.c_int32), ("end_coffset", C.c_int64), ("end_uoffset", C.c_int32)]


class _BgzfSample(C.Structure):
    _fields_ = [("n_chunks", C.c_int32), ("chunks", C.POINTER(_BgzfChunk)), ("broken_mates", _BamRecords)]


class _BgzfRegion(C.Structure):
    _fields_ = [("chrom", C.c_char_p), ("start", C.c_int32), ("end", C.c_int32), ("contig_seq", C.c_void_p), ("contig_len", C.c_int64),
                ("dev_contig_seq", C.c_void_p), ("tid", C.c_int32), ("itr_beg", C.c_int32), ("itr_end", C.c_int32), ("samples", C.POINTER(_BgzfSample))]


class _BamReadGroups(C.Structure):
    _fields_ = [("n_groups", C.c_int32), ("id", C.POINTER(C.c_char_p)), ("sample", C.c_void_p)]


class _BamFileRecords(C.Structure):
    _fields_ = [("records", _BamRecords), ("rec_len", C.c_void_p)]


class _BamFile(C.Structure):
    _fields_ = [("fetched", _BamFileRecords), ("broken_mates", _BamFileRecords)]


class _BgzfFile(C.Structure):
    _fields_ = [("n_chunks", C.c_int32), ("chunks", C.POINTER(_BgzfChunk)), ("broken_mates", _BamFileRecords)]


class _BamRgRegion(C.Structure):
    _fields_ = [("chrom", C.c_char_p), ("start", C.c_int32), ("end", C.c_int32), ("contig_seq", C.c_void_p),
                ("contig_len", C.c_int64), ("files", C.POINTER(_BamFile)), ("dev_contig_seq", C.c_void_p)]


class _BgzfRgRegion(C.Structure):
    _fields_ = [("chrom", C.c_char_p), ("start", C.c_int32), ("end", C.c_int32), ("contig_seq", C.c_void_p), ("contig_len", C.c_int64),
                ("dev_contig_seq", C.c_void_p), ("tid", C.c_int32), ("itr_beg", C.c_int32), ("itr_end", C.c_int32), ("files", C.POINTER(_BgzfFile))]


class _BamPlan(C.Structure):
    """plat_bam_plan (include/platypus_caller_bamfile.h)."""
    _fields_ = [("mode", C.c_int32), ("n_samples", C.c_int32), ("sample_names", C.POINTER(C.c_char_p)), ("sample_file", C.POINTER(C.c_int32)),
                ("groups", _BamReadGroups)]


class _BamCallRegion(C.Structure):
    """plat_bam_call_region."""
    _fields_ = [("chrom", C.c_char_p), ("start", C.c_int32), ("end", C.c_int32), ("contig_seq", C.c_void_p), ("contig_len", C.c_int64),
                ("dev_contig_seq", C.c_void_p)]


class _BamFetch(C.Structure):
    """plat_bam_fetch."""
    _fields_ = [("tid", C.c_int32), ("itr_beg", C.c_int32), ("itr_end", C.c_int32), ("n_chunks", C.c_int32), ("chunks", C.POINTER(_BgzfChunk))]


class _BamFetchPlan(C.Structure):
    """plat_bam_fetch_plan."""
    _fields_ = [("n_regions", C.c_int32), ("n_files", C.c_int32), ("fetches", C.POINTER(_BamFetch))] + \
               [(k, C.c_int64) for k in ("queries", "handed_over", "chunks", "device_calls")] + [("seconds", C.c_double)]


class _BamMateQuery(C.Structure):
    """plat_bam_mate_query."""
    _fields_ = [("tid", C.c_int32), ("_pad", C.c_int32), ("start", C.c_int64), ("end", C.c_int64)]


class _BamMates(C.Structure):
    """plat_bam_mates."""
    _fields_ = [("n_coords", C.c_int32), ("n_queries", C.c_int32), ("queries", C.POINTER(_BamMateQuery)), ("mates", _BamFileRecords)]


class _BamMatesPlan(C.Structure):
    """plat_bam_mates_plan."""
    _fields_ = [("n_regions", C.c_int32), ("n_files", C.c_int32), ("units", C.POINTER(_BamMates)), ("loaded", C.POINTER(C.c_int32))] + \
               [(k, C.c_int64) for k in ("coords", "queries", "chunks", "records_looked_at", "records_kept", "device_calls", "input_bytes")] + [("seconds", C.c_double)]


BAM_FILES_MODES = ("presplit", "merged")


class ReadTable:
    """One ReadArray as arrays (cAlignedRead fields, htslibWrapper.pxd:187-201).  `reads`: the order the ReadArray holds them in
    (sorted by pos; brokenMates by mate position)."""
    __slots__ = ("n", "seq", "qual", "off", "pos", "end", "mapq", "flags", "mate_pos", "cigar", "cig_off", "_pinned", "_struct", "encoding", "exc")

    def __init__(self, seq, qual, off, pos, end, mapq, flags, mate_pos, cigar, cig_off, pin=False, packed=False):
        """pin=True keeps the two byte blobs in page-locked memory (what a loader that decodes into pinned buffers hands over):
        their upload is then asynchronous and runs at link speed instead of going through the driver's staging copies.
        packed=True hands the reads over as PLAT_READS_PACKED (one byte per base + exceptions) instead of ASCII bases + qualities."""
        self.n = len(pos)
        pad = np.zeros(_lib.PLAT_BLOB_PAD, dtype=np.uint8)
        c = lambda a, dt: np.ascontiguousarray(a, dtype=dt)
        self.encoding, self.exc = READS_ASCII, None
        if packed:
            seq, qual = c(seq, np.uint8), c(qual, np.uint8)
            plain = (seq == 65) | (seq == 67) | (seq == 71) | (seq == 84)
            ex = np.nonzero(~plain | (qual > 63))[0].astype(np.int64)
            self.exc = (ex, seq[ex].copy(), qual[ex].copy())
            seq = (((seq >> 1) & 3) | (np.minimum(qual, 63) << 2)).astype(np.uint8)
            qual = np.zeros(0, dtype=np.uint8)
            self.encoding = READS_PACKED
        self.seq, self.qual = np.concatenate([c(seq, np.uint8), pad]), np.concatenate([c(qual, np.uint8), pad])
        self._pinned = None
        if pin and self.n:
            import torch
            self._pinned = [torch.from_numpy(self.seq).pin_memory(), torch.from_numpy(self.qual).pin_memory()]
            self.seq, self.qual = self._pinned[0].numpy(), self._pinned[1].numpy()
        self.off, self.pos, self.end = c(off, np.int64), c(pos, np.int32), c(end, np.int32)
        self.mapq, self.flags, self.mate_pos = c(mapq, np.uint8), c(flags, np.int32), c(mate_pos, np.int32)
        self.cigar, self.cig_off = np.concatenate([c(cigar, np.int16).reshape(-1), np.zeros(2, dtype=np.int16)]), c(cig_off, np.int32)
        assert len(self.off) == self.n + 1 and len(self.cig_off) == self.n + 1 and (self.n == 0 or self.off[0] == 0)

    @classmethod
    def from_reads(cls, reads, packed=False):
        """From hostapi.AlignedRead objects, in the given order."""
        lens = [r.rlen for r in reads]
        cig = [x for r in reads for c in r.cigarOps for x in c]
        return cls(np.frombuffer(b"".join(r.seq for r in reads), dtype=np.uint8), np.frombuffer(b"".join(r.qual for r in reads), dtype=np.uint8),
                   np.concatenate([[0], np.cumsum(lens)]), [r.pos for r in reads], [r.end for r in reads], [r.mapq for r in reads],
                   [r.bitFlag for r in reads], [r.matePos for r in reads], np.array(cig, dtype=np.int16),
                   np.concatenate([[0], np.cumsum([len(r.cigarOps) for r in reads])]), packed=packed)

    def struct(self):
        """The plat_read_table of these arrays (built once: the arrays are kept alive by, and never replaced on, this object)."""
        t = getattr(self, "_struct", None)
        if t is None:
            t = _ReadTable()
            t.n_reads, t.encoding = self.n, self.encoding
            for k in ("seq", "qual", "off", "pos", "end", "mapq", "flags", "mate_pos", "cigar", "cig_off"):
                setattr(t, k, getattr(self, k).ctypes.data)
            if self.exc is not None:
                t.n_exceptions = len(self.exc[0])
                t.exc_index, t.exc_base, t.exc_qual = (a.ctypes.data for a in self.exc)
            if self.n:                                                       # what ReadArray knows of itself (cwindow.pyx:173-174): one numpy pass here, none in the library
                t.longest_read = max(0, int((self.end[:self.n].astype(np.int64) - self.pos[:self.n]).max()))
                t.most_bases = max(0, int(np.diff(self.off[:self.n + 1]).max()))
            self._struct = t
        return t


def _u8(a):
    """bytes, a bytearray or an array as a contiguous uint8 array (no copy where it is one already)."""
    return np.ascontiguousarray(np.frombuffer(a, dtype=np.uint8) if isinstance(a, (bytes, bytearray)) else a, dtype=np.uint8)


def _fill_records(t, data, off):
    """A plat_bam_records over (data uint8 array, rec_off int64 array)."""
    t.n_records, t.data, t.data_len, t.rec_off = len(off), data.ctypes.data, len(data), off.ctypes.data


def _fill_file_records(t, rec):
    """A plat_bam_file_records over (data, rec_off, rec_len int32 array)."""
    _fill_records(t.records, rec[0], rec[1])
    t.rec_len = rec[2].ctypes.data


def _chunk_array(chunks):
    """The plat_bgzf_chunk array of [(data uint8 array, first_uoffset, end_coffset, end_uoffset)]."""
    cc = (_BgzfChunk * max(len(chunks), 1))()
    for q, (d, fu, ec, eu) in enumerate(chunks):
        cc[q].data, cc[q].data_len, cc[q].first_uoffset, cc[q].end_coffset, cc[q].end_uoffset = d.ctypes.data, len(d), fu, ec, eu
    return cc


class _RegionBase:
    """What every region class holds: chrom:start-end, the contig's sequence as a contiguous uint8 array, and -- built once, at the first
    fill -- the C array of its per-class member (UNITS: the samples, or the files of the merged-file regions).  A subclass writes that
    array in _c_units() and returns it, followed by whatever else has to stay alive with it."""
    UNITS = "samples"

    def __init__(self, chrom, start, end, contig_seq):
        self.chrom, self.start, self.end = chrom, int(start), int(end)
        self.contig = _u8(contig_seq)
        self._c = None

    def fill(self, a, n_units):
        """Write this region into the C region struct `a` (the arrays stay owned by, and alive with, this object)."""
        assert len(getattr(self, self.UNITS)) == n_units
        if self._c is None:
            self._c = (self.chrom.encode(),) + tuple(self._c_units())
        a.chrom, a.contig_seq, a.contig_len = self._c[0], self.contig.ctypes.data, len(self.contig)
        a.start, a.end = self.start, self.end
        setattr(a, self.UNITS, self._c[1])


class _BgzfWindow(_RegionBase):
    """... and the iterator's window of the two BGZF region classes."""

    def __init__(self, chrom, start, end, contig_seq, tid, itr_beg, itr_end):
        super().__init__(chrom, start, end, contig_seq)
        self.tid, self.itr_beg, self.itr_end = int(tid), int(itr_beg), int(itr_end)

    def fill(self, a, n_units):
        super().fill(a, n_units)
        a.tid, a.itr_beg, a.itr_end = self.tid, self.itr_beg, self.itr_end


class RegionReads(_RegionBase):
    """One region: chrom:start-end, the contig's sequence and per sample (reads, badReads, brokenMates) as ReadTables."""

    def __init__(self, chrom, start, end, contig_seq, samples):
        super().__init__(chrom, start, end, contig_seq)
        self.samples = samples                                  # [(reads, bad, broken)]

    def _c_units(self):
        ss = (_SampleReads * len(self.samples))()
        for i, (a, b, c) in enumerate(self.samples):
            ss[i].reads, ss[i].bad_reads, ss[i].broken_mates = a.struct(), b.struct(), c.struct()
        return (ss,)

    @classmethod
    def from_buffers(cls, chrom, start, end, fasta, buffers, packed=False):
        """From hostapi.bamReadBuffer objects and a hostapi.FastaFile (the inputs of caller.callVariantsInRegions)."""
        return cls(chrom, start, end, fasta._seq[chrom],
                   [(ReadTable.from_reads(b.reads.array, packed), ReadTable.from_reads(b.badReads.array, packed),
                     ReadTable.from_reads(b.brokenMates.array, packed)) for b in buffers])


class FetchedRegion(_RegionBase):
    """One region as loadBAMData has it in hand (platypusutils.pyx:449-686): per sample the reads a `fetch` returned, in fetch order,
    with chromID / mateChromID / insertSize per read, and the broken mates (sorted by mate position)."""

    def __init__(self, chrom, start, end, contig_seq, samples):
        super().__init__(chrom, start, end, contig_seq)
        self.samples = samples                                  # [(fetched ReadTable, broken ReadTable, chrom_id, mate_chrom_id, insert_size)]

    @classmethod
    def from_reads(cls, chrom, start, end, fasta, samples, packed=False):
        """samples: per sample (fetched, brokenMates), lists of hostapi.AlignedRead -- fetched in fetch order; brokenMates are sorted by
        mate position here, as bamReadBuffer.sortBrokenMates does (cwindow.pyx:759-766).  packed=True hands both tables over as
        PLAT_READS_PACKED (one byte per base + exceptions; the device then checks and trims the packed bytes)."""
        out = []
        for fetched, broken in samples:
            c = lambda f, dt: np.ascontiguousarray([f(r) for r in fetched], dtype=dt)
            out.append((ReadTable.from_reads(fetched, packed), ReadTable.from_reads(sorted(broken, key=lambda r: r.matePos), packed),
                        c(lambda r: r.chromID, np.int16), c(lambda r: r.mateChromID, np.int16), c(lambda r: r.insertSize, np.int32)))
        return cls(chrom, start, end, fasta._seq[chrom], out)

    def _c_units(self):
        ss = (_FetchedReads * len(self.samples))()
        for i, (f, b, cid, mcid, ins) in enumerate(self.samples):
            ss[i].fetched, ss[i].broken_mates = f.struct(), b.struct()
            ss[i].chrom_id, ss[i].mate_chrom_id, ss[i].insert_size = cid.ctypes.data, mcid.ctypes.data, ins.ctypes.data
        return (ss,)


class BamRegion(_RegionBase):
    """One region as the integrator holds it after sam_itr_next (include/platypus_caller_bam.h): per sample the uncompressed BAM alignment
    records of the fetch, in fetch order, and of the broken mates, in mate-position order -- each as (data uint8 array, rec_off int64
    array), record i starting at its refID at data[rec_off[i]]."""

    def __init__(self, chrom, start, end, contig_seq, samples):
        super().__init__(chrom, start, end, contig_seq)
        c = lambda t: (np.ascontiguousarray(t[0], dtype=np.uint8), np.ascontiguousarray(t[1], dtype=np.int64))
        self.samples = [(c(f), c(b)) for f, b in samples]    # [((data, rec_off) fetched, (data, rec_off) broken mates)]

    @classmethod
    def from_reads(cls, chrom, start, end, fasta, samples, **layout):
        """samples: per sample (fetched, brokenMates), lists of hostapi.AlignedRead as FetchedRegion.from_reads takes them, encoded as
        records (synth.bam_records; **layout: its names / aux / lead / block_size).  The broken mates are listed in mate-position order."""
        from . import synth
        return cls(chrom, start, end, fasta._seq[chrom],
                   [(synth.bam_records(fetched, **layout), synth.bam_records(sorted(broken, key=lambda r: r.matePos))) for fetched, broken in samples])

    def _c_units(self):
        ss = (_BamSample * len(self.samples))()
        for i, (f, b) in enumerate(self.samples):
            _fill_records(ss[i].fetched, *f)
            _fill_records(ss[i].broken_mates, *b)
        return (ss,)


class BgzfRegion(_BgzfWindow):
    """One region as an index lookup leaves it (include/platypus_caller_bgzf.h): the iterator's window (tid, itr_beg, itr_end) and per
    sample the chunks of the fetch -- each (data uint8 array of whole BGZF blocks, first_uoffset, end_coffset or -1, end_uoffset) -- and
    the broken mates as uncompressed records (data, rec_off), in mate-position order."""

    def __init__(self, chrom, start, end, contig_seq, tid, itr_beg, itr_end, samples):
        super().__init__(chrom, start, end, contig_seq, tid, itr_beg, itr_end)
        self.samples = [([(_u8(d), int(fu), int(ec), int(eu)) for d, fu, ec, eu in chunks],
                         (np.ascontiguousarray(b[0], dtype=np.uint8), np.ascontiguousarray(b[1], dtype=np.int64))) for chunks, b in samples]

    @property
    def compressed_bytes(self):
        return sum(len(d) for chunks, _ in self.samples for d, _, _, _ in chunks)

    @classmethod
    def from_reads(cls, chrom, start, end, fasta, samples, level=6, strategy=0, block_payload=0xff00, decoys=None, itr=None, n_chunks=1, **layout):
        """samples: per sample (fetched, brokenMates), lists of hostapi.AlignedRead as BamRegion.from_reads takes them.  The fetched reads
        become records behind their block_size words (synth.bam_records; **layout: its names / aux), then one BGZF stream of
        block_payload-byte blocks (synth.bgzf_stream at level / strategy; records span blocks wherever a boundary falls), then n_chunks
        chunks of it that meet at a record boundary inside a block both of them hold.  decoys = (in front, behind): reads whose records
        are written around the fetched ones -- what else the blocks of a lookup hold -- for the iterator to skip or stop at.  itr =
        (tid, beg, end): the iterator's window; by default the reads' chromID and the smallest window every fetched read passes."""
        from . import synth
        front, behind = decoys if decoys is not None else ([], [])
        out, window = [], []
        made = dict(chunks=0, records_spanning_blocks=0, blocks=0)        # what the layout came to (for tests and tools)
        for fetched, broken in samples:
            parts = [synth.bam_records(rs, block_size=True, **(layout if rs is fetched else {}))[0].tobytes() for rs in (front, fetched, behind)]
            data = b"".join(parts)
            stream, off = synth.bgzf_stream(data, block_payload=block_payload, level=level, strategy=strategy)
            off = [int(o) for o in off] + [len(stream)]
            # chunk boundaries: record starts among the fetched records, as evenly spread as they come
            rec_at, at = [], len(parts[0])
            while at < len(parts[0]) + len(parts[1]):
                rec_at.append(at)
                at += 4 + int.from_bytes(data[at:at + 4], "little")
            cuts = [rec_at[len(rec_at) * j // n_chunks] for j in range(1, n_chunks)] if len(rec_at) >= n_chunks else []
            made["records_spanning_blocks"] += sum(1 for a, b in zip(rec_at, rec_at[1:] + [at]) if a // block_payload != (b - 1) // block_payload)
            made["blocks"] += len(off) - 1
            chunks, lo = [], 0                                            # lo: inflated offset where the chunk starts
            for hi in cuts + [None]:
                b0 = lo // block_payload
                if hi is None:
                    chunks.append((stream[off[b0]:], lo % block_payload, -1, 0))
                else:
                    b1 = hi // block_payload                              # (the block of the chunk's end: a boundary at a block's end is offset 0 of the next)
                    chunks.append((stream[off[b0]:off[b1 + 1]], lo % block_payload, off[b1] - off[b0], hi % block_payload))
                    lo = hi
            out.append((chunks, synth.bam_records(sorted(broken, key=lambda r: r.matePos))))
            made["chunks"] = max(made["chunks"], len(chunks))
            for r in fetched:
                clip = r.cigarOps[0][1] if r.cigarOps and r.cigarOps[0][0] == 4 else 0
                b = r.pos + clip
                window.append((r.chromID, b, b + (sum(ln for op, ln in r.cigarOps if op in (0, 2, 3, 7, 8)) if r.cigarOps else 1)))
        if itr is None:
            itr = (window[0][0], min(e for _, _, e in window) - 1, max(b for _, b, _ in window) + 1) if window else (0, int(start), int(end))
        reg = cls(chrom, start, end, fasta._seq[chrom], itr[0], itr[1], itr[2], out)
        reg.made = made
        return reg

    def _c_units(self):
        ss = (_BgzfSample * len(self.samples))()
        keep = [_chunk_array(chunks) for chunks, _ in self.samples]
        for i, (chunks, broken) in enumerate(self.samples):
            ss[i].n_chunks, ss[i].chunks = len(chunks), keep[i]
            _fill_records(ss[i].broken_mates, *broken)
        return ss, keep


def merge_by_read_group(entries, key):
    """One merged file's record list from per-read-group lists: entries = [(sample_index, rg_id, reads)], each list in the order `key`
    sorts it; a k-way merge on the next read's key, ties to the earlier entry (list the entries by sample: the lower sample).  Returns
    (reads, aux): the merged reads and each one's aux bytes, RG:Z:<rg_id>."""
    import heapq
    heads = [(key(rs[0]), e, 0) for e, (_, _, rs) in enumerate(entries) if rs]
    heapq.heapify(heads)
    reads, aux = [], []
    while heads:
        _, e, i = heapq.heappop(heads)
        _, rg, rs = entries[e]
        reads.append(rs[i]); aux.append(b"RGZ" + (rg if isinstance(rg, bytes) else rg.encode()) + b"\0")
        if i + 1 < len(rs):
            heapq.heappush(heads, (key(rs[i + 1]), e, i + 1))
    return reads, aux


def _read_pos(r):
    return r.pos                                                # (what a sample's stream must be sorted by: the position moved back over a leading soft clip)


def _file_records(reads, aux):
    """(data, rec_off, rec_len) of reads encoded back to back (synth.bam_records) with their aux bytes."""
    from . import synth
    data, off = synth.bam_records(reads, aux=aux)
    return data, off, np.diff(np.append(off, len(data))).astype(np.int32)


class BamFileRegion(_RegionBase):
    """One region of MERGED files (include/platypus_caller_rg.h): per file the uncompressed records of its fetch, in fetch order, and of
    the broken mates it fetched, in mate-position order -- each as (data uint8 array, rec_off int64 array, rec_len int32 array).  Every
    record carries its read group; NativeCaller.call_bam_regions_rg routes them to samples on the device."""

    UNITS = "files"

    def __init__(self, chrom, start, end, contig_seq, files):
        super().__init__(chrom, start, end, contig_seq)
        c = lambda t: (np.ascontiguousarray(t[0], dtype=np.uint8), np.ascontiguousarray(t[1], dtype=np.int64), np.ascontiguousarray(t[2], dtype=np.int32))
        self.files = [(c(f), c(b)) for f, b in files]

    @property
    def record_bytes(self):
        return sum(len(f[0]) + len(b[0]) for f, b in self.files)

    @classmethod
    def from_reads(cls, chrom, start, end, fasta, files):
        """files: per file a list of (sample_index, rg_id, reads, brokenMates) -- the read groups the file holds, reads in fetch
        (position) order as BamRegion.from_reads takes them.  The groups' records are interleaved by a k-way merge on the next
        record's position (the read's pos; ties to the earlier entry), the broken mates on their mate position, and every record gets
        RG:Z:<rg_id>."""
        out = []
        for entries in files:
            f = merge_by_read_group([(s, g, rs) for s, g, rs, _ in entries], _read_pos)
            b = merge_by_read_group([(s, g, sorted(bs, key=lambda r: r.matePos)) for s, g, _, bs in entries], lambda r: r.matePos)
            out.append((_file_records(*f), _file_records(*b)))
        return cls(chrom, start, end, fasta._seq[chrom], out)

    def _c_units(self):
        ff = (_BamFile * len(self.files))()
        for i, (f, b) in enumerate(self.files):
            _fill_file_records(ff[i].fetched, f)
            _fill_file_records(ff[i].broken_mates, b)
        return (ff,)


class BgzfFileRegion(_BgzfWindow):
    """One region of MERGED files as index lookups leave it (include/platypus_caller_rg.h): the iterator's window and per file the chunks
    of its fetch (as BgzfRegion's samples hold them) and its broken mates as uncompressed records (data, rec_off, rec_len)."""

    UNITS = "files"

    def __init__(self, chrom, start, end, contig_seq, tid, itr_beg, itr_end, files):
        super().__init__(chrom, start, end, contig_seq, tid, itr_beg, itr_end)
        self.files = [([(_u8(d), int(fu), int(ec), int(eu)) for d, fu, ec, eu in chunks],
                       (np.ascontiguousarray(b[0], dtype=np.uint8), np.ascontiguousarray(b[1], dtype=np.int64), np.ascontiguousarray(b[2], dtype=np.int32)))
                      for chunks, b in files]

    @property
    def compressed_bytes(self):
        return sum(len(d) for chunks, _ in self.files for d, _, _, _ in chunks)

    @classmethod
    def from_reads(cls, chrom, start, end, fasta, files, **bgzf):
        """files: as BamFileRegion.from_reads takes them.  Each file's merged records become one BGZF stream and its chunks as
        BgzfRegion.from_reads makes them (**bgzf: its level / strategy / block_payload / decoys / n_chunks); the iterator's window is the
        smallest one every fetched read of every file passes."""
        out, windows = [], []
        for entries in files:
            reads, aux = merge_by_read_group([(s, g, rs) for s, g, rs, _ in entries], _read_pos)
            one = BgzfRegion.from_reads(chrom, start, end, fasta, [(reads, [])], aux=aux, **bgzf)
            b = merge_by_read_group([(s, g, sorted(bs, key=lambda r: r.matePos)) for s, g, _, bs in entries], lambda r: r.matePos)
            out.append((one.samples[0][0], _file_records(*b)))
            if reads:
                windows.append((one.tid, one.itr_beg, one.itr_end))
        itr = (windows[0][0], min(w[1] for w in windows), max(w[2] for w in windows)) if windows else (0, int(start), int(end))
        return cls(chrom, start, end, fasta._seq[chrom], itr[0], itr[1], itr[2], out)

    def _c_units(self):
        ff = (_BgzfFile * len(self.files))()
        keep = [_chunk_array(chunks) for chunks, _ in self.files]
        for i, (chunks, broken) in enumerate(self.files):
            ff[i].n_chunks, ff[i].chunks = len(chunks), keep[i]
            _fill_file_records(ff[i].broken_mates, broken)
        return ff, keep


def region_from_arrays(reg, pin=False, packed=False):
    """RegionReads of a synth.config4_region_arrays() region (every read in `reads`; no badReads / brokenMates)."""
    empty = ReadTable([], [], [0], [], [], [], [], [], [], [0])
    return RegionReads(reg["chrom"], reg["start"], reg["end"], reg["ref"],
                       [(ReadTable(s["seq"], s["qual"], s["off"], s["pos"], s["end"], s["mapq"], s["flags"], s["mate_pos"], s["cigar"], s["cig_off"],
                                   pin=pin, packed=packed), empty, empty) for s in reg["samples"]])


def arrays_from_region_struct(reg):
    """The arrays of a filled plat_region (copies), in the form of synth.config4_region_arrays(): what a region SOURCE handed over
    (tools/synth), for the parity tests that run the same reads through the Python region loop."""
    def arr(ptr, n, dt):
        if not ptr or n == 0:
            return np.zeros(0, dtype=dt)
        return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(np.ctypeslib.as_ctypes_type(dt))), shape=(n,)).copy()

    def table(t):
        n = t.n_reads
        off = arr(t.off, n + 1, np.int64) if n else np.zeros(1, dtype=np.int64)
        nb = int(off[-1])
        seq = arr(t.seq, nb, np.uint8)
        if t.encoding == READS_PACKED:
            qual = (seq >> 2).astype(np.uint8)
            seq = np.frombuffer(b"ACTG", dtype=np.uint8)[seq & 3].copy()
            ne = int(t.n_exceptions)
            if ne:
                ix = arr(t.exc_index, ne, np.int64)
                seq[ix], qual[ix] = arr(t.exc_base, ne, np.uint8), arr(t.exc_qual, ne, np.uint8)
        else:
            qual = arr(t.qual, nb, np.uint8)
        co = arr(t.cig_off, n + 1, np.int32) if n else np.zeros(1, dtype=np.int32)
        return dict(seq=seq, qual=qual, off=off, pos=arr(t.pos, n, np.int32), end=arr(t.end, n, np.int32), mapq=arr(t.mapq, n, np.uint8),
                    flags=arr(t.flags, n, np.int32), mate_pos=arr(t.mate_pos, n, np.int32), cigar=arr(t.cigar, 2 * int(co[-1]), np.int16), cig_off=co)
    return dict(chrom=reg.chrom.decode(), start=int(reg.start), end=int(reg.end), ref=arr(reg.contig_seq, int(reg.contig_len), np.uint8),
                samples=lambda n: [dict(reads=table(reg.samples[i].reads), bad=table(reg.samples[i].bad_reads),
                                        broken=table(reg.samples[i].broken_mates)) for i in range(n)])


def aligned_reads_from_arrays(s):
    """hostapi.AlignedRead objects of one sample of a synth.config4_region_arrays() region (for the Python region loop)."""
    from .hostapi import AlignedRead
    seq, qual, cig = s["seq"].tobytes(), s["qual"].tobytes(), s["cigar"].reshape(-1, 2)
    off, co = s["off"], s["cig_off"]
    return [AlignedRead(seq[off[i]:off[i + 1]], qual[off[i]:off[i + 1]], int(s["pos"][i]), int(s["mapq"][i]), int(s["flags"][i]), end=int(s["end"][i]),
                        cigarOps=[tuple(x) for x in cig[co[i]:co[i + 1]].tolist()], matePos=int(s["mate_pos"][i])) for i in range(len(s["pos"]))]


class TbiInfo(C.Structure):
    """plat_tbi_info (include/platypus_caller_tbi.h)."""
    _fields_ = [(k, C.c_int64) for k in ("n_blocks", "compressed_bytes", "inflated_bytes", "lines", "records", "runs", "contigs", "windows", "device_calls",
                                         "refused_line")] + [("seconds", C.c_double)]


def build(verbose=False):
    """g++ the host library and link it to libplat_mi355x.so (built first if needed)."""
    _lib.build()
    srcs = [os.path.join(HOST_SRC, f) for f in sorted(os.listdir(HOST_SRC)) if f.endswith((".cpp", ".hpp"))]
    srcs.append(os.path.join(_lib.CSRC, "bgzf_inflate.hpp"))           # (the BGZF front end reads block headers with the device's own parser)
    srcs.append(os.path.join(_lib.CSRC, "source_rule.hpp"))            # (... and the host parser of source VCF lines is the device's rule)
    srcs.append(os.path.join(_lib.CSRC, "refcov_rule.hpp"))            # (... as the host's loop over a REFCALL block's positions is)
    srcs.append(os.path.join(_lib.CSRC, "tabix_rule.hpp"))             # (... and the host's walk over a tabix fetch's lines)
    srcs.append(os.path.join(_lib.CSRC, "bgzf_deflate.hpp"))           # (... and the host twin of the BGZF encoder)
    srcs.append(os.path.join(_lib.CSRC, "tabix_index.hpp"))            # (... and the host twin of the tabix indexer, with its finishing stage)
    srcs.append(os.path.join(_lib.CSRC, "index_query.hpp"))            # (... and the flatten and the host twin of the index query)
    srcs.append(os.path.join(_lib.CSRC, "fasta_rule.hpp"))             # (... and the rule, the .fai parse and the host twin of the FASTA fetch)
    srcs.append(os.path.join(_lib.CSRC, "mate_rule.hpp"))              # (... and the rule of the broken-mate fetch)
    if os.path.exists(LIB_PATH) and os.path.getmtime(LIB_PATH) >= max([os.path.getmtime(f) for f in srcs] + [os.path.getmtime(_lib.LIB_PATH)]):
        return LIB_PATH
    # (-O3: the region loop is many small functions over small containers; +10 % windows/s over -O2 on the same box.  No -march: the library
    #  travels between machines; no fast-math: the records' numbers are the reference's)
    cmd = ["g++", "-O3", "-std=c++17", "-fPIC", "-shared", "-pthread", "-ffp-contract=off", "-fvisibility=hidden", os.path.join(HOST_SRC, "region_caller.cpp"), "-o", LIB_PATH,
           "-L" + HERE, "-lplat_mi355x", "-Wl,-rpath,$ORIGIN"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if verbose:
        print(" ".join(cmd), r.stdout, r.stderr)
    if r.returncode != 0:
        raise RuntimeError("building libplat_caller.so failed:\n" + r.stderr[-4000:])
    return LIB_PATH


def _bind(lib):
    lib.plat_caller_default_options.argtypes = [C.POINTER(CallerOptions)]
    lib.plat_caller_default_options.restype = None
    lib.plat_caller_create.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    lib.plat_caller_destroy.argtypes = [C.c_void_p]
    lib.plat_caller_count_cells.argtypes = [C.c_void_p, C.c_int]
    lib.plat_caller_time_kernel.argtypes = [C.c_void_p, C.c_int]
    lib.plat_call_regions.argtypes = [C.c_void_p, C.POINTER(_Region), C.c_int, C.c_int, C.POINTER(C.c_char_p), C.POINTER(CallerOptions),
                                      C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(CallerStats)]
    lib.plat_call_regions_stream.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_char_p), C.POINTER(CallerOptions), C.c_void_p, C.c_void_p,
                                             C.c_int, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(CallerStats)]
    lib.plat_caller_default_qc_options.argtypes = [C.POINTER(CallerQCOptions)]
    lib.plat_caller_default_qc_options.restype = None
    lib.plat_call_fetched_regions.argtypes = [C.c_void_p, C.POINTER(_FetchedRegion), C.c_int, C.c_int, C.POINTER(C.c_char_p), C.POINTER(CallerOptions),
                                              C.POINTER(CallerQCOptions), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(_FetchedRegionInfo),
                                              C.POINTER(CallerStats)]
    lib.plat_call_bam_regions.argtypes = [C.c_void_p, C.POINTER(_BamRegion), C.c_int, C.c_int, C.POINTER(C.c_char_p), C.POINTER(CallerOptions),
                                          C.POINTER(CallerQCOptions), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(_FetchedRegionInfo),
                                          C.POINTER(CallerStats)]
    lib.plat_call_bgzf_regions.argtypes = [C.c_void_p, C.POINTER(_BgzfRegion), C.c_int, C.c_int, C.POINTER(C.c_char_p), C.POINTER(CallerOptions),
                                           C.POINTER(CallerQCOptions), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(_FetchedRegionInfo),
                                           C.POINTER(CallerStats)]
    for name, struct in (("plat_call_bam_regions_rg", _BamRgRegion), ("plat_call_bgzf_regions_rg", _BgzfRgRegion)):
        getattr(lib, name).argtypes = [C.c_void_p, C.POINTER(struct), C.c_int, C.c_int, C.POINTER(_BamReadGroups), C.c_int, C.POINTER(C.c_char_p),
                                       C.POINTER(CallerOptions), C.POINTER(CallerQCOptions), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t),
                                       C.POINTER(_FetchedRegionInfo), C.POINTER(CallerStats)]
    lib.plat_merge_record_texts.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    lib.plat_caller_region_text_lengths.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    lib.plat_merge_region_blocks.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]
    lib.plat_caller_set_source_lines.argtypes = [C.c_void_p, C.POINTER(_SourceLines), C.c_int, C.c_int]
    lib.plat_caller_set_source_blocks.argtypes = [C.c_void_p, C.POINTER(_SourceBlocks), C.c_int, C.c_int, C.POINTER(SourceBlocksInfo)]
    lib.plat_caller_compress_text.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p),
                                              C.POINTER(C.c_size_t), C.c_void_p]
    lib.plat_caller_index_bgzf.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(TbiInfo)]
    lib.plat_index_open.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.POINTER(C.c_void_p)]
    lib.plat_index_close.argtypes = [C.c_void_p]
    lib.plat_index_n_refs.argtypes = [C.c_void_p]
    lib.plat_index_ref_name.argtypes = [C.c_void_p, C.c_int]
    lib.plat_index_ref_name.restype = C.c_char_p
    lib.plat_index_tid.argtypes = [C.c_void_p, C.c_char_p]
    lib.plat_index_query.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p] + [C.POINTER(C.c_void_p)] * 4 + [C.POINTER(IndexQueryInfo)]
    lib.plat_caller_set_source_files.argtypes = [C.c_void_p, C.POINTER(_SourceFile), C.c_int, C.POINTER(_SourceRegion), C.c_int, C.c_int, C.POINTER(SourceBlocksInfo)]
    lib.plat_caller_source_lines.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]
    lib.plat_fasta_open.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.POINTER(C.c_void_p)]
    lib.plat_fasta_close.argtypes = [C.c_void_p]
    lib.plat_fasta_n_refs.argtypes = [C.c_void_p]
    lib.plat_fasta_ref.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]
    lib.plat_fasta_ref_line.argtypes = [C.c_void_p, C.c_int] + [C.POINTER(C.c_int64)] * 3
    lib.plat_fasta_tid.argtypes = [C.c_void_p, C.c_char_p]
    lib.plat_fasta_total_length.argtypes = [C.c_void_p]
    lib.plat_fasta_total_length.restype = C.c_int64
    lib.plat_fasta_load.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(FastaInfo)]
    lib.plat_fasta_contig.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]
    lib.plat_fasta_get_sequences.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p] + [C.POINTER(C.c_void_p)] * 3 + [C.POINTER(FastaInfo)]
    lib.plat_fasta_get_character.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.POINTER(C.c_uint8), C.POINTER(C.c_int32)]
    lib.plat_bam_file_open.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_size_t, C.c_char_p, C.POINTER(C.c_void_p)]
    for name in ("close", "n_refs", "n_read_groups", "n_samples"):
        getattr(lib, "plat_bam_file_" + name).argtypes = [C.c_void_p]
    lib.plat_bam_file_ref_name.argtypes = [C.c_void_p, C.c_int]
    lib.plat_bam_file_ref_name.restype = C.c_char_p
    lib.plat_bam_file_ref_len.argtypes = [C.c_void_p, C.c_int]
    lib.plat_bam_file_ref_len.restype = C.c_int64
    lib.plat_bam_file_tid.argtypes = [C.c_void_p, C.c_char_p]
    lib.plat_bam_file_header_text.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
    lib.plat_bam_file_header_text.restype = C.c_void_p
    lib.plat_bam_file_read_group.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_char_p)]
    lib.plat_bam_file_sample.argtypes = [C.c_void_p, C.c_int]
    lib.plat_bam_file_sample.restype = C.c_char_p
    lib.plat_bam_file_header_raised.argtypes = [C.c_void_p, C.POINTER(C.c_char_p)]
    lib.plat_bam_file_n_header_sq.argtypes = [C.c_void_p]
    lib.plat_bam_file_header_sq.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int64)]
    lib.plat_bam_file_index.argtypes = [C.c_void_p]
    lib.plat_bam_file_index.restype = C.c_void_p
    lib.plat_bam_files_plan.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.POINTER(_BamPlan))]
    lib.plat_bam_plan_free.argtypes = [C.POINTER(_BamPlan)]
    lib.plat_bam_plan_free.restype = None
    lib.plat_bam_files_fetch_plan.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.POINTER(_BamCallRegion), C.c_int, C.POINTER(C.POINTER(_BamFetchPlan))]
    lib.plat_bam_fetch_plan_free.argtypes = [C.POINTER(_BamFetchPlan)]
    lib.plat_bam_fetch_plan_free.restype = None
    lib.plat_call_bam_files.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.POINTER(_BamCallRegion), C.c_int, C.POINTER(CallerOptions),
                                        C.POINTER(CallerQCOptions), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(_FetchedRegionInfo),
                                        C.POINTER(CallerStats)]
    lib.plat_call_bam_files_mates.argtypes = lib.plat_call_bam_files.argtypes
    lib.plat_bam_files_mates_plan.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.POINTER(_BamCallRegion), C.c_int, C.POINTER(_BamFetchPlan), C.POINTER(CallerOptions),
                                              C.POINTER(C.POINTER(_BamMatesPlan))]
    lib.plat_bam_mates_plan_free.argtypes = [C.POINTER(_BamMatesPlan)]
    lib.plat_bam_mates_plan_free.restype = None
    lib.plat_caller_free.argtypes = [C.c_void_p]
    lib.plat_caller_free.restype = None
    lib.plat_caller_last_error.argtypes = [C.c_void_p]
    lib.plat_caller_last_error.restype = C.c_char_p
    return lib


_caller_lib = None


def load():
    global _caller_lib
    if _caller_lib is None:
        _lib.load()                                             # (torch's HIP runtime first, see _lib.load)
        if not os.path.exists(LIB_PATH):
            build()
        _caller_lib = _bind(C.CDLL(LIB_PATH))
    return _caller_lib


def _native_text(lib, ptr, length, raw):
    """What a call hands back for a malloc'ed text: str; bytes (raw=True); or, raw="view", the block itself as a ctypes char array (no
    copy; freed with the array) -- a whole-genome share is ~100 MB of record text and every copy of it is a pass through memory."""
    if raw == "view":
        import weakref
        arr = (C.c_char * length).from_address(ptr.value) if length else (C.c_char * 0)()
        if length:
            weakref.finalize(arr, lib.plat_caller_free, C.c_void_p(ptr.value))
        else:
            lib.plat_caller_free(ptr)
        return arr
    try:
        out = C.string_at(ptr, length)
        return out if raw else out.decode("ascii")
    finally:
        lib.plat_caller_free(ptr)


def text_bytes(x):
    """bytes of a text returned with raw=True / raw="view"."""
    return x if isinstance(x, bytes) else bytes(x)


def merge_record_texts(texts, lib=None, raw=False):
    """runner.py:301-352 natively: k-way merge of record texts (bytes, each sorted by (chromosome key, position)) -> one str (bytes with raw=True)."""
    lib = lib if lib is not None else load()
    n = len(texts)
    keep = [t if isinstance(t, (bytes, C.Array)) else bytes(t) for t in texts]
    arr = (C.c_void_p * max(n, 1))(*[C.cast(C.c_char_p(t), C.c_void_p).value if isinstance(t, bytes) else C.addressof(t) for t in keep])
    lens = (C.c_size_t * max(n, 1))(*[len(t) for t in keep])
    out, length = C.c_void_p(), C.c_size_t()
    rc = lib.plat_merge_record_texts(arr, lens, n, C.byref(out), C.byref(length))
    del keep
    if rc != 0:
        raise _lib.PlatypusDeviceError(rc, "merge failed", "plat_merge_record_texts")
    return _native_text(lib, out, length.value, raw)


def text_address(t):
    """(address, length) of a text held as bytes, a ctypes array (raw="view"), a numpy uint8 array or a CPU torch uint8 tensor."""
    if isinstance(t, bytes):
        return C.cast(C.c_char_p(t), C.c_void_p).value or 0, len(t)
    if isinstance(t, C.Array):
        return C.addressof(t), len(t)
    if hasattr(t, "data_ptr"):
        return int(t.data_ptr()), int(t.numel())
    return int(t.ctypes.data), int(t.size)


def merge_region_blocks(texts, lengths, keys, lib=None):
    """The job's merge when every text is made of whole regions that do not interleave (the native region loop's output): texts[r] = rank
    r's text, lengths[r] = bytes of each of its regions' records (plat_caller_region_text_lengths), keys[r] = (chromosome key, start, end) of
    each of its regions.  The regions' blocks are put in (chromosome key, start) order -- runner.py:301-352's order -- by block copies on
    up to 16 threads, no line is looked at.  Returns the merged text (raw view), or None when two regions overlap (the caller then merges
    line by line: merge_record_texts)."""
    import numpy as np
    lib = lib if lib is not None else load()
    blocks = []
    for r, (lens, ks) in enumerate(zip(lengths, keys)):
        base, _ = text_address(texts[r])
        off = 0
        for ln, k in zip(lens, ks):
            blocks.append((k[0], k[1], k[2], r, base + off, int(ln)))
            off += int(ln)
    blocks.sort(key=lambda b: (b[0], b[1], b[3]))
    for a, b in zip(blocks, blocks[1:]):
        if a[0] == b[0] and a[2] > b[1] and a[5] and b[5]:
            return None                                              # overlapping regions: their records may interleave
    n = len(blocks)
    src = np.array([b[4] for b in blocks], dtype=np.uint64)
    ln = np.array([b[5] for b in blocks], dtype=np.uint64)
    at = np.zeros(n, dtype=np.uint64)
    if n:
        at[1:] = np.cumsum(ln)[:-1]
    total = int(ln.sum())
    out = C.c_void_p()
    rc = lib.plat_merge_region_blocks(n, src.ctypes.data, ln.ctypes.data, at.ctypes.data, total, C.byref(out))
    if rc != 0:
        raise _lib.PlatypusDeviceError(rc, "merge failed", "plat_merge_region_blocks")
    return _native_text(lib, out, total, "view")


class BlockOrder:
    """merge_region_blocks with everything that depends only on the job's region list worked out ONCE (before a timed region): the order
    of all blocks.  plan = BlockOrder(keys) with keys[r] = [(chromosome key, start, end), ...] of rank r's regions; plan.merge(texts,
    lengths) then costs two small numpy passes and the block copies.  plan.ok is False when regions overlap."""

    def __init__(self, keys):
        import numpy as np
        flat = [(k[0], k[1], k[2], r, j) for r, ks in enumerate(keys) for j, k in enumerate(ks)]
        order = sorted(range(len(flat)), key=lambda i: (flat[i][0], flat[i][1], flat[i][3]))
        self.ok = all(not (flat[a][0] == flat[b][0] and flat[a][2] > flat[b][1]) for a, b in zip(order, order[1:]))
        self.rank = np.array([flat[i][3] for i in order], dtype=np.int64)
        self.index = np.array([flat[i][4] for i in order], dtype=np.int64)
        self.counts = [len(ks) for ks in keys]
        # one rank whose list is already in (chromosome key, start) order: its text IS the merged text (runner.py:301-352 merges per-process
        # files; a job of one process has one), nothing is copied
        self.identity = len(keys) == 1 and bool(np.array_equal(self.index, np.arange(len(self.index))))

    def merge(self, texts, lengths, lib=None):
        import numpy as np
        if self.identity and self.ok and len(texts) == 1:
            assert int(np.asarray(lengths[0], dtype=np.int64).sum()) == text_address(texts[0])[1], "region lengths do not add up to the text"
            return texts[0]
        lib = lib if lib is not None else load()
        starts = []
        for r, lens in enumerate(lengths):
            lens = np.asarray(lens, dtype=np.int64)
            assert len(lens) == self.counts[r]
            base, size = text_address(texts[r])
            st = np.zeros(len(lens), dtype=np.int64)
            if len(lens):
                st[1:] = np.cumsum(lens)[:-1]
            assert int(lens.sum()) == size, "region lengths do not add up to the text"
            starts.append((base + st, lens))
        n = len(self.rank)
        src = np.zeros(n, dtype=np.uint64)
        ln = np.zeros(n, dtype=np.uint64)
        for r, (st, lens) in enumerate(starts):
            m = self.rank == r
            src[m] = st[self.index[m]].astype(np.uint64)
            ln[m] = lens[self.index[m]].astype(np.uint64)
        at = np.zeros(n, dtype=np.uint64)
        if n:
            at[1:] = np.cumsum(ln)[:-1]
        total = int(ln.sum())
        out = C.c_void_p()
        rc = lib.plat_merge_region_blocks(n, src.ctypes.data, ln.ctypes.data, at.ctypes.data, total, C.byref(out))
        if rc != 0:
            raise _lib.PlatypusDeviceError(rc, "merge failed", "plat_merge_region_blocks")
        return _native_text(lib, out, total, "view")


class NativeIndex:
    """plat_index (include/platypus_caller_index.h): a .tbi or .bai opened on a NativeCaller; close it before the caller."""

    def __init__(self, caller, handle):
        self.caller, self.h = caller, handle

    def close(self):
        if getattr(self, "h", None) and getattr(self.caller, "h", None):
            self.caller.lib.plat_index_close(self.h)
        self.h = None

    @property
    def n_refs(self):
        return self.caller.lib.plat_index_n_refs(self.h)

    def ref_name(self, tid):
        return self.caller.lib.plat_index_ref_name(self.h, int(tid))

    def tid(self, name):
        """-1 when the index does not hold the name (a name with a NUL byte cannot be one)."""
        name = name if isinstance(name, bytes) else name.encode()
        return -1 if b"\x00" in name else self.caller.lib.plat_index_tid(self.h, name)


class NativeFasta:
    """plat_fasta (include/platypus_caller_fasta.h): a FASTA file's bytes and its .fai opened on a NativeCaller; close it before the caller.
    The file's bytes are kept alive by this object."""

    def __init__(self, caller, handle, keep):
        self.caller, self.h, self._keep = caller, handle, keep
        self.info = None

    def _check(self, rc, entry):
        if rc != 0:
            raise _lib.PlatypusDeviceError(rc, (self.caller.lib.plat_caller_last_error(self.caller.h) or b"").decode(errors="replace"), entry)

    def close(self):
        if getattr(self, "h", None) and getattr(self.caller, "h", None):
            self.caller.lib.plat_fasta_close(self.h)
        self.h = None

    @property
    def refs(self):
        """[(name bytes, SeqLength, StartPos, LineLength, FullLineLength)] in file order."""
        lib, out = self.caller.lib, []
        for i in range(lib.plat_fasta_n_refs(self.h)):
            name, v = C.c_void_p(), [C.c_int64() for _ in range(4)]
            self._check(lib.plat_fasta_ref(self.h, i, C.byref(name), C.byref(v[0])), "plat_fasta_ref")
            self._check(lib.plat_fasta_ref_line(self.h, i, C.byref(v[1]), C.byref(v[2]), C.byref(v[3])), "plat_fasta_ref_line")
            out.append((C.string_at(name),) + tuple(x.value for x in v))
        return out

    def tid(self, name):
        """-1 when the index does not hold the name (a name with a NUL byte cannot be one)."""
        name = name if isinstance(name, bytes) else name.encode()
        return -1 if b"\x00" in name else self.caller.lib.plat_fasta_tid(self.h, name)

    @property
    def total_length(self):
        return self.caller.lib.plat_fasta_total_length(self.h)

    def load(self, tids=()):
        """plat_fasta_load: the contigs `tids` (none: all) fetched whole in one device batch; self.info describes the call."""
        t = np.ascontiguousarray(list(tids), dtype=np.int32)
        inf = FastaInfo()
        self._check(self.caller.lib.plat_fasta_load(self.h, t.ctypes.data if len(t) else None, len(t), C.byref(inf)), "plat_fasta_load")
        self.info = {k: getattr(inf, k) for k, _ in inf._fields_}

    def contig_pointers(self, tid):
        """plat_fasta_contig: (host address, device address or None, length) -- what goes into plat_region.contig_seq / dev_contig_seq / contig_len."""
        host, dev, n = C.c_void_p(), C.c_void_p(), C.c_int64()
        self._check(self.caller.lib.plat_fasta_contig(self.h, int(tid), C.byref(host), C.byref(dev), C.byref(n)), "plat_fasta_contig")
        return host.value, dev.value, n.value

    def contig(self, tid):
        """(the contig's bases as a uint8 array over the object's own host memory -- no copy, valid until close --, its device address or None)."""
        host, dev, n = self.contig_pointers(tid)
        arr = np.ctypeslib.as_array(C.cast(host, C.POINTER(C.c_uint8)), shape=(n,)) if n else np.zeros(0, dtype=np.uint8)
        return arr, dev

    def get_sequences(self, queries, info=False):
        """plat_fasta_get_sequences: queries [(tid, beg, end)] in one device batch.  Returns per query the bytes getSequence returns, or the
        status (an int, _lib.FASTA_*) where it does not return."""
        n = len(queries)
        t = np.ascontiguousarray([q[0] for q in queries], dtype=np.int32)
        b, e = (np.ascontiguousarray([q[k] for q in queries], dtype=np.int64) for k in (1, 2))
        first, data, status, inf = C.c_void_p(), C.c_void_p(), C.c_void_p(), FastaInfo()
        self._check(self.caller.lib.plat_fasta_get_sequences(self.h, n, t.ctypes.data, b.ctypes.data, e.ctypes.data, C.byref(first), C.byref(data), C.byref(status),
                                                             C.byref(inf)), "plat_fasta_get_sequences")
        fi = np.ctypeslib.as_array(C.cast(first, C.POINTER(C.c_int64)), shape=(n + 1,)).copy()
        st = np.ctypeslib.as_array(C.cast(status, C.POINTER(C.c_int32)), shape=(n,)).copy() if n else np.zeros(0, dtype=np.int32)
        blob = C.string_at(data, int(fi[n])) if fi[n] else b""
        out = [blob[fi[k]:fi[k + 1]] if st[k] == 0 else int(st[k]) for k in range(n)]
        self.info = {k: getattr(inf, k) for k, _ in inf._fields_}
        return (out, self.info) if info else out

    def get_character(self, tid, pos):
        c, n = C.c_uint8(), C.c_int32()
        self._check(self.caller.lib.plat_fasta_get_character(self.h, int(tid), int(pos), C.byref(c), C.byref(n)), "plat_fasta_get_character")
        return bytes([c.value]) if n.value else b""


class FastaContigRegion:
    """A region class over another (RegionReads, FetchedRegion, ...) whose contig is a NativeFasta's: contig_seq, dev_contig_seq and
    contig_len come from plat_fasta_contig."""

    def __init__(self, region, fasta, tid):
        self.region, self.chrom, self.start, self.end = region, region.chrom, region.start, region.end
        self.pointers = fasta.contig_pointers(tid)
        self._fasta = fasta

    def __getattr__(self, name):
        return getattr(self.region, name)

    def fill(self, a, n_units):
        self.region.fill(a, n_units)
        a.contig_seq, a.dev_contig_seq, a.contig_len = self.pointers


class NativeBamFile:
    """plat_bamfile (include/platypus_caller_bamfile.h): a BAM file's bytes and its .bai opened on a NativeCaller; close it before the
    caller.  The file's bytes are kept alive by this object."""

    def __init__(self, caller, handle, keep, file_name):
        self.caller, self.h, self._keep, self.file_name = caller, handle, keep, file_name

    def close(self):
        if getattr(self, "h", None) and getattr(self.caller, "h", None):
            self.caller.lib.plat_bam_file_close(self.h)
        self.h = None

    @property
    def data(self):
        return self._keep

    @property
    def refs(self):
        """The reference names (bytes) in header order."""
        lib = self.caller.lib
        return [lib.plat_bam_file_ref_name(self.h, t) for t in range(lib.plat_bam_file_n_refs(self.h))]

    @property
    def lengths(self):
        lib = self.caller.lib
        return [lib.plat_bam_file_ref_len(self.h, t) for t in range(lib.plat_bam_file_n_refs(self.h))]

    def tid(self, name):
        """-1 when the header does not hold the name (a name with a NUL byte cannot be one)."""
        name = name if isinstance(name, bytes) else name.encode()
        return -1 if b"\x00" in name else self.caller.lib.plat_bam_file_tid(self.h, name)

    @property
    def header_text(self):
        n = C.c_int64()
        p = self.caller.lib.plat_bam_file_header_text(self.h, C.byref(n))
        return C.string_at(p, n.value) if n.value else b""

    @property
    def read_groups(self):
        """[(ID, SM)] (bytes) in header order: what this file enters into the call's read-group table."""
        lib, out = self.caller.lib, []
        for i in range(lib.plat_bam_file_n_read_groups(self.h)):
            a, b = C.c_char_p(), C.c_char_p()
            lib.plat_bam_file_read_group(self.h, i, C.byref(a), C.byref(b))
            out.append((a.value, b.value))
        return out

    @property
    def samples(self):
        """The samples (bytes) this file adds to the sample list."""
        lib = self.caller.lib
        return [lib.plat_bam_file_sample(self.h, i) for i in range(lib.plat_bam_file_n_samples(self.h))]

    @property
    def header_sq(self):
        """[(SN bytes, LN)] of the header text's @SQ lines as getRegions reads them; None where that read raises."""
        lib = self.caller.lib
        n = lib.plat_bam_file_n_header_sq(self.h)
        if n < 0:
            return None
        out = []
        for i in range(n):
            name, length = C.c_char_p(), C.c_int64()
            lib.plat_bam_file_header_sq(self.h, i, C.byref(name), C.byref(length))
            out.append((name.value, length.value))
        return out

    @property
    def header_raised(self):
        """None, or the reference's words for why reading the header raised (the file's sample is then its name's)."""
        why = C.c_char_p()
        return (why.value or b"").decode(errors="replace") if self.caller.lib.plat_bam_file_header_raised(self.h, C.byref(why)) == 1 else None


class BamFilesRegion(_RegionBase):
    """One region of NativeCaller.call_bam_files: chrom:start-end and the contig (wrap it in FastaContigRegion for a NativeFasta's)."""

    def fill(self, a, n_units=0):
        if self._c is None:
            self._c = (self.chrom.encode(),)
        a.chrom, a.contig_seq, a.contig_len = self._c[0], self.contig.ctypes.data, len(self.contig)
        a.start, a.end = self.start, self.end


class NativeCaller:
    """plat_caller: `workers` threads, each with its own plat_ctx and stream on `device`; `regions_per_chunk` regions go through
    the device stages together."""

    def __init__(self, device=0, workers=4, regions_per_chunk=4, lib=None):
        self.lib = lib if lib is not None else load()
        h = C.c_void_p()
        rc = self.lib.plat_caller_create(device, workers, regions_per_chunk, C.byref(h))
        if rc != 0:
            raise _lib.PlatypusDeviceError(rc, "plat_caller_create failed (no GPU? the native region loop has no CPU fallback)", "plat_caller_create")
        self.h = h
        self.stats = None

    def time_kernel(self, kernel_id):
        """Measurement switch (plat_caller_time_kernel): the calls that follow time this one kernel (id of plat_kernel_timer_name; -1: none) inside the
        ordinary asynchronous runs; stats["kernel_ms"][id] / ["kernel_launches"][id] hold its summed duration and launches."""
        self.lib.plat_caller_time_kernel(self.h, int(kernel_id))

    def count_cells(self, on=True):
        """Measurement switch (plat_caller_count_cells): the calls that follow count the reference's DPs and band cells into stats
        (synchronous likelihood batches: not for timed runs)."""
        rc = self.lib.plat_caller_count_cells(self.h, 1 if on else 0)
        if rc != 0:
            raise _lib.PlatypusDeviceError(rc, "plat_caller_count_cells", "plat_caller_count_cells")

    def close(self):
        if getattr(self, "h", None):
            self.lib.plat_caller_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_source_lines(self, source_lines, long_haps=0):
        """plat_caller_set_source_lines: the source VCF lines of the NEXT call, per region of its list -- bytes (the text the region's fetches
        returned, the files' fetches back to back) or a list of bytes (one per source file).  Returns what keeps the memory alive: hold it
        until that call has returned.  The lines are gone when that call returns."""
        texts = [b"".join(t) if isinstance(t, (list, tuple)) else bytes(t) for t in source_lines]
        arr = (_SourceLines * max(len(texts), 1))()
        for k, t in enumerate(texts):
            arr[k].text, arr[k].len = C.cast(C.c_char_p(t), C.c_void_p).value if t else None, len(t)
        rc = self.lib.plat_caller_set_source_lines(self.h, arr, len(texts), int(long_haps))
        if rc != 0:
            raise _lib.PlatypusDeviceError(rc, "plat_caller_set_source_lines", "plat_caller_set_source_lines")
        return texts, arr

    def set_source_blocks(self, source_blocks, long_haps=0):
        """plat_caller_set_source_blocks: the source VCF lines of the NEXT call, fetched on the device from BGZF blocks.  Per region of its
        list a list of fetches, one per source file in file order: (seq_name, itr_beg, itr_end, chunks), chunks as BgzfRegion takes them --
        [(data uint8 array, first_uoffset, end_coffset, end_uoffset)] (tabixindex.TabixFile.fetch_blocks makes one).  The blocks are read
        inside this call; self.source_blocks_info describes it (plat_source_blocks_info as a dict)."""
        arr = (_SourceBlocks * max(len(source_blocks), 1))()
        keep = []
        for k, fetches in enumerate(source_blocks):
            ff = (_TabixFetch * max(len(fetches), 1))()
            for j, (name, beg, end, chunks) in enumerate(fetches):
                chunks = [(_u8(d), fu, ec, eu) for d, fu, ec, eu in chunks]
                cc = _chunk_array(chunks)
                ff[j].seq_name, ff[j].itr_beg, ff[j].itr_end = name if isinstance(name, bytes) else name.encode(), int(beg), int(end)
                ff[j].n_chunks, ff[j].chunks = len(chunks), C.cast(cc, C.c_void_p)
                keep.append((chunks, cc))
            arr[k].n_fetches, arr[k].fetches = len(fetches), C.cast(ff, C.c_void_p)
            keep.append(ff)
        info = SourceBlocksInfo()
        rc = self.lib.plat_caller_set_source_blocks(self.h, arr, len(source_blocks), int(long_haps), C.byref(info))
        del keep
        if rc != 0:
            raise _lib.PlatypusDeviceError(rc, (self.lib.plat_caller_last_error(self.h) or b"").decode(), "plat_caller_set_source_blocks")
        self.source_blocks_info = {k: getattr(info, k) for k, _ in info._fields_}

    def open_index(self, raw, kind="tbi"):
        """plat_index_open: the bytes of a .tbi (BGZF, as on disk) or a .bai flattened on the host and uploaded once.  Returns a NativeIndex."""
        raw = bytes(raw)
        h = C.c_void_p()
        rc = self.lib.plat_index_open(self.h, raw, len(raw), INDEX_KINDS[kind], C.byref(h))
        if rc != 0:
            raise _lib.PlatypusDeviceError(rc, (self.lib.plat_caller_last_error(self.h) or b"").decode(), "plat_index_open")
        return NativeIndex(self, h)

    def open_fasta(self, file_bytes, fai_bytes, parseNCBI=0):
        """plat_fasta_open: a FASTA file's bytes (bytes, or a uint8 array / mapped file, which is not copied) and its .fai's.  Returns a NativeFasta."""
        data = _u8(file_bytes)
        fai = bytes(fai_bytes)
        h = C.c_void_p()
        rc = self.lib.plat_fasta_open(self.h, data.ctypes.data if len(data) else None, len(data), fai, len(fai), int(parseNCBI), C.byref(h))
        if rc != 0:
            raise _lib.PlatypusDeviceError(rc, (self.lib.plat_caller_last_error(self.h) or b"").decode(errors="replace"), "plat_fasta_open")
        return NativeFasta(self, h, data)

    def _error(self, rc, entry):
        return _lib.PlatypusDeviceError(rc, (self.lib.plat_caller_last_error(self.h) or b"").decode(errors="replace"), entry)

    def open_bam(self, data, bai, file_name):
        """plat_bam_file_open: a BAM file's bytes (bytes, or a uint8 array / mapped file, which is not copied), its .bai's bytes and the
        name the sample falls back to.  Returns a NativeBamFile."""
        keep = _u8(data)
        bai = bytes(bai)
        name = file_name if isinstance(file_name, bytes) else file_name.encode()
        h = C.c_void_p()
        rc = self.lib.plat_bam_file_open(self.h, keep.ctypes.data if len(keep) else None, len(keep), bai, len(bai), name, C.byref(h))
        if rc != 0:
            raise self._error(rc, "plat_bam_file_open")
        return NativeBamFile(self, h, keep, file_name)

    @staticmethod
    def _bam_handles(files):
        return (C.c_void_p * max(len(files), 1))(*[f.h for f in files])

    def bam_plan(self, files):
        """plat_bam_files_plan: loadBAMData's decision for these NativeBamFiles.  Returns dict(mode "presplit" / "merged", samples [bytes]
        sorted, sample_file [file index per sample] or None, read_groups [(ID bytes, sample index)])."""
        plan = C.POINTER(_BamPlan)()
        rc = self.lib.plat_bam_files_plan(self._bam_handles(files), len(files), C.byref(plan))
        if rc != 0:
            raise self._error(rc, "plat_bam_files_plan")
        try:
            p = plan.contents
            groups = np.ctypeslib.as_array(C.cast(p.groups.sample, C.POINTER(C.c_int32)), shape=(p.groups.n_groups,)).tolist() if p.groups.n_groups else []
            return dict(mode=BAM_FILES_MODES[p.mode], samples=[p.sample_names[s] for s in range(p.n_samples)],
                        sample_file=[p.sample_file[s] for s in range(p.n_samples)] if p.sample_file else None,
                        read_groups=[(p.groups.id[g], groups[g]) for g in range(p.groups.n_groups)])
        finally:
            self.lib.plat_bam_plan_free(plan)

    @staticmethod
    def _bam_regions(regions):
        """The plat_bam_call_region array of region objects (fill) or (chrom, start, end) tuples, and what keeps it alive."""
        arr = (_BamCallRegion * max(len(regions), 1))()
        keep = []
        for k, r in enumerate(regions):
            if isinstance(r, (tuple, list)):
                chrom = r[0] if isinstance(r[0], bytes) else r[0].encode()
                keep.append(chrom)
                arr[k].chrom, arr[k].start, arr[k].end = chrom, int(r[1]), int(r[2])
            else:
                r.fill(arr[k], 0)
        return arr, keep

    def bam_fetch_plan(self, files, regions):
        """plat_bam_files_fetch_plan for regions [(chrom, start, end)]: per region and file dict(tid, itr_beg, itr_end, chunks), a chunk as
        (its offset in the file, data_len, first_uoffset, end_coffset, end_uoffset); self.bam_fetch_info holds the plan's counts."""
        arr, keep = self._bam_regions(regions)
        plan = C.POINTER(_BamFetchPlan)()
        rc = self.lib.plat_bam_files_fetch_plan(self._bam_handles(files), len(files), arr, len(regions), C.byref(plan))
        del keep
        if rc != 0:
            raise self._error(rc, "plat_bam_files_fetch_plan")
        try:
            p = plan.contents
            base = [f.data.ctypes.data for f in files]
            out = []
            for k in range(p.n_regions):
                per = []
                for f in range(p.n_files):
                    ft = p.fetches[k * p.n_files + f]
                    per.append(dict(tid=ft.tid, itr_beg=ft.itr_beg, itr_end=ft.itr_end,
                                    chunks=[(ft.chunks[q].data - base[f], ft.chunks[q].data_len, ft.chunks[q].first_uoffset, ft.chunks[q].end_coffset,
                                             ft.chunks[q].end_uoffset) for q in range(ft.n_chunks)]))
                out.append(per)
            self.bam_fetch_info = {k: getattr(p, k) for k in ("queries", "handed_over", "chunks", "device_calls", "seconds")}
            return out
        finally:
            self.lib.plat_bam_fetch_plan_free(plan)

    def bam_mates_plan(self, files, regions, options):
        """plat_bam_files_mates_plan for regions [(chrom, start, end)]: the broken-mate fetch of loadBAMData (platypusutils.pyx:522-559) on
        the device.  Per region and file dict(n_coords, queries [(tid, start, end)], records [bytes] in mate-position order);
        self.bam_mates_info holds the plan's counters and loaded [per region: 0 where round one reached maxReads]."""
        arr, keep = self._bam_regions(regions)
        handles = self._bam_handles(files)
        fetch = C.POINTER(_BamFetchPlan)()
        rc = self.lib.plat_bam_files_fetch_plan(handles, len(files), arr, len(regions), C.byref(fetch))
        if rc != 0:
            raise self._error(rc, "plat_bam_files_fetch_plan")
        plan = C.POINTER(_BamMatesPlan)()
        try:
            o = CallerOptions.from_options(options)
            rc = self.lib.plat_bam_files_mates_plan(handles, len(files), arr, len(regions), fetch, C.byref(o), C.byref(plan))
            if rc != 0:
                raise self._error(rc, "plat_bam_files_mates_plan")
            p = plan.contents
            out = []
            for k in range(p.n_regions):
                per = []
                for f in range(p.n_files):
                    u = p.units[k * p.n_files + f]
                    r = u.mates.records
                    n = r.n_records
                    off = np.ctypeslib.as_array(C.cast(r.rec_off, C.POINTER(C.c_int64)), shape=(n,)) if n else []
                    ln = np.ctypeslib.as_array(C.cast(u.mates.rec_len, C.POINTER(C.c_int32)), shape=(n,)) if n else []
                    per.append(dict(n_coords=u.n_coords, queries=[(u.queries[q].tid, u.queries[q].start, u.queries[q].end) for q in range(u.n_queries)],
                                    records=[C.string_at(r.data + int(off[i]), int(ln[i])) for i in range(n)]))
                out.append(per)
            self.bam_mates_info = {k: getattr(p, k) for k in ("coords", "queries", "chunks", "records_looked_at", "records_kept", "device_calls", "input_bytes", "seconds")}
            self.bam_mates_info["loaded"] = [p.loaded[k] for k in range(p.n_regions)]
            return out
        finally:
            del keep
            if plan:
                self.lib.plat_bam_mates_plan_free(plan)
            self.lib.plat_bam_fetch_plan_free(fetch)

    def call_bam_files_mates(self, files, regions, options, source_lines=None, source_blocks=None, source_files=None):
        """plat_call_bam_files_mates: call_bam_files with the broken mates fetched -- with options.assemble and options.assembleBrokenPairs
        set, the mates plan's records go into the BGZF call as broken_mates; with either 0 it is call_bam_files."""
        return self.call_bam_files(files, regions, options, source_lines, source_blocks, source_files, _entry="plat_call_bam_files_mates")

    def call_bam_files(self, files, regions, options, source_lines=None, source_blocks=None, source_files=None, _entry="plat_call_bam_files"):
        """plat_call_bam_files: files [NativeBamFile], regions [BamFilesRegion, or FastaContigRegion over one].  The samples, the mode, the
        windows and the chunks are the library's (bam_plan, bam_fetch_plan); from there it is call_bgzf_regions or call_bgzf_regions_rg:
        the same text, rlen, self.loaded and self.read_counts.  self.sample_names holds the call's samples (str)."""
        n = len(regions)
        names = self.bam_plan(files)["samples"]
        nS = len(names)
        if source_files is not None:
            if source_lines is not None or source_blocks is not None:
                raise ValueError("source_lines, source_blocks and source_files are three ways to say the same thing: give one")
            keep_source = self.set_source_files(source_files, [(r.chrom, r.start, r.end) for r in regions], getattr(options, "longHaps", 0))
        else:
            keep_source = self._set_source(source_lines, source_blocks, options)
        arr, keep = self._bam_regions(regions)
        o, text, length, st = CallerOptions.from_options(options), C.c_void_p(), C.c_size_t(), CallerStats()
        q = CallerQCOptions.from_options(options)
        counts = np.zeros((max(n, 1), nS, 10), dtype=np.int32)
        info = (_FetchedRegionInfo * max(n, 1))()
        for k in range(n):
            info[k].sample_counts = counts[k].ctypes.data
        rc = getattr(self.lib, _entry)(self.h, self._bam_handles(files), len(files), arr, n, C.byref(o), C.byref(q), C.byref(text), C.byref(length), info, C.byref(st))
        del keep_source, keep
        out = self._finish(rc, _entry, text, length, o, st, options)
        self.sample_names = [s.decode(errors="surrogateescape") for s in names]
        self.loaded = [int(info[k].loaded) for k in range(n)]
        self.read_counts = counts[:n]
        return out

    def query_index(self, index, queries, info=False):
        """plat_index_query: queries [(tid, beg, end)] in one device batch.  Returns per query the chunk list [(u, v)] ti_iter_query returns,
        None where it returns no iterator; with info=True (that, plat_index_query_info as a dict)."""
        n = len(queries)
        q = np.ascontiguousarray(np.asarray(queries, dtype=np.int32).reshape(n, 3).T)
        first, u, v, count, inf = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p(), IndexQueryInfo()
        rc = self.lib.plat_index_query(index.h, n, q[0].ctypes.data, q[1].ctypes.data, q[2].ctypes.data, C.byref(first), C.byref(u), C.byref(v), C.byref(count), C.byref(inf))
        if rc != 0:
            raise _lib.PlatypusDeviceError(rc, (self.lib.plat_caller_last_error(self.h) or b"").decode(), "plat_index_query")
        take = lambda ptr, k, dt: np.ctypeslib.as_array(C.cast(ptr, C.POINTER(np.ctypeslib.as_ctypes_type(dt))), shape=(k,)).copy() if k and ptr.value else np.zeros(0, dtype=dt)
        fi, cn = take(first, n + 1, np.int64), take(count, n, np.int32)
        total = int(fi[n]) if n else 0
        uu, vv = take(u, total, np.uint64).tolist(), take(v, total, np.uint64).tolist()
        out = [None if cn[k] < 0 else list(zip(uu[fi[k]:fi[k + 1]], vv[fi[k]:fi[k + 1]])) for k in range(n)]
        return (out, {k: getattr(inf, k) for k, _ in inf._fields_}) if info else out

    def set_source_files(self, files, regions, long_haps=0):
        """plat_caller_set_source_files: the source VCF lines of the NEXT call from whole files.  files: [(the .vcf.gz's bytes or uint8 array,
        its NativeIndex)]; regions: [(chrom, start, end)] in the order of that call's list.  self.source_blocks_info describes it."""
        ff = (_SourceFile * max(len(files), 1))()
        keep = [_u8(d) for d, _ in files]
        for k, (_, index) in enumerate(files):
            ff[k].data, ff[k].data_len, ff[k].index = keep[k].ctypes.data, len(keep[k]), index.h
        rr = (_SourceRegion * max(len(regions), 1))()
        for k, (chrom, start, end) in enumerate(regions):
            rr[k].chrom, rr[k].start, rr[k].end = chrom if isinstance(chrom, bytes) else chrom.encode(), int(start), int(end)
        info = SourceBlocksInfo()
        rc = self.lib.plat_caller_set_source_files(self.h, ff, len(files), rr, len(regions), int(long_haps), C.byref(info))
        del keep
        if rc != 0:
            raise _lib.PlatypusDeviceError(rc, (self.lib.plat_caller_last_error(self.h) or b"").decode(), "plat_caller_set_source_files")
        self.source_blocks_info = {k: getattr(info, k) for k, _ in info._fields_}

    def source_lines_set(self, n_regions):
        """plat_caller_source_lines: the source lines set for the next call, [bytes] per region of its list."""
        out = []
        for k in range(n_regions):
            text, length = C.c_void_p(), C.c_int64()
            rc = self.lib.plat_caller_source_lines(self.h, k, C.byref(text), C.byref(length))
            if rc != 0:
                raise _lib.PlatypusDeviceError(rc, "region %d: nothing is set for it" % k, "plat_caller_source_lines")
            out.append(C.string_at(text, length.value) if length.value else b"")
        return out

    def _set_source(self, source_lines, source_blocks, options):
        """The source of the next call, whichever way it was given (not both); returns what has to stay alive until it has returned."""
        if source_lines is not None and source_blocks is not None:
            raise ValueError("source_lines and source_blocks are two ways to say the same thing: give one")
        if source_blocks is not None:
            return self.set_source_blocks(source_blocks, getattr(options, "longHaps", 0))
        return self.set_source_lines(source_lines, getattr(options, "longHaps", 0)) if source_lines is not None else None

    def _finish(self, rc, entry, text, length, o, st, options, raw=False):
        """What follows every call into the region loop: the library's message as PlatypusDeviceError, or the text (as _native_text hands
        it over), options.rlen as the reference updates it, self.stats."""
        if rc != 0:
            raise _lib.PlatypusDeviceError(rc, (self.lib.plat_caller_last_error(self.h) or b"").decode(), entry)
        out = _native_text(self.lib, text, length.value, raw)
        options.rlen = int(o.rlen)
        self.stats = st.as_dict()
        return out

    def _call_args(self, sample_names, options):
        """(names array, plat_caller_options, text pointer, length, stats) of one call."""
        names = (C.c_char_p * len(sample_names))(*[s.encode() for s in sample_names])
        return names, CallerOptions.from_options(options), C.c_void_p(), C.c_size_t(), CallerStats()

    def call_regions(self, regions, sample_names, options, source_lines=None, source_blocks=None, source_files=None):
        """regions: list of RegionReads.  Returns the record lines of all regions (str), in region order; options.rlen is updated
        as the reference updates it.  source_lines: per region the text its source VCF fetches returned (set_source_lines; longHaps is
        options.longHaps): candidates from the source join those of the reads.  source_blocks: the same from the BGZF blocks of the
        fetches (set_source_blocks).  source_files: the same from whole files and their open indexes, [(data, NativeIndex)], fetched for
        every region's chrom:start-end (set_source_files)."""
        n, nS = len(regions), len(sample_names)
        if source_files is not None:
            if source_lines is not None or source_blocks is not None:
                raise ValueError("source_lines, source_blocks and source_files are three ways to say the same thing: give one")
            keep = self.set_source_files(source_files, [(r.chrom, r.start, r.end) for r in regions], getattr(options, "longHaps", 0))
        else:
            keep = self._set_source(source_lines, source_blocks, options)
        arr = (_Region * max(n, 1))()
        for k, r in enumerate(regions):
            r.fill(arr[k], nS)
        names, o, text, length, st = self._call_args(sample_names, options)
        rc = self.lib.plat_call_regions(self.h, arr, n, nS, names, C.byref(o), C.byref(text), C.byref(length), C.byref(st))
        del keep
        return self._finish(rc, "plat_call_regions", text, length, o, st, options)

    def call_bam_regions(self, regions, sample_names, options, source_lines=None, source_blocks=None):
        """regions: list of BamRegion.  As call_fetched_regions, with ReadIterator.get (htslibWrapper.pyx:328-406) on the device in front: the
        records are uploaded as they are and decoded there (plat_bam_decode_batch); the same text, rlen, self.loaded and self.read_counts."""
        return self._call_front("plat_call_bam_regions", _BamRegion, regions, sample_names, options, source_lines=source_lines, source_blocks=source_blocks)

    def call_bgzf_regions(self, regions, sample_names, options, source_lines=None, source_blocks=None):
        """regions: list of BgzfRegion.  As call_bam_regions, with the BGZF blocks inflated (plat_bgzf_inflate_batch) and sam_itr_next applied
        (plat_bam_find_records) on the device in front: the compressed bytes are uploaded as they are; the same text, rlen, self.loaded and
        self.read_counts; stats["input_bytes"] counts the compressed bytes."""
        return self._call_front("plat_call_bgzf_regions", _BgzfRegion, regions, sample_names, options, source_lines=source_lines, source_blocks=source_blocks)

    def call_bam_regions_rg(self, regions, read_groups, sample_names, options):
        """regions: list of BamFileRegion (all with the same number of files); read_groups: {read-group ID: sample index} or a list of
        (ID, sample index).  As call_bam_regions on the samples' records, with the split by read group (the second branch of loadBAMData,
        platypusutils.pyx:573-666) on the device in front (plat_bam_route_batch): the same text, rlen, self.loaded and self.read_counts."""
        return self._call_front("plat_call_bam_regions_rg", _BamRgRegion, regions, sample_names, options, groups=read_groups)

    def call_bgzf_regions_rg(self, regions, read_groups, sample_names, options):
        """regions: list of BgzfFileRegion.  As call_bam_regions_rg, from the files' BGZF blocks (inflate, find, route, decode on the device)."""
        return self._call_front("plat_call_bgzf_regions_rg", _BgzfRgRegion, regions, sample_names, options, groups=read_groups)

    def call_fetched_regions(self, regions, sample_names, options, source_lines=None, source_blocks=None):
        """regions: list of FetchedRegion.  The loader's work (addReadToBuffer's QC and split, isSorted, maxReads) on the device, then the
        region loop as call_regions runs it; the QC options come from the same `options`.  Returns the record lines (str); options.rlen is
        updated as the reference updates it.  self.loaded[k] (0: region k reached maxReads and was not called) and self.read_counts[k]
        (int32 [n_samples, 10]: n_good, n_bad, the 8 reason counts -- filteredReadCountsByType slots 0-6 and secondary alignments) describe
        the last call.  source_lines: as call_regions takes them, one entry per region of THIS list (the regions the loader gives up on
        included: their lines are dropped with them)."""
        return self._call_front("plat_call_fetched_regions", _FetchedRegion, regions, sample_names, options, source_lines=source_lines, source_blocks=source_blocks)

    def _call_front(self, entry, struct, regions, sample_names, options, groups=None, source_lines=None, source_blocks=None):
        """One call of a front end of the region loop (include/platypus_caller_{fetched,bam,bgzf,rg}.h): `struct` is its region struct,
        `groups` the read-group table of the merged-file calls."""
        n, nS = len(regions), len(sample_names)
        keep_source = self._set_source(source_lines, source_blocks, options)
        extra = ()
        n_units = nS
        if groups is not None:                                               # the merged-file calls: regions of files, and the read-group table
            n_units = len(regions[0].files) if regions else 1
            pairs = list(groups.items()) if isinstance(groups, dict) else list(groups)
            ids = (C.c_char_p * max(len(pairs), 1))(*[g if isinstance(g, bytes) else g.encode() for g, _ in pairs])
            smp = np.array([s for _, s in pairs], dtype=np.int32)
            table = _BamReadGroups(len(pairs), ids, smp.ctypes.data)
            extra = (n_units, C.byref(table), nS)
        arr = (struct * max(n, 1))()
        for k, r in enumerate(regions):
            r.fill(arr[k], n_units)
        names, o, text, length, st = self._call_args(sample_names, options)
        q = CallerQCOptions.from_options(options)
        counts = np.zeros((max(n, 1), nS, 10), dtype=np.int32)
        info = (_FetchedRegionInfo * max(n, 1))()
        for k in range(n):
            info[k].sample_counts = counts[k].ctypes.data
        rc = getattr(self.lib, entry)(self.h, arr, n, *(extra or (nS,)), names, C.byref(o), C.byref(q), C.byref(text), C.byref(length), info, C.byref(st))
        del keep_source
        out = self._finish(rc, entry, text, length, o, st, options)
        self.loaded = [int(info[k].loaded) for k in range(n)]
        self.read_counts = counts[:n]
        return out

    def region_text_lengths(self, n_regions):
        """Bytes of record text of every region of the last call, in list order (their blocks lie back to back in the text it returned)."""
        import numpy as np
        out = np.zeros(max(n_regions, 1), dtype=np.int64)
        rc = self.lib.plat_caller_region_text_lengths(self.h, out.ctypes.data, n_regions)
        if rc != 0:
            raise _lib.PlatypusDeviceError(rc, "no call yet, or another number of regions", "plat_caller_region_text_lengths")
        return out[:n_regions]

    def compress_text(self, text, lengths, level=1, eof=True):
        """plat_caller_compress_text (include/platypus_caller_bgzfout.h): a record text (str, bytes or a raw view) whose regions take
        `lengths` bytes each (region_text_lengths) deflated to BGZF blocks on the device, every region a whole number of blocks.  Returns
        (the compressed bytes as a ctypes char array -- no copy, freed with the array --, the regions' compressed lengths): again a text
        of per-region pieces, for RegionTextExchange and BlockOrder.merge.  eof=True appends the 28-byte EOF block (not counted in the
        lengths); level 0 stores."""
        import numpy as np
        if isinstance(text, str):
            text = text.encode("ascii")
        base, nbytes = text_address(text)
        lens = np.ascontiguousarray(lengths, dtype=np.int64)
        out_lens = np.zeros(max(len(lens), 1), dtype=np.int64)
        out, length = C.c_void_p(), C.c_size_t()
        rc = self.lib.plat_caller_compress_text(self.h, base, nbytes, lens.ctypes.data, len(lens), int(level), int(bool(eof)), C.byref(out), C.byref(length),
                                                out_lens.ctypes.data)
        if rc != 0:
            raise _lib.PlatypusDeviceError(rc, (self.lib.plat_caller_last_error(self.h) or b"").decode(), "plat_caller_compress_text")
        return _native_text(self.lib, out, length.value, "view"), out_lens[:len(lens)]

    def index_bgzf(self, data, info=False):
        """plat_caller_index_bgzf (include/platypus_caller_tbi.h): the tabix index of a whole bgzipped VCF (bytes, or a ctypes array as
        compress_text returns it, header blocks and EOF block included), built on the device.  Returns the .tbi's bytes (BGZF), with
        info=True (bytes, TbiInfo).  A file tabix would refuse raises PlatypusDeviceError naming the line."""
        base, nbytes = text_address(data)
        out, length, inf = C.c_void_p(), C.c_size_t(), TbiInfo()
        rc = self.lib.plat_caller_index_bgzf(self.h, base, nbytes, C.byref(out), C.byref(length), C.byref(inf))
        if rc != 0:
            raise _lib.PlatypusDeviceError(rc, (self.lib.plat_caller_last_error(self.h) or b"").decode(), "plat_caller_index_bgzf")
        try:
            tbi = C.string_at(out, length.value)
        finally:
            self.lib.plat_caller_free(out)
        return (tbi, inf) if info else tbi

    def call_stream(self, n_regions, load, user, sample_names, options, n_slots, n_loaders=2, raw=False, source_lines=None, source_blocks=None):
        """plat_call_regions_stream: regions loaded on demand.  `load`: a plat_region_load_fn -- the address of a native function (int,
        e.g. tools/synth's generator: no Python in the loader threads) or a Python callable (index, slot, region_struct) -> status (wrapped;
        tests).  Returns the record lines of all regions in region order: str, or bytes with raw=True (a whole-genome share is ~100 MB of
        text: every decode / encode of it is a pass through memory the caller may not want)."""
        nS = len(sample_names)
        keep_source = self._set_source(source_lines, source_blocks, options)   # (as call_regions)
        keep = None
        if callable(load):
            fn = load

            def tramp(_user, index, slot, out):
                try:
                    return int(fn(index, slot, out.contents) or 0)
                except Exception:                                       # an exception cannot cross the C frames
                    import traceback
                    traceback.print_exc()
                    return -9
            keep = LOAD_FN(tramp)
            load = C.cast(keep, C.c_void_p)
        names, o, text, length, st = self._call_args(sample_names, options)
        rc = self.lib.plat_call_regions_stream(self.h, n_regions, nS, names, C.byref(o), load, user, n_slots, n_loaders, C.byref(text), C.byref(length),
                                               C.byref(st))
        del keep, keep_source
        return self._finish(rc, "plat_call_regions_stream", text, length, o, st, options, raw)


LOAD_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_int, C.POINTER(_Region))
