"""ctypes binding of libplat_mi355x.so (include/platypus_mi355x.h).

The HIP library is the product path.  There is NO CPU fallback: if the shared object is missing it is
built with hipcc (gfx950); if that is impossible, or if no GPU is present when a device entry point is
called, an exception is raised.
"""
import ctypes as C
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libplat_mi355x.so")
CSRC = os.path.join(HERE, "csrc")

PLAT_BLOB_PAD = 32
PLAT_ABI_VERSION = 1

ERRORS = {
    0: "PLAT_OK", -1: "PLAT_ERR_INVALID", -2: "PLAT_ERR_HIP", -3: "PLAT_ERR_NOMEM", -4: "PLAT_ERR_HAP_TOO_LONG",
    -5: "PLAT_ERR_HAP_TOO_SHORT", -6: "PLAT_ERR_UNSUPPORTED", -7: "PLAT_ERR_NO_DEVICE", -8: "PLAT_ERR_OVERFLOW",
    -9: "PLAT_ERR_BAD_INPUT", -10: "PLAT_ERR_BAD_HINTS",
}


class PlatypusDeviceError(RuntimeError):
    def __init__(self, code, msg, where=""):
        self.code = code
        super().__init__("%s%s (%d): %s" % (where + ": " if where else "", ERRORS.get(code, "?"), code, msg))


class WindowBatch(C.Structure):
    _fields_ = [("n_windows", C.c_int32), ("n_haps", C.c_int32), ("n_reads", C.c_int32), ("_pad", C.c_int32),
                ("win_hap_begin", C.c_void_p), ("win_read_begin", C.c_void_p), ("win_start", C.c_void_p),
                ("win_end", C.c_void_p), ("win_flank", C.c_void_p), ("pair_off", C.c_void_p),
                ("hap_seq", C.c_void_p), ("hap_off", C.c_void_p), ("read_seq", C.c_void_p),
                ("read_qual", C.c_void_p), ("read_off", C.c_void_p), ("read_pos", C.c_void_p),
                ("read_end", C.c_void_p), ("read_mapq", C.c_void_p), ("read_flags", C.c_void_p),
                ("read_kind", C.c_void_p)]


class AlignStats(C.Structure):
    _fields_ = [("n_pairs", C.c_int64), ("n_pairs_aligned", C.c_int64), ("n_dp_launched", C.c_int64),
                ("n_dp_reference", C.c_int64), ("cells_reference", C.c_int64), ("cells_launched", C.c_int64),
                ("n_seed_fallback", C.c_int64), ("_reserved", C.c_int64)]


class Profile(C.Structure):
    _fields_ = [("ms_prepare", C.c_float), ("ms_seed", C.c_float), ("ms_dp", C.c_float), ("ms_finalize", C.c_float),
                ("ms_genotype", C.c_float), ("ms_seed_kernel", C.c_float), ("dp_jobs", C.c_int64), ("dp_alg_bytes", C.c_int64),
                ("ms_sweep", C.c_float), ("ms_pairs", C.c_float), ("ms_unpack", C.c_float), ("ms_candidates", C.c_float)]


class BatchHints(C.Structure):
    _fields_ = [("max_hap_len", C.c_int32), ("max_read_len", C.c_int32), ("max_reads_per_window", C.c_int32),
                ("_pad", C.c_int32), ("n_pairs", C.c_int64), ("hap_blob_len", C.c_int64), ("read_blob_len", C.c_int64),
                ("extra_jobs_cap", C.c_int64)]


class AssemblyBatch(C.Structure):
    _fields_ = [("n_regions", C.c_int32), ("n_reads", C.c_int32), ("ref_seq", C.c_void_p), ("ref_off", C.c_void_p),
                ("ref_start", C.c_void_p), ("assem_start", C.c_void_p), ("assem_end", C.c_void_p),
                ("reg_read_begin", C.c_void_p), ("read_seq", C.c_void_p), ("read_qual", C.c_void_p),
                ("read_off", C.c_void_p)]


class AssemblyHints(C.Structure):
    _fields_ = [("max_ref_len", C.c_int32), ("max_reads_per_region", C.c_int32), ("max_positions", C.c_int64)]


class CandidateBatch(C.Structure):
    _fields_ = [("n_regions", C.c_int32), ("n_reads", C.c_int32), ("ref_seq", C.c_void_p), ("ref_off", C.c_void_p),
                ("ref_seq_start", C.c_void_p), ("contig_len", C.c_void_p), ("read_seq", C.c_void_p),
                ("read_qual", C.c_void_p), ("read_off", C.c_void_p), ("read_pos", C.c_void_p), ("read_flags", C.c_void_p),
                ("cigar", C.c_void_p), ("cig_off", C.c_void_p)]


class ReadQCBatch(C.Structure):
    _fields_ = [("n_reads", C.c_int32), ("_pad", C.c_int32), ("read_qual", C.c_void_p), ("read_off", C.c_void_p),
                ("read_pos", C.c_void_p), ("read_mapq", C.c_void_p), ("read_flags", C.c_void_p), ("chrom_id", C.c_void_p),
                ("mate_chrom_id", C.c_void_p), ("insert_size", C.c_void_p), ("mate_pos", C.c_void_p), ("cigar", C.c_void_p),
                ("cig_off", C.c_void_p), ("stream_of", C.c_void_p)]


class ReadQCOptions(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("min_good_qual_bases", "min_map_qual", "min_base_qual", "trim_overlapping", "trim_adapter",
                                         "trim_read_flank", "trim_soft_clipped", "filter_mate_unmapped", "filter_mate_distant",
                                         "filter_small_insert", "filter_duplicates")]


class ReadBuffersIn(C.Structure):
    _fields_ = [("qc", ReadQCBatch), ("n_streams", C.c_int32), ("_pad", C.c_int32), ("stream_begin", C.c_void_p), ("read_seq", C.c_void_p),
                ("read_end", C.c_void_p)]


class ReadBuffersPackedIn(C.Structure):
    _fields_ = [("qc", ReadQCBatch), ("n_streams", C.c_int32), ("_pad", C.c_int32), ("stream_begin", C.c_void_p), ("read_packed", C.c_void_p),
                ("read_end", C.c_void_p), ("n_exc", C.c_int64), ("exc_index", C.c_void_p), ("exc_base", C.c_void_p), ("exc_qual", C.c_void_p)]


class ReadBuffersTables(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("off", "cig_off", "seq", "qual", "cigar", "pos", "end", "mapq", "flags", "mate_pos")]


class BamDecodeOut(C.Structure):
    _fields_ = [("cap_bases", C.c_int64), ("cap_pairs", C.c_int64)] + [(k, C.c_void_p) for k in (
        "read_off", "cig_off", "seq", "qual", "cigar", "pos", "end", "mapq", "flags", "chrom_id", "mate_chrom_id", "insert_size", "mate_pos",
        "status")]


class BgzfInflateOut(C.Structure):
    _fields_ = [("cap_bytes", C.c_int64), ("data", C.c_void_p), ("out_off", C.c_void_p), ("status", C.c_void_p)]


class BgzfDeflateIn(C.Structure):
    _fields_ = [("text", C.c_void_p), ("text_len", C.c_int64), ("n_pieces", C.c_int32), ("level", C.c_int32), ("piece_off", C.c_void_p)]


class BgzfDeflateOut(C.Structure):
    _fields_ = [("cap_bytes", C.c_int64), ("data", C.c_void_p), ("piece_out_off", C.c_void_p), ("status", C.c_void_p)]


class BamFindIn(C.Structure):
    _fields_ = [("n_streams", C.c_int32), ("n_chunks", C.c_int32), ("n_blocks", C.c_int32), ("_pad", C.c_int32)] + [(k, C.c_void_p) for k in (
        "data", "out_off", "stream_chunk_begin", "chunk_blk_first", "chunk_blk_end", "chunk_first_uoffset", "chunk_stop_blk", "chunk_stop_uoffset",
        "tid", "beg", "end")]


class BamFindOut(C.Structure):
    _fields_ = [("cap_records", C.c_int64), ("rec_off", C.c_void_p), ("rec_limit", C.c_void_p), ("stream_begin", C.c_void_p), ("status", C.c_void_p)]


class BamRouteIn(C.Structure):
    _fields_ = [("n_records", C.c_int32), ("n_streams", C.c_int32), ("n_groups", C.c_int32), ("n_samples", C.c_int32), ("blob", C.c_void_p),
                ("blob_len", C.c_int64)] + [(k, C.c_void_p) for k in ("rec_off", "rec_end", "stream_begin", "group_ids", "group_off", "group_sample")]


class BamRouteOut(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("rec_off", "rec_limit", "out_begin", "rec_sample", "status", "why")]


class BamMatesIn(C.Structure):
    """plat_bam_mates_in."""
    _fields_ = [("n_streams", C.c_int32), ("n_records", C.c_int32), ("mode", C.c_int32), ("_pad", C.c_int32), ("data", C.c_void_p), ("data_len", C.c_int64)] + \
               [(k, C.c_void_p) for k in ("rec_off", "rec_limit", "stream_begin", "want_tid", "lo", "hi")]


class BamMatesOut(C.Structure):
    """plat_bam_mates_out."""
    _fields_ = [("cap_records", C.c_int64), ("cap_bytes", C.c_int64)] + \
               [(k, C.c_void_p) for k in ("coords", "coord_begin", "out_data", "out_rec_off", "out_rec_len", "out_mpos", "out_begin", "status", "need_bytes")]


MATES_COORDS, MATES_FETCH = 0, 1


class SourceVariantsIn(C.Structure):
    _fields_ = [("n_regions", C.c_int32), ("maxSize", C.c_int32), ("longHaps", C.c_int32), ("_pad", C.c_int32), ("text", C.c_void_p),
                ("text_len", C.c_int64), ("text_off", C.c_void_p), ("name_hash", C.c_void_p)]


class SourceVariantsOut(C.Structure):
    _fields_ = [("cap_variants", C.c_int64)] + [(k, C.c_void_p) for k in (
        "region_begin", "pos", "rem_off", "n_rem", "add_off", "n_add", "hash", "line", "region_stats", "status")]


class TabixFetchIn(C.Structure):
    _fields_ = [("n_streams", C.c_int32), ("n_chunks", C.c_int32), ("n_blocks", C.c_int32), ("_pad", C.c_int32), ("data", C.c_void_p),
                ("data_len", C.c_int64)] + [(k, C.c_void_p) for k in (
        "out_off", "stream_chunk_begin", "chunk_blk_first", "chunk_blk_end", "chunk_first_uoffset", "chunk_stop_blk", "chunk_stop_uoffset",
        "names", "name_off", "beg", "end")]


class TabixFetchOut(C.Structure):
    _fields_ = [("cap_text", C.c_int64), ("text", C.c_void_p), ("stream_text_off", C.c_void_p), ("stream_counts", C.c_void_p), ("status", C.c_void_p)]


class TabixIndexIn(C.Structure):
    _fields_ = [("n_blocks", C.c_int32), ("_pad", C.c_int32), ("data", C.c_void_p), ("data_len", C.c_int64), ("out_off", C.c_void_p), ("blk_addr", C.c_void_p)]


class TabixIndexOut(C.Structure):
    _fields_ = [("cap_runs", C.c_int64), ("cap_names", C.c_int64), ("cap_windows", C.c_int64), ("cap_name_bytes", C.c_int64)] + [(k, C.c_void_p) for k in (
        "run_tid", "run_bin", "run_u", "name_off", "name_len", "name_bytes", "lin_first", "lin", "status")]


TBI_STATUS_WORDS, TBI_MAX_REF = 13, 65536
TBI_KINDS = ("", "a line of fewer than two columns", "a POS or END beyond 32 bits", "a negative END", "a position below the one in front of it",
             "a contig name that appeared before another")



class IndexQueryIn(C.Structure):
    """plat_index_query_in: the flat tables of one index (resident) and a call's queries."""
    _fields_ = [("n_ref", C.c_int32), ("n_queries", C.c_int32), ("n_bins", C.c_int64), ("n_chunks", C.c_int64), ("n_lin", C.c_int64)] + [(k, C.c_void_p) for k in (
        "ref_bin_first", "bin_id", "bin_chunk_first", "chunk_u", "chunk_v", "ref_lin_first", "lin_fill", "tid", "beg", "end")]


class IndexQueryOut(C.Structure):
    _fields_ = [("cap_chunks", C.c_int64)] + [(k, C.c_void_p) for k in ("count", "gathered", "q_first", "out_u", "out_v", "status")]


IDXQ_STATUS_WORDS, IDXQ_MAX_CHUNKS, IDXQ_NO_ITERATOR, IDXQ_HANDED_OVER = 6, 2048, -1, -2


class FastaFetchIn(C.Structure):
    """plat_fasta_fetch_in: a cut of a FASTA file on the device and a call's queries."""
    _fields_ = [("file", C.c_void_p), ("file_len", C.c_int64), ("file_base", C.c_int64), ("file_size", C.c_int64), ("n_queries", C.c_int64)] + [(k, C.c_void_p) for k in (
        "start_pos", "line_len", "full_len", "seq_len", "beg", "end", "mode")]


class FastaFetchOut(C.Structure):
    _fields_ = [("cap_bytes", C.c_int64)] + [(k, C.c_void_p) for k in ("out_off", "out_status", "out", "totals")]


FASTA_STATUS_WORDS = 4
FASTA_OK, FASTA_INDEX_ERROR, FASTA_ZERO_LINE, FASTA_BAD_INDEX, FASTA_LEFT_OF_CUT, FASTA_RIGHT_OF_CUT = range(6)
FASTA_MODE_SEQUENCE, FASTA_MODE_CONTIG = 0, 1

ROUTE_MAX_GROUPS, ROUTE_MAX_SAMPLES, ROUTE_LDS_ID_BYTES = 2048, 256, 24576
ROUTE_WHY = ("routed", "no RG field", "an RG field that is no string", "an RG value that is not in the table", "an aux field of unknown type",
             "a B array with a negative count", "aux data that runs past the record", "a fixed part that runs past the record")


class InfoStatsBatch(C.Structure):
    _fields_ = [("n_vars", C.c_int32), ("n_ind", C.c_int32)] + [(k, C.c_void_p) for k in (
        "var_window", "var_pos", "var_bam_min", "var_bam_max", "var_n_added", "var_n_removed", "var_added", "var_added_off",
        "var_in_genotype", "minq_off", "good_begin", "good_end", "bad_begin", "bad_end", "read_seq", "read_qual", "read_off",
        "read_pos", "read_end", "read_mapq", "read_flags", "cigar", "cig_off")]


class RefCovIn(C.Structure):
    _fields_ = ([(k, C.c_int32) for k in ("n_intervals", "n_slices", "n_tiles", "n_reads")] +
                [(k, C.c_void_p) for k in ("read_pos", "read_end", "slice_begin", "slice_n", "slice_longest", "iv_start", "iv_end", "iv_slice_first",
                                           "iv_n_samples", "iv_count_off", "iv_tile_first")])


class RefCovOut(C.Structure):
    _fields_ = [("cap_counts", C.c_int64), ("iv_min", C.c_void_p), ("counts", C.c_void_p)]


PLAT_REFCOV_RAISES, PLAT_REFCOV_EMPTY, PLAT_REFCOV_TILE = -1, 2147483647, 1024


class PackedReads(C.Structure):
    _fields_ = [("read_src", C.c_void_p), ("n_exc", C.c_int64), ("exc_index", C.c_void_p), ("exc_base", C.c_void_p), ("exc_qual", C.c_void_p)]


class UnpackPiece(C.Structure):
    _fields_ = [("src", C.c_void_p), ("dst", C.c_int64), ("n", C.c_int64)]


class StageBOptions(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("minReads", "maxSize", "mergeClusteredVariants", "maxVarDist", "minVarDist", "largeWindows", "maxVariants",
                                         "maxHaplotypes", "filterVarsByCoverage", "skipDifficultWindows")] + [("maxReads", C.c_double)]


class StageBIn(C.Structure):
    _fields_ = ([("n_regions", C.c_int32), ("cap_per_scan", C.c_int32)] +
                [(k, C.c_void_p) for k in ("cand", "cand_n", "cand_rec", "region_name_hash", "ref_seq", "ref_off", "ref_seq_start", "contig_len",
                                           "region_start", "region_end", "region_rlen", "read_seq", "read_off", "read_pos", "read_end",
                                           "tab_begin", "tab_n", "tab_longest", "broken_mate_pos")] +
                [(k, C.c_int32) for k in ("broken_base", "cap_vars", "cap_windows", "cap_added", "cap_batch_windows", "cap_batch_haps", "cap_batch_reads")] +
                [("cap_hap_bytes", C.c_int64)])


# the output arrays of plat_stage_b_out in the header's order, with the element type of each
STAGE_B_OUT_FIELDS = (
    ("hdr", "i4"), ("var_pos", "i4"), ("var_nrem", "i4"), ("var_nadd", "i4"), ("var_support", "i4"), ("var_bam_min", "i4"), ("var_bam_max", "i4"),
    ("var_rem_pos", "i4"), ("var_add_off", "i4"), ("added", "u1"), ("win_start", "i4"), ("win_end", "i4"), ("win_var_first", "i4"), ("win_var_n", "i4"),
    ("win_flags", "i4"), ("win_ptrs", "i4"), ("win_n_haps", "i4"), ("win_batch", "i4"), ("b_hap_begin", "i4"), ("b_read_begin", "i4"), ("b_start", "i4"),
    ("b_end", "i4"), ("b_flank", "i4"), ("b_pair_off", "i8"), ("b_gl_off", "i8"), ("b_seg_begin", "i4"), ("b_n_good", "i4"), ("b_hap_off", "i8"),
    ("b_hap_mask", "u4"), ("b_hap_seq", "u1"), ("b_read_off", "i8"), ("b_read_src", "i4"), ("b_read_kind", "u1"), ("totals", "i8"), ("scratch", "i4"))


class StageBOut(C.Structure):
    _fields_ = [(k, C.c_void_p) for k, _ in STAGE_B_OUT_FIELDS]


# symbol -> (restype, argtypes): exactly the declarations of include/platypus_mi355x.h
SIGNATURES = {
    "plat_abi_version": (C.c_int, []),
    "plat_strerror": (C.c_char_p, [C.c_int]),
    "plat_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "plat_ctx_create": (C.c_int, [C.c_int, C.POINTER(C.c_void_p)]),
    "plat_ctx_destroy": (C.c_int, [C.c_void_p]),
    "plat_last_hip_error": (C.c_int, [C.c_void_p]),
    "plat_malloc": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]),
    "plat_free": (C.c_int, [C.c_void_p, C.c_void_p]),
    "plat_memcpy_h2d": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "plat_memcpy_d2d": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "plat_memcpy_d2h": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "plat_memset": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]),
    "plat_stream_sync": (C.c_int, [C.c_void_p, C.c_void_p]),
    "plat_stream_create": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "plat_stream_destroy": (C.c_int, [C.c_void_p, C.c_void_p]),
    "plat_host_alloc": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]),
    "plat_host_free": (C.c_int, [C.c_void_p, C.c_void_p]),
    "plat_gather_reads": (C.c_int, [C.c_void_p, C.c_int64] + [C.c_void_p] * 16),
    "plat_unpack_reads": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "plat_profile_enable": (C.c_int, [C.c_void_p, C.c_int]),
    "plat_profile_last": (C.c_int, [C.c_void_p, C.POINTER(Profile)]),
    "plat_sync_poll_us": (C.c_int, [C.c_void_p, C.c_int]),
    "plat_kernel_timer_name": (C.c_char_p, [C.c_int]),
    "plat_kernel_times": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    "plat_kernel_timer_only": (C.c_int, [C.c_void_p, C.c_int]),
    "plat_dp_batch": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "plat_align_window_batch": (C.c_int, [C.c_void_p, C.POINTER(WindowBatch), C.c_int, C.c_int, C.c_void_p,
                                          C.c_void_p, C.POINTER(AlignStats), C.c_void_p]),
    "plat_align_window_batch_async": (C.c_int, [C.c_void_p, C.POINTER(WindowBatch), C.POINTER(BatchHints), C.c_int, C.c_int,
                                                C.c_void_p, C.c_void_p, C.c_void_p]),
    "plat_genotype_window_batch": (C.c_int, [C.c_void_p, C.POINTER(WindowBatch), C.c_int, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_void_p]),
    "plat_em_window_batch": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p]),
    "plat_variant_posterior_batch": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 11),
    "plat_genotype_call_batch": (C.c_int, [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 16),
    "plat_haplotype_score_batch": (C.c_int, [C.c_void_p, C.POINTER(WindowBatch), C.c_int, C.c_int] + [C.c_void_p] * 6),
    "plat_candidates_batch": (C.c_int, [C.c_void_p, C.POINTER(CandidateBatch), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "plat_candidates_merge_batch": (C.c_int, [C.c_void_p, C.POINTER(CandidateBatch), C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "plat_stage_b_batch": (C.c_int, [C.c_void_p, C.POINTER(StageBIn), C.POINTER(StageBOptions), C.POINTER(StageBOut), C.c_void_p]),
    "plat_unpack_reads_pieces": (C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p]),
    "plat_unpack_reads_pieces_codes": (C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p,
                                                 C.c_void_p, C.c_void_p, C.c_void_p]),
    "plat_ref_codes": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "plat_candidates_batch_codes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "plat_copy_pieces": (C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "plat_concat_read_tables": (C.c_int, [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 9 + [C.c_int64] * 3 + [C.c_void_p]),
    "plat_concat_read_tables_src": (C.c_int, [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 10 + [C.c_int64] * 3 + [C.c_void_p]),
    "plat_pack_codes_pieces": (C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "plat_candidates_batch_packed": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(PackedReads), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                               C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "plat_gather_reads_packed": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.POINTER(PackedReads)] + [C.c_void_p] * 12),
    "plat_variant_read_stats_packed_batch": (C.c_int, [C.c_void_p, C.POINTER(InfoStatsBatch), C.POINTER(PackedReads), C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                                       C.c_void_p, C.c_void_p, C.c_void_p]),
    "plat_read_qc_batch": (C.c_int, [C.c_void_p, C.POINTER(ReadQCBatch), C.POINTER(ReadQCOptions), C.c_void_p, C.c_void_p, C.c_void_p]),
    "plat_read_buffers_batch": (C.c_int, [C.c_void_p, C.POINTER(ReadBuffersIn), C.POINTER(ReadQCOptions), C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.POINTER(ReadBuffersTables), C.c_void_p]),
    "plat_read_buffers_packed_batch": (C.c_int, [C.c_void_p, C.POINTER(ReadBuffersPackedIn), C.POINTER(ReadQCOptions), C.c_void_p, C.c_void_p,
                                                 C.c_void_p, C.c_void_p, C.POINTER(ReadBuffersTables), C.c_void_p]),
    "plat_bam_decode_batch": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.POINTER(BamDecodeOut), C.c_void_p]),
    "plat_bgzf_inflate_batch": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.POINTER(BgzfInflateOut), C.c_void_p]),
    "plat_bgzf_deflate_batch": (C.c_int, [C.c_void_p, C.POINTER(BgzfDeflateIn), C.POINTER(BgzfDeflateOut), C.c_void_p]),
    "plat_bam_find_records": (C.c_int, [C.c_void_p, C.POINTER(BamFindIn), C.POINTER(BamFindOut), C.c_void_p]),
    "plat_bam_route_batch": (C.c_int, [C.c_void_p, C.POINTER(BamRouteIn), C.POINTER(BamRouteOut), C.c_void_p]),
    "plat_bam_mates_batch": (C.c_int, [C.c_void_p, C.POINTER(BamMatesIn), C.POINTER(BamMatesOut), C.c_void_p]),
    "plat_source_variants_batch": (C.c_int, [C.c_void_p, C.POINTER(SourceVariantsIn), C.POINTER(SourceVariantsOut), C.c_void_p]),
    "plat_tabix_fetch_batch": (C.c_int, [C.c_void_p, C.POINTER(TabixFetchIn), C.POINTER(TabixFetchOut), C.c_void_p]),
    "plat_tabix_index_batch": (C.c_int, [C.c_void_p, C.POINTER(TabixIndexIn), C.POINTER(TabixIndexOut), C.c_void_p]),
    "plat_index_query_batch": (C.c_int, [C.c_void_p, C.POINTER(IndexQueryIn), C.POINTER(IndexQueryOut), C.c_void_p]),
    "plat_fasta_fetch_batch": (C.c_int, [C.c_void_p, C.POINTER(FastaFetchIn), C.POINTER(FastaFetchOut), C.c_void_p]),
    "plat_fasta_tile_bytes": (C.c_int, []),
    "plat_refcall_coverage_batch": (C.c_int, [C.c_void_p, C.POINTER(RefCovIn), C.POINTER(RefCovOut), C.c_void_p]),
    "plat_refcov_lds_reads": (C.c_int, []),
    "plat_variant_read_stats_batch": (C.c_int, [C.c_void_p, C.POINTER(InfoStatsBatch), C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                                C.c_void_p, C.c_void_p, C.c_void_p]),
    "plat_variant_info_batch": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "plat_assemble_batch": (C.c_int, [C.c_void_p, C.POINTER(AssemblyBatch), C.c_int, C.c_int, C.c_int, C.c_int,
                                      C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_void_p]),
    "plat_assemble_batch_async": (C.c_int, [C.c_void_p, C.POINTER(AssemblyBatch), C.POINTER(AssemblyHints), C.c_int, C.c_int, C.c_int, C.c_int,
                                            C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_void_p]),
}

# entry points a stand-in library built against an earlier header may lack (the CPU suite's fake device): bind() leaves them
# unbound there; load() still requires every declared symbol of the real library
ADDED_LATER = ("plat_read_buffers_batch", "plat_read_buffers_packed_batch", "plat_bam_decode_batch", "plat_bgzf_inflate_batch", "plat_bam_find_records",
               "plat_bam_route_batch", "plat_source_variants_batch", "plat_tabix_fetch_batch", "plat_refcall_coverage_batch", "plat_refcov_lds_reads",
               "plat_bgzf_deflate_batch", "plat_tabix_index_batch", "plat_index_query_batch", "plat_fasta_fetch_batch", "plat_fasta_tile_bytes",
               "plat_concat_read_tables_src", "plat_pack_codes_pieces", "plat_candidates_batch_packed", "plat_gather_reads_packed",
               "plat_variant_read_stats_packed_batch", "plat_bam_mates_batch")

_lib = None


def build(verbose=False):
    """Compile libplat_mi355x.so for gfx950 with hipcc (cross-compiles without a GPU)."""
    r = subprocess.run(["make", "-C", CSRC, "-j8"], capture_output=True, text=True)
    if verbose:
        print(r.stdout)
    if r.returncode != 0:
        raise RuntimeError("building libplat_mi355x.so failed:\n" + r.stdout[-4000:] + r.stderr[-4000:])
    return LIB_PATH


def load():
    """Load the HIP library (building it first if needed).  Never falls back to a CPU implementation."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        build()
    try:
        # torch is the device-memory/stream plumbing of the Python host and ships its own libamdhip64:
        # import it first so the process holds ONE HIP runtime (loading /opt/rocm's copy first and torch's
        # second leaves this library without a usable device).  A host without torch simply uses /opt/rocm's.
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = bind(C.CDLL(LIB_PATH))
    missing = [name for name in SIGNATURES if not hasattr(lib, name)]
    if missing:
        raise RuntimeError("libplat_mi355x.so does not export %s" % ", ".join(missing))
    _lib = lib
    return _lib


def bind(lib):
    """Attach the prototypes of include/platypus_mi355x.h to a loaded library exporting that ABI."""
    for name, (res, args) in SIGNATURES.items():
        if name in ADDED_LATER and not hasattr(lib, name):
            continue
        fn = getattr(lib, name)      # AttributeError here == the library does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    if lib.plat_abi_version() != PLAT_ABI_VERSION:
        raise RuntimeError("libplat_mi355x.so ABI version mismatch")
    return lib


def check(code, where=""):
    if code != 0:
        msg = load().plat_strerror(code).decode()
        raise PlatypusDeviceError(code, msg, where)
