# cplat.pxd -- Cython declarations of libplat_mi355x.so (include/platypus_mi355x.h), the file a Platypus maintainer adds next to
# src/cython/chaplotype.pxd to call the MI355X library from the reference's own Cython modules:
#
#     cimport cplat                         # in chaplotype.pyx / cgenotype.pyx / cpopulation.pyx / assembler.pyx / variantcaller.pyx
#
# It replaces, at the call sites listed in INTEGRATION.md section 2, the per-read loops behind
#     cdef double* Haplotype.alignReads(...)                         src/cython/chaplotype.pxd:44
#     cdef double  Haplotype.alignSingleRead(...)                    src/cython/chaplotype.pxd:45
#     cdef double  DiploidGenotype.calculateDataLikelihood(...)      src/cython/cgenotype.pxd:14
#     cdef void    Population.setup(...)                             src/cython/cpopulation.pxd:55
#     cdef list    assembleReadsAndDetectVariants(...)               src/cython/assembler.pxd:3
#     int fastAlignmentRoutine(...)                                  src/c/align.h:8-10
# Every declaration below is checked by the compiler against the header: bindings/plat_binding_check.pyx cimports this
# file and tests/test_binding_cpu.py builds it with Cython 3 and links it to the library.
from libc.stdint cimport int16_t, int32_t, int64_t, uint8_t, uint32_t

cdef extern from "platypus_mi355x.h":
    int PLAT_ABI_VERSION
    int PLAT_BLOB_PAD
    int PLAT_OK
    int PLAT_ERR_INVALID
    int PLAT_ERR_HIP
    int PLAT_ERR_NOMEM
    int PLAT_ERR_HAP_TOO_LONG
    int PLAT_ERR_HAP_TOO_SHORT
    int PLAT_ERR_UNSUPPORTED
    int PLAT_ERR_NO_DEVICE
    int PLAT_ERR_OVERFLOW
    int PLAT_ERR_BAD_INPUT
    int PLAT_ERR_BAD_HINTS

    ctypedef struct plat_ctx:
        pass

    # ---- context & memory
    int plat_abi_version() nogil
    const char* plat_strerror(int code) nogil
    int plat_device_count(int* out_count) nogil
    int plat_ctx_create(int device, plat_ctx** out_ctx) nogil
    int plat_ctx_destroy(plat_ctx* ctx) nogil
    int plat_last_hip_error(const plat_ctx* ctx) nogil
    int plat_malloc(plat_ctx* ctx, size_t nbytes, void** out_dev_ptr) nogil
    int plat_free(plat_ctx* ctx, void* dev_ptr) nogil
    int plat_memcpy_h2d(plat_ctx* ctx, void* dst_dev, const void* src_host, size_t nbytes, void* stream) nogil
    int plat_memcpy_d2d(plat_ctx* ctx, void* dst_dev, const void* src_dev, size_t nbytes, void* stream) nogil
    int plat_memcpy_d2h(plat_ctx* ctx, void* dst_host, const void* src_dev, size_t nbytes, void* stream) nogil
    int plat_memset(plat_ctx* ctx, void* dst_dev, int value, size_t nbytes, void* stream) nogil
    int plat_stream_sync(plat_ctx* ctx, void* stream) nogil
    int plat_stream_create(plat_ctx* ctx, void** out_stream) nogil
    int plat_stream_destroy(plat_ctx* ctx, void* stream) nogil
    int plat_host_alloc(plat_ctx* ctx, size_t nbytes, void** out_host_ptr) nogil
    int plat_host_free(plat_ctx* ctx, void* host_ptr) nogil

    # ---- live kernel timing
    ctypedef struct plat_profile:
        float ms_prepare
        float ms_seed
        float ms_dp
        float ms_finalize
        float ms_genotype
        float ms_seed_kernel
        int64_t dp_jobs
        int64_t dp_alg_bytes
        float ms_sweep
        float ms_pairs
        float ms_unpack
        float ms_candidates
    int plat_profile_enable(plat_ctx* ctx, int on) nogil
    int plat_profile_last(plat_ctx* ctx, plat_profile* out) nogil
    int plat_sync_poll_us(plat_ctx* ctx, int microseconds) nogil
    const char* plat_kernel_timer_name(int id) nogil
    int plat_kernel_times(plat_ctx* ctx, double* out_ms, int64_t* out_launches) nogil
    int plat_kernel_timer_only(plat_ctx* ctx, int id) nogil

    # ---- fastAlignmentRoutine, score only (src/c/align.h:8-10)
    int plat_dp_batch(plat_ctx* ctx, int n, int lmax, const uint8_t* hap_slices, const uint8_t* reads, const uint8_t* quals,
                      const uint8_t* gapopen, const int32_t* len2, int gapextend, int nucprior, int32_t* out_score, void* stream) nogil

    # ---- Haplotype.alignReads / alignSingleRead for whole windows (chaplotype.pxd:44-45)
    ctypedef struct plat_window_batch:
        int32_t n_windows
        int32_t n_haps
        int32_t n_reads
        int32_t _pad
        const int32_t* win_hap_begin
        const int32_t* win_read_begin
        const int32_t* win_start
        const int32_t* win_end
        const int32_t* win_flank
        const int64_t* pair_off
        const uint8_t* hap_seq
        const int64_t* hap_off
        const uint8_t* read_seq
        const uint8_t* read_qual
        const int64_t* read_off
        const int32_t* read_pos
        const int32_t* read_end
        const uint8_t* read_mapq
        const int32_t* read_flags
        const uint8_t* read_kind
    ctypedef struct plat_align_stats:
        int64_t n_pairs
        int64_t n_pairs_aligned
        int64_t n_dp_launched
        int64_t n_dp_reference
        int64_t cells_reference
        int64_t cells_launched
        int64_t n_seed_fallback
        int64_t _reserved
    ctypedef struct plat_batch_hints:
        int32_t max_hap_len
        int32_t max_read_len
        int32_t max_reads_per_window
        int32_t _pad
        int64_t n_pairs
        int64_t hap_blob_len
        int64_t read_blob_len
        int64_t extra_jobs_cap
    int plat_align_window_batch(plat_ctx* ctx, const plat_window_batch* batch, int calc_flank_score, int use_mapq_cap,
                                double* out_loglik, int32_t* out_score, plat_align_stats* out_stats, void* stream) nogil
    int plat_align_window_batch_async(plat_ctx* ctx, const plat_window_batch* batch, const plat_batch_hints* hints, int calc_flank_score,
                                      int use_mapq_cap, double* out_loglik, int32_t* out_score, void* stream) nogil

    # ---- DiploidGenotype.calculateDataLikelihood + Population.setup (cgenotype.pxd:14, cpopulation.pxd:55)
    int plat_genotype_window_batch(plat_ctx* ctx, const plat_window_batch* batch, int n_ind, const int32_t* seg_read_begin,
                                   const int32_t* seg_n_good, const double* loglik, const int64_t* gl_off, double* out_gl,
                                   double* out_logl, double* out_gof, void* stream) nogil

    # ---- Population.call, calculatePosterior, computeGenotypeCallAndLikelihoods (cpopulation.pyx:384-703, vcfutils.pyx:163-334)
    int plat_em_window_batch(plat_ctx* ctx, int n_windows, int n_ind, int max_haps_per_window, const int32_t* win_hap_begin,
                             const int64_t* gl_off, const int32_t* n_reads, const double* gl, int max_iters, int use_em_likelihoods,
                             double* out_freq, double* out_em, int32_t* out_call, int32_t* out_iters, void* stream) nogil
    int plat_variant_posterior_batch(plat_ctx* ctx, int n_vars, int n_ind, int max_haps_per_window, const int32_t* win_hap_begin,
                                     const int64_t* gl_off, const int32_t* n_reads, const double* gl, const double* freq,
                                     const int32_t* var_window, const int64_t* var_mask_off, const uint8_t* hap_has_var,
                                     const double* prior, double* out_posterior, void* stream) nogil
    int plat_genotype_call_batch(plat_ctx* ctx, int n_sites, int n_ind, const int32_t* win_hap_begin, const int64_t* gl_off,
                                 const double* gl, const double* gof, const double* freq, const int32_t* site_window,
                                 const int32_t* site_nvar, const int64_t* site_vih_off, const int64_t* site_ref_off,
                                 const int32_t* var_in_hap, const int32_t* is_ref, const int64_t* lik_off, int32_t* out_phased,
                                 double* out_lik, double* out4, void* stream) nogil

    # ---- computeHaplotypeScore (vcfutils.pyx:1076-1114)
    int plat_haplotype_score_batch(plat_ctx* ctx, const plat_window_batch* batch, int n_ind, int max_haps_per_window,
                                   const int32_t* seg_read_begin, const int32_t* seg_n_good, const double* loglik,
                                   double* out_hap_like, int32_t* out_hap_score, void* stream) nogil

    # ---- VariantCandidateGenerator.addCandidatesFromReads (variant.pyx:722-743)
    ctypedef struct plat_candidate_batch:
        int32_t n_regions
        int32_t n_reads
        const uint8_t* ref_seq
        const int64_t* ref_off
        const int32_t* ref_seq_start
        const int32_t* contig_len
        const uint8_t* read_seq
        const uint8_t* read_qual
        const int64_t* read_off
        const int32_t* read_pos
        const int32_t* read_flags
        const int16_t* cigar
        const int32_t* cig_off
    int plat_candidates_batch(plat_ctx* ctx, const plat_candidate_batch* batch, int min_flank, int min_base_qual, int gen_snps,
                              int gen_indels, int max_per_read, const int32_t* read_region, int32_t* out_rec, int32_t* out_count,
                              int32_t* out_status, void* stream) nogil

    # ---- addVariantToList + the per-sample support filter (variant.pyx:499-527, variantcaller.pyx:456-467)
    int plat_candidates_merge_batch(plat_ctx* ctx, const plat_candidate_batch* batch, const int32_t* read_end, int n_scans,
                                    const int32_t* scan_read_begin, const int32_t* scan_longest, int max_per_read, const int32_t* rec,
                                    const int32_t* count, const int32_t* status, double min_var_freq, int cap_per_scan,
                                    int32_t* out_cand, int32_t* out_n, void* stream) nogil

    # ---- candidates -> variants -> windows -> haplotypes -> the window batch, one sample per region (variantcaller.pyx:456-531,
    #      platypusutils.pyx:806-931, variantFilter.pyx:98-171,377-441, window.py:49-238, chaplotype.pyx:127-191,397-449)
    ctypedef struct plat_stage_b_options:
        int32_t minReads
        int32_t maxSize
        int32_t mergeClusteredVariants
        int32_t maxVarDist
        int32_t minVarDist
        int32_t largeWindows
        int32_t maxVariants
        int32_t maxHaplotypes
        int32_t filterVarsByCoverage
        int32_t skipDifficultWindows
        double maxReads
    ctypedef struct plat_stage_b_in:
        int32_t n_regions
        int32_t cap_per_scan
        const int32_t* cand
        const int32_t* cand_n
        const int32_t* cand_rec
        const int64_t* region_name_hash
        const uint8_t* ref_seq
        const int64_t* ref_off
        const int32_t* ref_seq_start
        const int32_t* contig_len
        const int32_t* region_start
        const int32_t* region_end
        const int32_t* region_rlen
        const uint8_t* read_seq
        const int64_t* read_off
        const int32_t* read_pos
        const int32_t* read_end
        const int32_t* tab_begin
        const int32_t* tab_n
        const int32_t* tab_longest
        const int32_t* broken_mate_pos
        int32_t broken_base
        int32_t cap_vars
        int32_t cap_windows
        int32_t cap_added
        int32_t cap_batch_windows
        int32_t cap_batch_haps
        int32_t cap_batch_reads
        int64_t cap_hap_bytes
    ctypedef struct plat_stage_b_out:
        int32_t* hdr
        int32_t* var_pos
        int32_t* var_nrem
        int32_t* var_nadd
        int32_t* var_support
        int32_t* var_bam_min
        int32_t* var_bam_max
        int32_t* var_rem_pos
        int32_t* var_add_off
        uint8_t* added
        int32_t* win_start
        int32_t* win_end
        int32_t* win_var_first
        int32_t* win_var_n
        int32_t* win_flags
        int32_t* win_ptrs
        int32_t* win_n_haps
        int32_t* win_batch
        int32_t* b_hap_begin
        int32_t* b_read_begin
        int32_t* b_start
        int32_t* b_end
        int32_t* b_flank
        int64_t* b_pair_off
        int64_t* b_gl_off
        int32_t* b_seg_begin
        int32_t* b_n_good
        int64_t* b_hap_off
        uint32_t* b_hap_mask
        uint8_t* b_hap_seq
        int64_t* b_read_off
        int32_t* b_read_src
        uint8_t* b_read_kind
        int64_t* totals
        int32_t* scratch
    int plat_stage_b_batch(plat_ctx* ctx, const plat_stage_b_in* batch, const plat_stage_b_options* options, const plat_stage_b_out* out,
                           void* stream) nogil

    ctypedef struct plat_unpack_piece:
        const uint8_t* src
        int64_t dst
        int64_t n
    int plat_unpack_reads_pieces(plat_ctx* ctx, int n_pieces, int64_t max_piece_bytes, const plat_unpack_piece* pieces, uint8_t* out_seq, uint8_t* out_qual,
                                 int64_t total_bytes, int64_t n_exc, const int64_t* exc_index, const uint8_t* exc_base, const uint8_t* exc_qual, void* stream) nogil

    int plat_unpack_reads_pieces_codes(plat_ctx* ctx, int n_pieces, int64_t max_piece_bytes, const plat_unpack_piece* pieces, uint8_t* out_seq, uint8_t* out_qual,
                                       uint32_t* out_codes, int64_t total_bytes, int64_t n_exc, const int64_t* exc_index, const uint8_t* exc_base,
                                       const uint8_t* exc_qual, void* stream) nogil
    int plat_ref_codes(plat_ctx* ctx, int n_regions, const uint8_t* ref_seq, const int64_t* ref_off, int64_t n_bytes, uint32_t* out_codes,
                       int32_t* out_irregular, void* stream) nogil
    int plat_candidates_batch_codes(plat_ctx* ctx, const plat_candidate_batch* batch, const uint32_t* read_codes, const uint32_t* ref_codes,
                                    const int32_t* ref_irregular, int min_flank, int min_base_qual, int gen_snps, int gen_indels, int max_per_read,
                                    const int32_t* read_region, int32_t* out_rec, int32_t* out_count, int32_t* out_status, void* stream) nogil
    int plat_copy_pieces(plat_ctx* ctx, int n_pieces, int64_t max_piece_bytes, const plat_unpack_piece* pieces, uint8_t* dst_blob, void* stream) nogil

    # ---- a chunk's read table from tables resident on the device
    ctypedef struct plat_table_desc:
        const int64_t* off
        const int32_t* pos
        const int32_t* end
        const uint8_t* mapq
        const int32_t* flags
        const int16_t* cigar
        const int32_t* cig_off
        int32_t n
        int32_t scan
        int64_t first_read
        int64_t first_byte
        int64_t first_pair
    int plat_concat_read_tables(plat_ctx* ctx, int n_tables, int max_reads_per_table, const plat_table_desc* desc, int64_t* dst_off, int32_t* dst_pos,
                                int32_t* dst_end, uint8_t* dst_mapq, int32_t* dst_flags, int32_t* dst_cig_off, int16_t* dst_cigar, int32_t* dst_region,
                                int64_t n_total_reads, int64_t total_bytes, int64_t total_pairs, void* stream) nogil

    # ---- checkAndTrimRead (cwindow.pyx:332-481)
    ctypedef struct plat_readqc_batch:
        int32_t n_reads
        int32_t _pad
        uint8_t* read_qual
        const int64_t* read_off
        const int32_t* read_pos
        const uint8_t* read_mapq
        int32_t* read_flags
        const int16_t* chrom_id
        const int16_t* mate_chrom_id
        const int32_t* insert_size
        const int32_t* mate_pos
        const int16_t* cigar
        const int32_t* cig_off
        const int32_t* stream_of
    ctypedef struct plat_readqc_options:
        int32_t min_good_qual_bases
        int32_t min_map_qual
        int32_t min_base_qual
        int32_t trim_overlapping
        int32_t trim_adapter
        int32_t trim_read_flank
        int32_t trim_soft_clipped
        int32_t filter_mate_unmapped
        int32_t filter_mate_distant
        int32_t filter_small_insert
        int32_t filter_duplicates
    int plat_read_qc_batch(plat_ctx* ctx, const plat_readqc_batch* batch, const plat_readqc_options* options, int32_t* out_ok,
                           int32_t* out_reason, void* stream) nogil

    # ---- the read buffers of fetched streams: checkAndTrimRead + addReadToBuffer's split (cwindow.pyx:560-595), gathered on the device
    ctypedef struct plat_read_buffers_in:
        plat_readqc_batch qc
        int32_t n_streams
        int32_t _pad
        const int32_t* stream_begin
        const uint8_t* read_seq
        const int32_t* read_end
    ctypedef struct plat_read_buffers_tables:
        int64_t* off
        int32_t* cig_off
        uint8_t* seq
        uint8_t* qual
        int16_t* cigar
        int32_t* pos
        int32_t* end
        uint8_t* mapq
        int32_t* flags
        int32_t* mate_pos
    int plat_read_buffers_batch(plat_ctx* ctx, const plat_read_buffers_in* inp, const plat_readqc_options* options, int32_t* out_ok,
                                int32_t* out_reason, int32_t* out_perm, int32_t* out_counts, const plat_read_buffers_tables* tab,
                                void* stream) nogil
    # ---- read tables from raw BAM alignment records: ReadIterator.get (htslibWrapper.pyx:328-406) on the device
    ctypedef struct plat_bam_decode_out:
        int64_t cap_bases
        int64_t cap_pairs
        int64_t* read_off
        int32_t* cig_off
        uint8_t* seq
        uint8_t* qual
        int16_t* cigar
        int32_t* pos
        int32_t* end
        uint8_t* mapq
        int32_t* flags
        int16_t* chrom_id
        int16_t* mate_chrom_id
        int32_t* insert_size
        int32_t* mate_pos
        int64_t* status
    int plat_bam_decode_batch(plat_ctx* ctx, int n_records, const uint8_t* blob, int64_t blob_len, const int64_t* rec_off,
                              const int64_t* rec_limit, const plat_bam_decode_out* out, void* stream) nogil
    # ---- BGZF blocks inflated on the device, and the BAM iterator over the inflated bytes (sam_itr_next)
    ctypedef struct plat_bgzf_inflate_out:
        int64_t cap_bytes
        uint8_t* data
        int64_t* out_off
        int64_t* status
    int plat_bgzf_inflate_batch(plat_ctx* ctx, int n_blocks, const uint8_t* blob, int64_t blob_len, const int64_t* blk_off,
                                const int64_t* blk_limit, const plat_bgzf_inflate_out* out, void* stream) nogil
    # ---- record text deflated to BGZF blocks on the device (the .gz output)
    ctypedef struct plat_bgzf_deflate_in:
        const uint8_t* text
        int64_t text_len
        int32_t n_pieces
        int32_t level
        const int64_t* piece_off
    ctypedef struct plat_bgzf_deflate_out:
        int64_t cap_bytes
        uint8_t* data
        int64_t* piece_out_off
        int64_t* status
    int plat_bgzf_deflate_batch(plat_ctx* ctx, const plat_bgzf_deflate_in* inp, const plat_bgzf_deflate_out* out, void* stream) nogil
    ctypedef struct plat_bam_find_in:
        int32_t n_streams
        int32_t n_chunks
        int32_t n_blocks
        int32_t _pad
        const uint8_t* data
        const int64_t* out_off
        const int32_t* stream_chunk_begin
        const int32_t* chunk_blk_first
        const int32_t* chunk_blk_end
        const int32_t* chunk_first_uoffset
        const int32_t* chunk_stop_blk
        const int32_t* chunk_stop_uoffset
        const int32_t* tid
        const int32_t* beg
        const int32_t* end
    ctypedef struct plat_bam_find_out:
        int64_t cap_records
        int64_t* rec_off
        int64_t* rec_limit
        int32_t* stream_begin
        int64_t* status
    int plat_bam_find_records(plat_ctx* ctx, const plat_bam_find_in* inp, const plat_bam_find_out* out, void* stream) nogil
    # records routed to samples by read group (the second branch of loadBAMData, platypusutils.pyx:573-666)
    enum:
        PLAT_ROUTE_MAX_GROUPS
        PLAT_ROUTE_MAX_SAMPLES
        PLAT_ROUTE_LDS_ID_BYTES
    ctypedef struct plat_bam_route_in:
        int32_t n_records
        int32_t n_streams
        int32_t n_groups
        int32_t n_samples
        const uint8_t* blob
        int64_t blob_len
        const int64_t* rec_off
        const int64_t* rec_end
        const int32_t* stream_begin
        const uint8_t* group_ids
        const int32_t* group_off
        const int32_t* group_sample
    ctypedef struct plat_bam_route_out:
        int64_t* rec_off
        int64_t* rec_limit
        int32_t* out_begin
        int32_t* rec_sample
        int64_t* status
        int32_t* why
    int plat_bam_route_batch(plat_ctx* ctx, const plat_bam_route_in* inp, const plat_bam_route_out* out, void* stream) nogil
    # broken mates: the mate coordinates of kept records, the mates of a second-round fetch (platypusutils.pyx:522-559)
    enum:
        PLAT_MATES_COORDS
        PLAT_MATES_FETCH
    ctypedef struct plat_bam_mates_in:
        int32_t n_streams
        int32_t n_records
        int32_t mode
        int32_t _pad
        const uint8_t* data
        int64_t data_len
        const int64_t* rec_off
        const int64_t* rec_limit
        const int32_t* stream_begin
        const int32_t* want_tid
        const int32_t* lo
        const int32_t* hi
    ctypedef struct plat_bam_mates_out:
        int64_t cap_records
        int64_t cap_bytes
        int32_t* coords
        int32_t* coord_begin
        uint8_t* out_data
        int64_t* out_rec_off
        int32_t* out_rec_len
        int32_t* out_mpos
        int32_t* out_begin
        int64_t* status
        int64_t* need_bytes
    int plat_bam_mates_batch(plat_ctx* ctx, const plat_bam_mates_in* inp, const plat_bam_mates_out* out, void* stream) nogil
    # candidate alleles from source VCF lines (variantutils.py:72-159,168-197 on the device)
    ctypedef struct plat_source_variants_in:
        int32_t n_regions
        int32_t maxSize
        int32_t longHaps
        int32_t _pad
        const uint8_t* text
        int64_t text_len
        const int64_t* text_off
        const int64_t* name_hash
    ctypedef struct plat_source_variants_out:
        int64_t cap_variants
        int32_t* region_begin
        int32_t* pos
        int64_t* rem_off
        int32_t* n_rem
        int64_t* add_off
        int32_t* n_add
        int32_t* hash
        int32_t* line
        int32_t* region_stats
        int64_t* status
    int plat_source_variants_batch(plat_ctx* ctx, const plat_source_variants_in* inp, const plat_source_variants_out* out, void* stream) nogil
    # tabix's iterator over inflated blocks (ti_iter_read, index.c.pysam.c:872-911, on the device)
    ctypedef struct plat_tabix_fetch_in:
        int32_t n_streams
        int32_t n_chunks
        int32_t n_blocks
        int32_t _pad
        const uint8_t* data
        int64_t data_len
        const int64_t* out_off
        const int32_t* stream_chunk_begin
        const int32_t* chunk_blk_first
        const int32_t* chunk_blk_end
        const int32_t* chunk_first_uoffset
        const int32_t* chunk_stop_blk
        const int32_t* chunk_stop_uoffset
        const uint8_t* names
        const int32_t* name_off
        const int32_t* beg
        const int32_t* end
    ctypedef struct plat_tabix_fetch_out:
        int64_t cap_text
        uint8_t* text
        int64_t* stream_text_off
        int64_t* stream_counts
        int64_t* status
    int plat_tabix_fetch_batch(plat_ctx* ctx, const plat_tabix_fetch_in* inp, const plat_tabix_fetch_out* out, void* stream) nogil
    # the tabix index of a bgzipped VCF (ti_index_core, index.c.pysam.c:320-393, on the device)
    int PLAT_TBI_STATUS_WORDS
    int PLAT_TBI_MAX_REF
    ctypedef struct plat_tabix_index_in:
        int32_t n_blocks
        int32_t _pad
        const uint8_t* data
        int64_t data_len
        const int64_t* out_off
        const int64_t* blk_addr
    ctypedef struct plat_tabix_index_out:
        int64_t cap_runs
        int64_t cap_names
        int64_t cap_windows
        int64_t cap_name_bytes
        int32_t* run_tid
        int32_t* run_bin
        int64_t* run_u
        int64_t* name_off
        int32_t* name_len
        uint8_t* name_bytes
        int64_t* lin_first
        int64_t* lin
        int64_t* status
    int plat_tabix_index_batch(plat_ctx* ctx, const plat_tabix_index_in* inp, const plat_tabix_index_out* out, void* stream) nogil
    # region queries over a flattened tabix or BAM index (ti_iter_query, index.c.pysam.c:776-870, on the device)
    int PLAT_IDXQ_STATUS_WORDS
    int PLAT_IDXQ_MAX_CHUNKS
    int PLAT_IDXQ_NO_ITERATOR
    int PLAT_IDXQ_HANDED_OVER
    ctypedef struct plat_index_query_in:
        int32_t n_ref
        int32_t n_queries
        int64_t n_bins
        int64_t n_chunks
        int64_t n_lin
        const int64_t* ref_bin_first
        const int32_t* bin_id
        const int64_t* bin_chunk_first
        const int64_t* chunk_u
        const int64_t* chunk_v
        const int64_t* ref_lin_first
        const int64_t* lin_fill
        const int32_t* tid
        const int32_t* beg
        const int32_t* end
    ctypedef struct plat_index_query_out:
        int64_t cap_chunks
        int32_t* count
        int32_t* gathered
        int64_t* q_first
        int64_t* out_u
        int64_t* out_v
        int64_t* status
    int plat_index_query_batch(plat_ctx* ctx, const plat_index_query_in* inp, const plat_index_query_out* out, void* stream) nogil
    # indexed sequence fetch from the bytes of a FASTA file (FastaFile.getSequence, fastafile.pyx:173-207, on the device)
    int PLAT_FASTA_STATUS_WORDS
    int PLAT_FASTA_OK
    int PLAT_FASTA_INDEX_ERROR
    int PLAT_FASTA_ZERO_LINE
    int PLAT_FASTA_BAD_INDEX
    int PLAT_FASTA_LEFT_OF_CUT
    int PLAT_FASTA_RIGHT_OF_CUT
    int PLAT_FASTA_MODE_SEQUENCE
    int PLAT_FASTA_MODE_CONTIG
    ctypedef struct plat_fasta_fetch_in:
        const uint8_t* file
        int64_t file_len
        int64_t file_base
        int64_t file_size
        int64_t n_queries
        const int64_t* start_pos
        const int64_t* line_len
        const int64_t* full_len
        const int64_t* seq_len
        const int64_t* beg
        const int64_t* end
        const uint8_t* mode
    ctypedef struct plat_fasta_fetch_out:
        int64_t cap_bytes
        int64_t* out_off
        int32_t* out_status
        uint8_t* out
        int64_t* totals
    int plat_fasta_fetch_batch(plat_ctx* ctx, const plat_fasta_fetch_in* inp, const plat_fasta_fetch_out* out, void* stream) nogil
    int plat_fasta_tile_bytes() nogil
    # read counts of reference-call blocks (outputRefCall's loop over countReadsCoveringRegion)
    int PLAT_REFCOV_RAISES
    int PLAT_REFCOV_EMPTY
    int PLAT_REFCOV_TILE
    ctypedef struct plat_refcov_in:
        int32_t n_intervals
        int32_t n_slices
        int32_t n_tiles
        int32_t n_reads
        const int32_t* read_pos
        const int32_t* read_end
        const int32_t* slice_begin
        const int32_t* slice_n
        const int32_t* slice_longest
        const int32_t* iv_start
        const int32_t* iv_end
        const int32_t* iv_slice_first
        const int32_t* iv_n_samples
        const int64_t* iv_count_off
        const int32_t* iv_tile_first
    ctypedef struct plat_refcov_out:
        int64_t cap_counts
        int32_t* iv_min
        int32_t* counts
    int plat_refcall_coverage_batch(plat_ctx* ctx, const plat_refcov_in* inp, const plat_refcov_out* out, void* stream) nogil
    int plat_refcov_lds_reads() nogil
    # the same for a PLAT_READS_PACKED table (one byte per base + exceptions): QC and trimming on the packed bytes, no quality array
    ctypedef struct plat_read_buffers_packed_in:
        plat_readqc_batch qc
        int32_t n_streams
        int32_t _pad
        const int32_t* stream_begin
        uint8_t* read_packed
        const int32_t* read_end
        int64_t n_exc
        const int64_t* exc_index
        const uint8_t* exc_base
        uint8_t* exc_qual
    int plat_read_buffers_packed_batch(plat_ctx* ctx, const plat_read_buffers_packed_in* inp, const plat_readqc_options* options, int32_t* out_ok,
                                       int32_t* out_reason, int32_t* out_perm, int32_t* out_counts, const plat_read_buffers_tables* tab,
                                       void* stream) nogil

    # ---- window read slices out of a resident read table (cwindow.pyx:208-264,655-689)
    # the read table of a loader that wrote one byte per base (2-bit base | quality << 2) expanded to ASCII on the device
    int plat_unpack_reads(plat_ctx* ctx, int64_t n_bytes, const uint8_t* packed, uint8_t* out_seq, uint8_t* out_qual, int64_t n_exc,
                          const int64_t* exc_index, const uint8_t* exc_base, const uint8_t* exc_qual, void* stream) nogil
    int plat_gather_reads(plat_ctx* ctx, int64_t n_dst, const int32_t* src_index, const int64_t* dst_off, const uint8_t* src_seq,
                          const uint8_t* src_qual, const int64_t* src_off, const int32_t* src_pos, const int32_t* src_end,
                          const uint8_t* src_mapq, const int32_t* src_flags, uint8_t* dst_seq, uint8_t* dst_qual, int32_t* dst_pos,
                          int32_t* dst_end, uint8_t* dst_mapq, int32_t* dst_flags, void* stream) nogil

    # ---- the per-read loop of vcfINFO (vcfutils.pyx:1300-1390)
    ctypedef struct plat_infostats_batch:
        int32_t n_vars
        int32_t n_ind
        const int32_t* var_window
        const int32_t* var_pos
        const int32_t* var_bam_min
        const int32_t* var_bam_max
        const int32_t* var_n_added
        const int32_t* var_n_removed
        const uint8_t* var_added
        const int64_t* var_added_off
        const uint8_t* var_in_genotype
        const int64_t* minq_off
        const int32_t* good_begin
        const int32_t* good_end
        const int32_t* bad_begin
        const int32_t* bad_end
        const uint8_t* read_seq
        const uint8_t* read_qual
        const int64_t* read_off
        const int32_t* read_pos
        const int32_t* read_end
        const uint8_t* read_mapq
        const int32_t* read_flags
        const int16_t* cigar
        const int32_t* cig_off
    int plat_variant_read_stats_batch(plat_ctx* ctx, const plat_infostats_batch* batch, int bad_reads_window,
                                      int count_only_exact_indel_matches, int64_t* out_counts, int32_t* out_per_sample,
                                      int32_t* out_minq, int32_t* out_nminq, void* stream) nogil
    int plat_variant_info_batch(plat_ctx* ctx, int n_vars, const int64_t* counts, const int64_t* minq_off, const int32_t* minq,
                                const int32_t* n_minq, double* out_terms, int32_t* out_mmlq, void* stream) nogil

    # ---- packed bases read where they lie: the packed counterparts of the entry points above
    ctypedef struct plat_packed_reads:
        const uint8_t* const* read_src
        int64_t n_exc
        const int64_t* exc_index
        const uint8_t* exc_base
        const uint8_t* exc_qual
    ctypedef struct plat_table_src_desc:
        const int64_t* off
        const int32_t* pos
        const int32_t* end
        const uint8_t* mapq
        const int32_t* flags
        const int16_t* cigar
        const int32_t* cig_off
        int32_t n
        int32_t scan
        int64_t first_read
        int64_t first_byte
        int64_t first_pair
        const uint8_t* src
    int plat_concat_read_tables_src(plat_ctx* ctx, int n_tables, int max_reads_per_table, const plat_table_src_desc* desc, int64_t* dst_off, int32_t* dst_pos,
                                    int32_t* dst_end, uint8_t* dst_mapq, int32_t* dst_flags, int32_t* dst_cig_off, int16_t* dst_cigar, int32_t* dst_region,
                                    const uint8_t** dst_src, int64_t n_total_reads, int64_t total_bytes, int64_t total_pairs, void* stream) nogil
    int plat_pack_codes_pieces(plat_ctx* ctx, int n_pieces, int64_t max_piece_bytes, const plat_unpack_piece* pieces, uint32_t* out_codes,
                               int64_t total_bytes, int64_t n_exc, const int64_t* exc_index, const uint8_t* exc_base, void* stream) nogil
    int plat_candidates_batch_packed(plat_ctx* ctx, const plat_candidate_batch* batch, const plat_packed_reads* packed, const uint32_t* read_codes,
                                     const uint32_t* ref_codes, const int32_t* ref_irregular, int min_flank, int min_base_qual, int gen_snps, int gen_indels,
                                     int max_per_read, const int32_t* read_region, int32_t* out_rec, int32_t* out_count, int32_t* out_status, void* stream) nogil
    int plat_gather_reads_packed(plat_ctx* ctx, int64_t n_dst, const int32_t* src_index, const int64_t* dst_off, const plat_packed_reads* packed,
                                 const int64_t* src_off, const int32_t* src_pos, const int32_t* src_end, const uint8_t* src_mapq,
                                 const int32_t* src_flags, uint8_t* dst_seq, uint8_t* dst_qual, int32_t* dst_pos, int32_t* dst_end,
                                 uint8_t* dst_mapq, int32_t* dst_flags, void* stream) nogil
    int plat_variant_read_stats_packed_batch(plat_ctx* ctx, const plat_infostats_batch* batch, const plat_packed_reads* packed, int bad_reads_window,
                                             int count_only_exact_indel_matches, int64_t* out_counts, int32_t* out_per_sample,
                                             int32_t* out_minq, int32_t* out_nminq, void* stream) nogil

    # ---- assembleReadsAndDetectVariants (assembler.pxd:3)
    ctypedef struct plat_assembly_batch:
        int32_t n_regions
        int32_t n_reads
        const uint8_t* ref_seq
        const int64_t* ref_off
        const int32_t* ref_start
        const int32_t* assem_start
        const int32_t* assem_end
        const int32_t* reg_read_begin
        const uint8_t* read_seq
        const uint8_t* read_qual
        const int64_t* read_off
    int plat_assemble_batch(plat_ctx* ctx, const plat_assembly_batch* batch, int kmer_size, int min_qual, int min_weight, int no_cycles,
                            int max_vars_per_region, int blob_per_region, int32_t* var_count, int32_t* var_pos, int32_t* var_nrem,
                            int32_t* var_nadd, int32_t* var_off, uint8_t* var_blob, int32_t* status, void* stream) nogil
    ctypedef struct plat_assembly_hints:
        int32_t max_ref_len
        int32_t max_reads_per_region
        int64_t max_positions
    int plat_assemble_batch_async(plat_ctx* ctx, const plat_assembly_batch* batch, const plat_assembly_hints* hints, int kmer_size, int min_qual,
                                  int min_weight, int no_cycles, int max_vars_per_region, int blob_per_region, int32_t* var_count, int32_t* var_pos,
                                  int32_t* var_nrem, int32_t* var_nadd, int32_t* var_off, uint8_t* var_blob, int32_t* status, void* stream) nogil


# The region loop of libplat_caller.so fed with fetched reads (include/platypus_caller_fetched.h): what loadBAMData (platypusutils.pyx:449-686)
# would hand over instead of its bamReadBuffers.  The tables, options and statistics of platypus_caller.h are used through pointers here.
cdef extern from "platypus_caller_fetched.h":
    ctypedef struct plat_caller:
        pass
    ctypedef struct plat_read_table:
        pass
    ctypedef struct plat_caller_options:
        pass
    ctypedef struct plat_caller_stats:
        pass
    ctypedef struct plat_fetched_reads:
        plat_read_table fetched
        plat_read_table broken_mates
        const int16_t* chrom_id
        const int16_t* mate_chrom_id
        const int32_t* insert_size
    ctypedef struct plat_fetched_region:
        const char* chrom
        int32_t start
        int32_t end
        const uint8_t* contig_seq
        int64_t contig_len
        const plat_fetched_reads* samples
        const uint8_t* dev_contig_seq
    ctypedef struct plat_caller_qc_options:
        int32_t minGoodQualBases
        int32_t minMapQual
        int32_t minBaseQual
        int32_t trimOverlapping
        int32_t trimAdapter
        int32_t trimReadFlank
        int32_t trimSoftClipped
        int32_t filterDuplicates
        int32_t filterReadsWithUnmappedMates
        int32_t filterReadsWithDistantMates
        int32_t filterReadPairsWithSmallInserts
    ctypedef struct plat_fetched_region_info:
        int32_t loaded
        int32_t* sample_counts
    void plat_caller_default_qc_options(plat_caller_qc_options* out)
    int plat_call_fetched_regions(plat_caller* c, const plat_fetched_region* regions, int n_regions, int n_samples,
                                  const char* const* sample_names, plat_caller_options* options, const plat_caller_qc_options* qc,
                                  char** out_text, size_t* out_len, plat_fetched_region_info* info, plat_caller_stats* stats) nogil

# The region loop fed with raw BAM alignment records (include/platypus_caller_bam.h): what the integrator holds after sam_itr_next,
# decoded on the device (plat_bam_decode_batch).
cdef extern from "platypus_caller_bam.h":
    ctypedef struct plat_bam_records:
        int32_t n_records
        const uint8_t* data
        int64_t data_len
        const int64_t* rec_off
    ctypedef struct plat_bam_sample:
        plat_bam_records fetched
        plat_bam_records broken_mates
    ctypedef struct plat_bam_region:
        const char* chrom
        int32_t start
        int32_t end
        const uint8_t* contig_seq
        int64_t contig_len
        const plat_bam_sample* samples
        const uint8_t* dev_contig_seq
    int plat_call_bam_regions(plat_caller* c, const plat_bam_region* regions, int n_regions, int n_samples,
                              const char* const* sample_names, plat_caller_options* options, const plat_caller_qc_options* qc,
                              char** out_text, size_t* out_len, plat_fetched_region_info* info, plat_caller_stats* stats) nogil

# The region loop fed with the BGZF blocks of an index lookup (include/platypus_caller_bgzf.h): inflated, iterated and decoded on the
# device (plat_bgzf_inflate_batch, plat_bam_find_records, plat_bam_decode_batch).
cdef extern from "platypus_caller_bgzf.h":
    ctypedef struct plat_bgzf_chunk:
        const uint8_t* data
        int64_t data_len
        int32_t first_uoffset
        int64_t end_coffset
        int32_t end_uoffset
    ctypedef struct plat_bgzf_sample:
        int32_t n_chunks
        const plat_bgzf_chunk* chunks
        plat_bam_records broken_mates
    ctypedef struct plat_bgzf_region:
        const char* chrom
        int32_t start
        int32_t end
        const uint8_t* contig_seq
        int64_t contig_len
        const uint8_t* dev_contig_seq
        int32_t tid
        int32_t itr_beg
        int32_t itr_end
        const plat_bgzf_sample* samples
    int plat_call_bgzf_regions(plat_caller* c, const plat_bgzf_region* regions, int n_regions, int n_samples,
                               const char* const* sample_names, plat_caller_options* options, const plat_caller_qc_options* qc,
                               char** out_text, size_t* out_len, plat_fetched_region_info* info, plat_caller_stats* stats) nogil


# The record front ends for merged files (include/platypus_caller_rg.h): the fetch of every FILE and one table read-group ID -> sample;
# the records are routed to samples on the device (plat_bam_route_batch).
cdef extern from "platypus_caller_rg.h":
    ctypedef struct plat_bam_read_groups:
        int32_t n_groups
        const char* const* id
        const int32_t* sample
    ctypedef struct plat_bam_file_records:
        plat_bam_records records
        const int32_t* rec_len
    ctypedef struct plat_bam_file:
        plat_bam_file_records fetched
        plat_bam_file_records broken_mates
    ctypedef struct plat_bgzf_file:
        int32_t n_chunks
        const plat_bgzf_chunk* chunks
        plat_bam_file_records broken_mates
    ctypedef struct plat_bam_rg_region:
        const char* chrom
        int32_t start
        int32_t end
        const uint8_t* contig_seq
        int64_t contig_len
        const plat_bam_file* files
        const uint8_t* dev_contig_seq
    ctypedef struct plat_bgzf_rg_region:
        const char* chrom
        int32_t start
        int32_t end
        const uint8_t* contig_seq
        int64_t contig_len
        const uint8_t* dev_contig_seq
        int32_t tid
        int32_t itr_beg
        int32_t itr_end
        const plat_bgzf_file* files
    int plat_call_bam_regions_rg(plat_caller* c, const plat_bam_rg_region* regions, int n_regions, int n_files,
                                 const plat_bam_read_groups* groups, int n_samples, const char* const* sample_names,
                                 plat_caller_options* options, const plat_caller_qc_options* qc, char** out_text, size_t* out_len,
                                 plat_fetched_region_info* info, plat_caller_stats* stats) nogil
    int plat_call_bgzf_regions_rg(plat_caller* c, const plat_bgzf_rg_region* regions, int n_regions, int n_files,
                                  const plat_bam_read_groups* groups, int n_samples, const char* const* sample_names,
                                  plat_caller_options* options, const plat_caller_qc_options* qc, char** out_text, size_t* out_len,
                                  plat_fetched_region_info* info, plat_caller_stats* stats) nogil


# Candidates from source VCFs (include/platypus_caller_source.h): the lines the integrator's tabix fetches returned, per region of the
# next call; parsed on the device (plat_source_variants_batch).
cdef extern from "platypus_caller_source.h":
    ctypedef struct plat_source_lines:
        const char* text
        int64_t len
    int plat_caller_set_source_lines(plat_caller* c, const plat_source_lines* per_region, int n_regions, int longHaps) nogil


# Source VCFs as the BGZF blocks of their tabix fetches (include/platypus_caller_tabix.h): inflated and iterated on the device
# (plat_bgzf_inflate_batch, plat_tabix_fetch_batch); from there on plat_caller_set_source_lines.
cdef extern from "platypus_caller_tabix.h":
    ctypedef struct plat_tabix_fetch:
        const char* seq_name
        int32_t itr_beg
        int32_t itr_end
        int32_t n_chunks
        const plat_bgzf_chunk* chunks
    ctypedef struct plat_source_blocks:
        int32_t n_fetches
        const plat_tabix_fetch* fetches
    ctypedef struct plat_source_blocks_info:
        int64_t n_blocks
        int64_t compressed_bytes
        int64_t inflated_bytes
        int64_t lines_walked
        int64_t lines_kept
        int64_t kept_bytes
        double seconds
    int plat_caller_set_source_blocks(plat_caller* c, const plat_source_blocks* per_region, int n_regions, int longHaps,
                                      plat_source_blocks_info* info) nogil


cdef extern from "platypus_caller_index.h":
    int PLAT_INDEX_TBI
    int PLAT_INDEX_BAI
    ctypedef struct plat_index:
        pass
    int plat_index_open(plat_caller* c, const uint8_t* bytes, size_t len, int kind, plat_index** out) nogil
    int plat_index_close(plat_index* idx) nogil
    int plat_index_n_refs(const plat_index* idx) nogil
    const char* plat_index_ref_name(const plat_index* idx, int tid) nogil
    int plat_index_tid(const plat_index* idx, const char* name) nogil
    ctypedef struct plat_index_query_info:
        int64_t queries
        int64_t handed_over
        int64_t chunks
        int64_t device_calls
        double seconds
    int plat_index_query(plat_index* idx, int n, const int32_t* tid, const int32_t* beg, const int32_t* end, const int64_t** first,
                         const int64_t** u, const int64_t** v, const int32_t** count, plat_index_query_info* info) nogil
    ctypedef struct plat_source_file:
        const uint8_t* data
        int64_t data_len
        plat_index* index
    ctypedef struct plat_source_region:
        const char* chrom
        int32_t start
        int32_t end
    int plat_caller_set_source_files(plat_caller* c, const plat_source_file* files, int n_files, const plat_source_region* regions, int n_regions,
                                     int longHaps, plat_source_blocks_info* info) nogil
    int plat_caller_source_lines(const plat_caller* c, int region, const char** text, int64_t* len) nogil


cdef extern from "platypus_caller_bamfile.h":
    int PLAT_BAM_FILES_PRESPLIT
    int PLAT_BAM_FILES_MERGED
    ctypedef struct plat_bamfile:
        pass
    int plat_bam_file_open(plat_caller* c, const uint8_t* data, int64_t data_len, const uint8_t* bai, size_t bai_len, const char* file_name,
                           plat_bamfile** out) nogil
    int plat_bam_file_close(plat_bamfile* f) nogil
    int plat_bam_file_n_refs(const plat_bamfile* f) nogil
    const char* plat_bam_file_ref_name(const plat_bamfile* f, int tid) nogil
    int64_t plat_bam_file_ref_len(const plat_bamfile* f, int tid) nogil
    int plat_bam_file_tid(const plat_bamfile* f, const char* name) nogil
    const char* plat_bam_file_header_text(const plat_bamfile* f, int64_t* len) nogil
    int plat_bam_file_n_read_groups(const plat_bamfile* f) nogil
    int plat_bam_file_read_group(const plat_bamfile* f, int i, const char** id, const char** sm) nogil
    int plat_bam_file_n_samples(const plat_bamfile* f) nogil
    const char* plat_bam_file_sample(const plat_bamfile* f, int i) nogil
    int plat_bam_file_header_raised(const plat_bamfile* f, const char** why) nogil
    int plat_bam_file_n_header_sq(const plat_bamfile* f) nogil
    int plat_bam_file_header_sq(const plat_bamfile* f, int i, const char** name, int64_t* len) nogil
    plat_index* plat_bam_file_index(const plat_bamfile* f) nogil
    ctypedef struct plat_bam_plan:
        int32_t mode
        int32_t n_samples
        const char* const* sample_names
        const int32_t* sample_file
        plat_bam_read_groups groups
    int plat_bam_files_plan(plat_bamfile* const* files, int n_files, plat_bam_plan** plan) nogil
    void plat_bam_plan_free(plat_bam_plan* plan) nogil
    ctypedef struct plat_bam_call_region:
        const char* chrom
        int32_t start
        int32_t end
        const uint8_t* contig_seq
        int64_t contig_len
        const uint8_t* dev_contig_seq
    ctypedef struct plat_bam_fetch:
        int32_t tid
        int32_t itr_beg
        int32_t itr_end
        int32_t n_chunks
        const plat_bgzf_chunk* chunks
    ctypedef struct plat_bam_fetch_plan:
        int32_t n_regions
        int32_t n_files
        const plat_bam_fetch* fetches
        int64_t queries
        int64_t handed_over
        int64_t chunks
        int64_t device_calls
        double seconds
    int plat_bam_files_fetch_plan(plat_bamfile* const* files, int n_files, const plat_bam_call_region* regions, int n_regions,
                                  plat_bam_fetch_plan** plan) nogil
    void plat_bam_fetch_plan_free(plat_bam_fetch_plan* plan) nogil
    int plat_call_bam_files(plat_caller* c, plat_bamfile* const* files, int n_files, const plat_bam_call_region* regions, int n_regions,
                            plat_caller_options* options, const plat_caller_qc_options* qc, char** out_text, size_t* out_len,
                            plat_fetched_region_info* info, plat_caller_stats* stats) nogil
    ctypedef struct plat_bam_mate_query:
        int32_t tid
        int32_t _pad
        int64_t start
        int64_t end
    ctypedef struct plat_bam_mates:
        int32_t n_coords
        int32_t n_queries
        const plat_bam_mate_query* queries
        plat_bam_file_records mates
    ctypedef struct plat_bam_mates_plan:
        int32_t n_regions
        int32_t n_files
        const plat_bam_mates* units
        const int32_t* loaded
        int64_t coords
        int64_t queries
        int64_t chunks
        int64_t records_looked_at
        int64_t records_kept
        int64_t device_calls
        int64_t input_bytes
        double seconds
    int plat_bam_files_mates_plan(plat_bamfile* const* files, int n_files, const plat_bam_call_region* regions, int n_regions,
                                  const plat_bam_fetch_plan* fetch_plan, const plat_caller_options* options, plat_bam_mates_plan** plan) nogil
    void plat_bam_mates_plan_free(plat_bam_mates_plan* plan) nogil
    int plat_call_bam_files_mates(plat_caller* c, plat_bamfile* const* files, int n_files, const plat_bam_call_region* regions, int n_regions,
                                  plat_caller_options* options, const plat_caller_qc_options* qc, char** out_text, size_t* out_len,
                                  plat_fetched_region_info* info, plat_caller_stats* stats) nogil


cdef extern from "platypus_caller_fasta.h":
    ctypedef struct plat_fasta:
        pass
    int plat_fasta_open(plat_caller* c, const uint8_t* file_bytes, int64_t file_len, const uint8_t* fai_bytes, int64_t fai_len, int parseNCBI,
                        plat_fasta** out) nogil
    int plat_fasta_close(plat_fasta* ref) nogil
    int plat_fasta_n_refs(const plat_fasta* ref) nogil
    int plat_fasta_ref(const plat_fasta* ref, int i, const char** name, int64_t* seq_len) nogil
    int plat_fasta_ref_line(const plat_fasta* ref, int i, int64_t* start_pos, int64_t* line_len, int64_t* full_line_len) nogil
    int plat_fasta_tid(const plat_fasta* ref, const char* name) nogil
    int64_t plat_fasta_total_length(const plat_fasta* ref) nogil
    ctypedef struct plat_fasta_info:
        int64_t queries
        int64_t file_bytes
        int64_t out_bytes
        int64_t device_calls
        double seconds
    int plat_fasta_load(plat_fasta* ref, const int32_t* tids, int n, plat_fasta_info* info) nogil
    int plat_fasta_contig(plat_fasta* ref, int tid, const uint8_t** host_seq, const uint8_t** dev_seq, int64_t* len) nogil
    int plat_fasta_get_sequences(plat_fasta* ref, int n, const int32_t* tid, const int64_t* beg, const int64_t* end, const int64_t** first,
                                 const uint8_t** bytes, const int32_t** status, plat_fasta_info* info) nogil
    int plat_fasta_get_character(const plat_fasta* ref, int tid, int64_t pos, uint8_t* out, int32_t* n_out) nogil
