/*
 * platypus_caller_rg.h -- the record front ends of libplat_caller.so (platypus_caller_bam.h, platypus_caller_bgzf.h) for MERGED files:
 * a BAM file that holds several samples, or a sample spread over several files.
 *
 * plat_call_bam_regions and plat_call_bgzf_regions take records that somebody has split by sample.  The reference's second loader branch
 * (platypusutils.pyx:573-666) does the split itself: every record's read group (ReadIterator.get(1, &rgID), htslibWrapper.pyx:348-361:
 * bam_aux_get(b, "RG"), bam_aux2Z) picks the buffer, buffersBySample[samplesByID[rgID]], and the broken mates go the same way
 * (:646-654).  The two entry points here take the fetch of every FILE instead, with one table read-group ID -> sample index for the
 * whole call (what the integrator has from the files' @RG header lines; duplicates resolved as the reference's dict would), and route
 * the records on the device (plat_bam_route_batch, include/platypus_mi355x.h, where the rule is written out): the host never reads an
 * aux byte.  From there on each call IS its pre-split neighbour on the streams the route made: the same decode, QC, split, loop, text,
 * maxReads bail-out (on the region's record count over all files, which does not depend on the routing), rlen, info and
 * plat_caller_region_text_lengths.
 *
 * A sample's stream is its records of file 0, then of file 1, ... (the reference loops over the files and appends), each in fetch
 * order.  Where that concatenation is not sorted by position the call is refused with the "not sorted by position" message of the
 * pre-split calls (the reference would qsort).  The broken mates of a sample are concatenated the same way; the integrator lists each
 * file's in mate-position order, so a sample whose broken mates come from ONE file has them in the order sortBrokenMates
 * (cwindow.pyx:759-766) leaves.
 *
 * A record's aux area ends where the record ends, and the record's own fields do not say where that is: every record comes with its
 * length (rec_len, the block_size word in front of it).  The BGZF call takes the fetched records' lengths from the blocks themselves.
 *
 * Refused with a message in plat_caller_last_error naming region, file and record (PLAT_ERR_BAD_INPUT; the caller stays usable): a
 * record with no RG field, with an RG field that is no string (type Z or H) or whose value is not in the table, or with aux data that
 * does not parse or runs past the record.  PLAT_ERR_INVALID with a message: a NULL or empty ID, one ID twice with different samples,
 * a sample index outside 0 .. n_samples - 1, rec_len missing or below 32.  More than PLAT_ROUTE_MAX_GROUPS read groups or
 * PLAT_ROUTE_MAX_SAMPLES samples, or a device library without plat_bam_route_batch: PLAT_ERR_UNSUPPORTED.
 * plat_caller_stats.input_bytes counts the blobs as handed over plus the table's bytes.
 * Not handled: the CG-tag convention for CIGARs of more than 65535 operations, CRAM.  The table from the files' @RG header lines and
 * the choice between this call and its pre-split neighbour are include/platypus_caller_bamfile.h's (plat_bam_files_plan).
 */
#ifndef PLATYPUS_CALLER_RG_H
#define PLATYPUS_CALLER_RG_H

#include "platypus_caller_bgzf.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The call's read groups: ID (NUL-terminated, not empty) -> sample index. */
typedef struct plat_bam_read_groups {
    int32_t n_groups;
    const char* const* id;           /* [n_groups] */
    const int32_t* sample;           /* [n_groups] */
} plat_bam_read_groups;

/* Records as plat_bam_records, each with its length. */
typedef struct plat_bam_file_records {
    plat_bam_records records;
    const int32_t* rec_len;          /* [n_records] block_size: record i is data[rec_off[i] .. rec_off[i] + rec_len[i]) */
} plat_bam_file_records;

/* One file of one region: the records of its fetch, in fetch order, and the broken mates it fetched, in mate-position order. */
typedef struct plat_bam_file {
    plat_bam_file_records fetched, broken_mates;
} plat_bam_file;

/* ... as an index lookup leaves it: the chunks of the fetch (plat_bgzf_sample's), and the broken mates as records. */
typedef struct plat_bgzf_file {
    int32_t n_chunks;
    const plat_bgzf_chunk* chunks;   /* [n_chunks] */
    plat_bam_file_records broken_mates;
} plat_bgzf_file;

/* plat_bam_region with files in place of samples. */
typedef struct plat_bam_rg_region {
    const char* chrom;
    int32_t start, end;
    const uint8_t* contig_seq;
    int64_t contig_len;
    const plat_bam_file* files;          /* [n_files] */
    const uint8_t* dev_contig_seq;       /* optional, as plat_region.dev_contig_seq */
} plat_bam_rg_region;

/* plat_bgzf_region with files in place of samples. */
typedef struct plat_bgzf_rg_region {
    const char* chrom;
    int32_t start, end;
    const uint8_t* contig_seq;
    int64_t contig_len;
    const uint8_t* dev_contig_seq;       /* optional, as plat_region.dev_contig_seq */
    int32_t tid, itr_beg, itr_end;       /* sam_itr_queryi's arguments */
    const plat_bgzf_file* files;         /* [n_files] */
} plat_bgzf_rg_region;

/* As plat_call_bam_regions. */
int plat_call_bam_regions_rg(plat_caller* c, const plat_bam_rg_region* regions, int n_regions, int n_files,
                             const plat_bam_read_groups* groups, int n_samples, const char* const* sample_names,
                             plat_caller_options* options, const plat_caller_qc_options* qc, char** out_text, size_t* out_len,
                             plat_fetched_region_info* info /* may be NULL */, plat_caller_stats* stats /* may be NULL */);

/* As plat_call_bgzf_regions. */
int plat_call_bgzf_regions_rg(plat_caller* c, const plat_bgzf_rg_region* regions, int n_regions, int n_files,
                              const plat_bam_read_groups* groups, int n_samples, const char* const* sample_names,
                              plat_caller_options* options, const plat_caller_qc_options* qc, char** out_text, size_t* out_len,
                              plat_fetched_region_info* info /* may be NULL */, plat_caller_stats* stats /* may be NULL */);

#ifdef __cplusplus
}
#endif
#endif /* PLATYPUS_CALLER_RG_H */
