/*
 * platypus_caller_bgzf.h -- the region loop of libplat_caller.so (include/platypus_caller.h) for the BGZF blocks of a BAM file.
 *
 * plat_call_bam_regions (include/platypus_caller_bam.h) takes the uncompressed alignment records sam_itr_next returned: somebody has
 * inflated every block and walked every record on the host.  This entry point takes what an index lookup gives instead: per sample
 * the chunks of the fetch, each as the BGZF blocks it covers, exactly as they lie in the file, with the chunk's virtual offsets; and
 * the iterator's window (tid, itr_beg, itr_end, 0-based half-open).  The compressed bytes are uploaded as they are.  On the device
 * plat_bgzf_inflate_batch inflates and CRC-checks the blocks, plat_bam_find_records applies sam_itr_next's rule (both
 * include/platypus_mi355x.h: the block format, the rule and the refusals are stated there) and plat_bam_decode_batch decodes the kept
 * records, back to back without a host wait between them; from there on the call IS plat_call_bam_regions: the same text, rlen,
 * maxReads bail-out (on KEPT record counts: a region over the limit is dropped before its records are decoded), refusal of an unsorted
 * stream, info and plat_caller_region_text_lengths.
 *
 * The host reads the blocks' headers and trailers only (the BSIZE chain of each chunk and the ISIZE words that size the device's
 * output), and two status blocks and the kept counts back before the decode.
 *
 * A virtual offset is coffset << 16 | uoffset.  For a chunk [beg, end) of the index: data starts at the block at beg's coffset and
 * runs at least through the block at end's coffset (further blocks behind it are welcome: a record that starts before `end` may run
 * into them, and a record that runs past data refuses the call); first_uoffset = beg's uoffset; end_coffset = end's coffset MINUS
 * beg's coffset (an offset into data, which must be a block boundary of the chain, or data_len when end_uoffset is 0), end_uoffset =
 * end's uoffset; end_coffset -1: the chunk runs to the end of data.  A sample's chunks are one stream, in order: the first record
 * outside the window (refID != tid or pos >= itr_end) ends the stream, later chunks included.
 *
 * The broken mates stay uncompressed records (plat_bam_records): they come from other fetches.
 *
 * Refused with a message in plat_caller_last_error, the caller staying usable: a BSIZE chain that breaks or leaves data, an
 * end_coffset off a block boundary (PLAT_ERR_BAD_INPUT, naming region, sample and chunk, found on the host); a block the device
 * refuses (naming region, sample, chunk and block) or a stream whose record walk fails (naming region, sample and "record walk");
 * everything plat_call_bam_regions refuses.  plat_caller_stats.input_bytes counts the compressed bytes of the loaded regions'
 * chunks plus their broken-mate blobs.  A library linked against a device library without plat_bgzf_inflate_batch returns
 * PLAT_ERR_UNSUPPORTED.
 * Not handled: the CSI index, file I/O, CRAM.  The choice of chunks from a BAI is plat_index_query's (include/platypus_caller_index.h);
 * the BAM header and the cut of the chunks out of the file are include/platypus_caller_bamfile.h's, whose plat_call_bam_files ends in
 * this call.  For merged files, whose records are split by read group on the
 * device behind the iterator, see platypus_caller_rg.h.
 */
#ifndef PLATYPUS_CALLER_BGZF_H
#define PLATYPUS_CALLER_BGZF_H

#include "platypus_caller_bam.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One chunk of the index lookup. */
typedef struct plat_bgzf_chunk {
    const uint8_t* data;             /* whole BGZF blocks, from the block of the chunk's begin through (at least) the block of its end */
    int64_t data_len;
    int32_t first_uoffset;           /* low 16 bits of the chunk-begin virtual offset */
    int64_t end_coffset;             /* chunk end: block offset within data (may equal data_len), -1: to the end of data */
    int32_t end_uoffset;             /* ... and offset inside that block's inflated bytes */
} plat_bgzf_chunk;

/* One sample of one region: the chunks of the fetch, in order, and the broken mates it fetched, in mate-position order. */
typedef struct plat_bgzf_sample {
    int32_t n_chunks;
    const plat_bgzf_chunk* chunks;   /* [n_chunks] */
    plat_bam_records broken_mates;
} plat_bgzf_sample;

/* plat_region with chunk samples and the iterator's window. */
typedef struct plat_bgzf_region {
    const char* chrom;
    int32_t start, end;
    const uint8_t* contig_seq;
    int64_t contig_len;
    const uint8_t* dev_contig_seq;       /* optional, as plat_region.dev_contig_seq */
    int32_t tid, itr_beg, itr_end;       /* sam_itr_queryi's arguments */
    const plat_bgzf_sample* samples;     /* [n_samples] */
} plat_bgzf_region;

/* As plat_call_bam_regions. */
int plat_call_bgzf_regions(plat_caller* c, const plat_bgzf_region* regions, int n_regions, int n_samples,
                           const char* const* sample_names, plat_caller_options* options, const plat_caller_qc_options* qc,
                           char** out_text, size_t* out_len, plat_fetched_region_info* info /* may be NULL */,
                           plat_caller_stats* stats /* may be NULL */);

#ifdef __cplusplus
}
#endif
#endif /* PLATYPUS_CALLER_BGZF_H */
