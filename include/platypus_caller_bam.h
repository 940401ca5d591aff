/*
 * platypus_caller_bam.h -- the region loop of libplat_caller.so (include/platypus_caller.h) for raw BAM alignment records.
 *
 * plat_call_fetched_regions (include/platypus_caller_fetched.h) takes the reads of a fetch as tables: somebody has run
 * ReadIterator.get (htslibWrapper.pyx:328-406) over every record -- every base, every quality and every CIGAR word through the
 * host.  This entry point takes what the integrator holds right after sam_itr_next instead: the uncompressed alignment records
 * themselves, starting at refID, lying anywhere in a byte blob (the record format, the decode rules and the refusals are those of
 * plat_bam_decode_batch, include/platypus_mi355x.h).  The records are uploaded as they are and decoded on the device into the
 * tables the fetched call's device stages take; from there on the call IS plat_call_fetched_regions on PLAT_READS_ASCII tables: the
 * same QC, split, gather and loop, the same record text, the same maxReads bail-out (on record counts), rlen, refusal of an unsorted
 * stream, info and plat_caller_region_text_lengths.
 *
 * The host touches no base, no quality and no CIGAR word on the way in.  It reads the decoded per-read arrays, CIGAR pairs and bases
 * (one byte per base, no qualities) back once, for the copies its own stages keep (as the fetched call keeps them from the tables it
 * was handed).
 *
 * end follows the bam_endpos of the htslib the reference declares: pos + the reference length of the CIGAR, which may be 0 (later
 * htslib versions give pos + 1 for a mapped record whose CIGAR consumes no reference); see plat_bam_decode_batch.
 *
 * The broken-mate records are decoded and not QC'd; the integrator lists them in mate-position order, as sortBrokenMates
 * (cwindow.pyx:759-766) would leave them -- rec_off may list records in any order, so no bytes move for that.
 *
 * A bad record (PLAT_ERR_BAD_INPUT) or records that overlap so that the decoded tables outgrow the blob's own bound
 * (PLAT_ERR_OVERFLOW) refuse the call with a message in plat_caller_last_error naming region, sample, table and record index; the
 * caller stays usable.  plat_caller_stats.input_bytes counts the record bytes uploaded: the blobs as handed over, names and aux data
 * included -- more than either encoding of the fetched call puts on the link.  A library linked against a device library without
 * plat_bam_decode_batch returns PLAT_ERR_UNSUPPORTED.
 * Not handled: the CG-tag convention for CIGARs of more than 65535 operations and CRAM.  For the compressed BGZF blocks of a BAM file,
 * inflated and iterated on the device in front of this call, see platypus_caller_bgzf.h; for merged files, whose records are split by
 * read group on the device in front of it, see platypus_caller_rg.h.
 */
#ifndef PLATYPUS_CALLER_BAM_H
#define PLATYPUS_CALLER_BAM_H

#include "platypus_caller_fetched.h"

#ifdef __cplusplus
extern "C" {
#endif

/* n_records records inside data[0 .. data_len): record i starts at data[rec_off[i]] (at its refID; a slice of an inflated BGZF
 * stream can be handed over as it is, rec_off pointing past each block_size).  rec_off need not be ascending or gap-free. */
typedef struct plat_bam_records {
    int32_t n_records;
    const uint8_t* data;
    int64_t data_len;
    const int64_t* rec_off;          /* [n_records] */
} plat_bam_records;

/* One sample of one region: the records of the fetch, in fetch order, and the broken mates it fetched, in mate-position order. */
typedef struct plat_bam_sample {
    plat_bam_records fetched, broken_mates;
} plat_bam_sample;

/* plat_region with record samples. */
typedef struct plat_bam_region {
    const char* chrom;
    int32_t start, end;
    const uint8_t* contig_seq;
    int64_t contig_len;
    const plat_bam_sample* samples;      /* [n_samples] */
    const uint8_t* dev_contig_seq;       /* optional, as plat_region.dev_contig_seq */
} plat_bam_region;

/* As plat_call_fetched_regions. */
int plat_call_bam_regions(plat_caller* c, const plat_bam_region* regions, int n_regions, int n_samples,
                          const char* const* sample_names, plat_caller_options* options, const plat_caller_qc_options* qc,
                          char** out_text, size_t* out_len, plat_fetched_region_info* info /* may be NULL */,
                          plat_caller_stats* stats /* may be NULL */);

#ifdef __cplusplus
}
#endif
#endif /* PLATYPUS_CALLER_BAM_H */
