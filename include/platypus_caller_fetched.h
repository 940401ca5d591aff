/*
 * platypus_caller_fetched.h -- the region loop of libplat_caller.so (include/platypus_caller.h) for reads as a BAM fetch returns them.
 *
 * plat_call_regions takes every sample's read buffers already split the way the reference's loader leaves them.  This entry point takes
 * what loadBAMData (platypusutils.pyx:449-686) has in hand instead: per sample the records a `fetch` of the region returned, in fetch
 * order, plus the broken mates it fetched.  The loader's per-read work -- bamReadBuffer.addReadToBuffer (cwindow.pyx:560-595), i.e.
 * checkAndTrimRead (:332-481) on every read, `reads` / `badReads`, the filter counts, isSorted, and the maxReads bail-out of
 * loadBAMData (:538-541) -- runs on the device (plat_read_buffers_batch, include/platypus_mi355x.h), and the buffers it makes go
 * through the same loop as plat_call_regions: the same record text.
 *
 * Each fetched read's bases and qualities cross the host-to-device link once: the fetched tables are uploaded, checked, trimmed, split
 * and gathered on the device, and the loop builds its chunk tables from them there (plat_read_table.dev_*).  The host reads back the
 * split (a permutation, per-read flags after QC, per-stream counts), not bases or qualities; it keeps host copies of the split tables'
 * per-read arrays and bases for its own stages, whose `qual` is NULL (no host stage reads qualities).
 *
 * The fetched tables may be PLAT_READS_ASCII or PLAT_READS_PACKED (include/platypus_caller.h), one encoding for every fetched table of
 * a call (empty tables aside; a call that mixes them is refused, PLAT_ERR_UNSUPPORTED with a message naming the table).  Packed tables
 * are checked and trimmed on their packed bytes and exceptions (plat_read_buffers_packed_batch): no quality array is built or uploaded,
 * and the split tables are PLAT_READS_PACKED as well -- the gathered, trimmed bytes on the device, the exceptions re-indexed into each
 * table with their trimmed qualities (the host reads those back).  The host copy of a split table's packed bytes keeps the quality
 * bits it was handed (no host stage reads them).  The records are those of the same call on ASCII tables.  Broken-mate tables may each
 * be of either encoding; they pass through unchanged.  plat_caller_stats.input_bytes counts the bases and qualities that cross the
 * link: 2 bytes per base of an ASCII table, 1 per base + 10 per exception of a packed one.
 *
 * Differences from the reference, by design:
 *  - a stream whose reads are not sorted by position (isSorted = False in the reference) is refused (PLAT_ERR_BAD_INPUT, message in
 *    plat_caller_last_error): a BAM fetch is coordinate-sorted, and the reference's sortReads is a qsort whose order of equal keys is
 *    not reproduced here;
 *  - the fetched tables of the whole call are resident on the device at once (a caller with a very long region list calls in parts).
 * A library linked against a device library without plat_read_buffers_batch (packed tables: plat_read_buffers_packed_batch) returns
 * PLAT_ERR_UNSUPPORTED.
 */
#ifndef PLATYPUS_CALLER_FETCHED_H
#define PLATYPUS_CALLER_FETCHED_H

#include "platypus_caller.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One sample of one region: the reads of the fetch, in fetch order (PLAT_READS_ASCII: seq = ASCII bases, qual = raw phred;
 * PLAT_READS_PACKED: seq = packed bytes + exceptions; the table's dev_* fields and hints are ignored), and per fetched read the three
 * fields checkAndTrimRead reads that plat_read_table has no room for.  broken_mates: as plat_sample_reads.broken_mates (sorted by
 * mate_pos), passed through unchanged. */
typedef struct plat_fetched_reads {
    plat_read_table fetched;
    plat_read_table broken_mates;
    const int16_t* chrom_id;          /* [fetched.n_reads] cAlignedRead.chromID */
    const int16_t* mate_chrom_id;     /* mateChromID */
    const int32_t* insert_size;       /* insertSize */
} plat_fetched_reads;

/* plat_region with fetched samples. */
typedef struct plat_fetched_region {
    const char* chrom;
    int32_t start, end;
    const uint8_t* contig_seq;
    int64_t contig_len;
    const plat_fetched_reads* samples;   /* [n_samples] */
    const uint8_t* dev_contig_seq;       /* optional, as plat_region.dev_contig_seq */
} plat_fetched_region;

/* The options of bamReadBuffer's constructor (cwindow.pyx:490-526; names and defaults of runner.py).  minMapQual / minBaseQual are
 * the QC's; the loop after it reads those of plat_caller_options (the reference has one options object: give both the same values).
 * filter* = 0 switches a filter off. */
typedef struct plat_caller_qc_options {
    int32_t minGoodQualBases, minMapQual, minBaseQual;                      /* 20, 20, 20 */
    int32_t trimOverlapping, trimAdapter, trimReadFlank, trimSoftClipped;   /* 1, 1, 0, 1 */
    int32_t filterDuplicates, filterReadsWithUnmappedMates, filterReadsWithDistantMates, filterReadPairsWithSmallInserts;   /* 1, 1, 1, 1 */
} plat_caller_qc_options;

/* Optional output, per region: loaded (0: the region reached maxReads and was not called), and per sample {n_good, n_bad, the
 * 8 reason counts of plat_read_buffers_batch} -- filteredReadCountsByType (cwindow.pyx:40-46) and secondary alignments. */
typedef struct plat_fetched_region_info {
    int32_t loaded;
    int32_t* sample_counts;              /* [10 * n_samples], caller's memory; NULL: not written */
} plat_fetched_region_info;

void plat_caller_default_qc_options(plat_caller_qc_options* out);
/* As plat_call_regions, with the loader's work in front: a region whose fetched reads, summed over its samples, reach
 * (int)options->maxReads is not called and leaves options->rlen as it was; every other region is called on the buffers
 * addReadToBuffer would have built.  plat_caller_region_text_lengths then lists every region of the list (0 for the skipped).
 * info: [n_regions] or NULL. */
int plat_call_fetched_regions(plat_caller* c, const plat_fetched_region* regions, int n_regions, int n_samples,
                              const char* const* sample_names, plat_caller_options* options, const plat_caller_qc_options* qc,
                              char** out_text, size_t* out_len, plat_fetched_region_info* info /* may be NULL */,
                              plat_caller_stats* stats /* may be NULL */);

#ifdef __cplusplus
}
#endif
#endif /* PLATYPUS_CALLER_FETCHED_H */
