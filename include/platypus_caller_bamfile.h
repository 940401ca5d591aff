/*
 * platypus_caller_bamfile.h -- whole BAM files for the native region loop (libplat_caller.so): a file and its .bai opened once, the
 * samples of a list of files, the fetch of every region of a call, and the call itself.
 *
 * plat_call_bgzf_regions (include/platypus_caller_bgzf.h) and plat_call_bgzf_regions_rg (include/platypus_caller_rg.h) take, per region,
 * the chunks an index lookup chose, cut out of the file, with the iterator's window, the sample names and -- for merged files -- the
 * table read-group ID -> sample: the integrator parsed the BAM header, read the @RG lines, decided between "one sample per file" and
 * "merged files", turned chrom:start-end into (tid, itr_beg, itr_end), queried the .bai and cut the chunks.  Here the library does that:
 *
 *   plat_bam_file_open     the file's bytes (they may be a mapped file; they are read, never copied, and must outlive the handle) and
 *                          its .bai's.  The host walks the BGZF chain from offset 0 only as far as the header needs (the block list and
 *                          the host inflate of csrc/host/bgzf_blocks.hpp) and parses BAM\1, l_text, the text, n_ref and (l_name, name,
 *                          l_ref) per reference; the .bai is opened with plat_index_open(PLAT_INDEX_BAI).  A .bai whose n_ref differs
 *                          from the header's is refused.  The header text is what Samfile.text returns: l_text bytes, cut at the first
 *                          NUL byte
 *   header text -> read groups and samples   the rule of Samfile.header (htslibWrapper.pyx:247-289) as far as
 *                          getSampleNamesAndLoadIterators (platypusutils.pyx:92-156) reads it: lines split on '\n', lines that are blank
 *                          after strip() skipped; a line without '@', a record type outside HD SQ RG PG CO, a field without ':', a field
 *                          code the record type does not list, a second @HD line, or an @SQ LN that int() refuses RAISES; CO lines are
 *                          kept whole.  key, value = field.split(":", 1): a value may hold ':', a line's last value keeps a '\r'.  A
 *                          code twice in one line: the last one wins.  Then :114-147: no @RG line, or an @RG line without SM, raises
 *                          too; the file's samples are the distinct SM values (one: that one; several: all of them); its read groups
 *                          are (ID, SM) in header order, and an @RG line without ID raises AFTER the groups in front of it were
 *                          entered (they stay, as in the reference's dict).  Whenever the header raises, the file's ONE sample is
 *                          file_name.split("/")[-1][0:-4] and the file contributes no (further) read groups
 *   plat_bam_files_plan    loadBAMData's decision (platypusutils.pyx:478): as many distinct samples as files: the pre-split path, one
 *                          stream per sample, the file of sample s chosen as :481-484 choose it (`sample in samplesByBAM[x]`: membership
 *                          in the file's sample list, or -- for a file whose sample is its name -- Python's substring test on that
 *                          name; anything but exactly one file is the reference's failed assertion and is refused); otherwise the
 *                          merged path with one plat_bam_read_groups table for the call: every file's (ID, SM) in file order, one ID
 *                          seen twice resolved as the reference's dict does (the last one wins), SM as its index in the sample order.
 *                          An ID whose SM is not among the samples (the groups in front of an @RG line without ID) is left out: its
 *                          records are refused as the reference's lookup raises.  Either way the sample order is the one :683-686 leave:
 *                          sorted by name, bytewise
 *   plat_bam_files_fetch_plan   per region and file exactly what those entry points are handed: the tid by name (-1 leaves that file
 *                          empty for that region, as the reference's except branch does, :496-504); the window of
 *                          sam_itr_querys("%s:%s-%s" % (chrom, start, end)): itr_beg = max(start - 1, 0), itr_end = end; the chunks of ONE
 *                          plat_index_query batch per file for all regions of the call; each chunk [u, v) cut from the block at u's
 *                          coffset through the block at v's coffset, that block included when v's uoffset is non-zero, its length read
 *                          from its own BSIZE (the cut plat_caller_set_source_files makes for a .tbi)
 *   plat_call_bam_files    the fetch plan, then plat_call_bgzf_regions (pre-split) or plat_call_bgzf_regions_rg (merged) on those
 *                          structures: text, rlen, the maxReads bail-out, refusals, info, plat_caller_region_text_lengths and
 *                          stats.input_bytes are what those calls give
 *
 * The window rule restates htslib's hts_parse_reg ("chr:a-b" is 1-based inclusive: beg = a - 1, clamped at 0; end = b), which is not part
 * of the reference tree: it is this project's statement of a library the reference links against, not reference text.
 *
 * The region structs of both BGZF calls hold ONE tid per region.  Files of one call whose headers give a region's contig different tids
 * are refused (PLAT_ERR_UNSUPPORTED, naming region and files).
 *
 * Handles belong to the caller they were opened on, are used by one thread at a time and are closed before it is destroyed.
 *
 * Refused with a message in plat_caller_last_error, the caller staying usable: bytes that are not BGZF or do not inflate, a bad magic, a
 * count (l_text, n_ref, l_name) that runs past the inflated bytes, a negative count, a .bai that is none or whose n_ref differs
 * (PLAT_ERR_BAD_INPUT); a region with max(start - 1, 0) >= end (PLAT_ERR_INVALID, naming the region); a chunk whose coffset is no block
 * header inside the file (PLAT_ERR_BAD_INPUT, naming region, file and chunk); a sample that :481-484 find in no file or in several
 * (PLAT_ERR_BAD_INPUT); everything plat_index_query and the two BGZF calls refuse, PLAT_ERR_UNSUPPORTED for a device library without
 * their symbols included (PLAT_CALLER_HOST_INDEX=1 answers the index queries on the host: plat_bam_files_fetch_plan then needs no device).
 *
 * Broken mates (options.assemble && options.assembleBrokenPairs, platypusutils.pyx:522-559 and :617-654: a second round of fetches for
 * the mates of improper pairs) are fetched by plat_bam_files_mates_plan and handed on by plat_call_bam_files_mates:
 *
 *   plat_bam_files_mates_plan   round one, one device batch for the call: the fetch plan's chunks uploaded and inflated,
 *                          plat_bam_find_records, plat_bam_mates_batch(PLAT_MATES_COORDS): every kept record with
 *                          !(flag & 0x2) || (flag & 0x4) || (flag & 0x8) and mtid != -1 gives (mtid, mpos), QC playing no part.  A region
 *                          whose kept records, summed over the files, reach options.maxReads is dropped by the call before any mate is
 *                          fetched (:538-541): it gets no second round.  On the host, per file and region: the coordinates sorted by
 *                          (contig name bytewise, mtid, mpos) and merged as mergeQueries merges them (:690-707: a query [s, e) grows to
 *                          mpos + 1 while the name is equal, mpos - e < 10000 and mpos - s < 100000).  A query is fetched by NAME: its tid
 *                          is plat_bam_file_tid(name), its window max(s - 1, 0) .. e.  Round two: ONE plat_index_query batch per file for
 *                          all its queries, the chunks cut, then one device batch: inflate, plat_bam_find_records,
 *                          plat_bam_mates_batch(PLAT_MATES_FETCH) -- a record is a broken mate when mtid == the region's tid and
 *                          start <= mpos <= end with loadBAMData's arguments, both ends inclusive -- and one read-back of the kept
 *                          records.  A record that two queries return is kept twice, as the reference appends it twice.  Per (region,
 *                          file) the mates are ordered by mate position, equal positions in fetch order (query, then record):
 *                          sortBrokenMates (cwindow.pyx:761-766) as fastcaller.py states it
 *   plat_call_bam_files_mates   plat_call_bam_files with that plan: with assemble && assembleBrokenPairs the fetch plan, the mates plan,
 *                          then plat_call_bgzf_regions (a sample's broken_mates are its file's) or plat_call_bgzf_regions_rg (a file's
 *                          broken_mates, routed by RG as its fetched records are); stats.input_bytes then includes the second round's
 *                          compressed bytes.  With either option 0 it IS plat_call_bam_files: the same text and no added launch.
 *
 * plat_call_bam_files itself still returns PLAT_ERR_UNSUPPORTED with a message for that pair of options.
 * Refused by the mates plan, the caller staying usable: a coordinate with mpos < 0, for which nothing in the reference tree defines the
 * region string (PLAT_ERR_BAD_INPUT, naming region, file and record); an mtid outside the file's header (PLAT_ERR_BAD_INPUT); everything
 * the index query, the inflate and the record walk refuse (naming region, file, and query where there is one); a device library without
 * plat_bam_mates_batch (PLAT_ERR_UNSUPPORTED, naming the symbol).
 * Known cost: round one is inflated for the mates plan and again inside the BGZF call.
 * Not handled: CRAM, CSI indexes, file I/O, region files, the CG-tag convention for long CIGARs, fileCaching and locks.
 */
#ifndef PLATYPUS_CALLER_BAMFILE_H
#define PLATYPUS_CALLER_BAMFILE_H

#include "platypus_caller_index.h"
#include "platypus_caller_rg.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct plat_bamfile plat_bamfile;

int plat_bam_file_open(plat_caller* c, const uint8_t* data, int64_t data_len, const uint8_t* bai, size_t bai_len, const char* file_name,
                       plat_bamfile** out);
int plat_bam_file_close(plat_bamfile* f);
int plat_bam_file_n_refs(const plat_bamfile* f);
/* NUL-ended, the handle's memory; NULL outside the header. */
const char* plat_bam_file_ref_name(const plat_bamfile* f, int tid);
/* l_ref, -1 outside the header. */
int64_t plat_bam_file_ref_len(const plat_bamfile* f, int tid);
/* The tid of a name (the first of equal names), -1 when absent. */
int plat_bam_file_tid(const plat_bamfile* f, const char* name);
/* The header text (NUL-ended, the handle's memory) and its length. */
const char* plat_bam_file_header_text(const plat_bamfile* f, int64_t* len /* may be NULL */);
/* The read groups this file enters into the call's table, in header order. */
int plat_bam_file_n_read_groups(const plat_bamfile* f);
int plat_bam_file_read_group(const plat_bamfile* f, int i, const char** id, const char** sm);
/* The samples this file adds to the sample list (the distinct SM values in first-seen order, or the one name cut from file_name). */
int plat_bam_file_n_samples(const plat_bamfile* f);
const char* plat_bam_file_sample(const plat_bamfile* f, int i);
/* 1 when reading the header raised and the sample is the file name's, with the reference's words for why in *why (may be NULL). */
int plat_bam_file_header_raised(const plat_bamfile* f, const char** why);
/* The (SN, LN) pairs of the header text's @SQ lines as getRegions reads them (platypusutils.pyx:1002-1003): -1 where that read raises --
 * the header's getter, no @SQ line, or one without SN or LN -- and the reference turns to the FASTA index. */
int plat_bam_file_n_header_sq(const plat_bamfile* f);
int plat_bam_file_header_sq(const plat_bamfile* f, int i, const char** name, int64_t* len);
/* The file's .bai, opened on the same caller (the handle's: closed with it). */
plat_index* plat_bam_file_index(const plat_bamfile* f);

#define PLAT_BAM_FILES_PRESPLIT 0    /* one sample per file: plat_call_bgzf_regions */
#define PLAT_BAM_FILES_MERGED 1      /* records split by read group: plat_call_bgzf_regions_rg */

typedef struct plat_bam_plan {
    int32_t mode;
    int32_t n_samples;
    const char* const* sample_names;     /* [n_samples] sorted bytewise */
    const int32_t* sample_file;          /* [n_samples] pre-split: the file of sample s; merged: NULL */
    plat_bam_read_groups groups;         /* merged: the call's table; pre-split: empty */
} plat_bam_plan;

/* The plan is freed with plat_bam_plan_free; it does not outlive the files (PLAT_ERR_BAD_INPUT leaves its message with files[0]'s caller). */
int plat_bam_files_plan(plat_bamfile* const* files, int n_files, plat_bam_plan** plan);
void plat_bam_plan_free(plat_bam_plan* plan);

/* One region of a call: plat_bgzf_region without the fetch. */
typedef struct plat_bam_call_region {
    const char* chrom;
    int32_t start, end;
    const uint8_t* contig_seq;
    int64_t contig_len;
    const uint8_t* dev_contig_seq;       /* optional, as plat_region.dev_contig_seq */
} plat_bam_call_region;

/* The fetch of one file for one region. */
typedef struct plat_bam_fetch {
    int32_t tid;                         /* -1: the file's header lacks the contig; no chunks */
    int32_t itr_beg, itr_end;
    int32_t n_chunks;
    const plat_bgzf_chunk* chunks;       /* [n_chunks] into the file's bytes */
} plat_bam_fetch;

typedef struct plat_bam_fetch_plan {
    int32_t n_regions, n_files;
    const plat_bam_fetch* fetches;       /* [n_regions * n_files]: region k, file f at k * n_files + f */
    int64_t queries, handed_over, chunks, device_calls;      /* plat_index_query_info summed over the files */
    double seconds;
} plat_bam_fetch_plan;

int plat_bam_files_fetch_plan(plat_bamfile* const* files, int n_files, const plat_bam_call_region* regions, int n_regions,
                              plat_bam_fetch_plan** plan);
void plat_bam_fetch_plan_free(plat_bam_fetch_plan* plan);

/* As plat_call_bgzf_regions; the sample names are the plan's.  info: [n_regions] or NULL; stats may be NULL. */
int plat_call_bam_files(plat_caller* c, plat_bamfile* const* files, int n_files, const plat_bam_call_region* regions, int n_regions,
                        plat_caller_options* options, const plat_caller_qc_options* qc, char** out_text, size_t* out_len,
                        plat_fetched_region_info* info, plat_caller_stats* stats);

/* One query of the second round: the contig by name (the first of equal names) and [start, end) as mergeQueries leaves them. */
typedef struct plat_bam_mate_query {
    int32_t tid, _pad;
    int64_t start, end;
} plat_bam_mate_query;

/* The broken mates of one file for one region. */
typedef struct plat_bam_mates {
    int32_t n_coords;                    /* kept first-round records that gave a mate coordinate */
    int32_t n_queries;
    const plat_bam_mate_query* queries;  /* [n_queries] in fetch order */
    plat_bam_file_records mates;         /* in mate-position order; records (without rec_len) is what plat_bgzf_sample.broken_mates takes */
} plat_bam_mates;

typedef struct plat_bam_mates_plan {
    int32_t n_regions, n_files;
    const plat_bam_mates* units;         /* [n_regions * n_files]: region k, file f at k * n_files + f */
    const int32_t* loaded;               /* [n_regions] 0: the region reached maxReads in round one and has no second round */
    int64_t coords, queries, chunks, records_looked_at, records_kept, device_calls, input_bytes;     /* chunks, records and compressed bytes: the second round's */
    double seconds;
} plat_bam_mates_plan;

/* fetch_plan: plat_bam_files_fetch_plan's for the same files and regions.  options: maxReads is read.  Freed with plat_bam_mates_plan_free;
 * the plan does not outlive the files. */
int plat_bam_files_mates_plan(plat_bamfile* const* files, int n_files, const plat_bam_call_region* regions, int n_regions,
                              const plat_bam_fetch_plan* fetch_plan, const plat_caller_options* options, plat_bam_mates_plan** plan);
void plat_bam_mates_plan_free(plat_bam_mates_plan* plan);

/* As plat_call_bam_files, the broken mates fetched (see above). */
int plat_call_bam_files_mates(plat_caller* c, plat_bamfile* const* files, int n_files, const plat_bam_call_region* regions, int n_regions,
                              plat_caller_options* options, const plat_caller_qc_options* qc, char** out_text, size_t* out_len,
                              plat_fetched_region_info* info, plat_caller_stats* stats);

#ifdef __cplusplus
}
#endif
#endif /* PLATYPUS_CALLER_BAMFILE_H */
