/*
 * platypus_caller_index.h -- tabix (.tbi) and BAM (.bai) indexes for the native region loop (libplat_caller.so): opened once, queried in
 * batches on the device, and source VCFs taken as a file and its index instead of per-region fetch structures.
 *
 * plat_caller_set_source_blocks (include/platypus_caller_tabix.h) takes, per region and source file, the chunks an index lookup chose,
 * cut out of the file: the integrator ran ti_iter_query per (region, file) on the host.  Here the library does that itself:
 *
 *   plat_index_open        the index's bytes as they lie on disk (a .tbi is BGZF: it is inflated on the host with the library's own
 *                          inflate; a .bai is plain) are flattened ONCE into the tables plat_index_query_batch reads (include/
 *                          platypus_mi355x.h states the tables, the rule and the refusals; csrc/index_query.hpp is the flatten and the
 *                          host twin) and uploaded.  The format is serial -- every count moves what follows it -- so flattening is host
 *                          work in the size of the index, a few MB at most, once per file
 *   plat_index_query       n x (tid, beg, end) in ONE device batch on the caller's first stream and one wait: per query the chunk list
 *                          ti_iter_query / hts_itr_query would return.  A query that gathers more than PLAT_IDXQ_MAX_CHUNKS chunks is
 *                          handed over by the device and answered by the host twin (counted in info); a capacity the first call's guess
 *                          missed grows the buffers and calls again -- the caller sees neither
 *   plat_caller_set_source_files   per source file {the whole .vcf.gz in memory (it may be a mapped file), its open index}, per region
 *                          {chrom, start, end} as vcfFile.fetch(chromosome, start, end) takes them (variantutils.py:67).  Per region and file
 *                          the tid by name; a name the index does not hold or end < start leaves that file out of that region (the
 *                          reference's fetch raises there and the file is skipped, variantutils.py:68-70).  All queries of one file go
 *                          in one batch.  Each chunk [u, v) is cut from the block at u's coffset through the block at v's coffset, that
 *                          block included when v's uoffset is non-zero, its length read from its own BSIZE.  From there the call IS
 *                          plat_caller_set_source_blocks with those structures: the same text, the same refusals, the same info and
 *                          the same lifetime (the source lines of the NEXT plat_call_*)
 *
 * An index belongs to the caller it was opened on: it uses that caller's first stream, must be closed before the caller is destroyed,
 * and -- like every entry point of a caller -- is used by one thread at a time.  What plat_index_query returns is owned by the index
 * until its next query (plat_caller_set_source_files queries too) or its close.
 *
 * Refused with a message in plat_caller_last_error, the caller staying usable: bytes that are no index -- a .tbi that is not BGZF or
 * does not inflate, a bad magic, bytes that end before a count says they should, a negative count, a bin twice in one reference, a bin
 * id above 37450 (PLAT_ERR_BAD_INPUT); a preset other than VCF's, more than PLAT_TBI_MAX_REF references (PLAT_ERR_UNSUPPORTED); a
 * query whose tid lies outside the index (PLAT_ERR_INVALID, naming the query); a chunk whose coffset is no block header inside the
 * file's data (PLAT_ERR_BAD_INPUT, naming region, file and chunk); everything plat_caller_set_source_blocks refuses.  A library linked
 * against a device library without plat_index_query_batch returns PLAT_ERR_UNSUPPORTED from plat_index_query and
 * plat_caller_set_source_files, naming the symbol; PLAT_CALLER_HOST_INDEX=1 answers every query with the host twin instead (tests,
 * measurements; read once per call with the other switches).
 * Not handled: CSI indexes; the generic, SAM and UCSC presets; file I/O.  Whole BAM files -- the header, the samples, a call's queries
 * against the .bai and the cut of their chunks -- are include/platypus_caller_bamfile.h's.
 */
#ifndef PLATYPUS_CALLER_INDEX_H
#define PLATYPUS_CALLER_INDEX_H

#include "platypus_caller_tabix.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PLAT_INDEX_TBI 0
#define PLAT_INDEX_BAI 1

typedef struct plat_index plat_index;

int plat_index_open(plat_caller* c, const uint8_t* bytes, size_t len, int kind, plat_index** out);
int plat_index_close(plat_index* idx);
int plat_index_n_refs(const plat_index* idx);
/* The name of reference tid (NUL-ended, the index's memory), NULL outside the index and for a BAI, which has no names. */
const char* plat_index_ref_name(const plat_index* idx, int tid);
/* The tid of a name, -1 when absent; names compare byte by byte over their whole length. */
int plat_index_tid(const plat_index* idx, const char* name);

typedef struct plat_index_query_info {
    int64_t queries, handed_over;    /* handed_over: answered by the host twin (all of them under PLAT_CALLER_HOST_INDEX=1) */
    int64_t chunks;                  /* output chunks of all queries */
    int64_t device_calls;            /* 0 on the host path, 2 when the capacity was too small at first */
    double seconds;                  /* the whole call */
} plat_index_query_info;

/* first [n + 1] from 0, u / v [first[n]]: query q's chunks are first[q] .. first[q + 1]; count [n]: the chunks of q, or -1 where the
 * reference returns no iterator (end < beg).  The arrays are the index's.  info may be NULL. */
int plat_index_query(plat_index* idx, int n, const int32_t* tid, const int32_t* beg, const int32_t* end,
                     const int64_t** first, const int64_t** u, const int64_t** v, const int32_t** count, plat_index_query_info* info);

typedef struct plat_source_file {
    const uint8_t* data;             /* the whole bgzipped VCF */
    int64_t data_len;
    plat_index* index;               /* its .tbi, opened on this caller */
} plat_source_file;

typedef struct plat_source_region {
    const char* chrom;
    int32_t start, end;              /* 0-based half-open, as fetch(chromosome, start, end) */
} plat_source_region;

/* As plat_caller_set_source_blocks: the source lines of the NEXT plat_call_* on this caller.  The files are read inside this call only. */
int plat_caller_set_source_files(plat_caller* c, const plat_source_file* files, int n_files, const plat_source_region* regions, int n_regions,
                                 int longHaps, plat_source_blocks_info* info /* may be NULL */);

/* What is set for the next call, whichever entry point set it: region k's source lines (the caller's memory, or for the block and file
 * entry points the caller object's, until that call returns).  PLAT_ERR_INVALID for a region outside what was set, or when nothing is set. */
int plat_caller_source_lines(const plat_caller* c, int region, const char** text, int64_t* len);

#ifdef __cplusplus
}
#endif
#endif /* PLATYPUS_CALLER_INDEX_H */
