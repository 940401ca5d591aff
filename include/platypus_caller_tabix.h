/*
 * platypus_caller_tabix.h -- source VCFs for the native region loop (libplat_caller.so) as the BGZF blocks of their tabix fetches.
 *
 * plat_caller_set_source_lines (include/platypus_caller_source.h) takes the lines a tabix fetch returned: somebody has inflated every
 * block and walked every line through ti_iter_read on the host.  This entry point takes what the index lookup gives instead: per region
 * and source file the chunks of the fetch (ti_queryi's: variantutils.py:67 calls vcfFile.fetch(chromosome, start, end)), each as the
 * BGZF blocks it covers, exactly as they lie in the file, with the chunk's virtual offsets (a plat_bgzf_chunk, include/
 * platypus_caller_bgzf.h, says how); the sequence name the index holds for the queried tid; and the window (itr_beg, itr_end, 0-based
 * half-open).  Inside the call the compressed bytes are uploaded as they are, plat_bgzf_inflate_batch inflates and CRC-checks the
 * blocks and plat_tabix_fetch_batch applies ti_iter_read's rule (both include/platypus_mi355x.h: the block format, the rule and the
 * refusals are stated there), back to back on the caller's first stream; one wait, then the kept lines alone come back.  The caller
 * object owns that text until the next plat_call_* returns; from there on the call IS plat_caller_set_source_lines with it, so every
 * front end, the device parser and the stage-B routing work unchanged.  Nothing behind column 8 of any line is parsed anywhere.
 *
 * The host reads the blocks' headers and trailers only (the BSIZE chain of each chunk and the ISIZE words).
 *
 * Refused with a message in plat_caller_last_error, the caller staying usable and no source lines set: a BSIZE chain that breaks or
 * leaves data, an end_coffset off a block boundary (PLAT_ERR_BAD_INPUT, naming region, file and chunk); a block with ISIZE 0 that has
 * a block with bytes behind it in its chunk's data (PLAT_ERR_BAD_INPUT, naming region, file, chunk and block -- by design: the
 * reference ends the fetch, or cuts a line, at such a block; the empty blocks at the end of a chunk's data, the file's EOF marker, are
 * welcome); a block the inflate refuses (naming region, file, chunk and block); a stream whose walk fails (naming region, file and
 * "line walk": a line that runs past the end of a chunk that is not the fetch's last, or a POS or END beyond 32 bits).  A library
 * linked against a device library without plat_tabix_fetch_batch returns PLAT_ERR_UNSUPPORTED.  PLAT_CALLER_HOST_TABIX=1 inflates and
 * walks on the host instead (tests, measurements).
 * Not handled: the .csi index and file I/O (the integrator's; the .tbi and the choice of chunks are include/platypus_caller_index.h's:
 * plat_caller_set_source_files makes these structures itself), the generic, SAM and UCSC presets.
 */
#ifndef PLATYPUS_CALLER_TABIX_H
#define PLATYPUS_CALLER_TABIX_H

#include "platypus_caller_bgzf.h"
#include "platypus_caller_source.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One fetch of one source file for one region. */
typedef struct plat_tabix_fetch {
    const char* seq_name;            /* the name the index holds for the queried tid */
    int32_t itr_beg, itr_end;        /* ti_queryi's window */
    int32_t n_chunks;
    const plat_bgzf_chunk* chunks;   /* [n_chunks] in order */
} plat_tabix_fetch;

/* One region: its source files in file order (a file whose fetch raised in the reference, variantutils.py:68-70, is left out). */
typedef struct plat_source_blocks {
    int32_t n_fetches;
    const plat_tabix_fetch* fetches; /* [n_fetches] */
} plat_source_blocks;

typedef struct plat_source_blocks_info {
    int64_t n_blocks, compressed_bytes, inflated_bytes;
    int64_t lines_walked, lines_kept, kept_bytes;
    double seconds;                  /* the whole call */
} plat_source_blocks_info;

/* As plat_caller_set_source_lines: the source lines of the NEXT plat_call_* on this caller, here fetched from blocks.  The blocks are
 * read inside this call only.  n_regions = 0 takes back what was set; a second set before a call replaces the first. */
int plat_caller_set_source_blocks(plat_caller* c, const plat_source_blocks* per_region, int n_regions, int longHaps,
                                  plat_source_blocks_info* info /* may be NULL */);

#ifdef __cplusplus
}
#endif
#endif /* PLATYPUS_CALLER_TABIX_H */
