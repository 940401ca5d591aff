/*
 * platypus_caller_tbi.h -- the tabix index (.tbi) of a compressed VCF for the native region loop (libplat_caller.so).
 *
 * plat_caller_compress_text (include/platypus_caller_bgzfout.h) gives the .vcf.gz; the reference's next step, --source, opens such a file
 * only with its .tbi next to it (variantutils.py:67: pysam's Tabixfile).  This entry point takes the whole file as it will lie on disk --
 * header blocks, record blocks, the EOF block -- and returns the index `tabix -p vcf` would write for it (ti_index_build; the rule is
 * stated in include/platypus_mi355x.h next to the device entry point, plat_tabix_index_batch), itself BGZF-compressed with the project's
 * own encoder and ended by the EOF block.  Bins are written in ascending order, where the reference writes its hash table's order: a
 * reader (tabix, pysam, platypus_amd/tabixindex.py) sees the same index, the bytes differ.
 *
 * Inside the call: the host walks the block headers (the BSIZE chain and the ISIZE words, never a payload byte); the file goes up in one
 * copy; plat_bgzf_inflate_batch and plat_tabix_index_batch are enqueued back to back on the caller's first stream; one wait for the two
 * status blocks, then the runs, the contigs' names and the windows alone come back and the finishing stage (csrc/tabix_index.hpp: runs
 * grouped by contig and bin, chunks that meet in a block merged, missing windows filled, the serialisation) runs over them: host work in
 * the number of runs and windows, not of bytes.  The index call is repeated once with the sizes the device names when its first guess of
 * the runs, contigs or windows was too small.  PLAT_CALLER_HOST_TBI=1 inflates and indexes on the host instead (the serial statement of
 * the same rule; tests, measurements): same bytes.
 *
 * Refused with a message in plat_caller_last_error, the caller staying usable: a BSIZE chain that breaks, a block with ISIZE 0 that has a
 * block with bytes behind it (the reference's reader ends the file there), a block the inflate refuses (PLAT_ERR_BAD_INPUT, naming the
 * block); a file the reference's indexer exits on -- a record line of fewer than two columns, a negative END, a position below the one
 * in front of it, a contig that appears twice, and a POS or END beyond 32 bits (PLAT_ERR_BAD_INPUT, naming the line, counted from 1 with
 * the header lines); more than 65536 contigs, or a library linked against a device library without plat_tabix_index_batch
 * (PLAT_ERR_UNSUPPORTED).
 * Not handled: the CSI format; the generic, SAM and UCSC presets.
 */
#ifndef PLATYPUS_CALLER_TBI_H
#define PLATYPUS_CALLER_TBI_H

#include "platypus_caller.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct plat_tbi_info {
    int64_t n_blocks, compressed_bytes, inflated_bytes;
    int64_t lines, records, runs, contigs, windows;
    int64_t device_calls;            /* 0 on the host path, 2 when a capacity was too small at first */
    int64_t refused_line;            /* the line a refused file is refused for, or -1 */
    double seconds;                  /* the whole call */
} plat_tbi_info;

/* tbi: a malloc'ed block of tbi_len bytes, to be given back with plat_caller_free.  info may be NULL. */
int plat_caller_index_bgzf(plat_caller* c, const uint8_t* file, size_t len, uint8_t** tbi, size_t* tbi_len, plat_tbi_info* info);

#ifdef __cplusplus
}
#endif
#endif /* PLATYPUS_CALLER_TBI_H */
