/*
 * platypus_caller_source.h -- candidates from source VCFs for the native region loop (libplat_caller.so): genotyping known alleles.
 *
 * Replaces, inside generateVariantsInRegion (src/cython/variantcaller.pyx:490-493,521),
 *
 *     variantutils.VariantCandidateReader.Variants          src/python/variantutils.py:56-163, isValidVcfLine :168-197
 *
 * for lines the integrator's tabix fetches returned.  Tabix, the .tbi index and file I/O stay with the integrator; the library takes the
 * text a fetch of each region returned, as it is: '\n'-ended lines (the last may lack it), the fetches of several source files back to
 * back in file order.  The lines are uploaded with their region's chunk and parsed on the device (plat_source_variants_batch,
 * include/platypus_mi355x.h, states the rule): only CHROM, POS, ID, REF and ALT are ever looked at, the host reads none of the INFO or
 * genotype columns.  The host replays set() and sorted() of variantutils.py:161 (the Python-2 set's order decides between two records
 * at one position) and joins the candidates as rawBamVariants + vcfFileVariants + assemblerVariants; they carry Source=File and no
 * supporting reads, equal candidates merge (sources OR-ed).  A region that has source lines takes the host's stage B, exactly as
 * assemble=1 regions do.  A line with fewer than five columns or without a usable POS (where pysam raises) ends the call with
 * PLAT_ERR_BAD_INPUT and a message that names region and line.  PLAT_CALLER_HOST_SOURCE=1 parses the lines on the host instead (tests,
 * measurements).  Limit: the source lines of one chunk (regions_per_chunk regions) must stay below 2^31 - 1024 bytes together, or the call
 * ends with PLAT_ERR_OVERFLOW.  HLA mode (variantcaller.pyx:617+) is not built.
 */
#ifndef PLATYPUS_CALLER_SOURCE_H
#define PLATYPUS_CALLER_SOURCE_H

#include "platypus_caller.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct plat_source_lines {
    const char* text;   /* the lines of the region's fetches; may be NULL when len is 0 */
    int64_t len;
} plat_source_lines;

/* The source lines of the NEXT plat_call_* on this caller, whichever front end it is (regions, stream, fetched, BAM, BGZF, read-group):
 * per_region[k] belongs to region k of that call's list.  The lines are cleared when that call returns, however it returns; the memory
 * is the caller's until then.  n_regions must be the call's (else the call returns PLAT_ERR_INVALID).  longHaps: options.longHaps
 * (1: indel records are taken untrimmed).  With source lines set, getVariantsFromBAMs=0 without assemble=1 is legal (the source alone)
 * and options->rlen is left as it was.  n_regions = 0 takes back lines set earlier. */
int plat_caller_set_source_lines(plat_caller* c, const plat_source_lines* per_region, int n_regions, int longHaps);

#ifdef __cplusplus
}
#endif
#endif /* PLATYPUS_CALLER_SOURCE_H */
