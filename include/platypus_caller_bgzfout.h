/*
 * platypus_caller_bgzfout.h -- compressed VCF output for the native region loop (libplat_caller.so): record text deflated to BGZF.
 *
 * The reference writes a gzip stream when --output ends in .gz (filez.Open returns gzip.GzipFile, opened at variantcaller.pyx:951-956).
 * This entry point takes the record text a plat_call_* returned, with the per-region byte counts plat_caller_region_text_lengths gives,
 * and returns it as BGZF blocks (include/platypus_mi355x.h states the encoding rule next to the device entry point it names
 * plat_bgzf_deflate_batch): a valid multi-member gzip file, so whatever reads the reference's .gz output reads it, and tabix can index it.
 * Every region's text becomes a whole number of blocks (an empty region none), so the compressed text of a call is again a text of
 * per-region pieces: region_out_len are its byte counts, and sharding.RegionTextExchange and plat_merge_region_blocks move and merge
 * those pieces as they move and merge plain text.  with_eof appends the 28-byte EOF marker of SAM specification 4.1.2; a writer that
 * concatenates several results (a header, the merged records) asks for it once, at the end.
 *
 * The text is compressed in slices of whole regions of about 32 MiB each, on the caller's worker contexts and streams, one slice per
 * worker at a time: upload, the device's four kernels, the compressed bytes back.  A slice's output buffer is sized from the usual
 * ratio; the device reports the bytes it needs when that is too little and the slice is run once more with that size.
 * PLAT_CALLER_HOST_DEFLATE=1 runs the host's restatement of the rule instead (csrc/bgzf_deflate.hpp; tests, measurements): same bytes.
 *
 * Refused with a message in plat_caller_last_error, the caller staying usable: a negative region_len or lengths that do not sum to len,
 * a level other than 0 or 1 (PLAT_ERR_INVALID); a library linked against a device library without plat_bgzf_deflate_batch
 * (PLAT_ERR_UNSUPPORTED).
 */
#ifndef PLATYPUS_CALLER_BGZFOUT_H
#define PLATYPUS_CALLER_BGZFOUT_H

#include "platypus_caller.h"

#ifdef __cplusplus
extern "C" {
#endif

/* out: a malloc'ed block of out_len bytes, to be given back with plat_caller_free.  region_out_len [n_regions] may be NULL; its sum
 * is out_len less the EOF marker. */
int plat_caller_compress_text(plat_caller* c, const char* text, size_t len, const int64_t* region_len, int n_regions, int level, int with_eof,
                              uint8_t** out, size_t* out_len, int64_t* region_out_len);

#ifdef __cplusplus
}
#endif
#endif /* PLATYPUS_CALLER_BGZFOUT_H */
