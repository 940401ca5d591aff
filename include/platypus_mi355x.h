/*
 * platypus_mi355x.h -- C ABI of libplat_mi355x.so
 *
 * MI355X-native (gfx950, hand-written HIP) replacement for the read->haplotype likelihood and
 * local-assembly hot path of andyrimmer/Platypus v0.8.1.1.  Every entry point names the reference
 * interface it replaces (file:line relative to the reference tree).  Plain C, plain pointers and
 * sizes, no C++/torch types; intended to be bound with cgo / JNI / ctypes / Cython `cdef extern`
 * (see INTEGRATION.md for the Cython stub a Platypus maintainer would add).
 *
 * Conventions
 *  - every function returns int: 0 = PLAT_OK, negative = error (plat_strerror()).  No exceptions
 *    cross the boundary (the reference raises Python exceptions: chaplotype.pyx:325-334,585-586).
 *  - all *batch* entry points take DEVICE pointers (HBM-resident; obtain with plat_malloc or pass
 *    e.g. torch.Tensor.data_ptr()) and a `stream` (hipStream_t as void*; NULL = default stream).
 *    They enqueue work and return; call plat_stream_sync() (or synchronise the stream yourself)
 *    before reading results.  Exceptions are flagged "[syncs]".
 *  - byte blobs (sequences, qualities) are 7-bit ASCII exactly as the reference holds them in
 *    cAlignedRead.seq / .qual (raw phred, NOT +33; htslibWrapper.pyx:366-368) and
 *    Haplotype.cHaplotypeSequence.  Every blob must be followed by >= PLAT_BLOB_PAD readable bytes.
 *  - the caller owns all buffers it passes; the context owns only its internal scratch.
 *  - a context is bound to one GPU and is not thread-safe (the reference is single-threaded per
 *    process: SURVEY.md 8(b)); use one context per process/rank -- or, as libplat_caller.so does, one per
 *    worker thread.  That includes plat_stream_sync: it records and waits on ONE event owned by the
 *    context, so two threads syncing different streams of the same context at once may return early.
 */
#ifndef PLATYPUS_MI355X_H
#define PLATYPUS_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PLAT_ABI_VERSION 1
#define PLAT_BLOB_PAD 32

/* error codes */
#define PLAT_OK 0
#define PLAT_ERR_INVALID (-1)       /* bad argument (NULL pointer, negative size, ...)              */
#define PLAT_ERR_HIP (-2)           /* HIP runtime error; plat_last_hip_error() has the code        */
#define PLAT_ERR_NOMEM (-3)         /* device allocation failed ("Out of memory in cHaplotype.alignReads") */
#define PLAT_ERR_HAP_TOO_LONG (-4)  /* haplotype longer than 16384 (chaplotype.pyx:180-183)         */
/* Also the read-length side of that refusal: the exact vote keeps longest haplotype + longest read + 8 diagonal counters of 16 bits in
 * LDS next to the haplotype's index; where they do not fit 160 KB the host returns PLAT_ERR_HAP_TOO_LONG before any seeding kernel is
 * launched (a batch with a 16384-base haplotype and a read of 26221 bases or more, aligned or not; 26220 fits).  Reads of up to 32767
 * bases pass validation (longer: PLAT_ERR_BAD_INPUT), but a pair is aligned only when hapLen >= readLen + 15, i.e. up to 16369 bases. */
#define PLAT_ERR_HAP_TOO_SHORT (-5) /* hapLen < readLen+15: the reference reads past the buffer here */
#define PLAT_ERR_UNSUPPORTED (-6)   /* option combination not implemented on the device path         */
#define PLAT_ERR_NO_DEVICE (-7)     /* no gfx950 device / HIP runtime unavailable                    */
#define PLAT_ERR_OVERFLOW (-8)      /* an output capacity given by the caller was too small          */
#define PLAT_ERR_BAD_INPUT (-9)     /* device-side input validation failed (non-ASCII byte, ...)     */
#define PLAT_ERR_BAD_HINTS (-10)    /* plat_batch_hints do not cover the batch (asynchronous entry point) */

typedef struct plat_ctx plat_ctx;

/* ---- context & memory ------------------------------------------------------------------------- */
int plat_abi_version(void);
const char* plat_strerror(int code);
int plat_device_count(int* out_count);
int plat_ctx_create(int device, plat_ctx** out_ctx);
int plat_ctx_destroy(plat_ctx* ctx);
int plat_last_hip_error(const plat_ctx* ctx);               /* hipError_t of the last PLAT_ERR_HIP   */
int plat_malloc(plat_ctx* ctx, size_t bytes, void** out_dev_ptr);
int plat_free(plat_ctx* ctx, void* dev_ptr);
int plat_memcpy_h2d(plat_ctx* ctx, void* dst_dev, const void* src_host, size_t bytes, void* stream);
int plat_memcpy_d2h(plat_ctx* ctx, void* dst_host, const void* src_dev, size_t bytes, void* stream);
int plat_memcpy_d2d(plat_ctx* ctx, void* dst_dev, const void* src_dev, size_t bytes, void* stream);
int plat_memset(plat_ctx* ctx, void* dst_dev, int value, size_t bytes, void* stream);
int plat_stream_sync(plat_ctx* ctx, void* stream);          /* [syncs] */
int plat_sync_poll_us(plat_ctx* ctx, int microseconds);     /* how often plat_stream_sync looks at its event (default 40; 0 = hipEventSynchronize) */
/* plat_stream_sync waits asleep: it polls an event every plat_sync_poll_us microseconds (default 40: a caller whose waits last a
 * millisecond or more asks for more -- every look is a system call and a runtime query, and with two dozen waiting threads they add up:
 * the native region loop uses 500) -- or every PLAT_SYNC_POLL_US microseconds when the environment says so (0 = the
 * runtime's blocking hipEventSynchronize; PLAT_SYNC_SPIN=1 = hipStreamSynchronize).  While it naps it lowers the CALLING thread's
 * timer slack (prctl PR_SET_TIMERSLACK) to 2 us and puts the previous value back before it returns. */
/* a HIP stream of the context's device (hipStream_t as void*), for callers without a HIP runtime binding of their own;
 * pinned (page-locked) host memory for staging buffers: copies from / to it are asynchronous and run at link speed */
int plat_stream_create(plat_ctx* ctx, void** out_stream);
int plat_stream_destroy(plat_ctx* ctx, void* stream);
int plat_host_alloc(plat_ctx* ctx, size_t bytes, void** out_host_ptr);
int plat_host_free(plat_ctx* ctx, void* host_ptr);

/* ---- live kernel timing (HIP events recorded on the caller's stream around each kernel) ----------
 * Used by bench.py for the roofline line; off by default (no overhead).  plat_profile_last [syncs]
 * on the recorded events and returns the durations of the kernels of the most recent
 * plat_align_window_batch / plat_genotype_window_batch call, plus the algorithmic byte count of
 * the DP launch: sum over launched DPs of (4*len2 + 34) bytes.                  */
typedef struct plat_profile {
    float ms_prepare;     /* validation + haplotype->window map (+ read-back)                     */
    float ms_seed;        /* gap-open annotation + 7-mer index + diagonal vote + candidate lists  */
    float ms_dp;          /* banded DP kernel (the dominant kernel)                               */
    float ms_finalize;    /* candidate selection + score -> log-likelihood                        */
    float ms_genotype;    /* genotype likelihood kernel                                           */
    float ms_seed_kernel; /* k_sweep + k_pairs (the seed stage without k_seed_slow)               */
    int64_t dp_jobs;      /* DPs in the DP launch                                                 */
    int64_t dp_alg_bytes; /* algorithmic bytes of the DP launch                                   */
    float ms_sweep;       /* k_sweep alone (the seeding stage is two kernels)                       */
    float ms_pairs;       /* k_pairs alone                                                         */
    float ms_unpack;      /* the last plat_unpack_reads_pieces launch on this context since the profile was switched on (0: none) */
    float ms_candidates;  /* the last plat_candidates_batch launch (k_candidates)                     */
} plat_profile;
int plat_profile_enable(plat_ctx* ctx, int on);
int plat_profile_last(plat_ctx* ctx, plat_profile* out);   /* [syncs] */

/* The same for EVERY kernel of the region loop's chunk (round 6): while the profile is on, each launch listed below is bracketed by
 * its own pair of HIP events on the launch stream; plat_kernel_times [syncs] resolves the pairs recorded since the last call and ADDS
 * each launch's duration (ms) and 1 to out_ms[id] / out_launches[id] (arrays of PLAT_KT_COUNT entries, the caller zeroes them).  A kernel
 * shares the chip only with what the caller lets run beside it: bench.py's counting pass runs one chunk at a time. */
enum {
    PLAT_KT_CANDIDATES = 0, PLAT_KT_CAND_MERGE, PLAT_KT_CAND_FILTER, PLAT_KT_UNPACK_PIECES, PLAT_KT_CONCAT_TABLES, PLAT_KT_COPY_PIECES,
    PLAT_KT_GATHER_READS, PLAT_KT_SB_VARIANTS, PLAT_KT_SB_WINDOWS, PLAT_KT_SB_HAPS_RANK, PLAT_KT_SB_PREFIX, PLAT_KT_SB_SCAN,
    PLAT_KT_SB_HAPS_WRITE, PLAT_KT_SB_READS, PLAT_KT_VALIDATE, PLAT_KT_TILE_SCAN, PLAT_KT_PREP_READS, PLAT_KT_SWEEP, PLAT_KT_PAIRS,
    PLAT_KT_SEED_SLOW, PLAT_KT_DP_JOBS, PLAT_KT_FINALIZE, PLAT_KT_GENOTYPE, PLAT_KT_HAPLOTYPE_SCORE, PLAT_KT_EM, PLAT_KT_VARIANT_POSTERIOR,
    PLAT_KT_VARIANT_READ_STATS, PLAT_KT_VARIANT_INFO, PLAT_KT_GENOTYPE_CALL, PLAT_KT_ASSEMBLE, PLAT_KT_READ_QC, PLAT_KT_OTHER,
    PLAT_KT_COUNT
};
const char* plat_kernel_timer_name(int id);                 /* "k_candidates", ...; NULL outside 0 .. PLAT_KT_COUNT-1 */
int plat_kernel_times(plat_ctx* ctx, double* out_ms, int64_t* out_launches);   /* [syncs] */
/* ONE kernel timed while the profile is off (id < 0: none): two events per launch of that kernel, nothing else changes -- how bench.py times the
 * line's roofline kernel INSIDE its timed region, next to whatever shares the chip with it there.                                              */
int plat_kernel_timer_only(plat_ctx* ctx, int id);

/* ---- a1: fastAlignmentRoutine, score only -------------------------------------------------------
 * Replaces  int fastAlignmentRoutine(seq1, seq2, qual2, len1, len2, gapextend, nucprior,
 *                                    localgapopen, aln1=NULL, aln2=NULL, firstpos)
 *           src/c/align.h:8-10, src/c/align.c:77-586  (called from calign.pyx:232,258)
 * for n independent DP instances in padded rows:
 *   hap_slices [n][lmax+15], reads [n][lmax], quals [n][lmax], gapopen [n][lmax+15], len2 [n]
 *   (7 <= len2[i] <= lmax; rows need no particular alignment).  out_score [n].
 * The returned score is bit-identical to the reference's (8 x int16 wrapping lanes).          */
int plat_dp_batch(plat_ctx* ctx, int n, int lmax,
                  const uint8_t* hap_slices, const uint8_t* reads, const uint8_t* quals,
                  const uint8_t* gapopen, const int32_t* len2, int gapextend, int nucprior,
                  int32_t* out_score, void* stream);

/* ---- a3..a10: Haplotype.alignReads / alignSingleRead for whole windows -------------------------
 * Replaces, for every haplotype of every window in the batch,
 *   cdef double* Haplotype.alignReads(individualIndex, start,end, badStart,badEnd, brokenStart,
 *        brokenEnd, useMapQualCap)                       chaplotype.pxd:44, chaplotype.pyx:306-377
 *   cdef double  Haplotype.alignSingleRead(read, useMapQualCap)            chaplotype.pyx:379-384
 * including hash_sequence_multihit / hashReadForMapping / mapAndAlignReadToHaplotype
 * (calign.pyx:94-272), annotateWithGapOpen (chaplotype.pyx:552-590) and the score -> log
 * likelihood transform (chaplotype.pyx:621-676, standard mode).
 *
 * Ragged (CSR) layout, all arrays in device memory:
 *   windows  w in [0,n_windows):  haplotypes  win_hap_begin[w]..win_hap_begin[w+1]
 *                                 reads       win_read_begin[w]..win_read_begin[w+1]
 *                                 win_start[w], win_end[w] = Haplotype.startPos / endPos
 *                                 win_flank[w]             = Haplotype.endBufferSize
 *                                 pair_off[w]  = offset of the window's output block (int64)
 *   haplotypes h: bytes hap_seq[hap_off[h] .. hap_off[h+1])   (Haplotype.cHaplotypeSequence)
 *   reads r (reference order good -> bad -> brokenMates per sample, chaplotype.pyx:341-373):
 *       seq/qual bytes read_seq|read_qual[read_off[r] .. read_off[r+1]),
 *       read_pos[r], read_end[r] (cAlignedRead.pos/.end), read_mapq[r], read_flags[r] (bitFlag),
 *       read_kind[r] 0 = reads, 1 = badReads, 2 = brokenMates.
 * Output: out_loglik[pair_off[w] + hl*R_w + rl] for local haplotype hl, local read rl -- exactly
 * the concatenation of the per-haplotype likelihoodCache arrays without the 999 terminator
 * (0.0 for QCFail / overlap<7 reads, chaplotype.pyx:343-346).  out_score (optional, may be NULL)
 * receives the integer alignment score (-1 for skipped reads).
 * Options: calc_flank_score (--calculateFlankScore, runner.py:559, default 0): when 1 every DP runs in
 * the reference's traceback mode (align.c:96,345-365,494-577) and calculateFlankScore (align.c:593-644)
 * is subtracted as calign.pyx:235-245,261-264 do; needs win_flank > 0 (the reference dereferences a NULL
 * alignment buffer otherwise) else PLAT_ERR_UNSUPPORTED.  use_mapq_cap (HLATyping mode) must be 0 in this
 * version (PLAT_ERR_UNSUPPORTED otherwise).
 * [syncs] once internally (job-count read-back).                                                 */
typedef struct plat_window_batch {
    int32_t n_windows, n_haps, n_reads, _pad;
    const int32_t* win_hap_begin;   /* [n_windows+1] */
    const int32_t* win_read_begin;  /* [n_windows+1] */
    const int32_t* win_start;       /* [n_windows] */
    const int32_t* win_end;         /* [n_windows] */
    const int32_t* win_flank;       /* [n_windows] */
    const int64_t* pair_off;        /* [n_windows+1] */
    const uint8_t* hap_seq;         /* blob */
    const int64_t* hap_off;         /* [n_haps+1] */
    const uint8_t* read_seq;        /* blob */
    const uint8_t* read_qual;       /* blob, same offsets */
    const int64_t* read_off;        /* [n_reads+1] */
    const int32_t* read_pos;        /* [n_reads] */
    const int32_t* read_end;        /* [n_reads] */
    const uint8_t* read_mapq;       /* [n_reads] */
    const int32_t* read_flags;      /* [n_reads] */
    const uint8_t* read_kind;       /* [n_reads] */
} plat_window_batch;

typedef struct plat_align_stats {
    int64_t n_pairs;          /* read x haplotype pairs in the batch                                  */
    int64_t n_pairs_aligned;  /* pairs not skipped by the QCFail / overlap<7 rule                     */
    int64_t n_dp_launched;    /* banded DPs the device actually ran                                    */
    int64_t n_dp_reference;   /* fastAlignmentRoutine calls the reference would have made             */
    int64_t cells_reference;  /* sum over those calls of 16*len2 (the GCUPS numerator)   */
    int64_t cells_launched;   /* sum over launched DPs of 16*len2                                      */
    int64_t n_seed_fallback;  /* pairs whose candidate diagonals needed the full vote (not provably unique)   */
    int64_t _reserved;
} plat_align_stats;

int plat_align_window_batch(plat_ctx* ctx, const plat_window_batch* batch, int calc_flank_score,
                            int use_mapq_cap, double* out_loglik, int32_t* out_score,
                            plat_align_stats* out_stats /* host, may be NULL */, void* stream);

/* Asynchronous variant: the same work, but NOTHING is read back and the call never waits for the GPU
 * (plat_align_window_batch reads two small counters blocks back: after validation, to size its scratch
 * buffers, and after seeding, to size the DP launch -- ~55 us of idle GPU per call).  The caller, who
 * built the offset arrays, states the sizes up front:
 *   max_hap_len / max_read_len / max_reads_per_window  upper bounds over the batch
 *   n_pairs = pair_off[n_windows] (exact); hap_blob_len >= hap_off[n_haps]; read_blob_len >= read_off[n_reads]
 *   extra_jobs_cap  capacity for candidate DPs beyond one per pair (0 = n_pairs/4 + 4096)
 * The device checks the hints against the batch; errors that the synchronous call returns directly
 * (PLAT_ERR_BAD_INPUT, _HAP_TOO_LONG, ..., plus PLAT_ERR_BAD_HINTS and PLAT_ERR_OVERFLOW when
 * extra_jobs_cap was too small) are returned by the next plat_stream_sync(ctx, stream) instead; outputs of
 * a refused batch are undefined.  Scratch buffers grow on the host as before (hipMalloc may synchronise
 * the first time a larger batch is seen).                                                          */
typedef struct plat_batch_hints {
    int32_t max_hap_len, max_read_len, max_reads_per_window, _pad;
    int64_t n_pairs, hap_blob_len, read_blob_len, extra_jobs_cap;
} plat_batch_hints;

int plat_align_window_batch_async(plat_ctx* ctx, const plat_window_batch* batch, const plat_batch_hints* hints,
                                  int calc_flank_score, int use_mapq_cap, double* out_loglik,
                                  int32_t* out_score, void* stream);

/* ---- a11/a12: DiploidGenotype.calculateDataLikelihood + Population.setup ------------------------
 * Replaces  cdef double DiploidGenotype.calculateDataLikelihood(...)   cgenotype.pxd:14, .pyx:131-189
 *           cdef void   Population.setup(...)  (likelihood part)     cpopulation.pyx:283-309
 * Consumes the array written by plat_align_window_batch.  Individuals: the reads of window w are
 * segmented per individual by seg_read_begin[(w*n_ind + i)] .. [+1] (absolute read indices, must
 * tile win_read_begin) and seg_n_good[w*n_ind+i] = number of `reads` (good) entries
 * (bamReadBuffer.reads.windowEnd - windowStart, cpopulation.pyx:286).
 * Genotypes of a window are all unordered haplotype pairs (i<=j) in the order of
 * generateAllGenotypesFromHaplotypeList (cgenotype.pyx:193-218); G_w = H_w(H_w+1)/2;
 * gl_off[w] = offset of the window's block in units of genotypes*individuals:
 *   out_gl  [gl_off[w] + i*G_w + g]  = Population.genotypeLikelihoods[i][g] (rescaled, max 1.0)
 *   out_logl[same index]             = raw log-likelihood from calculateDataLikelihood
 *   out_gof [gl_off[w] + g*n_ind + i]= Population.goodnessOfFitValues[g][i]
 * Sums run over reads in index order, in fp64, without FMA contraction.                          */
int plat_genotype_window_batch(plat_ctx* ctx, const plat_window_batch* batch, int n_ind,
                               const int32_t* seg_read_begin, const int32_t* seg_n_good,
                               const double* loglik, const int64_t* gl_off,
                               double* out_gl, double* out_logl, double* out_gof, void* stream);

/* ---- what follows the genotype likelihoods in a calling window -----------------
 * All arrays are device pointers.  Windows/haplotypes/genotypes are indexed as in
 * plat_genotype_window_batch: win_hap_begin[n_windows+1]; gl[gl_off[w] + i*G_w + g]; n_reads[w*n_ind+i]
 * = seg_n_good (Population.nReads, cpopulation.pyx:286-287).  max_haps_per_window bounds H_w (LDS size); a window with more haplotypes is REFUSED: its out_iters and its out_call entries are -1, nothing else of it is written, and the next plat_stream_sync on this context returns PLAT_ERR_INVALID (no silent partial result).
 *
 * plat_em_window_batch replaces  cdef void Population.call(maxIters, ...)   cpopulation.pyx:678-703
 *   (EMiteration :384-457, callGenotypes :623-676) for every window:
 *     out_freq[win_hap_begin[w] + h]   = Population.frequencies[h]
 *     out_em  [gl_off[w] + i*G_w + g]  = Population.EMLikelihoods[i][g]  (rows of individuals without
 *                                         reads are zero; the reference leaves stale values there)
 *     out_call[w*n_ind + i]            = index of the called genotype, -1 for "None" (no reads);
 *                                         use_em_likelihoods = --useEMLikelihoods (runner.py:557)
 *     out_iters[w] (optional)          = EM iterations run (max_iters = 100 at variantcaller.pyx:140)
 *
 * plat_variant_posterior_batch replaces  cdef double Population.calculatePosterior(var)  :459-594
 *   for n_vars variants: variant v lives in window var_window[v]; hap_has_var[var_mask_off[v] + h] != 0
 *   iff the variant is one of haplotype h's variants (`var in hap.variants`); prior[v] =
 *   var.calculatePrior(refFile) computed by the caller (variant.pyx:219-259), or 0.5 for flatPrior;
 *   freq = out_freq of the EM.  out_posterior[v] = the rounded phred value the reference returns.
 *
 * plat_genotype_call_batch replaces  cdef tuple computeGenotypeCallAndLikelihoods(...)  vcfutils.pyx:163-334
 *   for n_sites VCF positions x n_ind samples: site s lies in window site_window[s] and holds
 *   site_nvar[s] variants; var_in_hap[site_vih_off[s] + h*nvar + k] = varThisPosInHap[h][k];
 *   is_ref[site_ref_off[s] + h] = haplotypeIsRefAtThisPos[h]; gof as written by
 *   plat_genotype_window_batch ([g][ind]).  Outputs per (s, i), t = s*n_ind + i:
 *     out_phased[2t..]  = (phasedIndex1, phasedIndex2)
 *     out_lik[lik_off[s] + i*NL_s ..], NL_s = (nvar+1)(nvar+2)/2 marginal likelihoods in the
 *                         reference's (index1, index2 <= index1) order
 *     out4[4t..]        = genotype posterior, non-ref posterior, ref posterior, best goodness of fit
 * Sums run in the reference's order in fp64 without FMA contraction.                               */
int plat_em_window_batch(plat_ctx* ctx, int n_windows, int n_ind, int max_haps_per_window,
                         const int32_t* win_hap_begin, const int64_t* gl_off, const int32_t* n_reads,
                         const double* gl, int max_iters, int use_em_likelihoods, double* out_freq,
                         double* out_em, int32_t* out_call, int32_t* out_iters, void* stream);

int plat_variant_posterior_batch(plat_ctx* ctx, int n_vars, int n_ind, int max_haps_per_window,
                                 const int32_t* win_hap_begin, const int64_t* gl_off, const int32_t* n_reads,
                                 const double* gl, const double* freq, const int32_t* var_window,
                                 const int64_t* var_mask_off, const uint8_t* hap_has_var, const double* prior,
                                 double* out_posterior, void* stream);

int plat_genotype_call_batch(plat_ctx* ctx, int n_sites, int n_ind, const int32_t* win_hap_begin,
                             const int64_t* gl_off, const double* gl, const double* gof, const double* freq,
                             const int32_t* site_window, const int32_t* site_nvar, const int64_t* site_vih_off,
                             const int64_t* site_ref_off, const int32_t* var_in_hap, const int32_t* is_ref,
                             const int64_t* lik_off, int32_t* out_phased, double* out_lik, double* out4,
                             void* stream);

/* ---- the HapScore of the INFO field ----------------------------------------------
 * Replaces  cdef int computeHaplotypeScore(list genotypes)                 vcfutils.pyx:1076-1114
 * together with the state it reads: DiploidGenotype.hap1Like / hap2Like, which calculateDataLikelihood resets
 * and refills on every call (cgenotype.pyx:148-161), so that after Population.setup they hold, per haplotype,
 * the sum over the reads of the LAST individual with reads of log10E * likelihood (read order, fp64).
 * Arguments as for plat_genotype_window_batch (loglik = the array written by plat_align_window_batch);
 * max_haps_per_window bounds H_w (LDS size).
 *   out_hap_like[h]  (optional, n_haps) = that sum for haplotype h of the batch
 *   out_hap_score[w] = the value vcfINFO stores as INFO['HapScore'] for every variant of window w          */
int plat_haplotype_score_batch(plat_ctx* ctx, const plat_window_batch* batch, int n_ind, int max_haps_per_window,
                               const int32_t* seg_read_begin, const int32_t* seg_n_good, const double* loglik,
                               double* out_hap_like, int32_t* out_hap_score, void* stream);

/* ---- VariantCandidateGenerator ------------------------------------------------
 * Replaces  VariantCandidateGenerator.addCandidatesFromReads(readStart, readEnd)   variant.pyx:722-743
 *           (getVariantCandidatesFromSingleRead :614-720, getSnpCandidatesFromReadSegment :529-612)
 * for the reads of n_regions regions.  Region g: reference bytes ref_seq[ref_off[g]..ref_off[g+1]) =
 * contig[ref_seq_start[g] ...) (the generator's cached pyRefSeq, region +- 2000, variant.pyx:486-489),
 * contig_len[g] = FastaFile SeqLength (deletions read the contig through getSequence, which clamps to it);
 * read r belongs to region read_region[r]: bases/qualities at read_off[r]..read_off[r+1], read_pos,
 * read_flags (bitFlag: QCFail reads are skipped), CIGAR as (op, length) int16 pairs
 * cigar[2*cig_off[r] .. 2*cig_off[r+1]).  Options: minFlank, minBaseQual, genSNPs, genIndels
 * (runner.py: 10, 20, 1, 1).
 * Output: read r owns records out_rec[5*(r*max_per_read + k)], k < out_count[r], in the reference's
 * emission order: {refPos, nRemoved, nAdded, offset of the removed bases in ref_seq (or -1), offset of
 * the added bases in read_seq (or -1)}.  out_status[r] = 0, PLAT_ERR_OVERFLOW (more than max_per_read;
 * out_count[r] is the number needed) or PLAT_ERR_BAD_INPUT (the read reaches outside the reference
 * window that was handed over).  Merging equal variants (addVariantToList :499-527) is left to the caller. */
typedef struct plat_candidate_batch {
    int32_t n_regions, n_reads;
    const uint8_t* ref_seq;
    const int64_t* ref_off;          /* [n_regions+1] */
    const int32_t* ref_seq_start;    /* [n_regions] */
    const int32_t* contig_len;       /* [n_regions] */
    const uint8_t* read_seq;
    const uint8_t* read_qual;
    const int64_t* read_off;         /* [n_reads+1] */
    const int32_t* read_pos;         /* [n_reads] */
    const int32_t* read_flags;       /* [n_reads] */
    const int16_t* cigar;            /* (op, len) pairs */
    const int32_t* cig_off;          /* [n_reads+1], in pairs */
} plat_candidate_batch;

int plat_candidates_batch(plat_ctx* ctx, const plat_candidate_batch* batch, int min_flank, int min_base_qual,
                          int gen_snps, int gen_indels, int max_per_read, const int32_t* read_region,
                          int32_t* out_rec, int32_t* out_count, int32_t* out_status, void* stream);

/* The dictionary step behind the scan and the per-sample support filter, on the device (one kernel, one workgroup per scan, the scan's
 * dictionary in LDS; the context keeps the first-record ids of every scan's distinct records for plat_stage_b_batch, written in full by every call):
 * Replaces  VariantCandidateGenerator.addVariantToList (variant.pyx:499-527: equal records merge, supporting reads count) and
 *           `computeVariantReadSupportFrac(v, buffer) >= minVarFreq or v.nAdded != v.nRemoved`  (variantcaller.pyx:456-467,
 *           variantFilter.pyx:359-373 over ReadArray.countReadsCoveringRegion, cwindow.pyx:176-206)
 * for n_scans scans (a scan = the `reads` of one sample of one region) of a batch whose records plat_candidates_batch wrote:
 * the reads of scan g are [scan_read_begin[g], scan_read_begin[g+1]) (sorted by position; read_end = cAlignedRead.end),
 * scan_longest[g] = ReadArray.getLengthOfLongestRead().  Output per scan (out_n[2g] counts only when out_n[2g+1] == 0): out_n[2g] candidates that pass, unordered, 8 ints each at
 * out_cand[8*(g*cap_per_scan + i)]: {id of the first record with this content (read index * max_per_read + k: sort by it for
 * the dictionary's order), reads showing it, reads covering its position, then the record's five fields}.  out_n[2g+1] = 0,
 * PLAT_ERR_BAD_INPUT (a read outside its reference window, or "Read start pointer > read end pointer" where the reference raises it: the
 * start pointer walks past the end pointer only over reads whose read_end lies at or before a site they start before -- read positions
 * out of order cannot bring it about by themselves, a read_end inconsistent with its read can),
 * PLAT_ERR_OVERFLOW (more than 6144 distinct records or more than cap_per_scan candidates: merge this scan on the host) or
 * -(2^20 + n) when a read has n > max_per_read records (scan again with room for n).                                        */
int plat_candidates_merge_batch(plat_ctx* ctx, const plat_candidate_batch* batch, const int32_t* read_end, int n_scans,
                                const int32_t* scan_read_begin, const int32_t* scan_longest, int max_per_read,
                                const int32_t* rec, const int32_t* count, const int32_t* status, double min_var_freq,
                                int cap_per_scan, int32_t* out_cand, int32_t* out_n, void* stream);

/* plat_unpack_reads for many pieces in ONE launch: piece k = n packed bytes at src (device memory: uploaded, or resident) expanded to
 * out_seq / out_qual [dst, dst + n).  `pieces` is device memory.  The exceptions of all pieces follow in one pass: exc_index holds byte
 * indices into out_seq / out_qual (ascending not required).                                                                        */
typedef struct plat_unpack_piece { const uint8_t* src; int64_t dst, n; } plat_unpack_piece;
int plat_unpack_reads_pieces(plat_ctx* ctx, int n_pieces, int64_t max_piece_bytes, const plat_unpack_piece* pieces, uint8_t* out_seq, uint8_t* out_qual,
                             int64_t total_bytes, int64_t n_exc, const int64_t* exc_index, const uint8_t* exc_base, const uint8_t* exc_qual, void* stream);

/* The scan on 2-bit base codes (round 6).  A code is (ASCII >> 1) & 3: A 0, C 1, T 2, G 3 (N counts as 3); base i of a blob sits at bits
 * 2 (i & 15) of dword i >> 4.  Equal bytes have equal codes, so the mismatch scan of plat_candidates_batch can compare 32 bases per 64-bit word
 * and look at bytes only where codes differ -- the same records as long as a position with equal codes and different bytes can only be one the
 * reference's loop ignores: true when the reads hold A, C, G, T, N only (THE CALLER'S PROMISE for the read blob; what a PLAT_READS_PACKED
 * table expands to unless an exception carries another byte) and for every reference region without other bytes (found here: the others
 * are scanned byte by byte).
 *   plat_unpack_reads_pieces_codes  = plat_unpack_reads_pieces + out_codes[(total_bytes + 15) / 16 + 8] (zeroed and filled by the call)
 *   plat_ref_codes                  codes of the reference blob (n_bytes = ref_off[n_regions]; out_codes[(n_bytes + 15) / 16 + 8]) and
 *                                   out_irregular[g] = 1 where region g holds a byte other than A, C, G, T, N
 *   plat_candidates_batch_codes     = plat_candidates_batch on them (both code buffers 8-byte aligned)                                       */
int plat_unpack_reads_pieces_codes(plat_ctx* ctx, int n_pieces, int64_t max_piece_bytes, const plat_unpack_piece* pieces, uint8_t* out_seq, uint8_t* out_qual,
                                   uint32_t* out_codes, int64_t total_bytes, int64_t n_exc, const int64_t* exc_index, const uint8_t* exc_base,
                                   const uint8_t* exc_qual, void* stream);
int plat_ref_codes(plat_ctx* ctx, int n_regions, const uint8_t* ref_seq, const int64_t* ref_off, int64_t n_bytes, uint32_t* out_codes,
                   int32_t* out_irregular, void* stream);
int plat_candidates_batch_codes(plat_ctx* ctx, const plat_candidate_batch* batch, const uint32_t* read_codes, const uint32_t* ref_codes,
                                const int32_t* ref_irregular, int min_flank, int min_base_qual, int gen_snps, int gen_indels, int max_per_read,
                                const int32_t* read_region, int32_t* out_rec, int32_t* out_count, int32_t* out_status, void* stream);

/* n pieces of device memory copied into one blob in ONE launch: piece k = n bytes at src -> dst_blob[dst, dst + n) (any alignment).
 * `pieces` is device memory (the struct of plat_unpack_reads_pieces).                                                              */
int plat_copy_pieces(plat_ctx* ctx, int n_pieces, int64_t max_piece_bytes, const plat_unpack_piece* pieces, uint8_t* dst_blob, void* stream);

/* ---- a chunk's read table from read tables that are resident on the device --------------------------------------------------------
 * Replaces  the loader's copy of a bamReadBuffer's reads into the arrays the kernels above take (no reference counterpart: the
 *           reference walks cAlignedRead pointers, cwindow.pyx:485-595).
 * n_tables tables, table t described by desc[t] (device memory): its seven per-read arrays on the device, n reads, and where it goes
 * in the destination: first read index, first byte of its bases in the chunk blob, first CIGAR pair, and the scan id written to
 * dst_region[] for its reads (or -1: none).  Writes dst_off (+ byte base), dst_pos, dst_end, dst_mapq, dst_flags, dst_cig_off (+ pair
 * base), dst_cigar, dst_region and the closing entries dst_off[N] = total_bytes, dst_cig_off[N] = total_pairs, one zero CIGAR pair.    */
typedef struct plat_table_desc {
    const int64_t* off; const int32_t* pos; const int32_t* end; const uint8_t* mapq; const int32_t* flags; const int16_t* cigar; const int32_t* cig_off;
    int32_t n, scan; int64_t first_read, first_byte, first_pair;
} plat_table_desc;
int plat_concat_read_tables(plat_ctx* ctx, int n_tables, int max_reads_per_table, const plat_table_desc* desc, int64_t* dst_off, int32_t* dst_pos,
                            int32_t* dst_end, uint8_t* dst_mapq, int32_t* dst_flags, int32_t* dst_cig_off, int16_t* dst_cigar,
                            int32_t* dst_region, int64_t n_total_reads, int64_t total_bytes, int64_t total_pairs, void* stream);

/* ---- candidates -> variants -> calling windows -> haplotypes -> the window batch, on the device ----------
 * Replaces, for regions with ONE sample, what callVariantsInRegion does between the candidate generator and Population.setup:
 *   sorted(varCandGen.getCandidates())                                             variantcaller.pyx:456-470, variant.pyx:282-363
 *   leftNormaliseIndel(v, refFile, maxReadLength)                                  platypusutils.pyx:806-931
 *   filterVariants(sorted(...), refFile, maxReadLength, minSupport, maxDiff, ...)  variantFilter.pyx:98-171
 *   WindowGenerator.getBunchesOfVariants / WindowsAndVariants                      window.py:49-127,140-238
 *   bamReadBuffer.setWindowPointers                                                cwindow.pyx:176-264,655-689
 *   getFilteredHaplotypes, the `nVars <= log2(maxHaplotypes)` branch: every combination of the window's variants that
 *   isHaplotypeValid accepts                                                       variantFilter.pyx:377-441, platypusutils.pyx:735-802
 *   Haplotype.__init__ / getMutatedSequence (the haplotypes' bytes)                chaplotype.pyx:127-191,397-449
 *   mergeHaplotypes' sorted(haplotypes) (the ORDER; two equal sequences are left to the caller)    variantcaller.pyx:325-383
 * Input: the candidates plat_candidates_merge_batch left on the device (cand / cand_n = its out_cand / out_n, cap_per_scan), the
 * reference windows and the read table the scan saw, and per region g its three read arrays inside that table
 * (tab_begin/tab_n/tab_longest[3g + k], k = 0 reads, 1 badReads, 2 brokenMates; broken_mate_pos[i] = mate position of read
 * tab_begin[3g+2] + i, indexed from broken_base).
 * Output, per region g (all device memory of the caller):
 *   hdr[8g..]   {status, n_variants, n_windows, candidate records, bytes used of the added-bases blob, why (status != 0: 1 capacity /
 *               an exception, 2 dictionary too large to replay, 4 windows, 5 the merge's own verdict, 6 cap_vars / cap_windows / cap_added too
 *               small for this region), dictionaries replayed, 0}; status 0, or
 *               PLAT_SB_HOST: this region needs the caller's own code (more candidates / variants / windows than the capacities, an
 *               indel at the edge of its reference window, an order that depends on a Python dictionary, an exception the reference
 *               would raise, ...) -- nothing else of the region is valid then (its slices of the arrays below may have been written,
 *               inside their capacities; hdr[3], hdr[4], hdr[6], hdr[7] are not).  The reason codes in use:
 *                 1  a pure insertion / deletion at refPos >= 100 whose normalisation window [wmin, wmax) = [max(1, pos - w), min(pos + w,
 *                    contig_len - 1)), w = max(nAdded, nRemoved) + rlen, is not inside the reference window handed over (wmin < ref_seq_start
 *                    or wmax > ref_seq_start + length), or whose tail is empty (cut + nRemoved + 1 >= wmax - wmin, cut = pos - wmin: it ends
 *                    where the contig does); "Error in variant conversion to standard format"; nRemoved >= 2^24 or nAdded >= 2^16
 *                 2  an order that depends on a dictionary (two kept variants with one (refPos, type, nRemoved), or three or more
 *                    candidates with one such key among which one variant occurs twice next to a different one; more than 48 candidates
 *                    with one key count as such) and no records to replay it with (cand_rec or region_name_hash NULL) or more than 5400
 *                    distinct records in the scan
 *                 3  the replayed dictionary does not hold every candidate (a candidate that is no record of the scan: a caller's error)
 *                 5  cand_n[2g + 1] != 0 (the merge's own verdict), more than 1024 candidates, more than cap_per_scan
 *                 6  more variants than cap_vars, more windows than cap_windows (windows wider than maxSize are dropped first and take no
 *                    room), more added bases than cap_added (every insertion that normalisation moved takes its bases, kept or not, then
 *                    every kept variant whose bases still lie in read_seq); 6 wins over 1
 *               (4 is reserved: no path sets it.)
 *   variants    [g*cap_vars + i]: var_pos, var_nrem, var_nadd, var_support (nSupportingReads), var_bam_min, var_bam_max
 *               (bamMinPos / bamMaxPos), var_rem_pos (contig coordinate of the removed bases; not specified when var_nrem is 0), var_add_off (offset of the added
 *               bases in added[g*cap_added ..]); sorted as the reference's list is.
 *   windows     [g*cap_windows + k]: win_start, win_end, win_var_first, win_var_n (its variants = a run of the region's list),
 *               win_flags (PLAT_SBW_*), win_ptrs[6 * ..] = {reads begin, end, badReads begin, end, brokenMates begin, end} (indices
 *               inside the region's arrays), win_n_haps (reference haplotype included), win_batch (index in the window batch or -1).
 * and, for the windows with win_flags == 0, a complete window batch in the arrays of `wb` (the plat_window_batch the likelihood
 * kernels take: windows in (region, window) order, haplotypes sorted by sequence, reads good -> bad -> brokenMates as indices
 * read_src[] into the read table + read_kind[]; read_off from the table's lengths; seg_begin / seg_n_good / gl_off for one sample)
 * plus b_hap_mask[h] = which of its window's variants haplotype h carries (bit i = variant win_var_first + i).
 *   totals[16]  {windows, haplotypes, reads, pairs, genotype likelihoods, haplotype bytes, read bytes, longest haplotype, most reads
 *               of a window, most haplotypes of a window, overflow (a batch capacity was too small: nothing of the batch is valid), ...}
 * No host round trip inside; the caller reads hdr / totals back once. */
#define PLAT_SB_HOST 1
#define PLAT_SBW_SKIP 1          /* no good reads / more than maxReads / more variants than maxVariants with skipDifficultWindows / one haplotype
                                  * left after equal sequences were merged: the loop does not call this window (win_n_haps = 0, not in the batch) */
#define PLAT_SBW_HOST 2          /* the caller prepares this window itself: more variants than maxVariants (filterVariantsByCoverage), more than
                                  * log2(maxHaplotypes - 1) or than 5 (the greedy haplotype filter), a haplotype the reference raises on (longer
                                  * than 16384, beginPos > endPos), "Read start pointer > read end pointer", a window whose haplotypes or variant
                                  * positions reach outside the reference window handed over ([max(start, 0) - flank, min(end, contig_len - 1) +
                                  * flank) clamped to the contig), 2^31 bytes of reads or haplotypes (win_n_haps = 0, not in the batch) */
#define PLAT_SBW_DUPLICATE 4     /* in the batch with EVERY valid combination (order unspecified), but two of its haplotypes have the same sequence and
                                  * an indel / replacement among their variants (or a multi-nucleotide variant with 0 or more than 16 differences), or
                                  * agree on the 384 bytes behind the window's common prefix and go on: mergeHaplotypes / the order is the caller's */
typedef struct plat_stage_b_options {
    int32_t minReads, maxSize, mergeClusteredVariants, maxVarDist, minVarDist, largeWindows, maxVariants, maxHaplotypes;
    int32_t filterVarsByCoverage, skipDifficultWindows;
    double maxReads;
} plat_stage_b_options;
typedef struct plat_stage_b_in {
    int32_t n_regions, cap_per_scan;
    const int32_t* cand; const int32_t* cand_n;
    /* for the replay of the candidate generator's Python-2 dictionaries where an order depends on them: the scan's records (out_rec of
     * plat_candidates_batch) and per region hash(refName) as CPython 2.7 computes it for the contig's name; either NULL: such a region is
     * flagged PLAT_SB_HOST instead.  (The distinct records themselves are read from the context's merge table: call this right behind
     * plat_candidates_merge_batch, on the same context and stream.) */
    const int32_t* cand_rec; const int64_t* region_name_hash;
    const uint8_t* ref_seq; const int64_t* ref_off; const int32_t* ref_seq_start; const int32_t* contig_len;
    const int32_t* region_start; const int32_t* region_end; const int32_t* region_rlen;    /* [n_regions]; rlen: options.rlen as the loop carries it */
    const uint8_t* read_seq; const int64_t* read_off; const int32_t* read_pos; const int32_t* read_end;
    const int32_t* tab_begin; const int32_t* tab_n; const int32_t* tab_longest;            /* [3 * n_regions] */
    const int32_t* broken_mate_pos; int32_t broken_base;
    /* capacities */
    int32_t cap_vars, cap_windows, cap_added;
    int32_t cap_batch_windows, cap_batch_haps, cap_batch_reads; int64_t cap_hap_bytes;
} plat_stage_b_in;
typedef struct plat_stage_b_out {
    int32_t* hdr;
    int32_t* var_pos; int32_t* var_nrem; int32_t* var_nadd; int32_t* var_support; int32_t* var_bam_min; int32_t* var_bam_max;
    int32_t* var_rem_pos; int32_t* var_add_off; uint8_t* added;
    int32_t* win_start; int32_t* win_end; int32_t* win_var_first; int32_t* win_var_n; int32_t* win_flags; int32_t* win_ptrs;
    int32_t* win_n_haps; int32_t* win_batch;
    /* the window batch */
    int32_t* b_hap_begin; int32_t* b_read_begin; int32_t* b_start; int32_t* b_end; int32_t* b_flank;       /* [cap_batch_windows (+1)] */
    int64_t* b_pair_off; int64_t* b_gl_off; int32_t* b_seg_begin; int32_t* b_n_good;                          /* [cap_batch_windows (+1)] */
    int64_t* b_hap_off; uint32_t* b_hap_mask; uint8_t* b_hap_seq;                                            /* [cap_batch_haps + 1], [cap_hap_bytes] */
    int64_t* b_read_off; int32_t* b_read_src; uint8_t* b_read_kind;                                           /* [cap_batch_reads (+1)] */
    int64_t* totals;                                                                                           /* [16] */
    int32_t* scratch;                                                                                          /* [56 * n_regions * cap_windows + 48 * n_regions + 64] */
} plat_stage_b_out;
int plat_stage_b_batch(plat_ctx* ctx, const plat_stage_b_in* batch, const plat_stage_b_options* options,
                       const plat_stage_b_out* out, void* stream);

/* ---- read QC / trimming ----------------------------------------------------------------------------
 * Replaces  cdef int checkAndTrimRead(theRead, theLastRead, ...)   cwindow.pyx:332-481
 * as driven by bamReadBuffer.addReadToBuffer (:560-595) for whole streams of reads: read r's
 * `theLastRead` is read r-1 when stream_of[r-1] == stream_of[r].  read_qual is modified in place (trimmed
 * bases get quality 0), read_flags get BAM_FQCFAIL (512) where the reference sets it.
 *   out_ok[r]      the function's return value (1: goes to `reads`, 0: goes to `badReads`)
 *   out_reason[r]  -1 accepted, else the filteredReadCountsByType slot that was bumped (cwindow.pyx:40-46:
 *                  0 LOW_QUAL_BASES, 1 UNMAPPED_READ, 2 MATE_UNMAPPED, 3 MATE_DISTANT, 4 SMALL_INSERT,
 *                  5 DUPLICATE, 6 LOW_MAP_QUAL) or 7 for a secondary alignment
 * filter_* = 0 switches a filter off (the reference uses a counter value of -1 for that).        */
typedef struct plat_readqc_batch {
    int32_t n_reads, _pad;
    uint8_t* read_qual;              /* raw phred, in/out */
    const int64_t* read_off;         /* [n_reads+1] */
    const int32_t* read_pos;
    const uint8_t* read_mapq;
    int32_t* read_flags;             /* bitFlag, in/out */
    const int16_t* chrom_id;
    const int16_t* mate_chrom_id;
    const int32_t* insert_size;
    const int32_t* mate_pos;
    const int16_t* cigar;            /* (op, len) pairs */
    const int32_t* cig_off;          /* [n_reads+1], in pairs */
    const int32_t* stream_of;        /* [n_reads] id of the read's stream (sample buffer) */
} plat_readqc_batch;

typedef struct plat_readqc_options {
    int32_t min_good_qual_bases, min_map_qual, min_base_qual;           /* minGoodQualBases 20, minMapQual 20, minBaseQual 20 */
    int32_t trim_overlapping, trim_adapter, trim_read_flank, trim_soft_clipped;   /* 1, 1, 0, 1 */
    int32_t filter_mate_unmapped, filter_mate_distant, filter_small_insert, filter_duplicates;
} plat_readqc_options;

int plat_read_qc_batch(plat_ctx* ctx, const plat_readqc_batch* batch, const plat_readqc_options* options,
                       int32_t* out_ok, int32_t* out_reason, void* stream);

/* ---- read buffers from fetched reads ----------------------------------------------------------------
 * Replaces  the loop of loadBAMData over a fetch (platypusutils.pyx:505-541) through bamReadBuffer.addReadToBuffer
 *           (cwindow.pyx:560-595): checkAndTrimRead on every read, then `reads.append` / `badReads.append` and the
 *           isSorted bookkeeping.
 * n_streams streams (one stream = the reads one bamReadBuffer is handed, in fetch order) lie back to back in one read table:
 * stream s = reads [stream_begin[s], stream_begin[s+1]), and qc.stream_of[r] must be the stream of read r.  The call runs
 * plat_read_qc_batch's checkAndTrimRead in place (qc.read_qual trimmed, BAM_FQCFAIL set in qc.read_flags; verdicts in out_ok /
 * out_reason) and then splits every stream, stably, in one pass over its verdicts (wave ballots and prefix sums):
 *   out_perm[stream_begin[s] + k]  the read (index into the table) at place k of the stream's buffers: its accepted reads in
 *                                  fetch order (`reads`), then its rejected reads in fetch order (`badReads`)
 *   out_counts[10*s + ..]          {n_good, unsorted (1: some read's pos is lower than the pos of the read before it -- the
 *                                  reference's isSorted = False), then the 8-slot histogram of out_reason (0..7)}
 * Optional, all or none (`tab.seq` NULL: none): the two buffers of every stream GATHERED into the tables of `tab` -- what
 * plat_read_table's dev_* arrays describe.  Reads go to tab.pos / end / mapq / flags / mate_pos[stream_begin[s] + k] in
 * out_perm's order; their bases and trimmed qualities to tab.seq / tab.qual and CIGAR pairs to tab.cigar at the same places as the
 * stream's input bytes and pairs (qc.read_off[stream_begin[s]], qc.cig_off[stream_begin[s]]), `reads` first.  tab.off / tab.cig_off
 * hold two tables per stream, each starting at 0 and closed by its total: `reads` at [stream_begin[s] + 2s, +n_good+1), `badReads`
 * right behind it, [stream_begin[s] + 2s + n_good + 1, +n_bad+1).  Sizes: off / cig_off n_reads + 2*n_streams, seq / qual the
 * input's bytes + PLAT_BLOB_PAD, cigar 2 * the input's pairs.                                                                  */
typedef struct plat_read_buffers_in {
    plat_readqc_batch qc;            /* the table; qc.read_off / qc.cig_off start at 0 */
    int32_t n_streams, _pad;
    const int32_t* stream_begin;     /* [n_streams+1], stream_begin[0] = 0, stream_begin[n_streams] = qc.n_reads */
    const uint8_t* read_seq;         /* for the gathered tables (NULL without them) */
    const int32_t* read_end;
} plat_read_buffers_in;

typedef struct plat_read_buffers_tables {
    int64_t* off; int32_t* cig_off;
    uint8_t* seq; uint8_t* qual; int16_t* cigar;
    int32_t* pos; int32_t* end; uint8_t* mapq; int32_t* flags; int32_t* mate_pos;
} plat_read_buffers_tables;

int plat_read_buffers_batch(plat_ctx* ctx, const plat_read_buffers_in* in, const plat_readqc_options* options, int32_t* out_ok,
                            int32_t* out_reason, int32_t* out_perm, int32_t* out_counts, const plat_read_buffers_tables* tab /* may be NULL */,
                            void* stream);

/* The same for a table in PLAT_READS_PACKED form (include/platypus_caller.h): one byte per base, bits 0..1 the base and bits 2..7 the
 * quality, plus exceptions (bases other than A/C/G/T, qualities above 63).  No quality array is read or written: qc.read_qual is
 * unused.  The quality of base i is exc_qual[k] when exc_index[k] == i (read as int8_t, as plat_read_qc_batch reads read_qual: a
 * quality >= 128 counts as below min_base_qual), else read_packed[i] >> 2.  checkAndTrimRead's verdicts and trimming are those of
 * plat_read_buffers_batch; a trimmed base keeps its base bits and gets quality bits 0, a trimmed exception exc_qual 0 (both in place).
 * Outputs as plat_read_buffers_batch, with tab.qual unused: tab.seq receives the trimmed packed bytes at the same places.  The
 * exceptions are not gathered: a gathered read's exceptions are those of its input bytes (exc_index, ascending, into read_packed). */
typedef struct plat_read_buffers_packed_in {
    plat_readqc_batch qc;            /* the table; qc.read_qual unused (NULL); qc.read_off / qc.cig_off start at 0 */
    int32_t n_streams, _pad;
    const int32_t* stream_begin;     /* [n_streams+1], as plat_read_buffers_in */
    uint8_t* read_packed;            /* [qc.read_off[n_reads] + PLAT_BLOB_PAD] packed bytes, in/out (trimmed in place) */
    const int32_t* read_end;         /* for the gathered tables (NULL without them) */
    int64_t n_exc;
    const int64_t* exc_index;        /* [n_exc] ascending byte indices into read_packed; the exc_* may be NULL when n_exc == 0 */
    const uint8_t* exc_base;         /* [n_exc] the real letters (not read by the QC) */
    uint8_t* exc_qual;               /* [n_exc] the real qualities, in/out (trimmed in place) */
} plat_read_buffers_packed_in;

int plat_read_buffers_packed_batch(plat_ctx* ctx, const plat_read_buffers_packed_in* in, const plat_readqc_options* options, int32_t* out_ok,
                                   int32_t* out_reason, int32_t* out_perm, int32_t* out_counts,
                                   const plat_read_buffers_tables* tab /* may be NULL; tab.qual unused */, void* stream);

/* ---- read tables from raw BAM alignment records ---------------------------------------------------------
 * Replaces  ReadIterator.get   htslibWrapper.pyx:328-406   (what the loader does with every record sam_itr_next returns: three
 *           mallocs, 4-bit code -> letter, quality bytes copied, CIGAR words unpacked, pos moved over a leading soft clip, bam_endpos)
 * for n_records uncompressed BAM alignment records lying anywhere in one byte blob.  Record i starts at blob[rec_off[i]]; rec_off need
 * not be ascending or gap-free, and nothing is assumed about alignment (the CIGAR words are in general not 4-byte aligned).
 *
 * A record is the alignment block of the SAM/BAM specification section 4.2, little-endian, STARTING AT refID (the 4-byte block_size is
 * not part of it):
 *     0 refID int32 | 4 pos int32 | 8 l_read_name uint8 | 9 mapq uint8 | 10 bin uint16 | 12 n_cigar_op uint16 | 14 flag uint16 |
 *     16 l_seq int32 | 20 next_refID int32 | 24 next_pos int32 | 28 tlen int32 | 32 read_name[l_read_name] |
 *     cigar[n_cigar_op] uint32, each len << 4 | op | seq[(l_seq + 1) / 2], high nibble first | qual[l_seq] | aux data (ignored)
 * Its extent is what its own fields say.  rec_limit (optional, [n_records]): record i must end at or before blob[rec_limit[i]] -- for a
 * blob made of several callers' blobs back to back, where a record must not run into the next one's bytes.
 *
 * Decode rules (get, restated):
 *   seq[i]  = "=ACMGRSVTWYHKDBN"[nibble i] (:363-365, _getBase); qual[i] = the raw byte (:366; get asserts qual <= 93 at :367,
 *             here a larger byte is passed through as it is, as the ASCII fetched path takes it)
 *   cigar   = (op, len) int16 pairs (:373-380)
 *   flags = flag, mapq = mapq, chrom_id = refID, mate_chrom_id = next_refID, mate_pos = next_pos, insert_size = tlen (:393-402)
 *   pos     = the record's pos, minus the length of the FIRST CIGAR operation when that is S (op 4) (:372,386-387,397); a leading H followed
 *             by S does not move it
 *   end     = bam_endpos (:398) of the htslib the reference declares (bit-field bam1_core_t and `int32_t bam_endpos` of
 *             htslibWrapper.pxd:116-183: an htslib 1.x before 1.10): the record's pos + 1 when flag & 4 or n_cigar_op == 0, else
 *             the record's pos + the summed lengths of the operations M, D, N, = and X -- a sum that may be 0: a mapped record whose
 *             CIGAR consumes no reference gets end == its pos.  (htslib from 1.10 on returns pos + 1 there.)  end counts from the
 *             record's own pos, not the soft-clip-adjusted one, and is kept in 32 bits as bam_endpos returns it.
 * Refused (status PLAT_ERR_BAD_INPUT; the record then decodes to an empty read: read_off[i+1] == read_off[i], its per-read fields
 * are not written) -- where get returns NULL (:334-338; loadBAMData, platypusutils.pyx:510-513, dereferences it) or cAlignedRead's
 * `short` fields (htslibWrapper.pxd:187-201) would silently wrap:
 *   a record that runs past the blob or its rec_limit (or rec_off < 0); l_seq <= 0; qual[0] == 0xff; l_seq, a CIGAR length, refID or next_refID above
 *   32767 (refID / next_refID below -32768); n_cigar_op above 32767; a CIGAR op above 8; pos after the soft-clip shift outside int32.
 *
 * Output: a plat_read_buffers_in without further work -- read_off [n+1] (from 0) and cig_off [n+1] by a device-wide scan of the
 * records' lengths, seq / qual [cap_bases + PLAT_BLOB_PAD] (the PLAT_BLOB_PAD bytes behind the last base are zeroed), cigar
 * [2 * cap_pairs], and the per-read arrays [n].  seq and qual must be 16-byte aligned.  The capacities are checked on the device: more
 * bases than cap_bases or more pairs than cap_pairs is status PLAT_ERR_OVERFLOW and no base, quality or pair is written.  A caller
 * can bound them without reading a record: every record has 32 fixed bytes and 1.5 bytes per base, so
 *   bases <= (blob_len - 32 n) * 2 / 3 + n   and   pairs <= (blob_len - 32 n) / 4   (records that do not overlap).
 * status [4] (device, written by the call): {0 or the error, the index of the first offending record (lowest index; for
 * PLAT_ERR_OVERFLOW the first record that does not fit) or -1, total bases, total pairs}.  A record error wins over an overflow.
 * The call enqueues three kernels (per-record parse, scan, expansion: 16 bases per lane, the record's bytes loaded as the aligned
 * words that cover them) and does not wait; errors are reported through status only, nothing traps.                           */
typedef struct plat_bam_decode_out {
    int64_t cap_bases, cap_pairs;
    int64_t* read_off; int32_t* cig_off;
    uint8_t* seq; uint8_t* qual; int16_t* cigar;
    int32_t* pos; int32_t* end; uint8_t* mapq; int32_t* flags;
    int16_t* chrom_id; int16_t* mate_chrom_id; int32_t* insert_size; int32_t* mate_pos;
    int64_t* status;
} plat_bam_decode_out;

int plat_bam_decode_batch(plat_ctx* ctx, int n_records, const uint8_t* blob, int64_t blob_len, const int64_t* rec_off,
                          const int64_t* rec_limit /* may be NULL */, const plat_bam_decode_out* out, void* stream);

/* ---- BGZF blocks inflated on the device ------------------------------------------------------------------
 * Replaces  bgzf_read_block / inflate / crc32  of the loader (what stands between a BAM file's bytes and the records above) for n_blocks
 * BGZF blocks lying anywhere in one byte blob.  blk_off[i] is the offset of block i's first byte (0x1f); blk_limit (optional): block i
 * must end at or before blob[blk_limit[i]].
 *
 * A block is RFC 1952 + SAM specification 4.1: 1f 8b 08, FLG == 4 (FEXTRA and nothing else), MTIME / XFL / OS ignored, XLEN, the extra
 * subfields walked for `BC` with SLEN 2 (BSIZE = block length - 1) wherever it stands among them, the deflate data up to 8 bytes before
 * the block's end, then CRC32 and ISIZE, little-endian.  ISIZE <= 65536; ISIZE 0 (the EOF block) is valid and yields nothing.  Inflate is
 * RFC 1951 in full: stored, fixed and dynamic blocks, several deflate blocks per BGZF block, distances up to 32768 inside the block's
 * own output.  The CRC32 is computed on the device over the inflated bytes.
 *
 * Refused (status PLAT_ERR_BAD_INPUT; a block refused by its header takes no room in the output, one refused later keeps its ISIZE
 * bytes of room and nothing is written there; the other blocks are inflated):
 *   a block that runs past blob_len or its blk_limit (or blk_off < 0); a bad magic or FLG, malformed subfields or none that is BC; BSIZE
 *   too small for header and trailer; ISIZE above 65536; block type 3; a stored LEN / NLEN mismatch; HLIT above 29 or HDIST above 29; an
 *   over-subscribed code-length set or an incomplete one (other than a single one-bit code), no end-of-block code, a repeat code with
 *   nothing to repeat, more code lengths than HLIT + HDIST; a symbol with no code, length symbols 286 / 287, distance symbols 30 / 31;
 *   a distance that reaches before the block's output; input exhausted before the end-of-block symbol of the last deflate block; output
 *   other than exactly ISIZE bytes; a CRC32 mismatch.
 * Every loop is bounded by the block's input bits and ISIZE: no input makes a lane write outside [out_off[i], out_off[i + 1]), read
 * outside its block, or spin.
 *
 * Output: data [cap_bytes + PLAT_BLOB_PAD], 16-byte aligned, the blocks' bytes back to back (the PLAT_BLOB_PAD bytes behind the last
 * one zeroed); out_off [n_blocks + 1] from 0, a device scan of the ISIZEs.  More bytes than cap_bytes is PLAT_ERR_OVERFLOW and no
 * payload byte is written (the blocks are still decoded and CRC-checked in LDS, so that a block error is found).
 * status [4] (device): {0 or the error, the lowest offending block (for PLAT_ERR_OVERFLOW the first that does not fit) or -1, total
 * inflated bytes, 0}.  A block error wins over an overflow.  The call enqueues four kernels (headers, scan, inflate: one wave per block
 * with the block's 64 KiB window in LDS, status) and does not wait; nothing traps.                                              */
typedef struct plat_bgzf_inflate_out {
    int64_t cap_bytes;
    uint8_t* data;
    int64_t* out_off;
    int64_t* status;
} plat_bgzf_inflate_out;

int plat_bgzf_inflate_batch(plat_ctx* ctx, int n_blocks, const uint8_t* blob, int64_t blob_len, const int64_t* blk_off,
                            const int64_t* blk_limit /* may be NULL */, const plat_bgzf_inflate_out* out, void* stream);

/* ---- record text deflated to BGZF blocks on the device ---------------------------------------------------
 * Replaces the gzip stream the reference writes when --output ends in .gz (filez.Open, variantcaller.pyx:951-956) by BGZF: a valid
 * multi-member gzip file whose blocks are independent and concatenate.  The encoder is the inverse of plat_bgzf_inflate_batch above and
 * is written from RFC 1951, RFC 1952 and SAM specification 4.1; csrc/bgzf_deflate.hpp holds the same rule serially and gives the same
 * bytes.
 *
 * Pieces and blocks.  The text is cut into n_pieces pieces, piece i being text[piece_off[i] .. piece_off[i + 1]) -- piece_off ascending
 * from 0, the last at most text_len; a piece is one region's record text.  Each piece is cut into blocks of 0xff00 payload bytes, the
 * last block of a piece possibly shorter.  An empty piece gives no block; a block never spans pieces.
 * A block is the 18-byte header 1f 8b 08 04, MTIME 0, XFL 0, OS ff, XLEN 6, 'B' 'C', SLEN 2, BSIZE = block length - 1; ONE deflate block
 * with BFINAL = 1; CRC32 and ISIZE.  No EOF marker is written: the standard 28-byte empty block is the writer's to append.
 * level 0: a stored deflate block (01, LEN, NLEN, the payload).
 * level 1: LZ77 with one candidate, then fixed Huffman codes (BTYPE 01).  For every position p <= n - 4 of a block of n bytes,
 *   h = (le32 at p * 2654435761u) >> 17 (15 bits); the candidate of p is the nearest q < p with the same h, every position being
 *   inserted, those inside matches included; its length is the common prefix of the bytes at q and at p, capped at min 258, n - p; the
 *   match is valid when the length is at least 4 and p - q at most 32768.  The parse is greedy from p = 0: a valid match emits
 *   length and distance and advances by the length, otherwise a literal is emitted and p advances by 1; positions past n - 4 are literals.
 *   Then end-of-block and zero bits to a byte.  When the deflate data would take n + 5 bytes or more the block is stored instead: a
 *   block is never longer than 18 + 5 + 0xff00 + 8 bytes and BSIZE always fits.
 *
 * Output: data [cap_bytes + PLAT_BLOB_PAD], 16-byte aligned, the blocks back to back in piece order (the PLAT_BLOB_PAD bytes behind
 * the last one zeroed); piece_out_off [n_pieces + 1] from 0: piece i's blocks are data[piece_out_off[i] .. piece_out_off[i + 1]).
 * status [4] (device): {0 or the error, for PLAT_ERR_OVERFLOW the first piece that does not fit, else -1, total compressed bytes,
 * blocks}.  More bytes than cap_bytes is PLAT_ERR_OVERFLOW: no payload byte is written, piece_out_off is clamped to cap_bytes and
 * status[2] still holds the bytes needed, so that a caller can size its buffer and call again; text_len + 31 * blocks always
 * suffices (blocks <= text_len / 0xff00 + n_pieces).  piece_off values that do not ascend from 0 inside text_len are
 * PLAT_ERR_BAD_INPUT in status[0] and nothing is read or written through them.  Invalid arguments (a NULL pointer, a negative count,
 * a level other than 0 or 1, data not 16-byte aligned) return PLAT_ERR_INVALID and nothing is enqueued.
 * The same input gives the same bytes, whatever the order in which lanes and workgroups run.  Four kernels (block plan; one
 * workgroup per block with payload, head table, step table and output words in LDS; a scan of the block sizes; the compaction of the
 * blocks from their slots in scratch memory); the call does not wait and nothing traps.                                          */
typedef struct plat_bgzf_deflate_in {
    const uint8_t* text;
    int64_t text_len;
    int32_t n_pieces, level;
    const int64_t* piece_off;        /* [n_pieces + 1] */
} plat_bgzf_deflate_in;

typedef struct plat_bgzf_deflate_out {
    int64_t cap_bytes;
    uint8_t* data;
    int64_t* piece_out_off;          /* [n_pieces + 1] */
    int64_t* status;                 /* [4] */
} plat_bgzf_deflate_out;

int plat_bgzf_deflate_batch(plat_ctx* ctx, const plat_bgzf_deflate_in* in, const plat_bgzf_deflate_out* out, void* stream);

/* ---- the BAM iterator over inflated blocks -----------------------------------------------------------------
 * Replaces  sam_itr_next  (htslibWrapper.pxd:175-177, htslibWrapper.pyx:312,412; the htslib 1.x before 1.10 the reference declares) for
 * n_streams fetches over the output of plat_bgzf_inflate_batch (data, out_off; n_blocks blocks), without the host knowing an inflated
 * offset.  Stream s is the chunks stream_chunk_begin[s] .. stream_chunk_begin[s + 1] of its index lookup, walked one after the other.
 * Chunk c is the contiguous inflated bytes of blocks chunk_blk_first[c] .. chunk_blk_end[c] - 1; its first block_size word starts
 * chunk_first_uoffset[c] bytes into them; it ends at offset chunk_stop_uoffset[c] of block chunk_stop_blk[c] (a block
 * of the same chunk; -1: at the end of its bytes; never past them).  tid, beg, end [n_streams]: the iterator's
 * window, 0-based half-open.
 *
 * The rule, per chunk, from its first offset on:
 *   stop the chunk at or past its end or the end of its bytes; read block_size (int32); refuse the stream (PLAT_ERR_BAD_INPUT) when
 *   block_size < 32 or the record runs past the chunk's bytes; t = refID, b = pos; when t != tid or b >= end the STREAM ends: the record
 *   is not kept and nothing behind it is read, later chunks included (the iterator's `finished`); else e = b + (n_cigar_op ? the summed
 *   lengths of M, D, N, = and X : 1) -- not bam_endpos: flag 4 plays no part and e may equal b -- and the record is kept when e > beg
 *   (and end > b); either way continue at the next record.  A kept or skipped record whose CIGAR words do not lie inside its
 *   block_size bytes refuses the stream too.  Records may span blocks: a chunk's bytes are contiguous.
 *
 * Output: rec_off / rec_limit [cap_records] for plat_bam_decode_batch (rec_off ascending per stream, pointing at refID past each
 * block_size; rec_limit the record's end), the kept records of all streams back to back; stream_begin [n_streams + 1].  status [4]:
 * {0 or the error, the lowest offending stream (for PLAT_ERR_OVERFLOW the first whose records do not fit cap_records) or -1, kept
 * records, records walked}.  On PLAT_ERR_OVERFLOW stream_begin is clamped to cap_records and nothing is written behind it, while
 * status[2] still counts every kept record: a caller can size its tables from it and call again (inflated bytes / 36 + 1 always
 * suffices).  Three kernels (count, scan, write), one workgroup per stream, the stream staged through LDS; no wait, nothing traps.
 * data must be followed by the PLAT_BLOB_PAD bytes plat_bgzf_inflate_batch zeroes.                                            */
typedef struct plat_bam_find_in {
    int32_t n_streams, n_chunks, n_blocks, _pad;
    const uint8_t* data; const int64_t* out_off;
    const int32_t* stream_chunk_begin;
    const int32_t* chunk_blk_first; const int32_t* chunk_blk_end; const int32_t* chunk_first_uoffset;
    const int32_t* chunk_stop_blk; const int32_t* chunk_stop_uoffset;
    const int32_t* tid; const int32_t* beg; const int32_t* end;
} plat_bam_find_in;

typedef struct plat_bam_find_out {
    int64_t cap_records;
    int64_t* rec_off; int64_t* rec_limit;
    int32_t* stream_begin;
    int64_t* status;
} plat_bam_find_out;

int plat_bam_find_records(plat_ctx* ctx, const plat_bam_find_in* in, const plat_bam_find_out* out, void* stream);

/* ---- records routed to samples by read group ------------------------------------------------------------------
 * Replaces  the second branch of loadBAMData  platypusutils.pyx:573-666  (a BAM file that holds several samples, or a sample spread over
 * several files: every record's rgID from ReadIterator.get(1, &rgID), htslibWrapper.pyx:348-361 -- bam_aux_get(b, "RG"), bam_aux2Z --
 * then buffersBySample[samplesByID[rgID]]) for n_streams fetches whose records (as plat_bam_decode_batch takes them) lie in one blob.
 * Stream s (one fetch of one file) is the records stream_begin[s] .. stream_begin[s + 1] - 1 of rec_off / rec_end; stream_begin[0] = 0,
 * ascending, stream_begin[n_streams] <= n_records (the records behind it belong to no stream and are not looked at: n_records may be
 * the capacity of a plat_bam_find_records whose counts the host has not read).  rec_end[i] (required): the offset of record i's end in
 * the blob, rec_off[i] + its block_size -- the record's own fields do not say where its aux data stops.
 *
 * The rule (the loader's, restated over the aux layout of the SAM/BAM specification section 4.2.4; the reference tree holds only the
 * htslib declarations, htslibWrapper.pxd:172-173):
 *   extent  the aux area runs from 32 + l_read_name + 4 n_cigar_op + (l_seq + 1) / 2 + l_seq (l_seq as an unsigned word) to the end
 *   walk    from its start, while at least 3 bytes are left: a 2-byte tag, a 1-byte type, then the value --
 *             A c C 1 byte | s S 2 bytes | i I f 4 bytes | d 8 bytes | Z H the bytes through the first NUL |
 *             B 1 subtype byte of cCsSiIf, an int32 count, count x size bytes
 *           the FIRST field whose tag is RG decides; later RG fields are not looked at
 *   value   the RG field must have type Z or H; its value is the bytes up to the NUL
 *   sample  group_sample[g] of the group g whose ID equals the value byte for byte (an ID that is a prefix of another is a
 *           different ID); of equal IDs the lowest g counts
 * Refused (PLAT_ERR_BAD_INPUT; where the reference dereferences NULL or raises KeyError) -- out->why names the rule for the lowest such
 * record: PLAT_ROUTE_NO_RG (no RG field), _RG_NOT_STRING (RG of another type), _NOT_IN_TABLE, _UNKNOWN_TYPE (a field's type or a B
 * subtype), _NEGATIVE_COUNT (of a B array), _AUX_OVERRUN (a field, a string's NUL or an array runs past the record's end),
 * _FIXED_OVERRUN (the fixed part already does, or rec_off / rec_end lie outside the blob).  A refused record is left out of the output;
 * the others are still routed.  Every loop is bounded by the record's end: no input makes a lane read outside [rec_off, rec_end) or spin.
 *
 * The group table: n_groups IDs, their bytes back to back in group_ids with group_off [n_groups + 1] (from 0), and group_sample
 * [n_groups] in 0 .. n_samples - 1.  Limits: n_groups <= PLAT_ROUTE_MAX_GROUPS and n_samples <= PLAT_ROUTE_MAX_SAMPLES, else
 * PLAT_ERR_UNSUPPORTED is returned and nothing is enqueued.  An ID may have any length: the table of (hash, group) pairs always lies in
 * LDS; the IDs' bytes lie there too while they hold at most PLAT_ROUTE_LDS_ID_BYTES in all, and are compared where they lie in device
 * memory beyond that.  n_streams * n_samples must stay below 2^31 (PLAT_ERR_OVERFLOW).
 *
 * Output: rec_off / rec_limit [n_records] for plat_bam_decode_batch -- stream s's records as sample 0's, then sample 1's, ..., each in
 * input order (a stable partition; stream s of sample m becomes the records out_begin[s * n_samples + m] .. out_begin[s * n_samples +
 * m + 1] - 1), all streams back to back without gaps; out_begin [n_streams * n_samples + 1]; rec_sample [n_records], -1 for a refused
 * record; status [4] {0 or the error, the lowest offending record or -1, records routed, records refused}; why [1] (may be NULL).  An
 * out-of-range group_sample or group_off, or a stream_begin that is no such partition, is status PLAT_ERR_INVALID {-1, -1, 0, 0} and
 * nothing else is written.  The call enqueues six kernels (checks and tile plan, tag: one lane per record; per-tile sample histogram;
 * scan over tiles; scan over streams and samples; placing), keeps its tile counts in the context's scratch, and does not wait; nothing
 * traps.                                                                                                                          */
#define PLAT_ROUTE_MAX_GROUPS 2048
#define PLAT_ROUTE_MAX_SAMPLES 256
#define PLAT_ROUTE_LDS_ID_BYTES 24576
#define PLAT_ROUTE_NO_RG 1
#define PLAT_ROUTE_RG_NOT_STRING 2
#define PLAT_ROUTE_NOT_IN_TABLE 3
#define PLAT_ROUTE_UNKNOWN_TYPE 4
#define PLAT_ROUTE_NEGATIVE_COUNT 5
#define PLAT_ROUTE_AUX_OVERRUN 6
#define PLAT_ROUTE_FIXED_OVERRUN 7

typedef struct plat_bam_route_in {
    int32_t n_records, n_streams, n_groups, n_samples;
    const uint8_t* blob; int64_t blob_len;
    const int64_t* rec_off; const int64_t* rec_end;
    const int32_t* stream_begin;
    const uint8_t* group_ids; const int32_t* group_off; const int32_t* group_sample;
} plat_bam_route_in;

typedef struct plat_bam_route_out {
    int64_t* rec_off; int64_t* rec_limit;
    int32_t* out_begin;
    int32_t* rec_sample;
    int64_t* status;
    int32_t* why;
} plat_bam_route_out;

int plat_bam_route_batch(plat_ctx* ctx, const plat_bam_route_in* in, const plat_bam_route_out* out, void* stream);

/* ---- broken mates: the mates of improper pairs ------------------------------------------------------------------
 * Replaces  the two record loops of loadBAMData's broken-mate fetch  platypusutils.pyx:522-533 / :617-627 (which kept record gives a
 * mate coordinate) and :555-559 / :646-654 (which record of a second-round fetch is a broken mate), over the output of
 * plat_bam_find_records: data (data_len bytes + PLAT_BLOB_PAD), rec_off / rec_limit, stream_begin [n_streams + 1] on the device.
 * n_records bounds stream_begin[n_streams] (it may be the find's capacity: the host need not have read a count).  csrc/mate_rule.hpp
 * holds the rule for host and device.  Fixed fields count from a record's refID and lie at any alignment: flag uint16 at 14, next_refID
 * (mtid) int32 at 20, next_pos (mpos) int32 at 24.
 *
 * PLAT_MATES_COORDS  a record gives (mtid, mpos) when (!(flag & 0x2) || (flag & 0x4) || (flag & 0x8)) && mtid != -1.  Output: coords
 *     [2 * cap_records], the pairs of stream after stream in record order, back to back; coord_begin [n_streams + 1].  A negative mpos is
 *     written as it is (the host refuses it).  want_tid / lo / hi are not read.
 * PLAT_MATES_FETCH   a record of stream s is a broken mate when mtid == want_tid[s] && lo[s] <= mpos <= hi[s] (loadBAMData's chromID,
 *     start and end, both ends inclusive).  Output: out_data [cap_bytes + PLAT_BLOB_PAD], 16-byte aligned: the kept records' bytes from
 *     refID through rec_limit back to back, PLAT_BLOB_PAD zero bytes behind the last; out_rec_off / out_rec_len / out_mpos [cap_records];
 *     out_begin [n_streams + 1].  A record two streams return is copied twice.
 *
 * status [4] (device): {0 or the error, the lowest offending stream or -1, records kept, records looked at}; need_bytes [1] (may be
 * NULL): the bytes all kept records take.  More kept records than cap_records, or more bytes than cap_bytes, is PLAT_ERR_OVERFLOW
 * naming the lowest stream with a record that does not fit: nothing is written behind a capacity (no pad either), coord_begin /
 * out_begin are clamped to cap_records, status[2] and need_bytes still hold the full counts, and the caller can size its buffers and
 * call again (n_records and data_len always suffice).  A record with rec_off < 0, rec_limit > data_len, or fewer than 32 bytes
 * (or more than 2^31 - 1) refuses its stream (PLAT_ERR_BAD_INPUT, which wins over an overflow): that record is left out, the other
 * streams are not touched by it.  A stream_begin that is no partition of [0, n_records] from 0 is status {PLAT_ERR_INVALID, -1, 0, 0}
 * and every begin 0.  Invalid arguments (a NULL pointer, a negative count, an unknown mode, out_data not 16-byte aligned) return
 * PLAT_ERR_INVALID and nothing is enqueued.
 * Three kernels (count: a lane per record, a workgroup per 256 records; scan: one workgroup over the tiles' sums; write: the slots by a
 * workgroup scan, the copy a wave per record with aligned 16-byte stores), the tile sums in the context's scratch; no wait, nothing
 * traps.                                                                                                                          */
#define PLAT_MATES_COORDS 0
#define PLAT_MATES_FETCH 1

typedef struct plat_bam_mates_in {
    int32_t n_streams, n_records, mode, _pad;
    const uint8_t* data; int64_t data_len;
    const int64_t* rec_off; const int64_t* rec_limit;
    const int32_t* stream_begin;
    const int32_t* want_tid; const int32_t* lo; const int32_t* hi;       /* [n_streams], PLAT_MATES_FETCH */
} plat_bam_mates_in;

typedef struct plat_bam_mates_out {
    int64_t cap_records, cap_bytes;
    int32_t* coords; int32_t* coord_begin;                               /* PLAT_MATES_COORDS */
    uint8_t* out_data; int64_t* out_rec_off; int32_t* out_rec_len; int32_t* out_mpos; int32_t* out_begin;       /* PLAT_MATES_FETCH */
    int64_t* status;
    int64_t* need_bytes;
} plat_bam_mates_out;

int plat_bam_mates_batch(plat_ctx* ctx, const plat_bam_mates_in* in, const plat_bam_mates_out* out, void* stream);

/* ---- candidate alleles from source VCF lines ---------------------------------------------------------------------
 * Replaces  VariantCandidateReader.Variants   src/python/variantutils.py:72-159   (the loop over the lines a tabix fetch returned: ALT
 *           split at commas, the size test, SNP / MNP / indel trimming) with  isValidVcfLine  :168-197  and the tabix proxy's
 *           pos = atoi(POS) - 1 (TabProxies.pyx:608)
 * for n_regions fetches whose text lines lie in one byte blob, as the fetches returned them: region k's lines are
 * text[text_off[k] .. text_off[k + 1]), every line ended by '\n' (the last line of a region may lack it); where a region has several
 * source files, their fetches back to back in file order.  text must be 16-byte aligned and followed by PLAT_BLOB_PAD readable bytes;
 * text_len < 2^31 - 1024.  name_hash [n_regions]: the Python-2 string hash of the region's chromosome, as plat_stage_b_in.region_name_hash.
 * The set() and sorted() of :161 are the caller's (they need every allele of the region at once and only the alleles).
 *
 * The rule, per line:
 *   skipped   an empty line, or one that starts with '#'.  A fetch never returns either; they are counted and otherwise ignored (by
 *             design: the reference would try to parse them)
 *   columns   split at tabs; CHROM, POS, ID, REF and ALT are looked at and NOTHING behind the tab or newline that ends ALT is read
 *   refused   (status PLAT_ERR_BAD_INPUT; the line yields nothing, the other lines and regions are parsed) -- where pysam raises or atoi
 *             is undefined: fewer than five columns; a POS that is not 1 to 10 decimal digits, or above 2^31 - 1; POS - 1 + len(REF)
 *             above 2^31 - 1 (a trimmed position would leave Variant's C int)
 *   pos       = POS - 1; a line with pos < 0 is invalid
 *   invalid   (isValidVcfLine: the line yields nothing, no error) REF holds a byte other than A C G T N (upper case), or any element
 *             of ALT.split(",") does: '.', '*', '<DEL>' and lower case are invalid; an EMPTY element is valid
 *   per ALT element, in order (lenRef, lenAlt: bytes of REF and of the element; an empty REF or element has length 0, as Python slices):
 *             |lenAlt - lenRef| > maxSize: skipped, counted
 *             lenRef == lenAlt == 1: (pos, REF, alt), also when they are equal
 *             lenRef == lenAlt otherwise: equal leading bases trimmed (pos advances), then equal trailing bases; what is left is emitted
 *               even when both are empty
 *             otherwise, longHaps == 1: (pos, REF, alt) untrimmed
 *             otherwise: the first base of both dropped WITHOUT comparing them (pos stays), then equal leading bases trimmed (pos
 *               advances); no trailing trim
 * Every loop is bounded by the end of the line's region: no input makes a lane read outside [text_off[k], text_off[k + 1]) -- apart from
 * the aligned 16-byte words that cover the text, inside text_len + PLAT_BLOB_PAD -- or spin.
 *
 * Output, alleles in input order (line ascending, then ALT element ascending), the regions back to back: region_begin [n_regions + 1];
 * per allele pos, rem_off / n_rem and add_off / n_add (OFFSETS INTO text: a trimmed allele is a substring of its line's REF or ALT, no
 * byte goes out), hash (py2_variant_hash of (name_hash, pos, removed, added) narrowed to 32 bits: what the set of :161 probes with) and
 * line (the line's index within its region, skipped lines counted); region_stats [4 * n_regions]: {lines, skipped, invalid, ALT
 * elements over maxSize}; status [4] (device): {0 or the error, the lowest refused (region << 32 | line) or -1, alleles, lines}.  More
 * alleles than cap_variants is PLAT_ERR_OVERFLOW: nothing is written behind the capacity, region_begin is clamped to it, and status[2]
 * still counts every allele, so that a caller can size its arrays and call again.  A refused line wins over an overflow.  A text_off
 * that does not ascend inside [0, text_len] is status {PLAT_ERR_INVALID, -1, 0, 0} and nothing else is written.
 * The call enqueues seven kernels -- checks; line starts marked from aligned 16-byte loads, one wave per 1024 bytes; scan; the regions'
 * first lines; one lane per line: columns, verdict, allele count; scan; one lane per line: alleles written -- keeps its marks (an
 * eighth of the text) and per-tile counts in the context's scratch, and does not wait; nothing traps.                             */
typedef struct plat_source_variants_in {
    int32_t n_regions, maxSize, longHaps, _pad;
    const uint8_t* text; int64_t text_len;
    const int64_t* text_off; const int64_t* name_hash;
} plat_source_variants_in;

typedef struct plat_source_variants_out {
    int64_t cap_variants;
    int32_t* region_begin;
    int32_t* pos; int64_t* rem_off; int32_t* n_rem; int64_t* add_off; int32_t* n_add; int32_t* hash; int32_t* line;
    int32_t* region_stats;
    int64_t* status;
} plat_source_variants_out;

int plat_source_variants_batch(plat_ctx* ctx, const plat_source_variants_in* in, const plat_source_variants_out* out, void* stream);

/* ---- tabix's iterator over inflated blocks -------------------------------------------------------------------------
 * Replaces  ti_iter_read  (src/tabix/index.c.pysam.c:872-911) with ti_readline (:86-120), ti_get_intv's VCF preset (:161-225) and
 *           get_intv (:227-241), as variantutils.py:67 reaches them: vcfFile.fetch(chrom, start, end) = ti_queryi(tid, start, end)
 * for n_streams fetches over the output of plat_bgzf_inflate_batch (data, out_off; n_blocks blocks; data_len: the room data has, the
 * inflate's cap_bytes, out_off[n_blocks] at most), without the host seeing an inflated byte.  The chunk geometry is plat_bam_find_in's:
 * stream s is the chunks stream_chunk_begin[s] .. stream_chunk_begin[s + 1] - 1 of its index lookup (stream_chunk_begin runs from 0 to
 * n_chunks); chunk c is the contiguous inflated bytes of blocks chunk_blk_first[c] .. chunk_blk_end[c] - 1, its first line starts
 * chunk_first_uoffset[c] bytes into them, it ends at offset chunk_stop_uoffset[c] of block chunk_stop_blk[c] (-1: at the end of its
 * bytes; an end outside them is clamped to them).  The chunks' blocks ascend: chunk_blk_first[c] >= chunk_blk_end[c - 1].  Stream s
 * queries the sequence whose name is names[name_off[s] .. name_off[s + 1]) (what the index holds for the tid) over [beg[s], end[s]),
 * 0-based half-open.
 *
 * The rule, per stream, chunk by chunk, p starting at the chunk's first offset:
 *   chunk end  when p is at or past the chunk's end E: the last chunk ends the stream; otherwise p > E refuses the stream
 *              (PLAT_ERR_BAD_INPUT: the reference asserts curr_off == off[i].v) and p == E continues at the next chunk's first offset
 *   line       the bytes from p up to the next '\n' in the chunk's bytes, or up to their end; p moves behind the '\n'.  A line may
 *              span blocks and may end behind E
 *   meta       a line whose first byte is '#' is passed over (it counts as walked)
 *   columns    split at '\t' and at a NUL byte.  v = strtol(column 2, base 0): leading C white space (a tab is some: an empty column
 *              2 reads the next one, as the reference's strtol does), an optional sign, 0x / 0X hex, a leading 0 octal, else decimal,
 *              up to the first byte that is no digit of the base; no digits gives 0.  b = max(v - 1, 0), e = max(v, 1); column 4, when
 *              it exists and is not empty: e = b + its length; column 8, when it exists: if it starts with END= e is the number behind
 *              it (the same strtol, inside the column), else if END= occurs in it e is the number behind its first ;END= (none: e
 *              stays).  Nothing behind the tab that ends column 8 is parsed
 *   refused    v or e outside +-(2^31 - 1) refuses the stream (the reference narrows a long to int32 there)
 *   stop       fewer than two columns (an empty line too), e < 0, column 1 differing from the stream's name in any byte or in length,
 *              or b >= end: the STREAM ends, the line is not kept and nothing behind it is read, later chunks included
 *   kept       otherwise the line is kept when e > beg and end > b; either way the walk goes on
 * Every loop is bounded by the line's end, and that by the chunk's bytes: no input makes a lane read outside its chunk -- apart from the
 * aligned 16-byte words that cover the data, inside data_len + PLAT_BLOB_PAD -- or spin.
 *
 * Output: text [cap_text + PLAT_BLOB_PAD], 16-byte aligned: every kept line's bytes (a '\r' stays) followed by one '\n', the streams
 * back to back in order -- the form plat_source_variants_batch takes -- and PLAT_BLOB_PAD zero bytes behind them; stream_text_off
 * [n_streams + 1]; stream_counts [2 * n_streams]: lines walked (those ahead of the stop or refusal) and lines kept; status [4]
 * (device): {0 or the error, the lowest refused stream or -1, kept lines, kept bytes}.  A refused stream yields no text and keeps no
 * line; the other streams are not touched by it.  More than cap_text bytes is PLAT_ERR_OVERFLOW: nothing is written behind the
 * capacity, stream_text_off is clamped to it and status[3] still holds the full size (inflated bytes + n_chunks always suffices).  A
 * refusal wins over an overflow.  Geometry that breaks the above is status {PLAT_ERR_INVALID, -1, 0, 0} and nothing else is written.
 * The call enqueues seven kernels -- checks; newlines and line starts marked from aligned 16-byte loads, one wave per 1024 bytes; scan;
 * one lane per line: its end (the r-th newline, by rank and select over the marks: no lane walks a line), columns 1 to 8, the verdict,
 * the stream's first stop as an atomic minimum in chunk order; the lines ahead of it counted; scan; the kept lines copied wave-wide,
 * 16 bytes per lane -- keeps its marks (a quarter of the data) and per-tile counts in the context's scratch, and does not wait;
 * nothing traps.                                                                                                                   */
typedef struct plat_tabix_fetch_in {
    int32_t n_streams, n_chunks, n_blocks, _pad;
    const uint8_t* data; int64_t data_len; const int64_t* out_off;
    const int32_t* stream_chunk_begin;
    const int32_t* chunk_blk_first; const int32_t* chunk_blk_end; const int32_t* chunk_first_uoffset;
    const int32_t* chunk_stop_blk; const int32_t* chunk_stop_uoffset;
    const uint8_t* names; const int32_t* name_off;
    const int32_t* beg; const int32_t* end;
} plat_tabix_fetch_in;

typedef struct plat_tabix_fetch_out {
    int64_t cap_text;
    uint8_t* text;
    int64_t* stream_text_off;
    int64_t* stream_counts;
    int64_t* status;
} plat_tabix_fetch_out;

int plat_tabix_fetch_batch(plat_ctx* ctx, const plat_tabix_fetch_in* in, const plat_tabix_fetch_out* out, void* stream);

/* ---- the tabix index of a bgzipped VCF ------------------------------------------------------------------------------
 * Replaces  ti_index_core  with ti_conf_vcf (src/tabix/index.c.pysam.c:320-393) over ti_readline (:86-120), get_intv (:227-241),
 *           insert_offset2 (:266-286) and bgzf_tell -- what `tabix -p vcf` reads of the file -- for the .gz output the caller writes
 * over the output of plat_bgzf_inflate_batch for the WHOLE file: data (data_len: the room it has, out_off[n_blocks] at most) and
 * out_off [n_blocks + 1], plus blk_addr [n_blocks + 1]: the file address of every block, the last entry the address behind the last block
 * that holds data.  out_off ascends from 0 in steps of at most 65536 and blk_addr ascends inside [0, 2^47); anything else is status
 * {PLAT_ERR_INVALID, -1, 0 ...} and nothing else is written.  csrc/tabix_index.hpp holds the same rule serially (the host twin) and
 * the finishing stage that turns what this call leaves into the .tbi's bytes.
 *
 * The rule:
 *   lines      a line runs to its '\n' or to the end of the data (a last line without a newline counts); '\r' is an ordinary byte; a line
 *              whose first byte is '#' is no record wherever it stands.  Lines are numbered from 1, '#' lines included
 *   offsets    the virtual offset of a line that starts at inflated offset t is blk_addr[b] << 16 | (t - out_off[b]), b the last block
 *              with out_off[b] <= t: a line behind a newline on a block's last byte sits at offset 0 of the next block.  The end of the
 *              file is blk_addr[n_blocks] << 16
 *   record     columns split at '\t' and at a NUL byte, as plat_tabix_fetch_batch above reads them: the name is column 1;
 *              v = strtol(column 2, base 0), beg = max(v - 1, 0), end = max(v, 1); a non-empty column 4 gives end = beg + its length; in
 *              column 8, END= at its start gives end = the number behind it, otherwise, when END= occurs at all, the first ;END= does.
 *              bin = ti_reg2bin(beg, end) in unsigned 32-bit arithmetic; the linear windows are beg >> 14 .. (end - 1) >> 14 in signed
 *              arithmetic.  END=0 and an END below POS give odd but defined bins and empty window ranges, as in the reference
 *   refused    where the reference exits -- a line of fewer than two columns, an empty one included (kind 1); end < 0 (kind 3); a beg below
 *              that of the record in front of it on one contig (kind 4); a contig name that was seen before another one (kind 5) -- and
 *              a v or an END outside +-(2^31 - 1), which the reference narrows to int32 (kind 2).  The verdict is that of the lowest such
 *              line; where two kinds hold of it, the lower kind
 *   contigs    names are compared byte by byte over their whole length (a name that is a prefix of another is another name); tid in order
 *              of first appearance.  Every contig's name is compared with every earlier one's (by a 64-bit hash and the length first), so a
 *              file holds at most 65536 contigs: more is status PLAT_ERR_UNSUPPORTED
 *   runs       a maximal stretch of consecutive records of one contig with one bin (a change of contig ends it even when the bin number
 *              repeats); u is the offset of its first record
 *   windows    per contig n = the largest (end - 1 >> 14) + 1 (0 at least) windows; window w holds the offset of the first record in file
 *              order whose range holds w, offset 0 counting as unset, and 0 where none does
 *
 * Output (device): the runs in file order run_tid / run_bin / run_u [cap_runs]; name_off / name_len [cap_names]: each contig's name as
 * offset and length into data, and name_bytes [cap_name_bytes]: the names' bytes back to back in tid order; lin_first [cap_names + 1] and lin [cap_windows]: contig t's windows are lin[lin_first[t] .. lin_first[t + 1]);
 * status [PLAT_TBI_STATUS_WORDS]: {0 or the error, the lowest offending line or -1, its kind, records, runs, contigs, windows, the end
 * offset, 1 when the first record sits at offset 0 and then its first and last window (the finishing stage zeroes those), lines, the names' bytes}.
 * More runs, contigs, name bytes or windows than the capacities is PLAT_ERR_OVERFLOW: nothing is written behind a capacity (runs and names up to
 * it, name bytes and windows not at all), the status holds the full counts and the caller calls again.  A refusal wins over PLAT_ERR_UNSUPPORTED and
 * that over an overflow; of a refused file only the status is defined.
 * Every loop is bounded by its line's end, the name's length, 64 words of a tile, the logarithm of a table, 65536 / 64 contigs per lane
 * or the 2^17 windows a 32-bit END spans; every offset is derived from the checked out_off.  No lane walks a contig or the file.
 * Eleven kernels (csrc/plat_tbxindex.hip names them), the marks in the scratch of plat_tabix_fetch_batch (one of the two calls at a
 * time per context); the call does not wait and nothing traps.                                                                      */
#define PLAT_TBI_STATUS_WORDS 13
#define PLAT_TBI_MAX_REF 65536
typedef struct plat_tabix_index_in {
    int32_t n_blocks, _pad;
    const uint8_t* data; int64_t data_len;
    const int64_t* out_off;          /* [n_blocks + 1] */
    const int64_t* blk_addr;         /* [n_blocks + 1] */
} plat_tabix_index_in;

typedef struct plat_tabix_index_out {
    int64_t cap_runs, cap_names, cap_windows, cap_name_bytes;
    int32_t* run_tid; int32_t* run_bin; int64_t* run_u;
    int64_t* name_off; int32_t* name_len; uint8_t* name_bytes;
    int64_t* lin_first; int64_t* lin;
    int64_t* status;                 /* [PLAT_TBI_STATUS_WORDS] */
} plat_tabix_index_out;

int plat_tabix_index_batch(plat_ctx* ctx, const plat_tabix_index_in* in, const plat_tabix_index_out* out, void* stream);

/* ---- region queries over a tabix or BAM index ---------------------------------------------------------------------------
 * Replaces  ti_iter_query  (src/tabix/index.c.pysam.c:799-870) over reg2bins (:776-789) -- the chunk list `fetch(chrom, start, end)`
 * reads -- for n_queries x (tid, beg, end) against ONE index in one call.  A BAM index (.bai) has the same bins, linear index and
 * rule, so the call serves both.  The index comes as flat tables that are resident on the device (csrc/index_query.hpp makes them of
 * the .tbi's or .bai's bytes on the host, once per file: the format is serial, every count moves what follows it):
 *   ref_bin_first [n_ref + 1] into bin_id [n_bins], bin ids ascending within a reference (the metadata pseudo-bin 37450 left out);
 *   bin_chunk_first [n_bins + 1] into chunk_u / chunk_v [n_chunks], a bin's chunks in file order;
 *   ref_lin_first [n_ref + 1] into lin_fill [n_lin]: the linear index with every zero entry replaced by the last non-zero one below it
 *   (0 where there is none) -- the reference's backward scan for indexes written before tabix 0.1.4, done once.
 * Offsets that do not ascend inside their tables from 0 to the tables' sizes, a bin id outside [0, 37450), ids that do not ascend within
 * a reference, or a query whose tid lies outside [0, n_ref) is status {PLAT_ERR_INVALID, the lowest such query or -1, 0 ...} and
 * nothing else is written.
 *
 * The rule, per query:
 *   window     beg = max(beg, 0).  end < beg: no iterator, count -1.  beg == end: an iterator without chunks, count 0
 *   bins       reg2bins(beg, end): end clamped to 2^29, then end - 1 used; bin 0 and, for the shifts 26, 23, 20, 17, 14, the bins
 *              first + (beg >> shift) .. first + (end - 1 >> shift), first = 1, 9, 73, 585, 4681.  The bins of a level range that the
 *              reference holds are consecutive in bin_id: a lower bound for the range's first bin, another for the bin behind its last
 *   min_off    lin_fill[min(beg >> 14, n - 1)] of the reference's n linear entries; 0 when it has none
 *   gathered   every chunk of every listed bin with v > min_off, strictly; virtual offsets compare as unsigned 64-bit numbers
 *   sorted     by (u, v) ascending (the reference's introsort leaves ties in u open; a valid index has none: u is a record's offset)
 *   resolved   chunk i goes when v[i] <= the largest v in front of it; then v[i] = min(v[i], u[i + 1]); then chunk i opens an output chunk
 *              exactly when v[i - 1] >> 16 != u[i] >> 16, and an output chunk ends at the v of the last member of its run.  These are the
 *              reference's three loops; with M[i] the largest v in front of i they are one scan: i opens an output chunk when i = 0 or
 *              v[i] > M[i] and M[i] >> 16 < u[i] >> 16, the output chunk in front of it ends at M[i], the last at the largest v of all
 *   limit      a query that gathers more than PLAT_IDXQ_MAX_CHUNKS chunks is HANDED OVER: count -2, no chunks; this is no error -- the
 *              caller answers it with the host twin (csrc/index_query.hpp, query)
 *
 * Output (device): count [n_queries] (the output chunks, -1, -2), gathered [n_queries] (0 for count -1), q_first [n_queries + 1] from 0
 * (a query with a negative count takes no room), out_u / out_v [cap_chunks]: query q's chunks at q_first[q] .. q_first[q + 1];
 * status [PLAT_IDXQ_STATUS_WORDS]: {0 or the error, the lowest query with a bad tid or -1, output chunks, gathered chunks, queries handed
 * over, queries without an iterator}.  More output chunks than cap_chunks is PLAT_ERR_OVERFLOW: count, gathered, q_first and the status
 * hold the full counts, no chunk is written, and the caller calls again.
 * Every loop is bounded by the chunks of one level range's bins, the logarithm of a table, or PLAT_IDXQ_MAX_CHUNKS; a whole-contig
 * query makes six pairs of searches, not 37449 probes.  One wave per query (up to 64 gathered chunks: sorted in registers), one workgroup
 * per query above that (32 KiB of LDS).  Seven kernels (csrc/plat_idxquery.hip names them), two words and the list of workgroup queries in
 * the scratch of plat_tabix_fetch_batch (one of these calls at a time per context); the call does not wait and nothing traps.           */
#define PLAT_IDXQ_STATUS_WORDS 6
#define PLAT_IDXQ_MAX_CHUNKS 2048
#define PLAT_IDXQ_NO_ITERATOR (-1)
#define PLAT_IDXQ_HANDED_OVER (-2)
typedef struct plat_index_query_in {
    int32_t n_ref, n_queries;
    int64_t n_bins, n_chunks, n_lin;
    const int64_t* ref_bin_first;    /* [n_ref + 1] */
    const int32_t* bin_id;           /* [n_bins] */
    const int64_t* bin_chunk_first;  /* [n_bins + 1] */
    const int64_t* chunk_u; const int64_t* chunk_v;      /* [n_chunks] */
    const int64_t* ref_lin_first;    /* [n_ref + 1] */
    const int64_t* lin_fill;         /* [n_lin] */
    const int32_t* tid; const int32_t* beg; const int32_t* end;      /* [n_queries] */
} plat_index_query_in;

typedef struct plat_index_query_out {
    int64_t cap_chunks;
    int32_t* count; int32_t* gathered;                   /* [n_queries] */
    int64_t* q_first;                /* [n_queries + 1] */
    int64_t* out_u; int64_t* out_v;  /* [cap_chunks] */
    int64_t* status;                 /* [PLAT_IDXQ_STATUS_WORDS] */
} plat_index_query_out;

int plat_index_query_batch(plat_ctx* ctx, const plat_index_query_in* in, const plat_index_query_out* out, void* stream);

/* ---- indexed sequence fetch from the bytes of a FASTA file -------------------------------------------------------------
 * Replaces  FastaFile.getSequence  (src/cython/fastafile.pyx:173-207; setCacheSequence :141-171 is the same arithmetic) for n_queries
 * queries against the bytes of ONE file in one call, and adds the whole-contig fetch the region loop needs (plat_region.contig_seq holds
 * all SeqLength bases; getSequence never returns the last one).  A query brings the four numbers of its contig's .fai line (StartPos,
 * LineLength, FullLineLength, SeqLength as FastaIndex.getRefs reads them, :64-82), beg, end and a mode.  csrc/fasta_rule.hpp is the
 * rule as code, for the device and for the host twin.
 *
 * The file: `file` [file_len], 16-byte aligned, is a CUT of the real file -- its bytes file_base .. file_base + file_len; file_size is
 * the real file's length.  An integrator uploads only the contigs it wants.  No byte outside [file, file + file_len) is read.
 *
 * The rule, per query:
 *   offset(p)  StartPos + p + (FullLineLength - LineLength) * (long long)((double)p / LineLength): the quotient in fp64, truncated
 *   mode 0     b = max(0, beg), e = min(SeqLength - 1, end); e < b is PLAT_FASTA_INDEX_ERROR (the reference's IndexError); the span is
 *              the file's bytes [offset(b), offset(e)) -- b == e is an empty answer, status 0
 *   mode 1     the whole contig: [offset(0), offset(SeqLength - 1) + 1); beg and end are not read; SeqLength <= 0 is an empty answer
 *   the end    both ends of the span are cut at file_size (a read at or past the end of a file returns what is there)
 *   bytes      every 0x0A of the span is dropped, a-z become A-Z, every other byte -- '\r', NUL, bytes >= 0x80 -- is kept.  The
 *              reference never looks at what it seeks over: an index that lies (a ragged line) returns whatever lies there, header
 *              bytes included, and so does this call
 *   other ends LineLength == 0, which the reference divides by: PLAT_FASTA_ZERO_LINE.  StartPos < 0, LineLength < 0,
 *              FullLineLength < LineLength or offsets that leave 63 bits (the reference would seek to a negative offset or read a
 *              negative count): PLAT_FASTA_BAD_INDEX -- a stated limit, not parity.  A non-empty span that begins in front of the cut:
 *              PLAT_FASTA_LEFT_OF_CUT; one that ends behind it: PLAT_FASTA_RIGHT_OF_CUT.  Such a query has no bytes
 *
 * Output (device): out_status [n_queries] (PLAT_FASTA_*), out_off [n_queries + 1] from 0 (an exclusive scan taken on the device),
 * out [cap_bytes]: query q's bytes at out_off[q] .. out_off[q + 1]; totals [PLAT_FASTA_STATUS_WORDS]: {0 or PLAT_ERR_OVERFLOW, the bytes
 * of all answers, the tiles walked, the queries whose status is not 0}.  More bytes than cap_bytes is PLAT_ERR_OVERFLOW in totals[0]:
 * out_off, out_status and the totals hold the full counts, no byte is written, and the caller calls again with totals[1] bytes of room.
 *
 * The work is cut by tiles of the file spans, plat_fasta_tile_bytes() bytes of aligned 16-byte words each, not by queries: tens of
 * thousands of 200-base contexts and a handful of 250 MB contigs go through the same five launches (csrc/plat_fasta.hip names them:
 * spans, a scan of the tile counts, a count pass, a scan of the byte counts, a write pass).  Scratch: three words per query and two
 * per wave of the grid, in the context (one of these calls at a time per context); the call does not wait, reads nothing back and
 * nothing traps.                                                                                                                  */
#define PLAT_FASTA_STATUS_WORDS 4
#define PLAT_FASTA_OK 0
#define PLAT_FASTA_INDEX_ERROR 1
#define PLAT_FASTA_ZERO_LINE 2
#define PLAT_FASTA_BAD_INDEX 3
#define PLAT_FASTA_LEFT_OF_CUT 4
#define PLAT_FASTA_RIGHT_OF_CUT 5
#define PLAT_FASTA_MODE_SEQUENCE 0
#define PLAT_FASTA_MODE_CONTIG 1
typedef struct plat_fasta_fetch_in {
    const uint8_t* file;             /* [file_len] 16-byte aligned */
    int64_t file_len, file_base, file_size;
    int64_t n_queries;
    const int64_t* start_pos; const int64_t* line_len; const int64_t* full_len; const int64_t* seq_len;      /* [n_queries] */
    const int64_t* beg; const int64_t* end;              /* [n_queries] */
    const uint8_t* mode;             /* [n_queries] PLAT_FASTA_MODE_* */
} plat_fasta_fetch_in;

typedef struct plat_fasta_fetch_out {
    int64_t cap_bytes;
    int64_t* out_off;                /* [n_queries + 1] */
    int32_t* out_status;             /* [n_queries] */
    uint8_t* out;                    /* [cap_bytes] */
    int64_t* totals;                 /* [PLAT_FASTA_STATUS_WORDS] */
} plat_fasta_fetch_out;

int plat_fasta_fetch_batch(plat_ctx* ctx, const plat_fasta_fetch_in* in, const plat_fasta_fetch_out* out, void* stream);
int plat_fasta_tile_bytes(void);                            /* the bytes of one tile of a file span */

/* ---- read counts of reference-call blocks ------------------------------------------------------------------------
 * Replaces the loop of  outputRefCall   variantcaller.pyx:774-784  over  ReadArray.countReadsCoveringRegion(p, p + 1)   cwindow.pyx:176-206
 * (one call per position of a block and per sample: the block's QUAL is computed from the smallest count)
 * for n_intervals half-open intervals [iv_start[k], iv_end[k]) over read tables that are resident and sorted: read_pos / read_end [n_reads]
 * as plat_stage_b_in takes them.  Interval k belongs to the iv_n_samples[k] slices iv_slice_first[k] ... of slice_begin / slice_n /
 * slice_longest [n_slices]: the GOOD reads of one sample of one region inside the table, `longest` their getLengthOfLongestRead (:167-172).
 *
 * The rule, per slice (pos, end, N, longest) and position p:
 *   N == 0:    c = 0
 *   otherwise  s0 = lower_bound(pos, max(1, p - longest)), e0 = lower_bound(pos, p + 1); s0 walks on while s0 < N and end[s0] <= p;
 *              c = e0 - s0.  c < 0 is where the reference raises ("Read start pointer > read end pointer"); the walk may stop there.
 * c is a difference of two pointers and not the number of covering reads: a short read lying between two covering reads is counted, and
 * a read at position 0 is never found by the first bound.  Both are reproduced.
 *
 * Output: iv_min[k] = the smallest c over the interval's samples and positions; PLAT_REFCOV_RAISES if any c < 0 (a data verdict, not an
 * error: the other intervals are unaffected); PLAT_REFCOV_EMPTY if iv_start >= iv_end or iv_n_samples == 0.  Where iv_count_off[k] >= 0
 * also counts[iv_count_off[k] + (p - iv_start[k])] = the smallest c over the samples at p, PLAT_REFCOV_RAISES where negative; an entry at
 * or behind cap_counts is not written.  A slice index outside [0, n_slices) or a slice outside [0, n_reads) is refused: it counts as
 * PLAT_REFCOV_RAISES wherever it is asked.
 *
 * One 256-thread workgroup per tile of at most PLAT_REFCOV_TILE consecutive positions of one interval; the caller (who made the
 * intervals) hands the tile list over as iv_tile_first [n_intervals + 1]: interval k owns the tiles iv_tile_first[k] ... iv_tile_first[k + 1]
 * - 1, max(1, ceil(length / PLAT_REFCOV_TILE)) of them, n_tiles = iv_tile_first[n_intervals].  With n_tiles == n_intervals (no interval
 * longer than a tile) iv_tile_first is not read and may be NULL, and the call is one kernel; otherwise a second kernel takes the
 * intervals' minima over their tiles' (kept in the context's scratch).  An interval's last tile goes on over positions the list left
 * out, so a list with too few tiles costs time and not values; an interval without any tile is reported as PLAT_REFCOV_RAISES.
 * Per sample the workgroup finds the index range that holds every bound of its tile by two bisections of the slice, stages the range's
 * pos / end in LDS when it holds at most plat_refcov_lds_reads() reads (a deeper pile runs the same code on global memory) and bisects
 * there, one thread per position.  Every output element is written by exactly one workgroup: no fill, no atomics.  The call does not
 * wait; nothing traps.                                                                                                          */
#define PLAT_REFCOV_RAISES (-1)
#define PLAT_REFCOV_EMPTY 2147483647
#define PLAT_REFCOV_TILE 1024

typedef struct plat_refcov_in {
    int32_t n_intervals, n_slices, n_tiles, n_reads;
    const int32_t* read_pos; const int32_t* read_end;
    const int32_t* slice_begin; const int32_t* slice_n; const int32_t* slice_longest;
    const int32_t* iv_start; const int32_t* iv_end; const int32_t* iv_slice_first; const int32_t* iv_n_samples;
    const int64_t* iv_count_off;
    const int32_t* iv_tile_first;
} plat_refcov_in;

typedef struct plat_refcov_out {
    int64_t cap_counts;
    int32_t* iv_min;
    int32_t* counts;
} plat_refcov_out;

int plat_refcall_coverage_batch(plat_ctx* ctx, const plat_refcov_in* in, const plat_refcov_out* out, void* stream);
int plat_refcov_lds_reads(void);                            /* reads of one sample a tile's range may hold to be staged in LDS */

/* ---- read statistics of the VCF INFO field ---------------------------------------
 * Replaces the per-variant loop over a window's reads in  cdef dict vcfINFO(...)   vcfutils.pyx:1300-1390
 * (readOverlapsVariant :901-913, readQualIsGoodVariantPosition :917-943, variantSupportedByRead :961-1072).
 * Variant v lies in window var_window[v]; sample i of window w owns the good reads
 * [good_begin[w*n_ind+i], good_end[..]) and the bad reads [bad_begin[..], bad_end[..]) of one read table
 * (bases, raw phred qualities, pos, end, mapq, bitFlag, CIGAR pairs); var_in_genotype[v*n_ind+i] =
 * `variant in genotypeCalls[i]`; the added bases of v at var_added[var_added_off[v] ..+var_n_added[v]).
 * Options: badReadsWindow (runner.py: 11), countOnlyExactIndelMatches (0).
 * Output: out_counts[16*v + k]: 0 TC, 1 TC_bad, 2 TR, 3 TC_ab, 4 TR_ab, 5 NR_sb, 6 NF_sb, 7 TCR, 8 TCF,
 * 9 TCR_sb, 10 TCF_sb, 11 NR, 12 NF, 13 nGoodReads, 14 nBadReads, 15 sum of mapq^2 (the reference keeps this
 * sum in a float: identical below 2^24); out_per_sample[(v*n_ind+i)*2 + {0,1}] = nReadsThisSample,
 * nVarReadsThisSample; out_minq[minq_off[v] + k], k < out_nminq[v]: the MMLQ window minima in read order
 * (room for the window's good reads).  The INFO values follow by arithmetic the caller keeps
 * (MQ = sqrt(sum/(TC+TC_bad)), BRF, MMLQ = median, ABPV / SbPval from the _ab / _sb counts).      */
typedef struct plat_infostats_batch {
    int32_t n_vars, n_ind;
    const int32_t* var_window;       /* [n_vars] */
    const int32_t* var_pos;          /* Variant.refPos */
    const int32_t* var_bam_min;      /* Variant.bamMinPos */
    const int32_t* var_bam_max;      /* Variant.bamMaxPos */
    const int32_t* var_n_added;
    const int32_t* var_n_removed;
    const uint8_t* var_added;
    const int64_t* var_added_off;    /* [n_vars] */
    const uint8_t* var_in_genotype;  /* [n_vars*n_ind] */
    const int64_t* minq_off;         /* [n_vars] */
    const int32_t* good_begin;       /* [n_windows*n_ind] */
    const int32_t* good_end;
    const int32_t* bad_begin;
    const int32_t* bad_end;
    const uint8_t* read_seq;
    const uint8_t* read_qual;
    const int64_t* read_off;         /* [n_reads+1] */
    const int32_t* read_pos;
    const int32_t* read_end;
    const uint8_t* read_mapq;
    const int32_t* read_flags;
    const int16_t* cigar;
    const int32_t* cig_off;          /* [n_reads+1] */
} plat_infostats_batch;

int plat_variant_read_stats_batch(plat_ctx* ctx, const plat_infostats_batch* batch, int bad_reads_window,
                                  int count_only_exact_indel_matches, int64_t* out_counts, int32_t* out_per_sample,
                                  int32_t* out_minq, int32_t* out_nminq, void* stream);

/* ---- the loops of two INFO fields, from the counts above ------------------------------------------------
 * Replaces, per variant, the work inside
 *     computeAlleleBiasPValue / computeStrandBiasPValue   vcfutils.pyx:1156-1222   (INFO ABPV -- used by the alleleBias filter -- and SbPval)
 *     betaBinomialCDF, threeFTwo, logBetaFunction          platypusutils.pyx:178-315
 *     sorted(minBaseQualsInWindow)[n // 2]                  vcfutils.pyx:1390-1399   (INFO MMLQ)
 * that is a LOOP: the hypergeometric series 3F2 (|k - n + 1| terms), the sums of log-factorials (a table of the reference's own
 * logFactorial, made with the HOST's libm when the context is created), the median.  What is left to the caller are the three libm
 * calls of a CDF on these terms, so that the value has the bits the host's code gives:
 *     cdf = max(1e-30, 1 - exp((terms[1] + log(terms[2])) - terms[3]))
 * counts / minq_off / minq / n_minq: the outputs of plat_variant_read_stats_batch, still on the device.
 * out_terms[8 v + 0..3] allele bias, [8 v + 4..7] strand bias: [0] = 0: the function returns [1] as it is (its early exits; the allele
 * bias value is then final, min(p, 1 - p) included); 1: [1..3] are the terms of betaBinomialCDF(k, n, alpha, beta) above (allele bias:
 * the caller still takes min(p, 1 - p)); 2: an argument of logFactorial beyond the table (4096): the caller computes the field itself.
 * out_mmlq[v] = the median as the reference takes it, 100 when the variant has no entries.                                       */
int plat_variant_info_batch(plat_ctx* ctx, int n_vars, const int64_t* counts, const int64_t* minq_off, const int32_t* minq,
                            const int32_t* n_minq, double* out_terms, int32_t* out_mmlq, void* stream);

/* ---- read tables that crossed the link at one byte per base --------------------------------------------
 * The loader's decode loop (htslibWrapper.pyx:330-370: 4-bit BAM code -> letter, quality byte copied, one pass over every base)
 * may write ONE byte per base instead of two: bits 0..1 = (letter >> 1) & 3 (A 0, C 1, T 2, G 3), bits 2..7 = quality 0..63
 * (PLAT_READS_PACKED of include/platypus_caller.h).  plat_unpack_reads expands n_bytes such bytes to the ASCII base and raw
 * quality arrays every other entry point takes (out_seq / out_qual [n_bytes]), then patches the n_exc exceptions (bases other
 * than A/C/G/T, qualities above 63): out_seq[exc_index[k]] = exc_base[k], out_qual[exc_index[k]] = exc_qual[k].  All device
 * pointers; exc_* may be NULL when n_exc == 0.                                                                          */
int plat_unpack_reads(plat_ctx* ctx, int64_t n_bytes, const uint8_t* packed, uint8_t* out_seq, uint8_t* out_qual,
                      int64_t n_exc, const int64_t* exc_index, const uint8_t* exc_base, const uint8_t* exc_qual, void* stream);

/* ---- window read slices out of a resident read table ---------------------------------------------
 * Replaces the per-window walk over  bamReadBuffer.reads / badReads / brokenMates  between the window
 * pointers (cwindow.pyx:208-264,655-689) that feeds Haplotype.alignReads: the reads of a whole region are
 * uploaded ONCE (one table: bases, qualities, offsets, pos, end, mapq, bitFlag) and the read arrays of a
 * plat_window_batch are gathered from it on the device.  Destination read d is source read src_index[d];
 * its bases / qualities go to dst_seq|dst_qual[dst_off[d] .. dst_off[d+1]) (dst_off is what the batch then
 * uses as read_off, computed by the caller from the read lengths), its pos / end / mapq / bitFlag to
 * dst_*[d].  All pointers are device pointers.                                                       */
int plat_gather_reads(plat_ctx* ctx, int64_t n_dst, const int32_t* src_index, const int64_t* dst_off,
                      const uint8_t* src_seq, const uint8_t* src_qual, const int64_t* src_off,
                      const int32_t* src_pos, const int32_t* src_end, const uint8_t* src_mapq,
                      const int32_t* src_flags, uint8_t* dst_seq, uint8_t* dst_qual, int32_t* dst_pos,
                      int32_t* dst_end, uint8_t* dst_mapq, int32_t* dst_flags, void* stream);

/* ---- packed bases read where they lie ------------------------------------------------------------------------------------------
 * A chunk whose reads all come out of PLAT_READS_PACKED tables (exceptions A/C/G/T/N or qualities above 63 only) need not be expanded to
 * ASCII at all: every kernel that starts from a READ takes the read's packed bytes at their source -- letter "ACTG"[b & 3], quality
 * b >> 2, or the exception's byte and quality where the blob index read_off[r] + i is listed.  The entry points below are the packed
 * counterparts of plat_concat_read_tables, plat_unpack_reads_pieces_codes, plat_candidates_batch_codes, plat_gather_reads and
 * plat_variant_read_stats_batch; each gives what its counterpart gives on the expanded table, bit for bit.
 *   plat_packed_reads      read_src[r] = device address of read r's packed bytes (any alignment; only the read's own bytes are read);
 *                          exc_index ascending, blob indices in read_off's units; exc_* may be NULL when n_exc == 0.  All device memory.
 *   plat_concat_read_tables_src   = plat_concat_read_tables + dst_src[first_read + i] = desc.src + desc.off[i] (src: the table's packed
 *                          bytes on the device)
 *   plat_pack_codes_pieces the 2-bit codes of plat_unpack_reads_pieces_codes WITHOUT the ASCII arrays: out_codes[(total_bytes + 15) / 16
 *                          + 8], exceptions patched in (exc_base only), the 8 words behind the last base zero.  The buffer need not be
 *                          zeroed: a dword every base of which belongs to one piece is stored whole, the dwords at a piece's two ends are
 *                          zeroed first and OR-ed in.  Dwords no piece reaches keep what they held.
 *   plat_candidates_batch_packed  = plat_candidates_batch_codes with the reads' letters and qualities taken from `packed`.
 *                          batch->read_seq is an OUTPUT here ([read_off[n_reads] + PLAT_BLOB_PAD], need not be initialised): the scan
 *                          writes the read-side allele of every record it finds, read_seq[rec[4] .. rec[4] + rec[2]), whether or not the
 *                          record fits the read's slice -- what plat_candidates_merge_batch and plat_stage_b_batch read.  batch->read_qual
 *                          is not used (may be NULL).
 *   plat_gather_reads_packed      = plat_gather_reads (ASCII destination) from packed sources
 *   plat_variant_read_stats_packed_batch = plat_variant_read_stats_batch; batch->read_seq / read_qual are not used (may be NULL)       */
typedef struct plat_packed_reads {
    const uint8_t* const* read_src;
    int64_t n_exc;
    const int64_t* exc_index;
    const uint8_t* exc_base;
    const uint8_t* exc_qual;
} plat_packed_reads;
typedef struct plat_table_src_desc {
    const int64_t* off; const int32_t* pos; const int32_t* end; const uint8_t* mapq; const int32_t* flags; const int16_t* cigar; const int32_t* cig_off;
    int32_t n, scan; int64_t first_read, first_byte, first_pair;
    const uint8_t* src;
} plat_table_src_desc;
int plat_concat_read_tables_src(plat_ctx* ctx, int n_tables, int max_reads_per_table, const plat_table_src_desc* desc, int64_t* dst_off, int32_t* dst_pos,
                                int32_t* dst_end, uint8_t* dst_mapq, int32_t* dst_flags, int32_t* dst_cig_off, int16_t* dst_cigar,
                                int32_t* dst_region, const uint8_t** dst_src, int64_t n_total_reads, int64_t total_bytes, int64_t total_pairs, void* stream);
int plat_pack_codes_pieces(plat_ctx* ctx, int n_pieces, int64_t max_piece_bytes, const plat_unpack_piece* pieces, uint32_t* out_codes,
                           int64_t total_bytes, int64_t n_exc, const int64_t* exc_index, const uint8_t* exc_base, void* stream);
int plat_candidates_batch_packed(plat_ctx* ctx, const plat_candidate_batch* batch, const plat_packed_reads* packed, const uint32_t* read_codes,
                                 const uint32_t* ref_codes, const int32_t* ref_irregular, int min_flank, int min_base_qual, int gen_snps, int gen_indels,
                                 int max_per_read, const int32_t* read_region, int32_t* out_rec, int32_t* out_count, int32_t* out_status, void* stream);
int plat_gather_reads_packed(plat_ctx* ctx, int64_t n_dst, const int32_t* src_index, const int64_t* dst_off, const plat_packed_reads* packed,
                             const int64_t* src_off, const int32_t* src_pos, const int32_t* src_end, const uint8_t* src_mapq,
                             const int32_t* src_flags, uint8_t* dst_seq, uint8_t* dst_qual, int32_t* dst_pos, int32_t* dst_end,
                             uint8_t* dst_mapq, int32_t* dst_flags, void* stream);
int plat_variant_read_stats_packed_batch(plat_ctx* ctx, const plat_infostats_batch* batch, const plat_packed_reads* packed, int bad_reads_window,
                                         int count_only_exact_indel_matches, int64_t* out_counts, int32_t* out_per_sample,
                                         int32_t* out_minq, int32_t* out_nminq, void* stream);

/* ---- a14..a18: assembleReadsAndDetectVariants ---------------------------------------------------
 * Replaces  cdef list assembleReadsAndDetectVariants(chrom, assemStart, assemEnd, refStart, refEnd,
 *                                                    readBuffers, refSeq, options)
 *           assembler.pxd:3, assembler.pyx:1429-1476
 * for n_regions independent assembly tiles.  Reads of a region are those loadBAMDataIntoGraph
 * (assembler.pyx:1391-1425) would load, in its order, QCFail reads already removed.
 *   region g: reference bytes ref_seq[ref_off[g]..ref_off[g+1]) starting at genome coordinate
 *             ref_start[g]; assembly interval [assem_start[g], assem_end[g]);
 *             reads reg_read_begin[g]..reg_read_begin[g+1].
 * Options: kmer_size (assemblerKmerSize, 15), min_qual (minBaseQual, 20), min_weight
 * (minReads*minBaseQual, 40), no_cycles (noCycles, 0).
 * Output (device): per region up to max_vars_per_region variants, in the reference's sorted()
 * order: var_count[g]; var_pos/var_nrem/var_nadd [g*max_vars+i]; removed||added bytes at
 * var_blob[g*blob_per_region + var_off[g*max_vars+i]].  status[g] = 0 or PLAT_ERR_OVERFLOW.     */
typedef struct plat_assembly_batch {
    int32_t n_regions, n_reads;
    const uint8_t* ref_seq;
    const int64_t* ref_off;          /* [n_regions+1] */
    const int32_t* ref_start;        /* [n_regions] */
    const int32_t* assem_start;      /* [n_regions] */
    const int32_t* assem_end;        /* [n_regions] */
    const int32_t* reg_read_begin;   /* [n_regions+1] */
    const uint8_t* read_seq;
    const uint8_t* read_qual;
    const int64_t* read_off;         /* [n_reads+1] */
} plat_assembly_batch;

int plat_assemble_batch(plat_ctx* ctx, const plat_assembly_batch* batch, int kmer_size, int min_qual,
                        int min_weight, int no_cycles, int max_vars_per_region, int blob_per_region,
                        int32_t* var_count, int32_t* var_pos, int32_t* var_nrem, int32_t* var_nadd,
                        int32_t* var_off, uint8_t* var_blob, int32_t* status, void* stream);
/* The same without the read-back that sizes the graphs: plat_assemble_batch learns the longest reference window, the most reads
 * and the most k-mer positions of a tile from the device and WAITS for them; a caller that built the batch knows them.  Nothing
 * is read back and the call never waits.  hints: max_ref_len >= ref_off[g+1] - ref_off[g], max_reads_per_region >=
 * reg_read_begin[g+1] - reg_read_begin[g], max_positions >= reference bytes + read bytes + 2 * reads + 2 of every tile g.  The device
 * checks them: hints that do not cover the batch give status[g] = PLAT_ERR_BAD_HINTS for EVERY tile (PLAT_ERR_BAD_INPUT for offsets
 * out of order) and no variants.                                                                     */
typedef struct plat_assembly_hints {
    int32_t max_ref_len, max_reads_per_region;
    int64_t max_positions;
} plat_assembly_hints;
int plat_assemble_batch_async(plat_ctx* ctx, const plat_assembly_batch* batch, const plat_assembly_hints* hints, int kmer_size,
                              int min_qual, int min_weight, int no_cycles, int max_vars_per_region, int blob_per_region,
                              int32_t* var_count, int32_t* var_pos, int32_t* var_nrem, int32_t* var_nadd,
                              int32_t* var_off, uint8_t* var_blob, int32_t* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PLATYPUS_MI355X_H */
