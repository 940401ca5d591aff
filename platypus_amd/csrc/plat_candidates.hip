// plat_candidates.hip -- VariantCandidateGenerator (src/cython/variant.pyx:459-751): variant candidates
// from the CIGAR strings and the mismatches of the reads of a region.
//
// One lane walks one read exactly as getVariantCandidatesFromSingleRead / getSnpCandidatesFromReadSegment do (the
// mismatch-run state machine is sequential in the read), and writes one record per candidate OCCURRENCE into the read's
// own slice of the output -- so records come out in the reference's emission order (read by read, left to right) without
// any ordering step.  Merging equal variants and counting their supporting reads (addVariantToList, :499-527) is a
// dictionary operation over the few records that come back; it stays on the host (hostapi.VariantCandidateGenerator).
#include "plat_internal.hpp"
#include "wave_tiles.hpp"
#include "read_source.hpp"

namespace plat {

struct CandEmit {
    int32_t* rec; int n, cap;
    __device__ __forceinline__ void put(int pos, int nrem, int nadd, long long rem_off, long long add_off) {
        if (n < cap) {
            int32_t* r = rec + 5 * (long long)n;
            r[0] = pos < 0 ? 0 : pos;                    // Variant.__init__: max(0, refPos), variant.pyx:118
            r[1] = nrem; r[2] = nadd; r[3] = (int32_t)rem_off; r[4] = (int32_t)add_off;
        }
        ++n;
    }
};

__global__ void __launch_bounds__(64)
k_candidates(plat_candidate_batch b, int min_flank, int min_base_qual, int gen_snps, int gen_indels, int max_per_read,
             const int32_t* __restrict__ read_region, int32_t* __restrict__ rec, int32_t* __restrict__ count, int32_t* __restrict__ status)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= b.n_reads) return;
    int st = 0;
    CandEmit out{rec + 5ll * (long long)r * max_per_read, 0, max_per_read};
    if (!(b.read_flags[r] & 512)) {                      // Read_IsQCFail reads are skipped, variant.pyx:729-731
        const int g = read_region[r];
        const long long roff = b.ref_off[g];
        const int refLen = (int)(b.ref_off[g + 1] - roff), refSeqStart = b.ref_seq_start[g], contigLen = b.contig_len[g];
        const uint8_t* ref = b.ref_seq + roff;
        const long long soff = b.read_off[r];
        const uint8_t* readSeq = b.read_seq + soff;
        const uint8_t* readQual = b.read_qual + soff;
        const int rlen = (int)(b.read_off[r + 1] - soff);
        const int readStart = b.read_pos[r];
        const int16_t* ops = b.cigar + 2ll * b.cig_off[r];
        const int cigarLength = b.cig_off[r + 1] - b.cig_off[r];
        int refOffset = 0, readOffset = 0;
        for (int ci = 0; ci < cigarLength; ++ci) {       // getVariantCandidatesFromSingleRead, :614-720
            const int flag = ops[2 * ci], length = ops[2 * ci + 1];
            if (flag == 1 || flag == 2) {                // insertion / deletion: needs a match of >= minFlank on one side
                bool flanked = false;
                if (ci > 0 && ops[2 * ci - 2] == 0 && ops[2 * ci - 1] >= min_flank) flanked = true;
                else if (ci < cigarLength - 1 && ops[2 * ci + 2] == 0 && ops[2 * ci + 3] >= min_flank) flanked = true;
                if (flag == 1) {
                    if (flanked && gen_indels && !has_n(readSeq + readOffset, length))
                        out.put(readStart + refOffset - 1, 0, length, -1, soff + readOffset);
                    readOffset += length;
                } else {
                    if (flanked) {
                        // refFile.getSequence(rname, a, a + length): clamped to [0, contigLen - 1], fastafile.pyx:186-187
                        int a = readStart + refOffset, e = a + length;
                        if (a < 0) a = 0;
                        if (e > contigLen - 1) e = contigLen - 1;
                        const int n = e > a ? e - a : 0;
                        if (a - refSeqStart < 0 || a - refSeqStart + n > refLen) st = PLAT_ERR_BAD_INPUT;   // outside the window handed over
                        else if (gen_indels && !has_n(ref + (a - refSeqStart), n))
                            out.put(readStart + refOffset - 1, n, 0, roff + (a - refSeqStart), -1);
                    }
                    refOffset += length;
                }
            } else if (flag == 0 || flag == 7 || flag == 8) {    // M, =, X
                if (!(flag == 7 || (length < min_flank && flag == 0)) && gen_snps) {
                    // getSnpCandidatesFromReadSegment, :529-612.  The loop there visits every base; only mismatches change its state
                    // (a run of mismatches is closed at the first MATCH more than minFlank behind its end -- or by the next mismatch that
                    // far behind it, which finds the same run and writes the same record), so whole words of equal bases are stepped over:
                    // 8 bases of the read against 8 of the reference per load.
                    int msr = -1, mer = -1, msd = -1, med = -1;
                    int lo = (readOffset == 0) ? (min_flank < length ? min_flank : length) : 0;                  // first index looked at
                    int hi = rlen - min_flank - readOffset;                                                       // one past the last
                    if (hi > length) hi = length;
                    // the reference reads past its buffer where refIndex leaves [0, refLen): it stops there (after the bases before)
                    const int refIndex0 = refOffset + readStart - refSeqStart;                                    // refIndex of index 0
                    if (lo < hi) {
                        if (refIndex0 + lo < 0) { st = PLAT_ERR_BAD_INPUT; hi = lo; }
                        else if (refIndex0 + hi > refLen) { st = PLAT_ERR_BAD_INPUT; hi = refLen - refIndex0; }
                    }
                    const uint8_t* rp = readSeq + readOffset;
                    const uint8_t* fp = ref + refIndex0;
                    auto mismatch = [&](int index) {
                        const int readIndex = index + readOffset, refIndex = refIndex0 + index;
                        const uint8_t readChar = rp[index], refChar = fp[index];
                        if (readChar != 'N' && refChar != 'N' && (int)readQual[readIndex] >= min_base_qual) {
                            if (msr == -1) { msr = mer = refIndex; msd = med = readIndex; }
                            else if (refIndex - mer <= min_flank) { mer = refIndex; med = readIndex; }
                            else {
                                out.put(msr + refSeqStart, mer - msr + 1, med - msd + 1, roff + msr, soff + msd);
                                msr = mer = refIndex; msd = med = readIndex;
                            }
                        }
                    };
                    int index = lo;
                    // (round 5: 32 bases per trip -- the eight loads of a trip do not depend on one another, so a trip waits for memory once
                    //  where four trips of 8 bases waited four times: the walk is a chain of such waits, not a stream.  The last trip reads
                    //  past `hi` -- blobs are followed by PLAT_BLOB_PAD readable bytes -- and masks what it read there.)
                    constexpr int CAND_TRIP = 4;                                     // words of 8 bases per trip
                    static_assert(PLAT_BLOB_PAD >= 8 * CAND_TRIP, "the last trip of the mismatch scan reads past a blob's end");
                    for (; index < hi; index += 8 * CAND_TRIP) {
                        const int nleft = hi - index;
                        unsigned long long x4[CAND_TRIP];
#pragma unroll
                        for (int q = 0; q < CAND_TRIP; ++q) x4[q] = load_u64_bytes(rp + index + 8 * q) ^ load_u64_bytes(fp + index + 8 * q);
                        if (nleft < 8 * CAND_TRIP) {
#pragma unroll
                            for (int q = 0; q < CAND_TRIP; ++q) {
                                const int nb = nleft - 8 * q;
                                if (nb <= 0) x4[q] = 0ull;
                                else if (nb < 8) x4[q] &= (1ull << (8 * nb)) - 1ull;
                            }
                        }
                        unsigned long long any = 0ull;
#pragma unroll
                        for (int q = 0; q < CAND_TRIP; ++q) any |= x4[q];
                        if (any == 0ull) continue;
#pragma unroll
                        for (int q = 0; q < CAND_TRIP; ++q) {
                            unsigned long long x = x4[q];
                            while (x) {
                                const int j = (__ffsll((long long)x) - 1) >> 3;
                                mismatch(index + 8 * q + j);
                                x &= ~(0xFFull << (8 * j));
                            }
                        }
                    }
                    if (msr != -1) out.put(msr + refSeqStart, mer - msr + 1, med - msd + 1, roff + msr, soff + msd);
                }
                readOffset += length;
                refOffset += length;
            } else if (flag == 3) {                      // N: skipped reference
                refOffset += length;
            } else if (flag == 4) {                      // soft clip: bases present in the read, positions were moved back
                readOffset += length;
                if (ci == 0) refOffset += length;
            }                                            // H, P, anything else: nothing
        }
    }
    if (out.n > max_per_read && st == 0) st = PLAT_ERR_OVERFLOW;
    count[r] = out.n;
    status[r] = st;
}

// ---- the scan on 2-bit base codes (round 6) --------------------------------------------------------------------------------------------
// k_candidates walks a read 8 bases per 64-bit word, 40 scattered loads for 150 bases and the same again for the reference: 1.07 GB of traffic
// per chunk of 128 regions against the 0.42 GB it has to read.  Equal bases have equal codes, so the mismatch scan can run on the codes -- 32 bases
// per word, one aligned load each for read and reference, the whole read in ONE round of loads -- and look at the bytes only where the codes
// differ: a position whose codes differ is a mismatch of the bytes or holds a byte that is not A, C, G, T (then the byte test of the
// reference's loop decides, as before); a position whose codes are equal while its bytes differ can only hold such a byte -- an N (which the loop
// ignores anyway: variant.pyx:560-567) or, in an "irregular" reference region (any other byte), anything: those regions take the byte scan.
__global__ void __launch_bounds__(256)
k_ref_codes(const uint8_t* __restrict__ ref, const int64_t* __restrict__ ref_off, int n_regions, long long n_bytes, uint32_t* __restrict__ codes,
            int32_t* __restrict__ irregular)
{
    const long long d = (long long)blockIdx.x * blockDim.x + threadIdx.x;        // one dword of codes = 16 bases
    if (16 * d >= n_bytes) return;
    uint32_t cw = 0;
    bool odd = false;
    for (int k = 0; k < 16; ++k) {
        const long long i = 16 * d + k;
        const unsigned b = i < n_bytes ? ref[i] : (unsigned)'A';
        cw |= ((b >> 1) & 3u) << (2 * k);
        odd = odd || !(b == 'A' || b == 'C' || b == 'G' || b == 'T' || b == 'N');
    }
    codes[d] = cw;
    if (odd)
        for (int k = 0; k < 16; ++k) {
            const long long i = 16 * d + k;
            if (i >= n_bytes) break;
            const unsigned b = ref[i];
            if (b == 'A' || b == 'C' || b == 'G' || b == 'T' || b == 'N') continue;
            int lo = 0, hi = n_regions;                                           // the region this byte belongs to: ref_off[g] <= i < ref_off[g + 1]
            while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (ref_off[mid] <= i) lo = mid; else hi = mid; }
            irregular[lo] = 1;
        }
}

// 32 bases of a code stream from base index i (any alignment): two aligned words and a funnel shift
__device__ __forceinline__ unsigned long long codes_at(const unsigned long long* __restrict__ c, long long i) {
    const long long w = i >> 5;
    const int sh = 2 * (int)(i & 31);
    const unsigned long long lo = c[w];
    if (sh == 0) return lo;
    return (lo >> sh) | (c[w + 1] << (64 - sh));
}

// the scan of read r on codes, over either storage.  SrcPacked: no expanded bytes exist, so the lane leaves the read-side allele of every
// record it finds in b.read_seq (the chunk's t_seq) at the record's own offset -- all that the kernels starting from a RECORD (merge, filter,
// stage B) ever read of it.  Written whether or not the record fits the slice: the same bytes again on the retry with more room.
template <class S>
__device__ __forceinline__ void candidates_codes_one(const plat_candidate_batch& b, const S& src, const unsigned long long* __restrict__ read_codes,
                   const unsigned long long* __restrict__ ref_codes,
                   const int32_t* __restrict__ ref_irregular, int min_flank, int min_base_qual, int gen_snps, int gen_indels, int max_per_read,
                   const int32_t* __restrict__ read_region, int32_t* __restrict__ rec, int32_t* __restrict__ count, int32_t* __restrict__ status)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= b.n_reads) return;
    int st = 0;
    CandEmit out{rec + 5ll * (long long)r * max_per_read, 0, max_per_read};
    if (!(b.read_flags[r] & 512)) {                      // Read_IsQCFail reads are skipped, variant.pyx:729-731
        const int g = read_region[r];
        const long long roff = b.ref_off[g];
        const int refLen = (int)(b.ref_off[g + 1] - roff), refSeqStart = b.ref_seq_start[g], contigLen = b.contig_len[g];
        const bool byBytes = ref_irregular[g] != 0;      // a reference byte other than A, C, G, T, N in this region: the byte scan
        const uint8_t* ref = b.ref_seq + roff;
        const long long soff = b.read_off[r];
        const int rlen = (int)(b.read_off[r + 1] - soff);
        const auto rd = src.read(r, soff, rlen);
        // the read-side allele [start, start + n) of a record about to be put
        auto allele = [&](int start, int n) {
            if constexpr (S::packed) { uint8_t* o = const_cast<uint8_t*>(b.read_seq) + soff + start; for (int i = 0; i < n; ++i) o[i] = rd.base(start + i); }
        };
        const int readStart = b.read_pos[r];
        const int16_t* ops = b.cigar + 2ll * b.cig_off[r];
        const int cigarLength = b.cig_off[r + 1] - b.cig_off[r];
        int refOffset = 0, readOffset = 0;
        for (int ci = 0; ci < cigarLength; ++ci) {       // getVariantCandidatesFromSingleRead, :614-720
            const int flag = ops[2 * ci], length = ops[2 * ci + 1];
            if (flag == 1 || flag == 2) {                // insertion / deletion: needs a match of >= minFlank on one side
                bool flanked = false;
                if (ci > 0 && ops[2 * ci - 2] == 0 && ops[2 * ci - 1] >= min_flank) flanked = true;
                else if (ci < cigarLength - 1 && ops[2 * ci + 2] == 0 && ops[2 * ci + 3] >= min_flank) flanked = true;
                if (flag == 1) {
                    if (flanked && gen_indels && !rd.has_n(readOffset, length)) {
                        allele(readOffset, length);
                        out.put(readStart + refOffset - 1, 0, length, -1, soff + readOffset);
                    }
                    readOffset += length;
                } else {
                    if (flanked) {
                        int a = readStart + refOffset, e = a + length;   // refFile.getSequence(rname, a, a + length): clamped to [0, contigLen - 1], fastafile.pyx:186-187
                        if (a < 0) a = 0;
                        if (e > contigLen - 1) e = contigLen - 1;
                        const int n = e > a ? e - a : 0;
                        if (a - refSeqStart < 0 || a - refSeqStart + n > refLen) st = PLAT_ERR_BAD_INPUT;   // outside the window handed over
                        else if (gen_indels && !has_n(ref + (a - refSeqStart), n))
                            out.put(readStart + refOffset - 1, n, 0, roff + (a - refSeqStart), -1);
                    }
                    refOffset += length;
                }
            } else if (flag == 0 || flag == 7 || flag == 8) {    // M, =, X
                if (!(flag == 7 || (length < min_flank && flag == 0)) && gen_snps) {
                    // getSnpCandidatesFromReadSegment, :529-612: only mismatches change the loop's state (k_candidates has the argument)
                    int msr = -1, mer = -1, msd = -1, med = -1;
                    int lo = (readOffset == 0) ? (min_flank < length ? min_flank : length) : 0;                  // first index looked at
                    int hi = rlen - min_flank - readOffset;                                                       // one past the last
                    if (hi > length) hi = length;
                    const int refIndex0 = refOffset + readStart - refSeqStart;                                    // refIndex of index 0
                    if (lo < hi) {
                        if (refIndex0 + lo < 0) { st = PLAT_ERR_BAD_INPUT; hi = lo; }
                        else if (refIndex0 + hi > refLen) { st = PLAT_ERR_BAD_INPUT; hi = refLen - refIndex0; }
                    }
                    const uint8_t* fp = ref + refIndex0;
                    auto mismatch = [&](int index) {
                        const int readIndex = index + readOffset, refIndex = refIndex0 + index;
                        const uint8_t readChar = rd.base(readIndex), refChar = fp[index];
                        if (readChar != refChar && readChar != 'N' && refChar != 'N' && (int)rd.qual(readIndex) >= min_base_qual) {
                            // the first mismatch opens a run; one within minFlank of the run's end extends it; any other closes it and opens the next
                            // (written as selects on the four values: as three branches that each store some of them, the compiler keeps two in scratch)
                            const bool extend = msr != -1 && refIndex - mer <= min_flank;
                            if (msr != -1 && !extend) {
                                allele(msd, med - msd + 1);
                                out.put(msr + refSeqStart, mer - msr + 1, med - msd + 1, roff + msr, soff + msd);
                            }
                            msr = extend ? msr : refIndex; msd = extend ? msd : readIndex;
                            mer = refIndex; med = readIndex;
                        }
                    };
                    if (byBytes) {
                        for (int index = lo; index < hi; ++index) if (rd.base(readOffset + index) != fp[index]) mismatch(index);
                    } else {
                        // 32 bases per word; CODE_TRIP words (160 bases: a whole 150-base read) are requested together
                        constexpr int CODE_TRIP = 5;
                        const long long rb = soff + readOffset, fb = roff + refIndex0;                           // blob index of index 0, read and reference
                        for (int index = lo; index < hi; index += 32 * CODE_TRIP) {
                            unsigned long long x[CODE_TRIP];
#pragma unroll
                            for (int q = 0; q < CODE_TRIP; ++q) {
                                const int at = index + 32 * q;
                                x[q] = at < hi ? codes_at(read_codes, rb + at) ^ codes_at(ref_codes, fb + at) : 0ull;
                            }
#pragma unroll
                            for (int q = 0; q < CODE_TRIP; ++q) {
                                const int at = index + 32 * q, nb = hi - at;
                                if (nb <= 0) continue;
                                unsigned long long y = x[q];
                                if (nb < 32) y &= (1ull << (2 * nb)) - 1ull;
                                y = (y | (y >> 1)) & 0x5555555555555555ull;                                         // one bit per base whose codes differ
                                while (y) {
                                    const int j = (__ffsll((long long)y) - 1) >> 1;
                                    mismatch(at + j);
                                    y &= y - 1ull;
                                }
                            }
                        }
                    }
                    if (msr != -1) { allele(msd, med - msd + 1); out.put(msr + refSeqStart, mer - msr + 1, med - msd + 1, roff + msr, soff + msd); }
                }
                readOffset += length;
                refOffset += length;
            } else if (flag == 3) {                      // N: skipped reference
                refOffset += length;
            } else if (flag == 4) {                      // soft clip: bases present in the read, positions were moved back
                readOffset += length;
                if (ci == 0) refOffset += length;
            }                                            // H, P, anything else: nothing
        }
    }
    if (out.n > max_per_read && st == 0) st = PLAT_ERR_OVERFLOW;
    count[r] = out.n;
    status[r] = st;
}

__global__ void __launch_bounds__(64)
k_candidates_codes(plat_candidate_batch b, const unsigned long long* __restrict__ read_codes, const unsigned long long* __restrict__ ref_codes,
                   const int32_t* __restrict__ ref_irregular, int min_flank, int min_base_qual, int gen_snps, int gen_indels, int max_per_read,
                   const int32_t* __restrict__ read_region, int32_t* __restrict__ rec, int32_t* __restrict__ count, int32_t* __restrict__ status)
{
    candidates_codes_one(b, SrcAscii{b.read_seq, b.read_qual}, read_codes, ref_codes, ref_irregular, min_flank, min_base_qual, gen_snps, gen_indels, max_per_read,
                         read_region, rec, count, status);
}

// ... and on packed bytes at their source (plat_candidates_batch_packed)
__global__ void __launch_bounds__(64)
k_candidates_packed(plat_candidate_batch b, plat_packed_reads pk, const unsigned long long* __restrict__ read_codes, const unsigned long long* __restrict__ ref_codes,
                    const int32_t* __restrict__ ref_irregular, int min_flank, int min_base_qual, int gen_snps, int gen_indels, int max_per_read,
                    const int32_t* __restrict__ read_region, int32_t* __restrict__ rec, int32_t* __restrict__ count, int32_t* __restrict__ status)
{
    candidates_codes_one(b, SrcPacked{pk}, read_codes, ref_codes, ref_irregular, min_flank, min_base_qual, gen_snps, gen_indels, max_per_read,
                         read_region, rec, count, status);
}

}  // namespace plat

PLAT_EXPORT int plat_ref_codes(plat_ctx* ctx, int n_regions, const uint8_t* ref_seq, const int64_t* ref_off, int64_t n_bytes, uint32_t* out_codes,
                               int32_t* out_irregular, void* stream)
{
    if (!ctx || n_regions < 0 || n_bytes < 0) return PLAT_ERR_INVALID;
    if (n_regions == 0 || n_bytes == 0) return PLAT_OK;
    if (!ref_seq || !ref_off || !out_codes || !out_irregular) return PLAT_ERR_INVALID;
    PLAT_HIP(ctx, hipSetDevice(ctx->device));
    PLAT_HIP(ctx, hipMemsetAsync(out_irregular, 0, (size_t)n_regions * sizeof(int32_t), (hipStream_t)stream));
    const long long nd = (n_bytes + 15) / 16;
    PLAT_HIP(ctx, hipMemsetAsync(out_codes + nd, 0, 8 * sizeof(uint32_t), (hipStream_t)stream));      // (the scan reads a 64-bit word past the last base)
    hipLaunchKernelGGL(plat::k_ref_codes, dim3((unsigned)((nd + 255) / 256)), dim3(256), 0, (hipStream_t)stream, ref_seq, ref_off, n_regions, (long long)n_bytes,
                       out_codes, out_irregular);
    PLAT_HIP(ctx, hipGetLastError());
    return PLAT_OK;
}

PLAT_EXPORT int plat_candidates_batch_codes(plat_ctx* ctx, const plat_candidate_batch* batch, const uint32_t* read_codes, const uint32_t* ref_codes,
                                            const int32_t* ref_irregular, int min_flank, int min_base_qual, int gen_snps, int gen_indels, int max_per_read,
                                            const int32_t* read_region, int32_t* out_rec, int32_t* out_count, int32_t* out_status, void* stream)
{
    if (!ctx || !batch || max_per_read < 1 || min_flank < 0 || !read_codes || !ref_codes || !ref_irregular) return PLAT_ERR_INVALID;
    if (((uintptr_t)read_codes & 7) || ((uintptr_t)ref_codes & 7)) return PLAT_ERR_INVALID;             // (read as 64-bit words)
    const plat_candidate_batch b = *batch;
    if (b.n_regions < 0 || b.n_reads < 0) return PLAT_ERR_INVALID;
    if (b.n_reads == 0) return PLAT_OK;
    if (!b.ref_seq || !b.ref_off || !b.ref_seq_start || !b.contig_len || !b.read_seq || !b.read_qual || !b.read_off ||
        !b.read_pos || !b.read_flags || !b.cigar || !b.cig_off || !read_region || !out_rec || !out_count || !out_status)
        return PLAT_ERR_INVALID;
    PLAT_HIP(ctx, hipSetDevice(ctx->device));
    PLAT_EV_TAB(ctx, 2, (hipStream_t)stream);
    PLAT_LAUNCH(ctx, PLAT_KT_CANDIDATES, stream, plat::k_candidates_codes, dim3((unsigned)((b.n_reads + 63) / 64)), dim3(64), 0, b, (const unsigned long long*)read_codes,
                         (const unsigned long long*)ref_codes, ref_irregular, min_flank, min_base_qual, gen_snps, gen_indels, max_per_read, read_region, out_rec, out_count,
                         out_status);
    PLAT_EV_TAB(ctx, 3, (hipStream_t)stream);
    ctx->ev_valid_cand = ctx->profile;
    PLAT_HIP(ctx, hipGetLastError());
    return PLAT_OK;
}

PLAT_EXPORT int plat_candidates_batch_packed(plat_ctx* ctx, const plat_candidate_batch* batch, const plat_packed_reads* packed, const uint32_t* read_codes,
                                             const uint32_t* ref_codes, const int32_t* ref_irregular, int min_flank, int min_base_qual, int gen_snps, int gen_indels,
                                             int max_per_read, const int32_t* read_region, int32_t* out_rec, int32_t* out_count, int32_t* out_status, void* stream)
{
    if (!ctx || !batch || !packed || max_per_read < 1 || min_flank < 0 || !read_codes || !ref_codes || !ref_irregular) return PLAT_ERR_INVALID;
    if (((uintptr_t)read_codes & 7) || ((uintptr_t)ref_codes & 7)) return PLAT_ERR_INVALID;             // (read as 64-bit words)
    const plat_candidate_batch b = *batch;
    const plat_packed_reads pk = *packed;
    if (b.n_regions < 0 || b.n_reads < 0 || pk.n_exc < 0) return PLAT_ERR_INVALID;
    if (b.n_reads == 0) return PLAT_OK;
    if (!b.ref_seq || !b.ref_off || !b.ref_seq_start || !b.contig_len || !b.read_seq || !b.read_off || !pk.read_src ||
        (pk.n_exc > 0 && (!pk.exc_index || !pk.exc_base || !pk.exc_qual)) ||
        !b.read_pos || !b.read_flags || !b.cigar || !b.cig_off || !read_region || !out_rec || !out_count || !out_status)
        return PLAT_ERR_INVALID;
    PLAT_HIP(ctx, hipSetDevice(ctx->device));
    PLAT_EV_TAB(ctx, 2, (hipStream_t)stream);
    PLAT_LAUNCH(ctx, PLAT_KT_CANDIDATES, stream, plat::k_candidates_packed, dim3((unsigned)((b.n_reads + 63) / 64)), dim3(64), 0, b, pk, (const unsigned long long*)read_codes,
                         (const unsigned long long*)ref_codes, ref_irregular, min_flank, min_base_qual, gen_snps, gen_indels, max_per_read, read_region, out_rec, out_count,
                         out_status);
    PLAT_EV_TAB(ctx, 3, (hipStream_t)stream);
    ctx->ev_valid_cand = ctx->profile;
    PLAT_HIP(ctx, hipGetLastError());
    return PLAT_OK;
}

PLAT_EXPORT int plat_candidates_batch(plat_ctx* ctx, const plat_candidate_batch* batch, int min_flank, int min_base_qual,
                                      int gen_snps, int gen_indels, int max_per_read, const int32_t* read_region,
                                      int32_t* out_rec, int32_t* out_count, int32_t* out_status, void* stream)
{
    if (!ctx || !batch || max_per_read < 1 || min_flank < 0) return PLAT_ERR_INVALID;
    const plat_candidate_batch b = *batch;
    if (b.n_regions < 0 || b.n_reads < 0) return PLAT_ERR_INVALID;
    if (b.n_reads == 0) return PLAT_OK;
    if (!b.ref_seq || !b.ref_off || !b.ref_seq_start || !b.contig_len || !b.read_seq || !b.read_qual || !b.read_off ||
        !b.read_pos || !b.read_flags || !b.cigar || !b.cig_off || !read_region || !out_rec || !out_count || !out_status)
        return PLAT_ERR_INVALID;
    PLAT_HIP(ctx, hipSetDevice(ctx->device));
    PLAT_EV_TAB(ctx, 2, (hipStream_t)stream);
    PLAT_LAUNCH(ctx, PLAT_KT_CANDIDATES, stream, plat::k_candidates, dim3((unsigned)((b.n_reads + 63) / 64)), dim3(64), 0, b,
                       min_flank, min_base_qual, gen_snps, gen_indels, max_per_read, read_region, out_rec, out_count, out_status);
    PLAT_EV_TAB(ctx, 3, (hipStream_t)stream);
    ctx->ev_valid_cand = ctx->profile;
    PLAT_HIP(ctx, hipGetLastError());
    return PLAT_OK;
}

// ------------------------------------------------------------------------------------------------
// The dictionary step behind the scan (VariantCandidateGenerator.addVariantToList, variant.pyx:499-527) and the per-sample support
// filter of generateVariantsInRegion (variantcaller.pyx:456-467) for every scan (= region x sample) of a candidate batch.
// k_candidates_merge: ONE WORKGROUP PER SCAN, the scan's hash table in LDS, four phases.
//   collect  the workgroup strides over the scan's reads (count[] and status[] coalesced, MERGE_READS loads in flight per thread) and
//            lists the ids of their records in a queue in LDS: a block scan over the counts gives every record its place, so a scan with
//            more records than the queue holds is worked off in rounds of MERGE_QUEUE records -- whatever its reads hold.
//   insert   threads stride over the queue, two records each per trip (the second record's loads are issued before the first is used):
//            slot = hash << 32 | id + 1 of the record with the smallest id among those of equal content (first occurrence: the reference's
//            dictionary order) + the number of reads showing it.  The hash beside the id means another record's words and bytes are
//            loaded only where it probably is the same one.
//   filter   the occupied slots, compacted in slot order; per distinct record the reads covering its position
//            (ReadArray.countReadsCoveringRegion, cwindow.pyx:176-206: both lower bounds bisected in lock-step, MERGE_LANES records of a
//            thread in flight together) and the support filter.
//   out      the counts, the status and the rep + 1 half of the scan's table (EVERY slot: what k_sb_variants' replay reads, so no memset
//            runs in front of this kernel).
// (Round 2 kept the table in LDS as well, but gave each thread twenty READS one after the other, each a chain of dependent loads: 140 us
//  for four scans.  Rounds 3-13 had the table in global memory, a thread per read and a second kernel, a thread per slot, for the filter.)
namespace plat {
constexpr int MERGE_SLOTS = 8192, MERGE_LIMIT = 6144;
constexpr int MERGE_THREADS = 1024;               // (1024 against 512: profiles/r14_merge_lds.md)
constexpr int MERGE_QUEUE = 8192;                 // record ids per round of collect + insert
constexpr int MERGE_READS = 4;                    // reads per thread and trip of the collect phase
constexpr int MERGE_LANES = 4;                    // distinct records of a thread whose searches run together in the filter phase
static_assert(MERGE_QUEUE >= MERGE_LIMIT, "the filter phase lists the occupied slots in the queue");
static_assert(MERGE_SLOTS % (4 * MERGE_THREADS) == 0, "a thread writes its slots of the table four at a time");

struct MergeLds {
    unsigned long long tab[MERGE_SLOTS];          // hash << 32 | rep + 1; 0 = empty
    int32_t cnt[MERGE_SLOTS];
    int32_t queue[MERGE_QUEUE];
    int32_t wsum[MERGE_THREADS / 64];
    int32_t distinct, full, bad, need, n_out, st_out;
};

__device__ __forceinline__ void merge_load(const int32_t* __restrict__ rec, int id, int32_t* w) {
    const int32_t* me = rec + 5ll * id;
#pragma unroll
    for (int i = 0; i < 5; ++i) w[i] = me[i];
}

// fr / fa: the first removed / added byte, loaded by the caller (together with another record's)
__device__ __forceinline__ unsigned merge_hash(const uint8_t* __restrict__ ref_seq, const uint8_t* __restrict__ read_seq, const int32_t* w, unsigned fr, unsigned fa) {
    unsigned h = (unsigned)w[0] * 2654435761u + (unsigned)w[1] * 40503u + (unsigned)w[2] * 97u;
    if (w[1] > 0) { h = h * 31u + fr; for (int i = 1; i < w[1]; ++i) h = h * 31u + ref_seq[(long long)w[3] + i]; }
    if (w[2] > 0) { h = h * 37u + fa; for (int i = 1; i < w[2]; ++i) h = h * 37u + read_seq[(long long)w[4] + i]; }
    return h;
}

__device__ __forceinline__ bool rec_same(const uint8_t* __restrict__ ref_seq, const uint8_t* __restrict__ read_seq, const int32_t* x, const int32_t* y) {
    if (x[0] != y[0] || x[1] != y[1] || x[2] != y[2]) return false;
    for (int i = 0; i < x[1]; ++i) if (ref_seq[(long long)x[3] + i] != ref_seq[(long long)y[3] + i]) return false;
    for (int i = 0; i < x[2]; ++i) if (read_seq[(long long)x[4] + i] != read_seq[(long long)y[4] + i]) return false;
    return true;
}

// record `id` (words w, hash h) into the table; -> 1 where it is the first of its content.  A probe that comes round (the table is full:
// MERGE_SLOTS > MERGE_LIMIT distinct records) raises L.full, and nothing more is inserted.
__device__ __forceinline__ int merge_probe(MergeLds& L, const uint8_t* __restrict__ ref_seq, const uint8_t* __restrict__ read_seq, const int32_t* __restrict__ rec,
                                           int id, const int32_t* w, unsigned h)
{
    if (__hip_atomic_load(&L.full, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) return 0;
    const unsigned long long mine = ((unsigned long long)h << 32) | (unsigned)(id + 1);
    unsigned sl = (h ^ (h >> 15)) & (MERGE_SLOTS - 1);
    for (int tries = 0; tries < MERGE_SLOTS; ++tries) {
        unsigned long long cur = __hip_atomic_load(&L.tab[sl], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (cur == 0ull) {
            cur = atomicCAS(&L.tab[sl], 0ull, mine);
            if (cur == 0ull) { atomicAdd(&L.cnt[sl], 1); return 1; }
        }
        if ((unsigned)(cur >> 32) == h) {
            int32_t o[5];
            merge_load(rec, (int)(unsigned)cur - 1, o);
            // (equal content = equal hash: the smaller of two such words is the one with the smaller id)
            if (rec_same(ref_seq, read_seq, o, w)) { atomicMin(&L.tab[sl], mine); atomicAdd(&L.cnt[sl], 1); return 0; }
        }
        sl = (sl + 1u) & (MERGE_SLOTS - 1);
    }
    __hip_atomic_store(&L.full, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    return 0;
}

// the first n ids of the queue into the table; -> the table has taken more than MERGE_LIMIT distinct records (the same for every thread).
// Ends behind a barrier: the queue may be written again.
__device__ __forceinline__ bool merge_insert(MergeLds& L, int n, bool full, const uint8_t* __restrict__ ref_seq, const uint8_t* __restrict__ read_seq,
                                             const int32_t* __restrict__ rec)
{
    int fresh = 0;
    for (int i = threadIdx.x; i < n && !full; i += 2 * MERGE_THREADS) {
        const bool two = i + MERGE_THREADS < n;
        const int ida = L.queue[i], idb = two ? L.queue[i + MERGE_THREADS] : ida;
        int32_t wa[5], wb[5];
        merge_load(rec, ida, wa);
        merge_load(rec, idb, wb);
        const unsigned fra = wa[1] > 0 ? ref_seq[(long long)wa[3]] : 0u, faa = wa[2] > 0 ? read_seq[(long long)wa[4]] : 0u;
        const unsigned frb = wb[1] > 0 ? ref_seq[(long long)wb[3]] : 0u, fab = wb[2] > 0 ? read_seq[(long long)wb[4]] : 0u;
        const unsigned ha = merge_hash(ref_seq, read_seq, wa, fra, faa), hb = merge_hash(ref_seq, read_seq, wb, frb, fab);
        fresh += merge_probe(L, ref_seq, read_seq, rec, ida, wa, ha);
        if (two) fresh += merge_probe(L, ref_seq, read_seq, rec, idb, wb, hb);
    }
    if (fresh) atomicAdd(&L.distinct, fresh);
    __syncthreads();
    return L.distinct > MERGE_LIMIT || L.full != 0;
}

__global__ void __launch_bounds__(MERGE_THREADS)
k_candidates_merge(const uint8_t* __restrict__ ref_seq, const uint8_t* __restrict__ read_seq, const int32_t* __restrict__ read_pos,
                   const int32_t* __restrict__ read_end, const int32_t* __restrict__ scan_read_begin, const int32_t* __restrict__ scan_longest,
                   int max_per_read, const int32_t* __restrict__ rec, const int32_t* __restrict__ count, const int32_t* __restrict__ status,
                   int32_t* __restrict__ mtab, double min_var_freq, int cap, int32_t* __restrict__ out_cand, int32_t* __restrict__ out_n)
{
    extern __shared__ __align__(16) unsigned char merge_lds[];
    MergeLds& L = *reinterpret_cast<MergeLds*>(merge_lds);
    const int g = blockIdx.x, tid = threadIdx.x;
    const int r0 = scan_read_begin[g], N = scan_read_begin[g + 1] - r0;
    for (int sl = tid; sl < MERGE_SLOTS; sl += MERGE_THREADS) { L.tab[sl] = 0ull; L.cnt[sl] = 0; }
    if (tid == 0) { L.distinct = 0; L.full = 0; L.bad = 0; L.need = 0; L.n_out = 0; L.st_out = 0; }
    __syncthreads();

    // ---- collect + insert.  The scan's records in the order (trip, thread, read of the thread, k): record number `base + off + ...`; the
    // queue holds the numbers [qstart, qstart + MERGE_QUEUE)
    int bad = 0, need = 0, base = 0, qstart = 0;
    bool full = false;
    for (int q0 = 0; q0 < N; q0 += MERGE_THREADS * MERGE_READS) {
        int c[MERGE_READS], st[MERGE_READS];
#pragma unroll
        for (int j = 0; j < MERGE_READS; ++j) {
            const int q = q0 + j * MERGE_THREADS + tid;
            c[j] = q < N ? count[r0 + q] : 0;
            st[j] = q < N ? status[r0 + q] : 0;
        }
        int mine = 0;
#pragma unroll
        for (int j = 0; j < MERGE_READS; ++j) {
            if (st[j] == PLAT_ERR_BAD_INPUT) bad = 1;
            if (c[j] > max_per_read) { need = c[j] > need ? c[j] : need; c[j] = 0; }      // more records than the read's slice holds: none of them is read
            if (c[j] < 0) c[j] = 0;
            mine += c[j];
        }
        int tot;
        const int off = block_excl_scan<MERGE_THREADS>(mine, L.wsum, tot);
        const int hi = base + tot;
        for (;;) {
            int at = base + off - qstart;
#pragma unroll
            for (int j = 0; j < MERGE_READS; ++j) {
                const int id0 = (r0 + q0 + j * MERGE_THREADS + tid) * max_per_read;
                for (int k = 0; k < c[j]; ++k, ++at) if (at >= 0 && at < MERGE_QUEUE) L.queue[at] = id0 + k;
            }
            if (hi - qstart <= MERGE_QUEUE) break;
            __syncthreads();
            full = merge_insert(L, MERGE_QUEUE, full, ref_seq, read_seq, rec);         // the queue is full and this trip has more
            qstart += MERGE_QUEUE;
        }
        base = hi;
    }
    __syncthreads();
    full = merge_insert(L, base - qstart, full, ref_seq, read_seq, rec);
    if (bad) L.bad = 1;
    if (need) atomicMax(&L.need, need);
    __syncthreads();

    // ---- out, for a scan that is refused: a read the scan refused | -(2^20 + needed records per read) | overflow of the table
    int4* gtab = reinterpret_cast<int4*>(mtab + (size_t)g * 2 * MERGE_SLOTS);         // (64 KB per scan in a hipMalloc'ed block)
    constexpr int SPT = MERGE_SLOTS / MERGE_THREADS;                                  // slots per thread: [tid * SPT, tid * SPT + SPT)
    const int f_bad = L.bad, f_need = L.need;
    if (f_bad || f_need > 0 || full) {
#pragma unroll
        for (int j = 0; j < SPT / 4; ++j) gtab[tid * (SPT / 4) + j] = make_int4(0, 0, 0, 0);
        if (tid == 0) { out_n[2 * g] = 0; out_n[2 * g + 1] = f_bad ? PLAT_ERR_BAD_INPUT : (f_need > 0 ? -(1 << 20) - f_need : PLAT_ERR_OVERFLOW); }
        return;
    }

    // ---- the table's rep + 1 half, every slot, and the occupied slots in slot order (into the queue)
    int32_t idp[SPT];
    int occ = 0;
#pragma unroll
    for (int j = 0; j < SPT; ++j) { idp[j] = (int32_t)(unsigned)L.tab[tid * SPT + j]; occ += idp[j] != 0; }
#pragma unroll
    for (int j = 0; j < SPT / 4; ++j) gtab[tid * (SPT / 4) + j] = make_int4(idp[4 * j], idp[4 * j + 1], idp[4 * j + 2], idp[4 * j + 3]);
    int n_occ;
    {
        int at = block_excl_scan<MERGE_THREADS>(occ, L.wsum, n_occ);
#pragma unroll
        for (int j = 0; j < SPT; ++j) if (idp[j] != 0) L.queue[at++] = tid * SPT + j;
    }
    __syncthreads();

    // ---- filter: per distinct record the reads covering its position (countReadsCoveringRegion(start, start + 1), cwindow.pyx:176-206) and
    // the per-sample support filter (variantcaller.pyx:456-467).  A record exists, so N > 0 and index 0 of the scan's reads can be read.
    const int32_t* pos = read_pos + r0;
    const int32_t* endp = read_end + r0;
    const int longest = scan_longest[g];
    for (int i0 = tid; i0 < n_occ; i0 += MERGE_THREADS * MERGE_LANES) {
        int id[MERGE_LANES], sup[MERGE_LANES], w[MERGE_LANES][5];
        bool on[MERGE_LANES];
#pragma unroll
        for (int k = 0; k < MERGE_LANES; ++k) {
            const int i = i0 + k * MERGE_THREADS;
            on[k] = i < n_occ;
            const int sl = L.queue[on[k] ? i : i0];
            id[k] = (int)(unsigned)L.tab[sl] - 1;
            sup[k] = L.cnt[sl];
            merge_load(rec, id[k], w[k]);
        }
        // the two lower bounds of every record, all in one loop: each search takes the steps it takes by itself, their loads travel together
        int lo1[MERGE_LANES], hi1[MERGE_LANES], lo2[MERGE_LANES], hi2[MERGE_LANES];
        long long key[MERGE_LANES];
#pragma unroll
        for (int k = 0; k < MERGE_LANES; ++k) {
            const int start = w[k][0];
            key[k] = (long long)start - longest > 1 ? (long long)start - longest : 1;
            lo1[k] = lo2[k] = 0;
            hi1[k] = hi2[k] = on[k] ? N : 0;
        }
        for (bool any = true; any;) {
            int p1[MERGE_LANES], p2[MERGE_LANES];
#pragma unroll
            for (int k = 0; k < MERGE_LANES; ++k) {
                p1[k] = pos[lo1[k] < hi1[k] ? (lo1[k] + hi1[k]) >> 1 : 0];
                p2[k] = pos[lo2[k] < hi2[k] ? (lo2[k] + hi2[k]) >> 1 : 0];
            }
            any = false;
#pragma unroll
            for (int k = 0; k < MERGE_LANES; ++k) {
                if (lo1[k] < hi1[k]) { const int mid = (lo1[k] + hi1[k]) >> 1; if ((long long)p1[k] < key[k]) lo1[k] = mid + 1; else hi1[k] = mid; }
                if (lo2[k] < hi2[k]) { const int mid = (lo2[k] + hi2[k]) >> 1; if (p2[k] < w[k][0] + 1) lo2[k] = mid + 1; else hi2[k] = mid; }
                any = any || lo1[k] < hi1[k] || lo2[k] < hi2[k];
            }
        }
        // the start pointer walks on over the reads that end at or before the site
        int s[MERGE_LANES];
        bool walk[MERGE_LANES];
#pragma unroll
        for (int k = 0; k < MERGE_LANES; ++k) { s[k] = lo1[k]; walk[k] = on[k]; }
        for (bool any = true; any;) {
            int e[MERGE_LANES];
#pragma unroll
            for (int k = 0; k < MERGE_LANES; ++k) e[k] = endp[walk[k] && s[k] < N ? s[k] : 0];
            any = false;
#pragma unroll
            for (int k = 0; k < MERGE_LANES; ++k) {
                walk[k] = walk[k] && s[k] < N && e[k] <= w[k][0];
                if (walk[k]) { ++s[k]; any = true; }
            }
        }
#pragma unroll
        for (int k = 0; k < MERGE_LANES; ++k) {
            if (!on[k]) continue;
            if (s[k] > lo2[k]) { L.st_out = PLAT_ERR_BAD_INPUT; continue; }             // "Read start pointer > read end pointer": the reference raises
            const int total = lo2[k] - s[k];
            const double frac = total == 0 ? 0.0 : (double)sup[k] / (double)total;
            if (frac >= min_var_freq || w[k][1] != w[k][2]) {
                const int at = atomicAdd(&L.n_out, 1);
                if (at < cap) {
                    int32_t* o = out_cand + 8ll * ((long long)g * cap + at);
                    o[0] = id[k]; o[1] = sup[k]; o[2] = total; o[3] = w[k][0]; o[4] = w[k][1]; o[5] = w[k][2]; o[6] = w[k][3]; o[7] = w[k][4];
                }
            }
        }
    }
    __syncthreads();
    if (tid == 0) {
        const int n = L.n_out;
        out_n[2 * g] = n;
        // (more candidates than the caller's room: its status says so, the count is the full one)
        out_n[2 * g + 1] = L.st_out != 0 ? L.st_out : (n > cap ? PLAT_ERR_OVERFLOW : 0);
    }
}
}  // namespace plat

PLAT_EXPORT int plat_candidates_merge_batch(plat_ctx* ctx, const plat_candidate_batch* batch, const int32_t* read_end, int n_scans,
                                            const int32_t* scan_read_begin, const int32_t* scan_longest, int max_per_read,
                                            const int32_t* rec, const int32_t* count, const int32_t* status, double min_var_freq,
                                            int cap_per_scan, int32_t* out_cand, int32_t* out_n, void* stream)
{
    if (!ctx || !batch || n_scans < 0 || max_per_read < 1 || cap_per_scan < 1) return PLAT_ERR_INVALID;
    if (n_scans == 0) return PLAT_OK;
    if (n_scans > PLAT_GRID_Y_MAX) return PLAT_ERR_OVERFLOW;       // (one scan = one region of a chunk; the merge table is per scan)
    const plat_candidate_batch b = *batch;
    if (!b.ref_seq || !b.read_seq || !b.read_pos || !read_end || !scan_read_begin || !scan_longest || !rec || !count || !status || !out_cand || !out_n)
        return PLAT_ERR_INVALID;
    PLAT_HIP(ctx, hipSetDevice(ctx->device));
    // the context's table: per scan rep + 1 [MERGE_SLOTS] (0 = empty), written in full by the kernel, then MERGE_SLOTS words and, behind
    // all scans, 4 words per scan that nothing reads any more (the size and the offsets are what plat_stage_b_batch knows)
    const size_t tab_bytes = ((size_t)n_scans * 2 * plat::MERGE_SLOTS + 4 * (size_t)n_scans) * sizeof(int32_t);
    int rcm = plat_reserve(ctx, ctx->merge_tab, tab_bytes);
    if (rcm) return rcm;
    int32_t* mtab = (int32_t*)ctx->merge_tab.ptr;
    if (!ctx->merge_attr_set) {                                     // (the attribute is per device: remembered per context, as k_sb_variants')
        PLAT_HIP(ctx, hipFuncSetAttribute((const void*)plat::k_candidates_merge, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(plat::MergeLds)));
        ctx->merge_attr_set = true;
    }
    PLAT_LAUNCH(ctx, PLAT_KT_CAND_MERGE, stream, plat::k_candidates_merge, dim3((unsigned)n_scans), dim3(plat::MERGE_THREADS), sizeof(plat::MergeLds), b.ref_seq, b.read_seq,
                         b.read_pos, read_end, scan_read_begin, scan_longest, max_per_read, rec, count, status, mtab, min_var_freq, cap_per_scan, out_cand, out_n);
    PLAT_HIP(ctx, hipGetLastError());
    return PLAT_OK;
}
