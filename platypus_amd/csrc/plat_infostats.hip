// plat_infostats.hip -- the read statistics of the VCF INFO field: the loop over a window's reads (k_variant_read_stats, on ASCII or packed
// reads) and the ABPV / SbPval / MMLQ loops on its counts (k_variant_info, with the log-factorial table of the host's libm).
#include "plat_internal.hpp"
#include "read_source.hpp"
#include <mutex>
#include <math.h>

// ------------------------------------------------------------------------------------------------
// Read statistics of the VCF INFO field: vcfINFO's loop over the reads of a window
// (vcfutils.pyx:1300-1390) with readOverlapsVariant (:901-913), readQualIsGoodVariantPosition (:917-943) and
// variantSupportedByRead (:961-1072).  One wave per variant; lanes over the reads of one sample at a time; every count is a
// ballot popcount, the MMLQ window minima are written in read order (prefix popcount).
namespace plat {

template <class R>
__device__ __forceinline__ bool qual_good_at(const R& rd, int rlen, int readPos, int vmin, int vmax) {
    int a = max(0, min(rlen, vmin - readPos)), e = max(0, min(rlen, vmax - readPos));
    for (int i = a; i < e; ++i) if ((int8_t)rd.qual(i) < 5) return false;
    return true;
}

template <class R>
__device__ __forceinline__ bool bytes_equal(const R& rd, int at, const uint8_t* b, int n) {
    for (int i = 0; i < n; ++i) if (rd.base(at + i) != b[i]) return false;
    return true;
}

template <class R>
__device__ __forceinline__ bool read_supports(const R& seq, int rlen, int readStart, const int16_t* ops, int ncig, int varPos,
                                              int nAdded, int nRemoved, const uint8_t* added, int exact)
{
    int refOffset = 0, readOffset = 0;
    for (int ci = 0; ci < ncig; ++ci) {
        const int flag = ops[2 * ci], length = ops[2 * ci + 1];
        if (flag == 1) {                                                     // insertion, :984-1003
            if (nAdded != nRemoved) {
                if (!exact) return true;
                if (nAdded - nRemoved == length && readOffset + nAdded <= rlen && bytes_equal(seq, readOffset, added, nAdded)) return true;
                return false;
            }
            readOffset += length;
        } else if (flag == 2) {                                              // deletion, :1005-1024
            if (nAdded != nRemoved) return exact ? (nRemoved - nAdded == length) : true;
            refOffset += length;
        } else if (flag == 0 || flag == 7 || flag == 8) {                    // M, =, X, :1027-1048
            const int start = varPos - readStart + readOffset - refOffset;
            if (refOffset + readStart <= varPos && refOffset + readStart + length > varPos && nAdded == nRemoved &&
                start >= 0 && start + nAdded <= rlen && bytes_equal(seq, start, added, nAdded))
                return true;
            readOffset += length;
            refOffset += length;
        } else if (flag == 3) {                                              // N: the reference advances both, :1051-1053
            readOffset += length;
            refOffset += length;
        } else if (flag == 4) {
            readOffset += length;
            if (ci == 0) refOffset += length;
        }
    }
    return false;
}

template <class S>
__device__ __forceinline__ void variant_read_stats_one(const plat_infostats_batch& b, const S& src, int bad_reads_window, int exact, int64_t* __restrict__ out,
                                                       int32_t* __restrict__ per_sample, int32_t* __restrict__ minq, int32_t* __restrict__ nminq)
{
    const int v = blockIdx.x, lane = threadIdx.x;
    const int w = b.var_window[v];
    const int vmin = b.var_bam_min[v], vmax = b.var_bam_max[v], varPos = b.var_pos[v];
    const int nAdded = b.var_n_added[v], nRemoved = b.var_n_removed[v];
    const uint8_t* added = b.var_added + b.var_added_off[v];
    int32_t* mq = minq + b.minq_off[v];
    long long c[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) c[k] = 0;
    int nmq = 0;
    const int half = (bad_reads_window - 1) / 2;
    for (int i = 0; i < b.n_ind; ++i) {
        const long long seg = (long long)w * b.n_ind + i;
        const bool inGt = b.var_in_genotype[(long long)v * b.n_ind + i] != 0;
        const int gb = b.good_begin[seg], ge = b.good_end[seg], bb = b.bad_begin[seg], be = b.bad_end[seg];
        c[13] += ge - gb; c[14] += be - bb;
        for (int r0 = bb; r0 < be; r0 += 64) {                               // bad reads: coverage and mapping quality only
            const int r = r0 + lane;
            bool hit = false; long long m2 = 0;
            if (r < be) {
                const int rlen = (int)(b.read_off[r + 1] - b.read_off[r]);
                hit = b.read_pos[r] <= vmax && b.read_end[r] > vmin &&
                      qual_good_at(src.read(r, b.read_off[r], rlen), rlen, b.read_pos[r], vmin, vmax);
                if (hit) m2 = (long long)b.read_mapq[r] * b.read_mapq[r];
            }
            c[1] += __popcll(__ballot(hit));
#pragma unroll
            for (int s = 32; s > 0; s >>= 1) m2 += __shfl_xor(m2, s);
            c[15] += m2;
        }
        int nReads = 0, nVarReads = 0;
        for (int r0 = gb; r0 < ge; r0 += 64) {
            const int r = r0 + lane;
            bool hit = false, rev = false, sup = false; long long m2 = 0; int wmin = 0;
            if (r < ge) {
                const long long so = b.read_off[r];
                const int rlen = (int)(b.read_off[r + 1] - so);
                const int rp = b.read_pos[r];
                if (rp <= vmax && b.read_end[r] > vmin) {
                    const auto rd = src.read(r, so, rlen);
                    hit = qual_good_at(rd, rlen, rp, vmin, vmax);
                    if (hit) {
                    rev = (b.read_flags[r] & 16) != 0;
                    m2 = (long long)b.read_mapq[r] * b.read_mapq[r];
                    sup = read_supports(rd, rlen, rp, b.cigar + 2ll * b.cig_off[r], b.cig_off[r + 1] - b.cig_off[r], varPos,
                                        nAdded, nRemoved, added, exact);
                    if (sup && inGt) {                                       // MMLQ window, :1372-1383
                        const int ws = max(0, vmin - rp - half), we = min(rlen, vmax - rp + half);
                        for (int k = ws; k < we; ++k) { const int qk = (int)(int8_t)rd.qual(k); wmin = (k == ws) ? qk : min(wmin, qk); }
                    }
                    }
                }
            }
            const unsigned long long mh = __ballot(hit), mr = __ballot(hit && rev), ms = __ballot(sup), msr = __ballot(sup && rev);
            const int nh = __popcll(mh), nhr = __popcll(mr), ns = __popcll(ms), nsr = __popcll(msr);
            nReads += nh; c[0] += nh; c[7] += nhr; c[8] += nh - nhr;
            c[2] += ns; nVarReads += ns; c[11] += nsr; c[12] += ns - nsr;
            if (inGt) {
                c[3] += nh; c[9] += nhr; c[10] += nh - nhr;
                c[4] += ns; c[5] += nsr; c[6] += ns - nsr;
                if (sup) mq[nmq + __popcll(ms & ((1ull << lane) - 1ull))] = wmin;
                nmq += ns;
            }
#pragma unroll
            for (int s = 32; s > 0; s >>= 1) m2 += __shfl_xor(m2, s);
            c[15] += m2;
        }
        if (lane == 0) {
            per_sample[((long long)v * b.n_ind + i) * 2] = nReads;
            per_sample[((long long)v * b.n_ind + i) * 2 + 1] = nVarReads;
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 16; ++k) out[16ll * v + k] = c[k];
        nminq[v] = nmq;
    }
}

__global__ void __launch_bounds__(64)
k_variant_read_stats(plat_infostats_batch b, int bad_reads_window, int exact, int64_t* __restrict__ out, int32_t* __restrict__ per_sample,
                     int32_t* __restrict__ minq, int32_t* __restrict__ nminq)
{
    variant_read_stats_one(b, SrcAscii{b.read_seq, b.read_qual}, bad_reads_window, exact, out, per_sample, minq, nminq);
}

// ... and on packed bytes at their source (plat_variant_read_stats_packed_batch)
__global__ void __launch_bounds__(64)
k_variant_read_stats_packed(plat_infostats_batch b, plat_packed_reads pk, int bad_reads_window, int exact, int64_t* __restrict__ out,
                            int32_t* __restrict__ per_sample, int32_t* __restrict__ minq, int32_t* __restrict__ nminq)
{
    variant_read_stats_one(b, SrcPacked{pk}, bad_reads_window, exact, out, per_sample, minq, nminq);
}

}  // namespace plat

PLAT_EXPORT int plat_variant_read_stats_batch(plat_ctx* ctx, const plat_infostats_batch* batch, int bad_reads_window,
                                              int count_only_exact_indel_matches, int64_t* out_counts, int32_t* out_per_sample,
                                              int32_t* out_minq, int32_t* out_nminq, void* stream)
{
    if (!ctx || !batch || bad_reads_window < 1) return PLAT_ERR_INVALID;
    const plat_infostats_batch b = *batch;
    if (b.n_vars < 0 || b.n_ind < 1) return PLAT_ERR_INVALID;
    if (b.n_vars == 0) return PLAT_OK;
    if (!b.var_window || !b.var_pos || !b.var_bam_min || !b.var_bam_max || !b.var_n_added || !b.var_n_removed || !b.var_added ||
        !b.var_added_off || !b.var_in_genotype || !b.minq_off || !b.good_begin || !b.good_end || !b.bad_begin || !b.bad_end ||
        !b.read_seq || !b.read_qual || !b.read_off || !b.read_pos || !b.read_end || !b.read_mapq || !b.read_flags || !b.cigar ||
        !b.cig_off || !out_counts || !out_per_sample || !out_minq || !out_nminq)
        return PLAT_ERR_INVALID;
    PLAT_HIP(ctx, hipSetDevice(ctx->device));
    PLAT_LAUNCH(ctx, PLAT_KT_VARIANT_READ_STATS, stream, plat::k_variant_read_stats, dim3(b.n_vars), dim3(64), 0, b, bad_reads_window,
                       count_only_exact_indel_matches, out_counts, out_per_sample, out_minq, out_nminq);
    PLAT_HIP(ctx, hipGetLastError());
    return PLAT_OK;
}

PLAT_EXPORT int plat_variant_read_stats_packed_batch(plat_ctx* ctx, const plat_infostats_batch* batch, const plat_packed_reads* packed, int bad_reads_window,
                                                     int count_only_exact_indel_matches, int64_t* out_counts, int32_t* out_per_sample,
                                                     int32_t* out_minq, int32_t* out_nminq, void* stream)
{
    if (!ctx || !batch || !packed || bad_reads_window < 1) return PLAT_ERR_INVALID;
    const plat_infostats_batch b = *batch;
    const plat_packed_reads pk = *packed;
    if (b.n_vars < 0 || b.n_ind < 1 || pk.n_exc < 0) return PLAT_ERR_INVALID;
    if (b.n_vars == 0) return PLAT_OK;
    if (!b.var_window || !b.var_pos || !b.var_bam_min || !b.var_bam_max || !b.var_n_added || !b.var_n_removed || !b.var_added ||
        !b.var_added_off || !b.var_in_genotype || !b.minq_off || !b.good_begin || !b.good_end || !b.bad_begin || !b.bad_end ||
        !pk.read_src || (pk.n_exc > 0 && (!pk.exc_index || !pk.exc_base || !pk.exc_qual)) || !b.read_off || !b.read_pos || !b.read_end ||
        !b.read_mapq || !b.read_flags || !b.cigar || !b.cig_off || !out_counts || !out_per_sample || !out_minq || !out_nminq)
        return PLAT_ERR_INVALID;
    PLAT_HIP(ctx, hipSetDevice(ctx->device));
    PLAT_LAUNCH(ctx, PLAT_KT_VARIANT_READ_STATS, stream, plat::k_variant_read_stats_packed, dim3(b.n_vars), dim3(64), 0, b, pk,
                       bad_reads_window, count_only_exact_indel_matches, out_counts, out_per_sample, out_minq, out_nminq);
    PLAT_HIP(ctx, hipGetLastError());
    return PLAT_OK;
}

// ---- the loops of INFO ABPV / SbPval / MMLQ on the device (plat_variant_info_batch) -----------------------------------------------------
namespace plat {
constexpr int LOGFACT_N = 4096;
// betaBinomialCDF(k, n, alpha, beta) as its three terms (platypusutils.pyx:267-315): t[1] = logBeta(beta + n - k - 1, alpha + k + 1),
// t[2] = threeFTwo(k, n, alpha, beta), t[3] = logBeta(alpha, beta) + logBeta(n - k, k + 2) + log(n + 1).  Returns the state word: 1, or 2
// when a log-factorial lies beyond the table.  (k == n is the caller's: the function returns 1.0 there.)
__device__ __forceinline__ double cdf_terms(long long k, long long n, long long alpha, long long beta, const double* __restrict__ LF, double* t)
{
    const double* LOGI = LF + LOGFACT_N;                                  // LOGI[m - 1] = log((double)m), m = 1 .. 4096
    auto in = [](long long x) { return x >= 0 && x < LOGFACT_N; };
    const long long x1 = beta + n - k - 1, y1 = alpha + k + 1, x3 = n - k, y3 = k + 2;
    if (!in(x1 - 1) || !in(y1 - 1) || !in(x1 + y1 - 1) || !in(alpha - 1) || !in(beta - 1) || !in(alpha + beta - 1) || !in(x3 - 1) || !in(y3 - 1) ||
        !in(x3 + y3 - 1) || n + 1 < 1 || n + 1 > LOGFACT_N)
        return 2.0;
    auto logBeta = [&](long long x, long long y) { return (LF[x - 1] + LF[y - 1]) - LF[x + y - 1]; };
    const double a_2 = (double)alpha + (double)k + 1.0, a_3 = (double)k - (double)n + 1.0, b_1 = (double)k + 2.0,
                 b_2 = -(double)beta - (double)n + (double)k + 2.0;
    double theSum = 1.0, lastTerm = 1.0;
    const long long m = k - n + 1 < 0 ? -(k - n + 1) : k - n + 1;
    for (long long i = 1; i <= m; ++i) {
        const double di = (double)i;
        const double newTerm = lastTerm * (a_2 + di - 1) * (a_3 + di - 1) / ((b_1 + di - 1) * (b_2 + di - 1));
        theSum += newTerm;
        lastTerm = newTerm;
    }
    t[1] = logBeta(x1, y1);
    t[2] = theSum;
    t[3] = logBeta(alpha, beta) + logBeta(x3, y3) + LOGI[n];              // log((double)(n + 1))
    return 1.0;
}

// one wave per variant: lane 0 the two p-values' terms, the wave the median
__global__ void __launch_bounds__(64)
k_variant_info(int n_vars, const int64_t* __restrict__ counts, const int64_t* __restrict__ minq_off, const int32_t* __restrict__ minq,
               const int32_t* __restrict__ n_minq, const double* __restrict__ LF, double* __restrict__ out_terms, int32_t* __restrict__ out_mmlq)
{
    const int v = blockIdx.x, lane = threadIdx.x;
    if (v >= n_vars) return;
    const int64_t* c = counts + 16ll * v;
    if (lane == 0) {
        double* t = out_terms + 8ll * v;
        // computeAlleleBiasPValue(totalReads = TC_ab, variantReads = TR_ab), vcfutils.pyx:1156-1173
        const long long total = c[3], var = c[4];
        t[0] = 0.0; t[1] = 1.0; t[2] = 0.0; t[3] = 0.0;
        if (!(total > 0 && (double)var / (double)total >= 0.5) && total != 0) {
            if (var == total) { t[1] = 0.0; }                            // betaBinomialCDF == 1.0: min(1.0, 0.0)
            else t[0] = cdf_terms(var, total, 20, 20, LF, t);
        }
        // computeStrandBiasPValue(nFwdReads = TCF_sb, nRevReads = TCR_sb, nFwdVarReads = NF_sb, nRevVarReads = NR_sb), :1177-1222
        double* u = t + 4;
        const long long nF = c[10], nR = c[9], vF = c[6], vR = c[5];
        u[0] = 0.0; u[1] = 1.0; u[2] = 0.0; u[3] = 0.0;
        if (!(nF == 0 || nR == 0) && nF + nR > 0 && vF + vR > 0) {
            const bool useForward = !(nF < nR);
            const double freq = (double)(useForward ? nF : nR) / (double)(nF + nR);
            long long alpha, beta;
            if (freq < 0.5) { alpha = 20; beta = (long long)((double)alpha / freq - (double)alpha); }
            else if (freq > 0.5) { beta = 20; alpha = (long long)((double)beta * freq / (1.0 - freq)); }
            else alpha = beta = 20;
            const long long k = useForward ? vF : vR, n = vF + vR;
            if (k == n) u[1] = 1.0;                                      // betaBinomialCDF's own early exit
            else u[0] = cdf_terms(k, n, alpha, beta, LF, u);
        }
    }
    // sorted(values)[n // 2]: the element with n // 2 smaller-or-earlier-equal ones in front of it
    const int n = n_minq[v];
    const int32_t* q = minq + minq_off[v];
    int med = 100;
    for (int i0 = 0; i0 < n; i0 += 64) {
        const int i = i0 + lane;
        const int mine = i < n ? q[i] : 0;
        int rank = 0;
        for (int j = 0; j < n; ++j) { const int o = q[j]; rank += (o < mine) || (o == mine && j < i); }
        const unsigned long long hit = __ballot(i < n && rank == n / 2);
        if (hit) med = __shfl(mine, (int)__builtin_ctzll(hit), 64);
    }
    if (lane == 0) out_mmlq[v] = med;
}
}  // namespace plat

PLAT_EXPORT int plat_variant_info_batch(plat_ctx* ctx, int n_vars, const int64_t* counts, const int64_t* minq_off, const int32_t* minq,
                                        const int32_t* n_minq, double* out_terms, int32_t* out_mmlq, void* stream)
{
    if (!ctx || n_vars < 0) return PLAT_ERR_INVALID;
    if (n_vars == 0) return PLAT_OK;
    if (!counts || !minq_off || !minq || !n_minq || !out_terms || !out_mmlq) return PLAT_ERR_INVALID;
    PLAT_HIP(ctx, hipSetDevice(ctx->device));
    if (!ctx->d_logfact) {
        // logFactorial as the reference computes it (platypusutils.pyx:178-191: a sum of logs below 15, Stirling's series with pow() above) and
        // log(m), both with the HOST's libm: the device adds table entries, it never calls a transcendental function for these fields
        static double lut[2 * plat::LOGFACT_N];
        static bool made = false;
        static std::mutex mk;
        {
            std::lock_guard<std::mutex> g(mk);
            if (!made) {
                for (int x = 0; x < plat::LOGFACT_N; ++x) {
                    double ans = 0.0;
                    if (x < 15) for (int i = 1; i <= x; ++i) ans += log((double)i);
                    else {
                        const double y = (double)x;
                        ans = (y * log(y) + log(2.0 * M_PI * y) / 2 - y + (pow(y, -1)) / 12 - (pow(y, -3)) / 360 + (pow(y, -5)) / 1260 - (pow(y, -7)) / 1680 + (pow(y, -9)) / 1188);
                    }
                    lut[x] = ans;
                    lut[plat::LOGFACT_N + x] = log((double)(x + 1));
                }
                made = true;
            }
        }
        PLAT_HIP(ctx, hipMalloc(&ctx->d_logfact, sizeof(lut)));
        PLAT_HIP(ctx, hipMemcpy(ctx->d_logfact, lut, sizeof(lut), hipMemcpyHostToDevice));
    }
    PLAT_LAUNCH(ctx, PLAT_KT_VARIANT_INFO, stream, plat::k_variant_info, dim3((unsigned)n_vars), dim3(64), 0, n_vars, counts, minq_off, minq, n_minq,
                       (const double*)ctx->d_logfact, out_terms, out_mmlq);
    PLAT_HIP(ctx, hipGetLastError());
    return PLAT_OK;
}
