// plat_readbuf.hip -- the read buffers of fetched streams (plat_read_buffers_batch, include/platypus_mi355x.h):
// checkAndTrimRead (k_read_qc, below) in place, then bamReadBuffer.addReadToBuffer's split into `reads` / `badReads`
// (cwindow.pyx:560-595) as a stable per-stream partition, then, optionally, the two buffers gathered into device tables.
// plat_read_buffers_packed_batch: the same for PLAT_READS_PACKED tables (k_read_qc_packed, then the same split and a gather of the packed
// bytes).
#include "plat_internal.hpp"
#include "wave_tiles.hpp"

// ------------------------------------------------------------------------------------------------
// Read QC / trimming: checkAndTrimRead (cwindow.pyx:332-481).  One lane per read; `theLastRead` of
// bamReadBuffer.addReadToBuffer (:560-595) is simply the previous read of the same stream and only its position, length
// and mate position are looked at, so the reads of a stream are independent of each other.
namespace plat {

// The qualities of one read as checkAndTrimRead sees them: get(i) (a signed char, as the reference's `char*`) and trim(i) (quality 0).
// ASCII tables: the raw phred bytes.
struct QualBytes {
    int8_t* q;
    __device__ __forceinline__ int get(int i) const { return q[i]; }
    __device__ __forceinline__ void trim(int i) const { q[i] = 0; }
};

// PLAT_READS_PACKED tables: the quality bits of the packed byte, or the exception's quality where the byte is listed.  e0 / e1: the
// read's exceptions (exc_index[e0, e1) lie inside the read's bytes); a read without exceptions never touches the exception arrays.
struct QualPacked {
    uint8_t* p;                       // the read's first byte
    int64_t at;                       // its index in the blob
    const int64_t* idx;
    uint8_t* eq;
    int64_t e0, e1;
    __device__ __forceinline__ int64_t find(int i) const {
        if (e0 == e1) return -1;
        int64_t lo = e0, hi = e1;
        while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (idx[mid] < at + i) lo = mid + 1; else hi = mid; }
        return lo < e1 && idx[lo] == at + i ? lo : -1;
    }
    __device__ __forceinline__ int get(int i) const { const int64_t k = find(i); return k >= 0 ? (int)(int8_t)eq[k] : (int)(p[i] >> 2); }
    __device__ __forceinline__ void trim(int i) const { p[i] &= 3; const int64_t k = find(i); if (k >= 0) eq[k] = 0; }
};

// ... and a read of such a table without exceptions (most of them): the quality bits only, loops as tight as QualBytes'
struct QualPackedPlain {
    uint8_t* p;
    __device__ __forceinline__ int get(int i) const { return p[i] >> 2; }
    __device__ __forceinline__ void trim(int i) const { p[i] &= 3; }
};

// checkAndTrimRead on read r over either storage: the one copy of the verdicts and the trimming
template <class Q>
__device__ __forceinline__ void read_qc_one(const plat_readqc_batch& b, const plat_readqc_options& o, int r, const Q& q, int32_t* __restrict__ ok,
                                            int32_t* __restrict__ reason)
{
    const int rlen = (int)(b.read_off[r + 1] - b.read_off[r]);
    const int f = b.read_flags[r];
    const bool paired = f & 1, proper = f & 2, unmapped = f & 4, mateUnmapped = f & 8, reverse = f & 16, mateReverse = f & 32;
    const int ins = b.insert_size[r];
    const int absIns = ins < 0 ? -ins : ins;
    int why = -1, qcfail = 1;
    if (f & 256) why = 7;                                                            // secondary alignment, :337-339
    else if ((int)b.read_mapq[r] < o.min_map_qual) why = 6;                          // :341-344
    else {
        int nBelow = 0;
        for (int i = 0; i < rlen; ++i) nBelow += q.get(i) < o.min_base_qual;
        if (rlen - nBelow < o.min_good_qual_bases) why = 0;                          // :354-357
        else if (unmapped) why = 1;                                                  // :360-363
        else if (o.filter_mate_unmapped && paired && mateUnmapped) { why = 2; qcfail = 0; }          // :367-371 (no QCFail flag)
        else if (o.filter_mate_distant && paired && (b.chrom_id[r] != b.mate_chrom_id[r] || !proper)) { why = 3; qcfail = 0; }
        else if (o.filter_small_insert && paired && ins != 0 && absIns < rlen) why = 4;
        else if (o.filter_duplicates) {                                              // :389-409
            if (f & 1024) why = 5;
            else if (r > 0 && b.stream_of[r - 1] == b.stream_of[r] && b.read_pos[r] == b.read_pos[r - 1] &&
                     rlen == (int)(b.read_off[r] - b.read_off[r - 1])) {
                if (!paired || b.mate_pos[r - 1] == b.mate_pos[r]) why = 5;
            }
        }
    }
    if (why >= 0) {
        if (qcfail) b.read_flags[r] = f | 512;
        ok[r] = 0; reason[r] = why;
        return;
    }
    if (!reverse) {                                                                  // low-quality tail, :415-421
        for (int i = 1; i <= rlen; ++i) {
            if (i < o.trim_read_flank || q.get(rlen - i) < 5) q.trim(rlen - i); else break;
        }
    } else {
        for (int i = 0; i < rlen; ++i) {
            if (i < o.trim_read_flank || q.get(i) < 5) q.trim(i); else break;
        }
    }
    if (o.trim_overlapping == 1 && paired && absIns > 0 && !reverse && mateReverse && absIns < 2 * rlen) {   // :438-440
        int lim = (2 * rlen - ins) + 1;
        if (lim > rlen) lim = rlen;
        for (int i = 1; i <= lim; ++i) q.trim(rlen - i);
    }
    if (o.trim_adapter == 1 && paired && absIns > 0 && absIns < rlen) {               // :445-452
        if (reverse) { for (int i = 1; i < rlen - absIns + 1; ++i) q.trim(rlen - i); }
        else { for (int i = absIns; i < rlen; ++i) q.trim(i); }
    }
    if (o.trim_soft_clipped == 1) {                                                   // :462-479 (only M and I advance the cursor)
        int index = 0;
        for (int c = b.cig_off[r]; c < b.cig_off[r + 1]; ++c) {
            const int op = b.cigar[2 * c], len = b.cigar[2 * c + 1];
            if (op == 0 || op == 1) index += len;
            else if (op == 4) for (int j = 0; j < len && index < rlen; ++j) q.trim(index++);
        }
    }
    ok[r] = 1; reason[r] = -1;
}

__global__ void __launch_bounds__(64)
k_read_qc(plat_readqc_batch b, plat_readqc_options o, int32_t* __restrict__ ok, int32_t* __restrict__ reason)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= b.n_reads) return;
    read_qc_one(b, o, r, QualBytes{(int8_t*)b.read_qual + b.read_off[r]}, ok, reason);
}

// The same on PLAT_READS_PACKED bytes: the read's exceptions by two lower bounds of its byte range in exc_index
__global__ void __launch_bounds__(64)
k_read_qc_packed(plat_readqc_batch b, plat_readqc_options o, uint8_t* __restrict__ packed, int64_t n_exc, const int64_t* __restrict__ exc_index,
                 uint8_t* __restrict__ exc_qual, int32_t* __restrict__ ok, int32_t* __restrict__ reason)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= b.n_reads) return;
    const int64_t a = b.read_off[r], z = b.read_off[r + 1];
    int64_t e0 = 0, e1 = 0;
    if (n_exc > 0) {
        int64_t lo = 0, hi = n_exc;
        while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (exc_index[mid] < a) lo = mid + 1; else hi = mid; }
        e0 = lo; hi = n_exc;
        while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (exc_index[mid] < z) lo = mid + 1; else hi = mid; }
        e1 = lo;
    }
    if (e0 == e1) read_qc_one(b, o, r, QualPackedPlain{packed + a}, ok, reason);
    else read_qc_one(b, o, r, QualPacked{packed + a, a, exc_index, exc_qual, e0, e1}, ok, reason);
}

}  // namespace plat

PLAT_EXPORT int plat_read_qc_batch(plat_ctx* ctx, const plat_readqc_batch* batch, const plat_readqc_options* options,
                                   int32_t* out_ok, int32_t* out_reason, void* stream)
{
    if (!ctx || !batch || !options) return PLAT_ERR_INVALID;
    const plat_readqc_batch b = *batch;
    if (b.n_reads < 0) return PLAT_ERR_INVALID;
    if (b.n_reads == 0) return PLAT_OK;
    if (!b.read_qual || !b.read_off || !b.read_pos || !b.read_mapq || !b.read_flags || !b.chrom_id || !b.mate_chrom_id ||
        !b.insert_size || !b.mate_pos || !b.cigar || !b.cig_off || !b.stream_of || !out_ok || !out_reason)
        return PLAT_ERR_INVALID;
    PLAT_HIP(ctx, hipSetDevice(ctx->device));
    PLAT_LAUNCH(ctx, PLAT_KT_READ_QC, stream, plat::k_read_qc, dim3((unsigned)((b.n_reads + 63) / 64)), dim3(64), 0, b, *options,
                       out_ok, out_reason);
    PLAT_HIP(ctx, hipGetLastError());
    return PLAT_OK;
}

// (plat_read_buffers_packed_batch: the packed table's checkAndTrimRead; arguments checked there)
static int plat_read_qc_packed_launch(plat_ctx* ctx, const plat_read_buffers_packed_in& in, const plat_readqc_options& options, int32_t* out_ok,
                               int32_t* out_reason, hipStream_t stream)
{
    const plat_readqc_batch& b = in.qc;
    if (b.n_reads == 0) return PLAT_OK;
    PLAT_LAUNCH(ctx, PLAT_KT_READ_QC, stream, plat::k_read_qc_packed, dim3((unsigned)((b.n_reads + 63) / 64)), dim3(64), 0, b, options,
                       in.read_packed, in.n_exc, in.exc_index, in.exc_qual, out_ok, out_reason);
    PLAT_HIP(ctx, hipGetLastError());
    return PLAT_OK;
}

// ------------------------------------------------------------------------------------------------
// The split of the verdicts into `reads` / `badReads` and the gather of the two buffers.
namespace plat {
constexpr int SPLIT_THREADS = 512;                       // 8 waves per stream
constexpr int SPLIT_WAVES = SPLIT_THREADS / 64;
constexpr int SPLIT_MASKS = 4096;                        // verdict masks kept in LDS (32 KB): streams up to 256 k reads are read once

// One workgroup per stream.  Pass 1 walks the verdicts once in tiles of 512 reads: per wave a ballot of out_ok (kept in LDS), popcounts
// of the 8 reasons, and the sortedness test against the previous read.  Pass 2 walks the ballots (LDS; re-taken from out_ok only past
// SPLIT_MASKS tiles' worth) and places every read: its rank among the accepted (or the rejected) reads of the stream = the counts of the
// tiles before + of the waves before (LDS) + the popcount of its wave's ballot below its lane.  With tables, the same prefix sums over
// the reads' byte lengths and CIGAR pair counts give each read's offsets inside its buffer.
__global__ void __launch_bounds__(SPLIT_THREADS)
k_read_split(int n_reads, const int32_t* __restrict__ stream_begin, const int32_t* __restrict__ ok, const int32_t* __restrict__ reason,
             const int32_t* __restrict__ pos, const int64_t* __restrict__ read_off, const int32_t* __restrict__ cig_off,
             int32_t* __restrict__ perm, int32_t* __restrict__ counts, int64_t* __restrict__ t_off, int32_t* __restrict__ t_cigoff)
{
    __shared__ unsigned long long s_mask[SPLIT_MASKS];
    __shared__ int s_hist[8], s_good, s_unsorted;
    __shared__ long long s_wave[SPLIT_WAVES][6];
    const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = stream_begin[s], n = stream_begin[s + 1] - b;
    if (b < 0 || n < 0 || (long long)b + n > n_reads || (s == 0 && b != 0)) {      // not a partition of the table: nothing of the stream is written
        if (tid == 0) counts[10 * s] = -1;
        return;
    }
    if (tid < 8) s_hist[tid] = 0;
    if (tid == 0) { s_good = 0; s_unsorted = 0; }
    __syncthreads();
    // pass 1
    int good = 0, hist[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    bool unsorted = false;
    for (int t0 = 0; t0 < n; t0 += SPLIT_THREADS) {
        const int i = t0 + tid;
        const bool in = i < n;
        const bool g = in && ok[b + i] != 0;
        const int why = in ? reason[b + i] : -1;
        if (in && i > 0 && pos[b + i] < pos[b + i - 1]) unsorted = true;
        const unsigned long long m = __ballot(g);
        const int tile = t0 / SPLIT_THREADS;
        if (lane == 0 && tile * SPLIT_WAVES + wave < SPLIT_MASKS) s_mask[tile * SPLIT_WAVES + wave] = m;
        good += __popcll(m);
        for (int k = 0; k < 8; ++k) hist[k] += __popcll(__ballot(why == k));
    }
    if (lane == 0) {
        atomicAdd(&s_good, good);
        for (int k = 0; k < 8; ++k) if (hist[k]) atomicAdd(&s_hist[k], hist[k]);
    }
    if (unsorted) s_unsorted = 1;
    __syncthreads();
    const int nGood = s_good;
    if (tid < 8) counts[10 * s + 2 + tid] = s_hist[tid];
    if (tid == 0) { counts[10 * s] = nGood; counts[10 * s + 1] = s_unsorted; }
    // pass 2
    const bool tables = t_off != nullptr;
    const long long offBase = (long long)b + 2ll * s;                 // the stream's two offset tables
    long long run[6] = {0, 0, 0, 0, 0, 0};                            // good, bad, good bytes, bad bytes, good pairs, bad pairs placed so far
    const unsigned long long below = lane ? (~0ull >> (64 - lane)) : 0ull;
    for (int t0 = 0; t0 < n; t0 += SPLIT_THREADS) {
        const int i = t0 + tid, tile = t0 / SPLIT_THREADS;
        const bool in = i < n;
        const unsigned long long vmask = __ballot(in);
        const unsigned long long m = tile * SPLIT_WAVES + wave < SPLIT_MASKS ? s_mask[tile * SPLIT_WAVES + wave] : __ballot(in && ok[b + i] != 0);
        const bool g = (m >> lane) & 1ull;
        long long v[6];
        v[0] = __popcll(m & below); v[1] = __popcll(~m & vmask & below);
        v[2] = v[3] = v[4] = v[5] = 0;
        long long len = 0, pairs = 0;
        if (tables) {
            if (in) { len = read_off[b + i + 1] - read_off[b + i]; pairs = cig_off[b + i + 1] - cig_off[b + i]; }
            const long long sl = wave_incl_scan(g ? len : 0, lane), bl = wave_incl_scan(in && !g ? len : 0, lane);
            const long long sp = wave_incl_scan(g ? pairs : 0, lane), bp = wave_incl_scan(in && !g ? pairs : 0, lane);
            v[2] = sl - (g ? len : 0); v[3] = bl - (in && !g ? len : 0); v[4] = sp - (g ? pairs : 0); v[5] = bp - (in && !g ? pairs : 0);
            if (lane == 63) { s_wave[wave][2] = sl; s_wave[wave][3] = bl; s_wave[wave][4] = sp; s_wave[wave][5] = bp; }
        }
        if (lane == 0) { s_wave[wave][0] = __popcll(m); s_wave[wave][1] = __popcll(~m & vmask); }
        __syncthreads();
        long long before[6] = {run[0], run[1], run[2], run[3], run[4], run[5]};
        for (int w = 0; w < wave; ++w) for (int k = 0; k < 6; ++k) before[k] += s_wave[w][k];
        if (in) {
            const long long rank = g ? before[0] + v[0] : before[1] + v[1];
            perm[b + (g ? rank : nGood + rank)] = b + i;
            if (tables) {
                const long long at = offBase + (g ? rank : nGood + 1 + rank);
                t_off[at] = g ? before[2] + v[2] : before[3] + v[3];
                t_cigoff[at] = (int32_t)(g ? before[4] + v[4] : before[5] + v[5]);
            }
        }
        for (int w = 0; w < SPLIT_WAVES; ++w) for (int k = 0; k < 6; ++k) run[k] += s_wave[w][k];
        __syncthreads();                                              // (s_wave is rewritten by the next tile)
    }
    if (tables && tid == 0) {                                         // the closing entries: each buffer's bytes and pairs
        t_off[offBase + nGood] = run[2]; t_cigoff[offBase + nGood] = (int32_t)run[4];
        t_off[offBase + n + 1] = run[3]; t_cigoff[offBase + n + 1] = (int32_t)run[5];
    }
}

// One wave per place of the split: lane 0 the read's scalars, the lanes its bases, qualities and CIGAR pairs.  QUAL = false: a packed
// table (bases and qualities in one byte; t.qual is not written)
template <bool QUAL>
__global__ void __launch_bounds__(256)
k_read_gather(int n_reads, int n_streams, const int32_t* __restrict__ stream_begin, plat_readqc_batch q, const uint8_t* __restrict__ seq,
              const int32_t* __restrict__ end, const int32_t* __restrict__ perm, const int32_t* __restrict__ counts, plat_read_buffers_tables t)
{
    const int place = (int)((blockIdx.x * (long long)blockDim.x + threadIdx.x) >> 6), lane = threadIdx.x & 63;
    if (place >= n_reads) return;
    const int src = perm[place];
    if (src < 0 || src >= n_reads) return;
    const int s = q.stream_of[src];
    if (s < 0 || s >= n_streams) return;
    const int b = stream_begin[s], n = stream_begin[s + 1] - b, nGood = counts[10 * s], k = place - b;
    if (nGood < 0 || nGood > n || k < 0 || k >= n || src < b || src >= b + n) return;        // (a stream_of that does not match stream_begin)
    const bool g = k < nGood;
    const long long offBase = (long long)b + 2ll * s;
    const long long at = offBase + (g ? k : k + 1);
    const long long byte = q.read_off[b] + (g ? 0 : t.off[offBase + nGood]) + t.off[at];
    const long long pair = (long long)q.cig_off[b] + (g ? 0 : t.cig_off[offBase + nGood]) + t.cig_off[at];
    const long long from = q.read_off[src], len = q.read_off[src + 1] - from;
    const int c0 = q.cig_off[src], nc = q.cig_off[src + 1] - c0;
    if (byte < 0 || byte + len > q.read_off[n_reads] || pair < 0 || pair + nc > q.cig_off[n_reads]) return;
    for (long long j = lane; j < len; j += 64) {
        t.seq[byte + j] = seq[from + j];
        if (QUAL) t.qual[byte + j] = q.read_qual[from + j];
    }
    for (int j = lane; j < 2 * nc; j += 64) t.cigar[2 * pair + j] = q.cigar[2ll * c0 + j];
    if (lane == 0) {
        t.pos[place] = q.read_pos[src]; t.end[place] = end[src]; t.mapq[place] = q.read_mapq[src];
        t.flags[place] = q.read_flags[src]; t.mate_pos[place] = q.mate_pos[src];
    }
}
}  // namespace plat

namespace {
// the split of every stream and, with tables, the gather: shared by both entry points (the verdicts are in out_ok / out_reason)
template <bool QUAL>
int split_and_gather(plat_ctx* ctx, const plat_readqc_batch& q, int n_streams, const int32_t* stream_begin, const uint8_t* seq, const int32_t* end,
                     const int32_t* out_ok, const int32_t* out_reason, int32_t* out_perm, int32_t* out_counts, const plat_read_buffers_tables* tab,
                     bool tables, hipStream_t st)
{
    PLAT_LAUNCH(ctx, PLAT_KT_OTHER, st, plat::k_read_split, dim3((unsigned)n_streams), dim3(plat::SPLIT_THREADS), 0, q.n_reads, stream_begin,
                out_ok, out_reason, q.read_pos, tables ? q.read_off : nullptr, tables ? q.cig_off : nullptr, out_perm, out_counts,
                tables ? tab->off : nullptr, tables ? tab->cig_off : nullptr);
    if (tables && q.n_reads > 0) {
        const unsigned blocks = (unsigned)(((long long)q.n_reads + 3) / 4);
        PLAT_LAUNCH(ctx, PLAT_KT_OTHER, st, plat::k_read_gather<QUAL>, dim3(blocks), dim3(256), 0, q.n_reads, n_streams, stream_begin, q,
                    seq, end, out_perm, out_counts, *tab);
    }
    PLAT_HIP(ctx, hipGetLastError());
    return PLAT_OK;
}
}  // namespace

PLAT_EXPORT int plat_read_buffers_batch(plat_ctx* ctx, const plat_read_buffers_in* in, const plat_readqc_options* options, int32_t* out_ok,
                                        int32_t* out_reason, int32_t* out_perm, int32_t* out_counts, const plat_read_buffers_tables* tab, void* stream)
{
    if (!ctx || !in || !options || in->n_streams < 0 || in->qc.n_reads < 0) return PLAT_ERR_INVALID;
    const plat_readqc_batch& q = in->qc;
    if (in->n_streams == 0) return q.n_reads == 0 ? PLAT_OK : PLAT_ERR_INVALID;
    if (!in->stream_begin || !out_ok || !out_reason || !out_perm || !out_counts || (q.n_reads > 0 && !q.read_pos)) return PLAT_ERR_INVALID;
    const bool tables = tab && tab->seq;
    if (tables && (!in->read_seq || !in->read_end || !tab->off || !tab->cig_off || !tab->qual || !tab->cigar || !tab->pos || !tab->end ||
                   !tab->mapq || !tab->flags || !tab->mate_pos))
        return PLAT_ERR_INVALID;
    PLAT_HIP(ctx, hipSetDevice(ctx->device));
    const hipStream_t st = (hipStream_t)stream;
    if (q.n_reads > 0) {
        const int rc = plat_read_qc_batch(ctx, &q, options, out_ok, out_reason, stream);
        if (rc != PLAT_OK) return rc;
    }
    return split_and_gather<true>(ctx, q, in->n_streams, in->stream_begin, in->read_seq, in->read_end, out_ok, out_reason, out_perm, out_counts,
                                  tab, tables, st);
}

PLAT_EXPORT int plat_read_buffers_packed_batch(plat_ctx* ctx, const plat_read_buffers_packed_in* in, const plat_readqc_options* options,
                                               int32_t* out_ok, int32_t* out_reason, int32_t* out_perm, int32_t* out_counts,
                                               const plat_read_buffers_tables* tab, void* stream)
{
    if (!ctx || !in || !options || in->n_streams < 0 || in->qc.n_reads < 0 || in->n_exc < 0) return PLAT_ERR_INVALID;
    const plat_readqc_batch& q = in->qc;
    if (in->n_streams == 0) return q.n_reads == 0 ? PLAT_OK : PLAT_ERR_INVALID;
    if (!in->stream_begin || !out_ok || !out_reason || !out_perm || !out_counts) return PLAT_ERR_INVALID;
    if (q.n_reads > 0 && (!in->read_packed || !q.read_off || !q.read_pos || !q.read_mapq || !q.read_flags || !q.chrom_id || !q.mate_chrom_id ||
                          !q.insert_size || !q.mate_pos || !q.cigar || !q.cig_off || !q.stream_of))
        return PLAT_ERR_INVALID;
    if (in->n_exc > 0 && (!in->exc_index || !in->exc_qual)) return PLAT_ERR_INVALID;
    const bool tables = tab && tab->seq;
    if (tables && (!in->read_end || !tab->off || !tab->cig_off || !tab->cigar || !tab->pos || !tab->end || !tab->mapq || !tab->flags || !tab->mate_pos))
        return PLAT_ERR_INVALID;
    PLAT_HIP(ctx, hipSetDevice(ctx->device));
    const hipStream_t st = (hipStream_t)stream;
    const int rc = plat_read_qc_packed_launch(ctx, *in, *options, out_ok, out_reason, st);
    if (rc != PLAT_OK) return rc;
    return split_and_gather<false>(ctx, q, in->n_streams, in->stream_begin, in->read_packed, in->read_end, out_ok, out_reason, out_perm, out_counts,
                                   tab, tables, st);
}
