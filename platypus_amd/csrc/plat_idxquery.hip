// plat_idxquery.hip -- region queries over a flattened tabix or BAM index on the device (plat_index_query_batch, include/platypus_mi355x.h
// has the rule): ti_iter_query (src/tabix/index.c.pysam.c:776-870) for a whole call's queries in one batch.  The rule of one query, the
// flatten that makes the tables and the host twin are index_query.hpp.  The index's tables are resident (uploaded once when the index is
// opened); a call brings (tid, beg, end) per query and takes a CSR of chunks back.  Seven launches:
//   k_iq_reset     the verdict key, the tables' flag and the list of workgroup queries reset
//   k_iq_check     the tables entry by entry (offsets that ascend inside their tables, bin ids that ascend inside a reference) and every
//                  query's tid: what is wrong lowers the key or raises the flag, and every later kernel then writes nothing but the status
//   k_iq_wave      (count) one wave per query, four queries per workgroup: lanes 0..5 search the six level ranges in the reference's
//                  ascending bin ids (two lower bounds each: the bins a range holds are consecutive, and so are their chunks); lanes over the
//                  ranges' chunks, those with v > min_off handed to lanes by ballot and rank; up to 64 are sorted in registers (a bitonic
//                  network over lane shuffles), one wave scan gives the prefix maximum, the heads and their ranks (index_query.hpp,
//                  resolve_fused, says why that is the reference's three loops).  More than 64 go to the list, more than
//                  PLAT_IDXQ_MAX_CHUNKS are handed over (count -2)
//   k_iq_group     (count) one workgroup per listed query: the gathered chunks in LDS (32 KiB), a bitonic sort there, the same scan over eight
//                  chunks per thread
//   k_iq_scan      one workgroup: the counts to q_first, the totals, the status block
//   k_iq_wave, k_iq_group (write) the same again, now writing each query's chunks at its q_first -- nothing when they do not all fit
// Every loop is bounded by the chunks of a level range's bins, the logarithm of a table or PLAT_IDXQ_MAX_CHUNKS.  Nothing traps.
#include <algorithm>

#include "plat_internal.hpp"
#include "index_query.hpp"
#include "wave_tiles.hpp"

namespace plat {
constexpr unsigned long long IQ_NO_KEY = ~0ull;
constexpr int IQ_WAVES = 4;                               // queries in flight per workgroup of k_iq_wave
constexpr int IQ_GROUP_THREADS = 256;
constexpr int IQ_PER_THREAD = idxq::MAX_CHUNKS / IQ_GROUP_THREADS;
static_assert(IQ_PER_THREAD * IQ_GROUP_THREADS == idxq::MAX_CHUNKS && (idxq::MAX_CHUNKS & (idxq::MAX_CHUNKS - 1)) == 0, "the limit is a power of two, a multiple of the workgroup");
static_assert(idxq::MAX_CHUNKS == PLAT_IDXQ_MAX_CHUNKS && idxq::ST_WORDS == PLAT_IDXQ_STATUS_WORDS && idxq::MAX_REF == PLAT_TBI_MAX_REF, "index_query.hpp and the header agree");

struct IqScratch {
    unsigned long long* key;                              // [1] the lowest query whose tid lies outside the index
    int* bad;                                             // [1] the tables break their contract
    int* n_list;                                          // [1]
    int32_t* list;                                        // [n_queries] the queries that gather 65 .. PLAT_IDXQ_MAX_CHUNKS chunks
};

__device__ __forceinline__ bool iq_refused(const IqScratch& z) { return *z.bad != 0 || *z.key != IQ_NO_KEY; }

__global__ void __launch_bounds__(64)
k_iq_reset(IqScratch z)
{
    if (threadIdx.x == 0) { *z.key = IQ_NO_KEY; *z.bad = 0; *z.n_list = 0; }
}

// offsets first[0 .. n] that ascend from 0 to total: entry i against its neighbour
__device__ __forceinline__ bool iq_offsets_ok(const int64_t* first, long long n, long long total, long long i)
{
    const long long a = first[i];
    if (a < 0 || a > total || (i == 0 && a != 0) || (i == n && a != total)) return false;
    return i == n || a <= first[i + 1];
}

__global__ void __launch_bounds__(256)
k_iq_check(plat_index_query_in in, IqScratch z)
{
    const long long step = (long long)gridDim.x * 256, me = (long long)blockIdx.x * 256 + threadIdx.x;
    bool bad = false;
    for (long long t = me; t <= in.n_ref; t += step)
        bad |= !iq_offsets_ok(in.ref_bin_first, in.n_ref, in.n_bins, t) || !iq_offsets_ok(in.ref_lin_first, in.n_ref, in.n_lin, t);
    for (long long b = me; b <= in.n_bins; b += step) {
        bad |= !iq_offsets_ok(in.bin_chunk_first, in.n_bins, in.n_chunks, b);
        if (b == in.n_bins) continue;
        const int32_t id = in.bin_id[b];
        bad |= id < 0 || id >= idxq::MAX_BIN;
        if (b + 1 < in.n_bins && id >= in.bin_id[b + 1]) {                  // ids fall only where the next reference begins
            long long lo = 0, hi = (long long)in.n_ref + 1;                 // (a search inside [0, n_ref] whatever the table holds)
            while (lo < hi) { const long long mid = lo + (hi - lo) / 2; if (in.ref_bin_first[mid] < b + 1) lo = mid + 1; else hi = mid; }
            bad |= lo > in.n_ref || in.ref_bin_first[lo] != b + 1;
        }
    }
    if (bad) *z.bad = 1;
    for (long long q = me; q < in.n_queries; q += step)
        if (in.tid[q] < 0 || in.tid[q] >= in.n_ref) atomicMin(z.key, (unsigned long long)q);
}

// what a query asks of the tables: the chunks of its six level ranges, c0[l] .. c1[l], and min_off
struct IqRanges { long long c0, c1; };

__device__ __forceinline__ IqRanges iq_level(const plat_index_query_in& in, int32_t tid, int32_t beg, int32_t end, int level)
{
    int32_t lo, hi;
    idxq::level_range(level, beg, end, &lo, &hi);
    const int64_t b0 = in.ref_bin_first[tid], b1 = in.ref_bin_first[tid + 1];
    const int64_t p = idxq::lower_bound(in.bin_id, b0, b1, lo), e = idxq::lower_bound(in.bin_id, p, b1, hi + 1);
    return IqRanges{in.bin_chunk_first[p], in.bin_chunk_first[e]};
}
__device__ __forceinline__ unsigned long long iq_min_off(const plat_index_query_in& in, int32_t tid, int32_t beg)
{
    const int64_t l0 = in.ref_lin_first[tid], slot = idxq::lin_slot(beg, in.ref_lin_first[tid + 1] - l0);
    return slot < 0 ? 0ull : (unsigned long long)in.lin_fill[l0 + slot];
}
// the position of set bit number n (from 0) of m; n < popcount(m)
__device__ __forceinline__ int iq_nth_set(unsigned long long m, int n)
{
    int pos = 0;
    for (int w = 32; w > 0; w >>= 1) {
        const int c = __popcll((m >> pos) & ((1ull << w) - 1ull));
        if (n >= c) { n -= c; pos += w; }
    }
    return pos;
}
__device__ __forceinline__ unsigned long long iq_max(unsigned long long a, unsigned long long b) { return a > b ? a : b; }

template <bool WRITE> __global__ void __launch_bounds__(IQ_WAVES * 64)
k_iq_wave(plat_index_query_in in, plat_index_query_out o, IqScratch z)
{
    if (iq_refused(z)) return;
    if (WRITE && o.status[idxq::ST_VERDICT] != 0) return;
    const int lane = threadIdx.x & 63;
    for (long long q = (long long)blockIdx.x * IQ_WAVES + (threadIdx.x >> 6); q < in.n_queries; q += (long long)gridDim.x * IQ_WAVES) {
        const int32_t tid = in.tid[q], end = in.end[q];
        const int32_t beg = in.beg[q] < 0 ? 0 : in.beg[q];
        if (beg >= end) {                                                   // (wave-uniform) no iterator, or one without chunks
            if (!WRITE && lane == 0) { o.count[q] = end < beg ? idxq::COUNT_NO_ITER : 0; o.gathered[q] = 0; o.q_first[q] = 0; }
            continue;
        }
        IqRanges mine{0, 0};
        if (lane < idxq::LEVELS) mine = iq_level(in, tid, beg, end, lane);
        const unsigned long long minOff = iq_min_off(in, tid, beg);
        unsigned long long u = ~0ull, v = ~0ull;                            // this lane's gathered chunk; lanes behind the last sort last
        long long g = 0;
        for (int level = 0; level < idxq::LEVELS; ++level) {
            const long long c0 = __shfl(mine.c0, level, 64), c1 = __shfl(mine.c1, level, 64);
            for (long long base = c0; base < c1; base += 64) {              // (bounded by the chunks of the level range's bins)
                const long long c = base + lane;
                unsigned long long cu = 0, cv = 0;
                if (c < c1) { cu = (unsigned long long)in.chunk_u[c]; cv = (unsigned long long)in.chunk_v[c]; }
                const unsigned long long pass = __ballot(c < c1 && cv > minOff);
                // the lane that takes gathered chunk number g + k reads it from the lane of the ballot's k-th bit
                const long long k = lane - g;
                const bool take = k >= 0 && k < __popcll(pass);
                const int src = take ? iq_nth_set(pass, (int)k) : 0;
                const unsigned long long tu = __shfl(cu, src, 64), tv = __shfl(cv, src, 64);
                if (take) { u = tu; v = tv; }
                g += __popcll(pass);
            }
        }
        if (g > 64) {                                                       // (wave-uniform)
            if (!WRITE && lane == 0) {
                o.gathered[q] = (int32_t)std::min<long long>(g, INT32_MAX);
                if (g <= idxq::MAX_CHUNKS) z.list[atomicAdd(z.n_list, 1)] = (int32_t)q;
                else { o.count[q] = idxq::COUNT_HANDED; o.q_first[q] = 0; }
            }
            continue;
        }
        for (int k = 2; k <= 64; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) {
                const unsigned long long ou = __shfl_xor(u, j, 64), ov = __shfl_xor(v, j, 64);
                const bool keepLow = ((lane & j) == 0) == ((lane & k) == 0);
                if (keepLow ? idxq::pair_less(ou, ov, u, v) : idxq::pair_less(u, v, ou, ov)) { u = ou; v = ov; }
            }
        const bool valid = lane < g;
        unsigned long long incl = valid ? v : 0ull;                         // the prefix maximum of v
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned long long t = __shfl_up(incl, d, 64);
            if (lane >= d) incl = iq_max(incl, t);
        }
        unsigned long long M = __shfl_up(incl, 1, 64);
        if (lane == 0) M = 0;
        const bool head = valid && (lane == 0 || (v > M && (M >> 16) < (u >> 16)));
        const unsigned long long heads = __ballot(head);
        const int n = __popcll(heads), rank = __popcll(heads & ((1ull << lane) - 1ull));
        const unsigned long long all = __shfl(incl, 63, 64);
        if (!WRITE) {
            if (lane == 0) { o.count[q] = n; o.gathered[q] = (int32_t)g; o.q_first[q] = n; }
        } else if (n > 0) {
            const long long at = o.q_first[q];
            if (head) {
                o.out_u[at + rank] = (int64_t)u;
                if (rank > 0) o.out_v[at + rank - 1] = (int64_t)M;
            }
            if (lane == 0) o.out_v[at + n - 1] = (int64_t)all;
        }
    }
}

template <bool WRITE> __global__ void __launch_bounds__(IQ_GROUP_THREADS)
k_iq_group(plat_index_query_in in, plat_index_query_out o, IqScratch z)
{
    __shared__ unsigned long long s_u[idxq::MAX_CHUNKS], s_v[idxq::MAX_CHUNKS];
    __shared__ unsigned long long s_max[IQ_GROUP_THREADS / 64];
    __shared__ long long s_c0[idxq::LEVELS], s_c1[idxq::LEVELS];
    __shared__ int s_heads[IQ_GROUP_THREADS / 64], s_n;
    if (iq_refused(z)) return;
    if (WRITE && o.status[idxq::ST_VERDICT] != 0) return;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int nList = std::min(*z.n_list, in.n_queries);
    for (int item = blockIdx.x; item < nList; item += gridDim.x) {
        const long long q = z.list[item];
        const int32_t tid = in.tid[q], end = in.end[q];
        const int32_t beg = in.beg[q] < 0 ? 0 : in.beg[q];
        if (t < idxq::LEVELS) { const IqRanges r = iq_level(in, tid, beg, end, t); s_c0[t] = r.c0; s_c1[t] = r.c1; }
        if (t == 0) s_n = 0;
        __syncthreads();
        const unsigned long long minOff = iq_min_off(in, tid, beg);
        for (int level = 0; level < idxq::LEVELS; ++level)
            for (long long c = s_c0[level] + t; c < s_c1[level]; c += IQ_GROUP_THREADS) {      // (bounded by the chunks of the level range's bins)
                const unsigned long long cu = (unsigned long long)in.chunk_u[c], cv = (unsigned long long)in.chunk_v[c];
                if (cv > minOff) {                                          // (any order: the sort follows)
                    const int slot = atomicAdd(&s_n, 1);
                    if (slot < idxq::MAX_CHUNKS) { s_u[slot] = cu; s_v[slot] = cv; }
                }
            }
        __syncthreads();
        const int g = std::min(s_n, (int)idxq::MAX_CHUNKS);                 // (the count pass listed it for g <= the limit)
        int P = 128;
        while (P < g) P <<= 1;
        for (int i = g + t; i < P; i += IQ_GROUP_THREADS) { s_u[i] = ~0ull; s_v[i] = ~0ull; }
        __syncthreads();
        for (int k = 2; k <= P; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int x = t; x < P / 2; x += IQ_GROUP_THREADS) {
                    const int i = ((x & ~(j - 1)) << 1) | (x & (j - 1)), l = i | j;
                    const unsigned long long ui = s_u[i], vi = s_v[i], ul = s_u[l], vl = s_v[l];
                    if (idxq::pair_less(ul, vl, ui, vi) == ((i & k) == 0)) { s_u[i] = ul; s_v[i] = vl; s_u[l] = ui; s_v[l] = vi; }
                }
                __syncthreads();
            }
        // thread t holds chunks t * IQ_PER_THREAD ...: the largest v in front of them, then their heads' ranks
        const int e0 = t * IQ_PER_THREAD;
        unsigned long long mine = 0;
        for (int k = 0; k < IQ_PER_THREAD; ++k) if (e0 + k < g) mine = iq_max(mine, s_v[e0 + k]);
        unsigned long long incl = mine;
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned long long x = __shfl_up(incl, d, 64);
            if (lane >= d) incl = iq_max(incl, x);
        }
        unsigned long long M = __shfl_up(incl, 1, 64);
        if (lane == 0) M = 0;
        if (lane == 63) s_max[wave] = incl;
        __syncthreads();
        unsigned long long all = 0;
        for (int w = 0; w < IQ_GROUP_THREADS / 64; ++w) { if (w < wave) M = iq_max(M, s_max[w]); all = iq_max(all, s_max[w]); }
        unsigned headBits = 0;
        unsigned long long before[IQ_PER_THREAD];
        for (int k = 0; k < IQ_PER_THREAD; ++k) {
            before[k] = M;
            if (e0 + k < g) {
                const unsigned long long u = s_u[e0 + k], v = s_v[e0 + k];
                if (e0 + k == 0 || (v > M && (M >> 16) < (u >> 16))) headBits |= 1u << k;
                M = iq_max(M, v);
            }
        }
        const int nMine = __popc(headBits), inclHeads = wave_incl_scan(nMine, lane);
        if (lane == 63) s_heads[wave] = inclHeads;
        __syncthreads();
        int rank = inclHeads - nMine, n = 0;
        for (int w = 0; w < IQ_GROUP_THREADS / 64; ++w) { if (w < wave) rank += s_heads[w]; n += s_heads[w]; }
        if (!WRITE) {
            if (t == 0) { o.count[q] = n; o.q_first[q] = n; }
        } else {
            const long long at = o.q_first[q];
            for (int k = 0; k < IQ_PER_THREAD; ++k)
                if (headBits & (1u << k)) {
                    o.out_u[at + rank] = (int64_t)s_u[e0 + k];
                    if (rank > 0) o.out_v[at + rank - 1] = (int64_t)before[k];
                    ++rank;
                }
            if (t == 0 && n > 0) o.out_v[at + n - 1] = (int64_t)all;
        }
        __syncthreads();                                                    // (the next query rewrites the LDS)
    }
}

__global__ void __launch_bounds__(BLOCK_SCAN_THREADS)
k_iq_scan(plat_index_query_in in, plat_index_query_out o, IqScratch z)
{
    __shared__ long long s_wave[BLOCK_SCAN_THREADS / 64];
    __shared__ unsigned long long s_sum[3];
    const int t = threadIdx.x;
    if (iq_refused(z)) {
        if (t < idxq::ST_WORDS) o.status[t] = t == idxq::ST_VERDICT ? PLAT_ERR_INVALID : t == idxq::ST_QUERY ? (*z.key == IQ_NO_KEY ? -1 : (int64_t)*z.key) : 0;
        return;
    }
    if (t < 3) s_sum[t] = 0;
    __syncthreads();
    unsigned long long gathered = 0, handed = 0, noIter = 0;
    for (long long q = t; q < in.n_queries; q += BLOCK_SCAN_THREADS) {
        gathered += (unsigned long long)o.gathered[q]; handed += o.count[q] == idxq::COUNT_HANDED; noIter += o.count[q] == idxq::COUNT_NO_ITER;
    }
    atomicAdd(&s_sum[0], gathered); atomicAdd(&s_sum[1], handed); atomicAdd(&s_sum[2], noIter);
    const long long total = block_scan_inplace<BLOCK_SCAN_THREADS>(o.q_first, in.n_queries, s_wave);
    __syncthreads();
    if (t == 0) {
        o.q_first[in.n_queries] = total;
        int64_t* st = o.status;
        st[idxq::ST_VERDICT] = total > o.cap_chunks ? PLAT_ERR_OVERFLOW : 0; st[idxq::ST_QUERY] = -1; st[idxq::ST_CHUNKS] = total;
        st[idxq::ST_GATHERED] = (int64_t)s_sum[0]; st[idxq::ST_HANDED] = (int64_t)s_sum[1]; st[idxq::ST_NO_ITER] = (int64_t)s_sum[2];
    }
}
}  // namespace plat

PLAT_EXPORT int plat_index_query_batch(plat_ctx* ctx, const plat_index_query_in* in, const plat_index_query_out* out, void* stream)
{
    if (!ctx || !in || !out) return PLAT_ERR_INVALID;
    const plat_index_query_in& q = *in;
    const plat_index_query_out& o = *out;
    if (q.n_ref < 0 || q.n_ref > PLAT_TBI_MAX_REF || q.n_bins < 0 || q.n_chunks < 0 || q.n_lin < 0 || q.n_queries < 0 || o.cap_chunks < 0) return PLAT_ERR_INVALID;
    if (!q.ref_bin_first || !q.bin_chunk_first || !q.ref_lin_first || (q.n_bins && !q.bin_id) || (q.n_chunks && (!q.chunk_u || !q.chunk_v)) || (q.n_lin && !q.lin_fill)) return PLAT_ERR_INVALID;
    if (q.n_queries && (!q.tid || !q.beg || !q.end || !o.count || !o.gathered)) return PLAT_ERR_INVALID;
    if (!o.q_first || !o.status || (o.cap_chunks && (!o.out_u || !o.out_v))) return PLAT_ERR_INVALID;
    PLAT_HIP(ctx, hipSetDevice(ctx->device));
    const hipStream_t st = (hipStream_t)stream;
    const int rc = plat_reserve(ctx, ctx->tabix, 32 + (size_t)q.n_queries * sizeof(int32_t));      // (the fetch's scratch: one call at a time per context)
    if (rc != PLAT_OK) return rc;
    plat::IqScratch z;
    uint8_t* base = (uint8_t*)ctx->tabix.ptr;
    z.key = (unsigned long long*)base; z.bad = (int*)(base + 8); z.n_list = (int*)(base + 12); z.list = (int32_t*)(base + 32);
    const long long most = std::max<long long>(std::max<long long>(q.n_bins, q.n_ref), q.n_queries) + 1;
    const unsigned checkBlocks = (unsigned)std::min<long long>((most + 255) / 256, plat::TILE_GRID_CAP);
    const unsigned waveBlocks = (unsigned)std::max<long long>(1, std::min<long long>(((long long)q.n_queries + plat::IQ_WAVES - 1) / plat::IQ_WAVES, plat::TILE_GRID_CAP));
    const unsigned groupBlocks = (unsigned)std::max<long long>(1, std::min<long long>(q.n_queries, 1024));
    PLAT_LAUNCH(ctx, PLAT_KT_OTHER, st, plat::k_iq_reset, dim3(1), dim3(64), 0, z);
    PLAT_LAUNCH(ctx, PLAT_KT_OTHER, st, plat::k_iq_check, dim3(checkBlocks), dim3(256), 0, q, z);
    PLAT_LAUNCH(ctx, PLAT_KT_OTHER, st, plat::k_iq_wave<false>, dim3(waveBlocks), dim3(plat::IQ_WAVES * 64), 0, q, o, z);
    PLAT_LAUNCH(ctx, PLAT_KT_OTHER, st, plat::k_iq_group<false>, dim3(groupBlocks), dim3(plat::IQ_GROUP_THREADS), 0, q, o, z);
    PLAT_LAUNCH(ctx, PLAT_KT_OTHER, st, plat::k_iq_scan, dim3(1), dim3(plat::BLOCK_SCAN_THREADS), 0, q, o, z);
    PLAT_LAUNCH(ctx, PLAT_KT_OTHER, st, plat::k_iq_wave<true>, dim3(waveBlocks), dim3(plat::IQ_WAVES * 64), 0, q, o, z);
    PLAT_LAUNCH(ctx, PLAT_KT_OTHER, st, plat::k_iq_group<true>, dim3(groupBlocks), dim3(plat::IQ_GROUP_THREADS), 0, q, o, z);
    PLAT_HIP(ctx, hipGetLastError());
    return PLAT_OK;
}
