// plat_refcov.hip -- read counts of reference-call blocks (plat_refcall_coverage_batch, include/platypus_mi355x.h has the rule in words):
// the loop of outputRefCall (variantcaller.pyx:774-784) over ReadArray.countReadsCoveringRegion(p, p + 1) (cwindow.pyx:176-206), one
// workgroup per tile of REFCOV_TILE positions of one interval.  The rule itself is refcov_rule.hpp, shared with the host's loop.
#include <algorithm>

#include "plat_internal.hpp"
#include "refcov_rule.hpp"

namespace plat {

constexpr int REFCOV_THREADS = 256;
constexpr int REFCOV_TILE = refcov::TILE;
constexpr int REFCOV_PER_THREAD = REFCOV_TILE / REFCOV_THREADS;
// reads of one sample whose pos / end a tile stages: ~235 at 30x with 150-base reads (a tile and one read length in front of it), so this is
// room for a pile nine times as deep; what does not fit is read where it lies
constexpr int REFCOV_LDS_READS = 2048;
constexpr size_t REFCOV_STATIC_LDS = sizeof(int32_t) * (REFCOV_LDS_READS + (REFCOV_LDS_READS + 1) + REFCOV_THREADS / 64);
static_assert(PLAT_REFCOV_RAISES == refcov::RAISES && PLAT_REFCOV_EMPTY == refcov::EMPTY && PLAT_REFCOV_TILE == refcov::TILE, "the header's constants are the rule's");
static_assert(REFCOV_TILE % REFCOV_THREADS == 0 && REFCOV_THREADS % 64 == 0, "whole waves, a whole number of positions per thread");

// tile t -> dst[t]: the smallest count of its positions over the interval's samples (dst is iv_min itself when every interval is one tile)
__global__ void __launch_bounds__(REFCOV_THREADS)
k_refcov_tiles(plat_refcov_in in, plat_refcov_out o, int32_t* __restrict__ dst)
{
    __shared__ int32_t s_pos[REFCOV_LDS_READS];
    __shared__ int32_t s_end[REFCOV_LDS_READS + 1];
    __shared__ int32_t s_red[REFCOV_THREADS / 64];
    static_assert(sizeof s_pos + sizeof s_end + sizeof s_red == REFCOV_STATIC_LDS, "REFCOV_STATIC_LDS is this kernel's static LDS");
    const int tid = threadIdx.x, t = blockIdx.x;
    // the tile's interval (everything up to the per-position loops is the same in every thread of the workgroup)
    int k = t, j0 = 0;
    bool last = true;
    if (in.iv_tile_first) {
        int lo = 0, hi = in.n_intervals;                               // the last k with iv_tile_first[k] <= t
        while (lo < hi) { const int mid = lo + ((hi - lo) >> 1); if (in.iv_tile_first[mid] <= t) lo = mid + 1; else hi = mid; }
        k = lo > 0 ? lo - 1 : 0;
        j0 = std::max(0, t - in.iv_tile_first[k]);
        last = in.iv_tile_first[k + 1] == t + 1;
    }
    const int64_t start = in.iv_start[k], end = in.iv_end[k];
    const int nS = in.iv_n_samples[k], slice0 = in.iv_slice_first[k];
    const int64_t countOff = in.iv_count_off ? in.iv_count_off[k] : -1;
    const int64_t nTiles = end > start ? (end - start + REFCOV_TILE - 1) / REFCOV_TILE : 0;
    int32_t tileMin = refcov::EMPTY;
    for (int64_t j = j0; j < nTiles && (j == j0 || last) && nS > 0; ++j) {
        const int a = (int)(start + j * REFCOV_TILE), b = (int)std::min<int64_t>(end, start + (j + 1) * REFCOV_TILE);      // a < b, both inside [start, end]
        int32_t c[REFCOV_PER_THREAD];
        for (int q = 0; q < REFCOV_PER_THREAD; ++q) c[q] = refcov::EMPTY;
        for (int i = 0; i < nS; ++i) {
            const int sl = slice0 + i;
            int begin = 0, N = -1, longest = 0;
            if (sl >= 0 && sl < in.n_slices) { begin = in.slice_begin[sl]; N = in.slice_n[sl]; longest = in.slice_longest[sl]; }
            if (N < 0 || begin < 0 || (int64_t)begin + N > in.n_reads) {                 // a refused slice
                for (int q = 0; q < REFCOV_PER_THREAD; ++q) c[q] = refcov::RAISES;
                continue;
            }
            if (N == 0) {
                for (int q = 0; q < REFCOV_PER_THREAD; ++q) c[q] = std::min(c[q], 0);
                continue;
            }
            const int32_t* pos = in.read_pos + begin;
            const int32_t* rend = in.read_end + begin;
            int iLo, iHi;
            refcov::tile_range(pos, N, longest, a, b, &iLo, &iHi);
            const int n = iHi - iLo, nEnd = n + (iHi < N ? 1 : 0);
            if (n <= REFCOV_LDS_READS) {
                __syncthreads();                                        // (the sample before this one has been counted)
                for (int x = tid; x < nEnd; x += REFCOV_THREADS) { if (x < n) s_pos[x] = pos[iLo + x]; s_end[x] = rend[iLo + x]; }
                __syncthreads();
                for (int q = 0; q < REFCOV_PER_THREAD; ++q) {
                    const int p = a + tid + REFCOV_THREADS * q;
                    if (p < b) c[q] = std::min(c[q], refcov::canonical(refcov::count_in(s_pos, s_end, iLo, iLo, iHi, N, longest, p)));
                }
            } else {
                for (int q = 0; q < REFCOV_PER_THREAD; ++q) {
                    const int p = a + tid + REFCOV_THREADS * q;
                    if (p < b) c[q] = std::min(c[q], refcov::canonical(refcov::count_in(pos, rend, 0, iLo, iHi, N, longest, p)));
                }
            }
        }
        for (int q = 0; q < REFCOV_PER_THREAD; ++q) {
            const int p = a + tid + REFCOV_THREADS * q;
            if (p >= b) continue;
            tileMin = std::min(tileMin, c[q]);
            if (countOff >= 0 && o.counts) {
                const int64_t at = countOff + ((int64_t)p - start);
                if (at < o.cap_counts) o.counts[at] = c[q];
            }
        }
    }
    for (int d = 32; d > 0; d >>= 1) tileMin = std::min(tileMin, __shfl_xor(tileMin, d, 64));
    __syncthreads();
    if ((tid & 63) == 0) s_red[tid >> 6] = tileMin;
    __syncthreads();
    if (tid == 0) {
        int32_t m = s_red[0];
        for (int w = 1; w < REFCOV_THREADS / 64; ++w) m = std::min(m, s_red[w]);
        dst[t] = m;
    }
}

// interval k -> iv_min[k]: the smallest of its tiles' minima (PLAT_REFCOV_RAISES is the smallest value there is)
__global__ void __launch_bounds__(REFCOV_THREADS)
k_refcov_intervals(plat_refcov_in in, plat_refcov_out o, const int32_t* __restrict__ tileMin)
{
    const int k = blockIdx.x * REFCOV_THREADS + threadIdx.x;
    if (k >= in.n_intervals) return;
    const int t0 = std::max(0, in.iv_tile_first[k]), t1 = std::min(in.n_tiles, in.iv_tile_first[k + 1]);
    int32_t m = t0 < t1 ? refcov::EMPTY : refcov::RAISES;               // (an interval without a tile was not counted)
    for (int t = t0; t < t1; ++t) m = std::min(m, tileMin[t]);
    o.iv_min[k] = m;
}
}  // namespace plat

PLAT_EXPORT int plat_refcov_lds_reads(void) { return plat::REFCOV_LDS_READS; }

PLAT_EXPORT int plat_refcall_coverage_batch(plat_ctx* ctx, const plat_refcov_in* in, const plat_refcov_out* out, void* stream)
{
    if (!ctx || !in || !out) return PLAT_ERR_INVALID;
    const plat_refcov_in& q = *in;
    const plat_refcov_out& o = *out;
    if (q.n_intervals < 0 || q.n_slices < 0 || q.n_reads < 0 || q.n_tiles < q.n_intervals || o.cap_counts < 0) return PLAT_ERR_INVALID;
    if (q.n_intervals == 0) return q.n_tiles == 0 ? PLAT_OK : PLAT_ERR_INVALID;
    if (!q.iv_start || !q.iv_end || !q.iv_slice_first || !q.iv_n_samples || !o.iv_min) return PLAT_ERR_INVALID;
    if (q.n_slices > 0 && (!q.slice_begin || !q.slice_n || !q.slice_longest)) return PLAT_ERR_INVALID;
    if (q.n_reads > 0 && (!q.read_pos || !q.read_end)) return PLAT_ERR_INVALID;
    if (o.cap_counts > 0 && !o.counts) return PLAT_ERR_INVALID;
    const bool tiled = q.n_tiles != q.n_intervals;
    if (tiled && !q.iv_tile_first) return PLAT_ERR_INVALID;
    PLAT_HIP(ctx, hipSetDevice(ctx->device));
    const hipStream_t st = (hipStream_t)stream;
    plat_refcov_in k = q;
    int32_t* dst = o.iv_min;
    if (tiled) {
        const int rc = plat_reserve(ctx, ctx->refcov, (size_t)q.n_tiles * sizeof(int32_t));
        if (rc != PLAT_OK) return rc;
        dst = (int32_t*)ctx->refcov.ptr;
    } else k.iv_tile_first = nullptr;
    PLAT_LAUNCH(ctx, PLAT_KT_OTHER, st, plat::k_refcov_tiles, dim3((unsigned)q.n_tiles), dim3(plat::REFCOV_THREADS), 0, k, o, dst);
    if (tiled)
        PLAT_LAUNCH(ctx, PLAT_KT_OTHER, st, plat::k_refcov_intervals, dim3((unsigned)((q.n_intervals + plat::REFCOV_THREADS - 1) / plat::REFCOV_THREADS)),
                    dim3(plat::REFCOV_THREADS), 0, k, o, (const int32_t*)dst);
    PLAT_HIP(ctx, hipGetLastError());
    return PLAT_OK;
}
