// plat_fasta.hip -- indexed sequence fetch from the bytes of a FASTA file on the device (plat_fasta_fetch_batch, include/platypus_mi355x.h
// has the rule in words): FastaFile.getSequence (src/cython/fastafile.pyx:173-207) for a whole batch of queries, and the whole-contig
// mode the region loop needs.  The rule of one query -- the span's arithmetic, the byte map -- is fasta_rule.hpp, which the host twin
// reads too.  A query's answer is its file span without the newlines, upper-cased: a stream compaction.  The work is cut by TILES OF THE
// FILE SPANS, not by queries: a query of 200 bases is one or two tiles, a contig of 250 MB a quarter of a million, and both go through the
// same launches.  A tile is TILE_BYTES of the cut, one aligned 16-byte word per lane of a wave (wave_tiles.hpp); the first and last word
// of a span are masked, and a word that reaches past file_len -- only the cut's last one can -- is loaded byte by byte, so no byte
// outside [file, file + file_len) is read.  Five launches:
//   k_fa_spans     one thread per query: status and span (fasta::span_of, cut_of), the query's tile count, its byte count reset
//   k_fa_scan      one workgroup: the tile counts to their prefix q_tile_first [n + 1]
//   k_fa_tiles<0>  (count) the (query, tile) pairs 0 .. P in order are dealt to the grid's W waves in W equal runs; a wave finds its first
//                  pair's query by a search in the prefix and walks on from there.  Per tile: the kept bytes of each lane's word, a wave
//                  sum.  Per query the wave adds what it counted to the query's byte count (one 64-bit atomic add per wave and query, by
//                  one lane) and keeps two numbers of its run: the bytes of its first and of its last query
//   k_fa_scan      one workgroup: the byte counts to out_off [n + 1], the totals block, the verdict
//   k_fa_tiles<1>  (write) the same walk.  A wave that starts inside a query sums what the runs in front of it counted for that query (the
//                  last-query number of the run that holds the query's first tile, the first-query numbers of the runs between); from
//                  there every tile's place is the running count.  The tile's kept bytes are ranked by a wave scan, upper-cased four at a
//                  time, put into LDS at the output's own alignment, and go out as aligned 16-byte stores with byte stores at both ends.
//                  Nothing is written when the total exceeds cap_bytes
// Launches order everything that one kernel reads of another; inside a launch no workgroup reads what another wrote.  Every loop is
// bounded by a wave's run of pairs, the logarithm of n or the number of runs.  Nothing traps.
#include <algorithm>

#include "plat_internal.hpp"
#include "fasta_rule.hpp"
#include "wave_tiles.hpp"

namespace plat {
static_assert(fasta::ST_OK == PLAT_FASTA_OK && fasta::ST_INDEX_ERROR == PLAT_FASTA_INDEX_ERROR && fasta::ST_ZERO_LINE == PLAT_FASTA_ZERO_LINE &&
              fasta::ST_BAD_INDEX == PLAT_FASTA_BAD_INDEX && fasta::ST_LEFT_OF_CUT == PLAT_FASTA_LEFT_OF_CUT && fasta::ST_RIGHT_OF_CUT == PLAT_FASTA_RIGHT_OF_CUT &&
              fasta::MODE_SEQUENCE == PLAT_FASTA_MODE_SEQUENCE && fasta::MODE_CONTIG == PLAT_FASTA_MODE_CONTIG, "fasta_rule.hpp and the header agree");
constexpr int FA_ST_VERDICT = 0, FA_ST_BYTES = 1, FA_ST_TILES = 2, FA_ST_NOT_OK = 3;
static_assert(PLAT_FASTA_STATUS_WORDS == 4, "the totals block");

struct FaScratch {
    int64_t* q_lo;                                        // [n] the span inside the cut: bytes [q_lo, q_hi) of `file`
    int64_t* q_hi;                                        // [n]
    int64_t* q_tile_first;                                // [n + 1] counts, then their prefix
    int64_t* run_first;                                   // [W] kept bytes a wave counted for the first query of its run
    int64_t* run_last;                                    // [W] ... and for the last
};

__global__ void __launch_bounds__(256)
k_fa_spans(plat_fasta_fetch_in in, plat_fasta_fetch_out o, FaScratch z)
{
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < in.n_queries; q += (long long)gridDim.x * 256) {
        const fasta::Entry e{in.start_pos[q], in.line_len[q], in.full_len[q], in.seq_len[q]};
        const fasta::Span s = fasta::span_of(e, in.beg[q], in.end[q], in.mode[q] ? fasta::MODE_CONTIG : fasta::MODE_SEQUENCE, in.file_size);
        const int32_t st = fasta::cut_of(s, in.file_base, in.file_len);
        long long lo = 0, hi = 0;
        if (st == fasta::ST_OK && s.lo < s.hi) { lo = s.lo - in.file_base; hi = s.hi - in.file_base; }       // (cut_of: 0 <= lo < hi <= file_len)
        z.q_lo[q] = lo; z.q_hi[q] = hi;
        z.q_tile_first[q] = hi > lo ? (hi - (lo & ~15ll) + TILE_BYTES - 1) / TILE_BYTES : 0;
        o.out_off[q] = 0;
        o.out_status[q] = st;
    }
}

// a[0 .. n) to its prefix, a[n] the total; WHICH 1: the byte counts, and with them the totals block
template <int WHICH> __global__ void __launch_bounds__(BLOCK_SCAN_THREADS)
k_fa_scan(plat_fasta_fetch_in in, plat_fasta_fetch_out o, FaScratch z)
{
    __shared__ long long s_wave[BLOCK_SCAN_THREADS / 64];
    __shared__ unsigned long long s_bad;
    const int t = threadIdx.x;
    int64_t* a = WHICH == 0 ? z.q_tile_first : o.out_off;
    if (WHICH == 1) {
        if (t == 0) s_bad = 0;
        __syncthreads();
        unsigned long long bad = 0;
        for (long long q = t; q < in.n_queries; q += BLOCK_SCAN_THREADS) bad += o.out_status[q] != fasta::ST_OK;
        if (bad) atomicAdd(&s_bad, bad);
    }
    const long long total = block_scan_inplace<BLOCK_SCAN_THREADS>(a, in.n_queries, s_wave);
    __syncthreads();
    if (t == 0) {
        a[in.n_queries] = total;
        if (WHICH == 1) {
            o.totals[FA_ST_VERDICT] = total > o.cap_bytes ? PLAT_ERR_OVERFLOW : 0; o.totals[FA_ST_BYTES] = total;
            o.totals[FA_ST_TILES] = z.q_tile_first[in.n_queries]; o.totals[FA_ST_NOT_OK] = (int64_t)s_bad;
        }
    }
}

// the word of `file` at `at` (a multiple of 16 below file_len): one 16-byte load, or the bytes in front of file_len one by one
__device__ __forceinline__ uint4 fa_load_word(const uint8_t* __restrict__ file, long long at, long long file_len)
{
    if (at + 16 <= file_len) return *reinterpret_cast<const uint4*>(file + at);
    unsigned v[4] = {0, 0, 0, 0};
    for (int j = 0; j < 16 && at + j < file_len; ++j) v[j >> 2] |= (unsigned)file[at + j] << (8 * (j & 3));
    return make_uint4(v[0], v[1], v[2], v[3]);
}

// the last q in [0, n) with first[q] <= p, for p < first[n]: the query of pair p (queries without tiles are stepped over)
__device__ __forceinline__ long long fa_query_of(const int64_t* __restrict__ first, long long n, long long p)
{
    long long lo = 0, hi = n;                                               // the first index in [0, n] whose entry exceeds p, less one
    while (lo < hi) { const long long mid = lo + (hi - lo) / 2; if (first[mid + 1] <= p) lo = mid + 1; else hi = mid; }
    return lo;
}

template <bool WRITE> __global__ void __launch_bounds__(TILE_WAVES * 64)
k_fa_tiles(plat_fasta_fetch_in in, plat_fasta_fetch_out o, FaScratch z)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_out[TILE_WAVES][TILE_BYTES + 16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long W = (long long)gridDim.x * TILE_WAVES, w = (long long)blockIdx.x * TILE_WAVES + wave;
    const long long n = in.n_queries, P = z.q_tile_first[n];
    if (WRITE && o.totals[FA_ST_VERDICT] != 0) return;
    const long long K = (P + W - 1) / W;                                    // pairs per run
    const long long p0 = w * K, p1 = std::min(P, p0 + K);
    if (p0 >= p1) {                                                         // (wave-uniform) a run without pairs
        if (!WRITE && lane == 0) { z.run_first[w] = 0; z.run_last[w] = 0; }
        return;
    }
    long long q = fa_query_of(z.q_tile_first, n, p0);
    long long run = 0;                                                      // kept bytes of query q that this wave has seen
    long long base = 0;                                                     // WRITE: where query q's bytes of this run begin in the blob
    bool firstQuery = true;
    if (WRITE) {
        const long long qFirst = z.q_tile_first[q], ws = qFirst / K;        // the run that holds q's first tile
        long long part = 0;
        if (ws < w) {                                                       // (wave-uniform) bounded by the number of runs
            for (long long x = ws + lane; x < w; x += 64) part += x == ws ? z.run_last[x] : z.run_first[x];
            part = __shfl(wave_incl_scan(part, lane), 63, 64);
        }
        base = o.out_off[q] + part;
    }
    uint8_t* mine = s_out[wave];
    for (long long p = p0; p < p1; ++p) {                                   // (wave-uniform throughout)
        while (p >= z.q_tile_first[q + 1]) {                                // the next query that has tiles: p is its first
            if (!WRITE && lane == 0) {
                if (run) atomicAdd((unsigned long long*)&o.out_off[q], (unsigned long long)run);
                if (firstQuery) z.run_first[w] = run;
            }
            firstQuery = false;
            ++q; run = 0;
            if (WRITE) base = o.out_off[q];
        }
        const long long lo = z.q_lo[q], hi = z.q_hi[q];
        const long long at = (lo & ~15ll) + (p - z.q_tile_first[q]) * TILE_BYTES + 16 * lane;
        const unsigned inside = word_inside(at, lo, hi);
        uint4 word = make_uint4(0, 0, 0, 0);
        if (inside) word = fa_load_word(in.file, at, in.file_len);          // (inside: at < hi <= file_len)
        const unsigned keep = inside & ~loaded_word_newlines(word);
        const int c = __popc(keep);
        const int incl = wave_incl_scan(c, lane), total = __shfl(incl, 63, 64);
        if (WRITE && total > 0) {
            uint8_t* dst = o.out + base + run;                              // the tile's bytes go to dst[0 .. total)
            const int shift = (int)(reinterpret_cast<uintptr_t>(dst) & 15);
            const unsigned v[4] = {fasta::upper4(word.x), fasta::upper4(word.y), fasta::upper4(word.z), fasta::upper4(word.w)};
            int at_lds = shift + incl - c;
#pragma unroll
            for (int j = 0; j < 16; ++j)
                if (keep & (1u << j)) mine[at_lds++] = (uint8_t)(v[j >> 2] >> (8 * (j & 3)));
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            // LDS bytes [shift, shift + total) are dst[0 ..): LDS word i is the aligned output word at dst - shift + 16 i
            const int end = shift + total;
            for (int i = lane; 16 * i < end; i += 64) {
                const int a = 16 * i, b = a + 16;
                if (a >= shift && b <= end) *reinterpret_cast<uint4*>(dst - shift + a) = *reinterpret_cast<const uint4*>(mine + a);
                else for (int k = std::max(a, shift); k < std::min(b, end); ++k) dst[k - shift] = mine[k];
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();                                // (the next tile rewrites the wave's LDS)
        }
        run += total;
    }
    if (!WRITE && lane == 0) {
        if (run) atomicAdd((unsigned long long*)&o.out_off[q], (unsigned long long)run);
        if (firstQuery) z.run_first[w] = run;
        z.run_last[w] = run;
    }
}
}  // namespace plat

PLAT_EXPORT int plat_fasta_tile_bytes(void) { return plat::TILE_BYTES; }

PLAT_EXPORT int plat_fasta_fetch_batch(plat_ctx* ctx, const plat_fasta_fetch_in* in, const plat_fasta_fetch_out* out, void* stream)
{
    if (!ctx || !in || !out) return PLAT_ERR_INVALID;
    const plat_fasta_fetch_in& q = *in;
    const plat_fasta_fetch_out& o = *out;
    if (q.file_len < 0 || q.file_base < 0 || q.file_size < 0 || q.n_queries < 0 || o.cap_bytes < 0) return PLAT_ERR_INVALID;
    if ((q.file_len && !q.file) || (reinterpret_cast<uintptr_t>(q.file) & 15)) return PLAT_ERR_INVALID;
    if (q.n_queries && (!q.start_pos || !q.line_len || !q.full_len || !q.seq_len || !q.beg || !q.end || !q.mode || !o.out_status)) return PLAT_ERR_INVALID;
    if (!o.out_off || !o.totals || (o.cap_bytes && !o.out)) return PLAT_ERR_INVALID;
    PLAT_HIP(ctx, hipSetDevice(ctx->device));
    const hipStream_t st = (hipStream_t)stream;
    const long long n = q.n_queries;
    // the runs: enough waves to fill the device on a genome, a few tiles each on a batch of short queries
    const long long likely = n + q.file_len / plat::TILE_BYTES;
    const unsigned tileBlocks = (unsigned)std::max<long long>(1, std::min<long long>((likely + 2 * plat::TILE_WAVES - 1) / (2 * plat::TILE_WAVES), plat::TILE_GRID_CAP));
    const long long W = (long long)tileBlocks * plat::TILE_WAVES;
    const int rc = plat_reserve(ctx, ctx->fasta, (size_t)(3 * n + 1 + 2 * W) * sizeof(int64_t));      // (one of these calls at a time per context)
    if (rc != PLAT_OK) return rc;
    plat::FaScratch z;
    int64_t* base = (int64_t*)ctx->fasta.ptr;
    z.q_lo = base; z.q_hi = base + n; z.q_tile_first = base + 2 * n; z.run_first = base + 3 * n + 1; z.run_last = z.run_first + W;
    const unsigned spanBlocks = (unsigned)std::max<long long>(1, std::min<long long>((n + 255) / 256, plat::TILE_GRID_CAP));
    PLAT_LAUNCH(ctx, PLAT_KT_OTHER, st, plat::k_fa_spans, dim3(spanBlocks), dim3(256), 0, q, o, z);
    PLAT_LAUNCH(ctx, PLAT_KT_OTHER, st, plat::k_fa_scan<0>, dim3(1), dim3(plat::BLOCK_SCAN_THREADS), 0, q, o, z);
    PLAT_LAUNCH(ctx, PLAT_KT_OTHER, st, plat::k_fa_tiles<false>, dim3(tileBlocks), dim3(plat::TILE_WAVES * 64), 0, q, o, z);
    PLAT_LAUNCH(ctx, PLAT_KT_OTHER, st, plat::k_fa_scan<1>, dim3(1), dim3(plat::BLOCK_SCAN_THREADS), 0, q, o, z);
    PLAT_LAUNCH(ctx, PLAT_KT_OTHER, st, plat::k_fa_tiles<true>, dim3(tileBlocks), dim3(plat::TILE_WAVES * 64), 0, q, o, z);
    PLAT_HIP(ctx, hipGetLastError());
    return PLAT_OK;
}
