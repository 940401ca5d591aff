// wave_tiles.hpp -- device-only pieces the kernel files share: the wave and workgroup scans (wave_incl_scan, block_excl_scan: the hot path's
// too -- candidate merge, k_sb_variants and k_sb_prefix of stage B, the assembler; block_scan_inplace), and for the line front ends (plat_sourcevcf.hip,
// plat_tabix.hip; plat_fasta.hip takes the geometry, the scans and the masks of a loaded word) the tile geometry, a word's newline mask, the rank of a byte among a tile table's marks and the hand-out of a tile's
// marked bytes to the lanes of a wave.  A byte stream is cut into tiles of TILE_BYTES = 64 aligned 16-byte words, one word per lane of a
// wave; a table of marks holds 16 bits per word, and next to it goes a table of the tiles' running mark counts ([tiles + 1]).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace plat {
constexpr int TILE_BYTES = 1024;                          // bytes per tile = 64 lanes x 16 bytes
constexpr int TILE_WAVES = 4;                             // waves (tiles in flight) per workgroup of the tile kernels
constexpr int TILE_GRID_CAP = 4096;                       // the tile kernels' grids are capped (grid-stride over tiles)
constexpr int BLOCK_SCAN_THREADS = 1024;                  // the workgroup of the one-workgroup scan kernels
static_assert(TILE_BYTES == 64 * 16, "a tile is one 16-byte word per lane of a wave");

// inclusive prefix sums over the lanes of a wave
template <class T> __device__ __forceinline__ T wave_incl_scan(T v, int lane)
{
    for (int d = 1; d < 64; d <<= 1) {
        const T u = __shfl_up(v, d, 64);
        if (lane >= d) v += u;
    }
    return v;
}

// exclusive prefix of v over the THREADS threads of a workgroup; every thread gets the total in a register (s_wave: THREADS / 64 entries
// of LDS).  Two barriers; every thread calls it.
template <int THREADS, class T> __device__ __forceinline__ T block_excl_scan(T v, T* s_wave, T& total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const T incl = wave_incl_scan(v, lane);
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    T before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < THREADS / 64; ++w) { const T s = s_wave[w]; if (w < wave) before += s; all += s; }
    __syncthreads();                                                    // (s_wave is rewritten by the next call)
    total = all;
    return before + incl - v;
}

// a[0 .. n) to its exclusive prefix sums in place, by all THREADS threads of one workgroup (s_wave: THREADS / 64 entries of LDS); returns
// the total.  Sums are taken in 64 bits whatever T is.
template <int THREADS, class T> __device__ long long block_scan_inplace(T* a, long long n, long long* s_wave)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    long long run = 0;
    for (long long t0 = 0; t0 < n; t0 += THREADS * 4) {
        const long long i0 = t0 + (long long)tid * 4;
        long long v[4], sum = 0;
        for (int k = 0; k < 4; ++k) { v[k] = i0 + k < n ? a[i0 + k] : 0; sum += v[k]; }
        const long long incl = wave_incl_scan(sum, lane);
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        long long at = run + incl - sum, all = 0;
        for (int w = 0; w < THREADS / 64; ++w) {
            if (w < wave) at += s_wave[w];
            all += s_wave[w];
        }
        for (int k = 0; k < 4; ++k) {
            if (i0 + k >= n) break;
            a[i0 + k] = (T)at;
            at += v[k];
        }
        run += all;
        __syncthreads();                                                // (s_wave is rewritten by the next round)
    }
    return run;
}

// the '\n' among the bytes of the aligned 16-byte word at `at` that lie in [lo, hi), one bit per byte: one aligned 16-byte load, which may
// run up to 15 bytes past hi (inside PLAT_BLOB_PAD); a word outside [lo, hi) is not loaded
__device__ __forceinline__ unsigned word_newlines(const uint8_t* text, long long at, long long lo, long long hi)
{
    unsigned nl = 0;
    if (at < hi && at + 16 > lo) {
        const uint4 w = *reinterpret_cast<const uint4*>(text + at);
        const unsigned v[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (int j = 0; j < 16; ++j)
            if (((v[j >> 2] >> (8 * (j & 3))) & 0xffu) == '\n' && at + j >= lo && at + j < hi) nl |= 1u << j;
    }
    return nl;
}

// ... of a word the caller has loaded (plat_fasta.hip loads a file's last word byte by byte): the '\n' among its sixteen bytes, one bit per byte
__device__ __forceinline__ unsigned loaded_word_newlines(const uint4& w)
{
    const unsigned v[4] = {w.x, w.y, w.z, w.w};
    unsigned nl = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const unsigned x = v[j] ^ 0x0a0a0a0au;                              // a zero byte where v has a newline
        const unsigned zero = ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x | 0x7f7f7f7fu);     // 0x80 in exactly those bytes
        nl |= (((zero >> 7) & 1u) | ((zero >> 14) & 2u) | ((zero >> 21) & 4u) | ((zero >> 28) & 8u)) << (4 * j);
    }
    return nl;
}

// the bytes of the word at `at` that lie in [lo, hi), one bit per byte
__device__ __forceinline__ unsigned word_inside(long long at, long long lo, long long hi)
{
    const long long a = lo > at ? lo - at : 0, b = hi - at < 16 ? hi - at : 16;
    return a < b ? ((1u << b) - 1u) & ~((1u << a) - 1u) : 0u;
}

// the bytes of a lane's word that lie behind a newline (nl: word_newlines of the wave's 64 words): the carry from the word before comes
// over a lane shuffle, lane 0's is the caller's (whether the byte in front of the tile is a newline)
__device__ __forceinline__ unsigned behind_newlines(unsigned nl, int lane, unsigned carry_for_lane0)
{
    unsigned carry = __shfl_up(nl >> 15, 1, 64);
    if (lane == 0) carry = carry_for_lane0;
    return ((nl << 1) | carry) & 0xffffu;
}

// set bits of `marks` in front of byte x (x >= the tiles' bytes: all of them); tile_run: the tiles' running counts
__device__ __forceinline__ long long marks_rank(const uint16_t* __restrict__ marks, const long long* __restrict__ tile_run, long long tiles, long long x)
{
    const long long tile = x / TILE_BYTES;
    if (tile >= tiles) return tile_run[tiles];
    long long rank = tile_run[tile];
    const int word = (int)((x - tile * TILE_BYTES) >> 4), bit = (int)(x & 15);
    for (int w = 0; w < word; ++w) rank += __popc((unsigned)marks[tile * 64 + w]);
    return rank + __popc((unsigned)marks[tile * 64 + word] & ((1u << bit) - 1u));
}

// The marked bytes (line starts) of one tile, handed to the lanes of one wave 64 at a time.  Every lane of the wave must call next()
// together (shuffles).
struct TileLines {
    unsigned m; int incl, total, round;
    long long tile;
    __device__ __forceinline__ void open(const uint16_t* __restrict__ marks, long long t, int lane) {
        tile = t; round = 0;
        m = marks[t * 64 + lane];
        incl = wave_incl_scan((int)__popc(m), lane);
        total = __shfl(incl, 63, 64);
    }
    // the start of line j = 64 * round + lane of the tile, or -1; *index = j
    __device__ __forceinline__ long long next(int lane, int* index) {
        const int j = 64 * round + lane;
        ++round;
        *index = j;
        const int want = j < total ? j : total - 1;                       // (lanes without a line search too: the shuffles need every lane)
        int lo = 0, hi = 63;                                              // the first word whose running count exceeds `want`
        for (int step = 0; step < 6; ++step) {
            const int mid = (lo + hi) >> 1;
            const int c = __shfl(incl, mid, 64);
            if (c > want) hi = mid; else lo = mid + 1;
        }
        unsigned mw = (unsigned)__shfl((int)m, lo, 64);
        const int before = __shfl(incl, lo, 64) - __popc(mw);
        for (int t = want - before; t > 0; --t) mw &= mw - 1;             // (at most 15 rounds)
        const int bit = __ffs((int)mw) - 1;
        return j < total ? tile * TILE_BYTES + 16 * lo + bit : -1;
    }
};

// One round per distinct key among the wave's active lanes -- nearly always one: f(leader, the leader's key, this lane is active and holds
// that key) with every lane of the wave present, so f may shuffle and leave what it summed to lane `leader`.
template <class F> __device__ __forceinline__ void wave_groups(bool active, int key, F f)
{
    unsigned long long todo = __ballot(active);
    while (todo) {                                                      // (todo is the same in every lane; each round clears at least one bit)
        const int leader = __ffsll((long long)todo) - 1;
        const int kk = __shfl(key, leader, 64);
        const bool mine = active && key == kk;
        f(leader, kk, mine);
        todo &= ~__ballot(mine);
    }
}
}  // namespace plat
