// plat_bgzfout.hip -- record text deflated to BGZF blocks on the device (plat_bgzf_deflate_batch, include/platypus_mi355x.h has the rule).
// The codes, the token word, the header and the trailer are bgzf_deflate.hpp, which also restates the rule serially for the host: same bytes.
//   k_dfl_plan    one workgroup: piece_off checked, blocks per piece scanned to piece_blk (the first block of every piece)
//   k_dfl_block   one workgroup of 1024 per block (grid-stride over the blocks), 131 KiB of LDS in two 64 KiB regions that change hands:
//       A  payload | head table.   A1, all waves: the hash of every position and, by a bitonic sort of (hash, lane) inside each wave's
//          tile of 64 positions, the nearest earlier position of the tile with the same hash and whether a later one exists.  A2, wave 0,
//          tile after tile in order: the head table read, then written by each hash's last position of the tile -- one writer per entry, so
//          no atomics and no dependence on lane order; the candidate is the one inside the tile if there is one, else the table's.  A3, all
//          threads: the match length of every position against the payload in LDS, four bytes a step -> the token word of every position.
//       B  step bytes | last-position bytes.   The greedy parse is a chain p -> p + max(1, len).  Per segment of 252 positions one thread
//          walks right to left: the last chain position inside the segment from every entry; thread 0 then hops from segment to
//          segment (at most 260 hops); one thread per segment marks the chain inside it from the segment's entry.
//       C  output words | payload again.   Each thread owns 64 positions (a 64-bit mask of the chain): bits per thread, a workgroup scan,
//          the codes put together with LDS atomicOr (commutative: deterministic); stored instead when that is no shorter; CRC32 over 64-byte
//          slices combined with crc_shift; the block goes to its slot in scratch memory, the deflate data as aligned dwords.
//   k_dfl_scan    one workgroup: block sizes to offsets, the capacity check, piece_out_off, the status block, the zeroed slack
//   k_dfl_copy    one workgroup per block: slot -> its place in the output (nothing on overflow)
// The per-position words between the phases (4 bytes each) live in scratch memory, 256 KiB per workgroup of the grid.
// Block b, whose payload begins at text offset t, has the slot at align4(t) + 36 b + 2: slots never overlap (a block is at most 31 bytes
// longer than its payload) and the deflate data, 18 bytes in, is dword aligned.
#include <algorithm>
#include "plat_internal.hpp"
#include "bgzf_deflate.hpp"
#include "wave_tiles.hpp"

namespace plat {
constexpr int DFL_THREADS = 1024, DFL_WAVES = DFL_THREADS / 64;
constexpr uint32_t DFL_PAYLOAD = bgzf::DEFLATE_PAYLOAD;
constexpr uint32_t DFL_REGION = 65536;                                                // bytes of each LDS region
constexpr uint32_t DFL_SEG = 252;                                                     // (63 dwords: the segments' threads fall on different banks)
constexpr uint32_t DFL_MAX_SEGS = (DFL_PAYLOAD + DFL_SEG - 1) / DFL_SEG;
constexpr long long DFL_SLOT_STEP = 36;
constexpr int DFL_COPY_THREADS = 256, DFL_COPY_GRID_CAP = 4096;
static_assert(DFL_PAYLOAD <= DFL_REGION && DFL_PAYLOAD + 5 <= DFL_REGION && DFL_PAYLOAD == 64u * 1020u, "a block fits a region; 1020 tiles of 64 positions");
static_assert(DFL_MAX_SEGS <= DFL_THREADS && DFL_SEG <= 256, "one thread per segment; an offset inside a segment is a byte");
static_assert(DFL_PAYLOAD <= 64u * DFL_THREADS, "64 positions per thread cover a block");
static_assert(DFL_PAYLOAD + 8 <= DFL_REGION, "the match compare reads one aligned dword ahead");

struct DflLds {
    uint8_t r0[DFL_REGION];
    uint8_t r1[DFL_REGION];
    uint32_t crc[256];
    uint32_t entry[DFL_MAX_SEGS];
    uint8_t tile[DFL_WAVES][64];
    long long wave_sum[DFL_WAVES];
    uint32_t wave_crc[DFL_WAVES];
};

struct DflScratch {                                                                   // the call's carve of ctx->deflate
    long long* piece_blk;                                                             // [n_pieces + 1]
    long long* meta;                                                                  // {blocks, piece_off refused, the copy may run, -}
    long long* blk_at;                                                                // [max_blocks + 1] sizes, then offsets
    long long* blk_slot;                                                              // [max_blocks]
    uint32_t* words;                                                                  // [grid][DFL_REGION]
    uint8_t* slots;
};

// LDS writes of this wave's lanes are visible to its other lanes behind this.  The lanes that talk are one wave's, whose LDS operations
// complete in order: fences of wavefront scope order the compiler and wait for nothing (a workgroup fence would drain the wave's
// global loads and stores at every tile step of A2)
__device__ __forceinline__ void dfl_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// src[0 .. n) to LDS: whole aligned dwords of src, the bytes in front of and behind them one by one (nothing outside src[0 .. n) is read)
__device__ __forceinline__ void dfl_stage(uint8_t* dst, const uint8_t* __restrict__ src, uint32_t n, int tid) {
    const uint32_t lead = min((uint32_t)((4u - (uint32_t)((uintptr_t)src & 3u)) & 3u), n);
    const uint32_t words = (n - lead) >> 2;
    if ((uint32_t)tid < lead) dst[tid] = src[tid];
    for (uint32_t w = tid; w < words; w += DFL_THREADS) {
        const uint32_t v = *(const uint32_t*)(src + lead + 4u * w);
        uint8_t* d = dst + lead + 4u * w;
        d[0] = (uint8_t)v; d[1] = (uint8_t)(v >> 8); d[2] = (uint8_t)(v >> 16); d[3] = (uint8_t)(v >> 24);
    }
    const uint32_t tail = lead + 4u * words;
    if (tail + (uint32_t)tid < n) dst[tail + tid] = src[tail + tid];
}

__device__ __forceinline__ void dfl_zero(uint8_t* region, int tid) {
    for (uint32_t k = tid; k < DFL_REGION / 4u; k += DFL_THREADS) ((uint32_t*)region)[k] = 0u;
}

__device__ __forceinline__ uint32_t dfl_step(uint32_t step_byte) { return step_byte ? step_byte + 3u : 1u; }      // (the byte: 0 a literal, else length - 3)

__global__ void __launch_bounds__(BLOCK_SCAN_THREADS)
k_dfl_plan(plat_bgzf_deflate_in in, DflScratch s)
{
    __shared__ long long s_wave[BLOCK_SCAN_THREADS / 64];
    __shared__ int s_bad;
    const int tid = threadIdx.x;
    if (tid == 0) s_bad = 0;
    __syncthreads();
    for (long long i = tid; i < in.n_pieces; i += BLOCK_SCAN_THREADS) {
        const long long a = in.piece_off[i], b = in.piece_off[i + 1];
        if (a < 0 || b < a || b > in.text_len || (i == 0 && a != 0)) s_bad = 1;
    }
    __syncthreads();
    const bool bad = s_bad != 0;
    for (long long i = tid; i < in.n_pieces; i += BLOCK_SCAN_THREADS)
        s.piece_blk[i] = bad ? 0 : (in.piece_off[i + 1] - in.piece_off[i] + (long long)DFL_PAYLOAD - 1) / (long long)DFL_PAYLOAD;
    __syncthreads();
    const long long blocks = block_scan_inplace<BLOCK_SCAN_THREADS>(s.piece_blk, (long long)in.n_pieces, s_wave);
    if (tid == 0) { s.piece_blk[in.n_pieces] = blocks; s.meta[0] = blocks; s.meta[1] = bad ? 1 : 0; s.meta[2] = 0; s.meta[3] = 0; }
}

// one block: src[0 .. n), 1 <= n <= DFL_PAYLOAD, to slot; returns the block's length (the same in every thread)
__device__ uint32_t dfl_block(DflLds& L, const uint8_t* __restrict__ src, uint32_t n, int level, uint32_t* __restrict__ words, uint8_t* __restrict__ slot)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint8_t* const r0 = L.r0;
    uint8_t* const r1 = L.r1;
    bool stored = level <= 0;
    uint32_t body = n + 5u;
    if (!stored) {
        // ---- A: payload in r0, the head table (per hash the last position + 1, 16 bits) in r1
        uint16_t* const head = (uint16_t*)r1;
        dfl_stage(r0, src, n, tid);
        dfl_zero(r1, tid);
        __syncthreads();
        const uint32_t tiles = (n + 63u) >> 6;
        // A1: words[p] = hash | last of its hash in the tile << 15 | (the nearest earlier position of the tile with the same hash + 1) << 16
        for (uint32_t t = wave; t < tiles; t += DFL_WAVES) {
            const uint32_t p = 64u * t + lane;
            const bool valid = p + 4u <= n;
            const uint32_t h = valid ? bgzf::deflate_hash(bgzf::ld32(r0 + p)) : 0x8000u;                  // (positions without a hash sort behind the others)
            uint32_t key = (h << 6) | (uint32_t)lane;
            for (int k = 2; k <= 64; k <<= 1)
                for (int j = k >> 1; j > 0; j >>= 1) {
                    const uint32_t other = (uint32_t)__shfl_xor((int)key, j, 64);
                    const bool up = (lane & k) == 0, low = (lane & j) == 0;
                    key = (low == up) ? min(key, other) : max(key, other);
                }
            const uint32_t before = (uint32_t)__shfl_up((int)key, 1, 64), behind = (uint32_t)__shfl_down((int)key, 1, 64);
            const bool has = lane > 0 && (before >> 6) == (key >> 6), last = lane == 63 || (behind >> 6) != (key >> 6);
            dfl_wave_sync();                                                                            // (the round before has read its answers)
            L.tile[wave][key & 63u] = (uint8_t)((has ? (before & 63u) + 1u : 0u) | (last ? 0x80u : 0u));
            dfl_wave_sync();
            const uint32_t r = L.tile[wave][lane];
            if (valid) words[p] = h | ((r & 0x80u) ? 0x8000u : 0u) | ((r & 0x7fu) ? (64u * t + (r & 0x7fu)) << 16 : 0u);
        }
        __syncthreads();
        // A2: words[p] = the candidate + 1, or 0.  Four tiles' words are loaded ahead of the table walk.
        if (wave == 0) {
            uint32_t cur[4], nxt[4];
            for (int j = 0; j < 4; ++j) { const uint32_t p = 64u * j + lane; cur[j] = p + 4u <= n ? words[p] : 0u; }
            for (uint32_t t0 = 0; t0 < tiles; t0 += 4) {
                for (int j = 0; j < 4; ++j) { const uint32_t p = 64u * (t0 + 4u + j) + lane; nxt[j] = p + 4u <= n ? words[p] : 0u; }
                for (int j = 0; j < 4; ++j) {
                    const uint32_t p = 64u * (t0 + j) + lane;
                    const bool valid = p + 4u <= n;
                    const uint32_t a = cur[j], h = a & 0x7fffu;
                    const uint32_t prior = valid ? head[h] : 0u;
                    dfl_wave_sync();                                                                    // (every lane has read before one writes)
                    if (valid && (a & 0x8000u)) head[h] = (uint16_t)(p + 1u);
                    dfl_wave_sync();
                    if (valid) words[p] = (a >> 16) ? (a >> 16) : prior;
                }
                for (int j = 0; j < 4; ++j) cur[j] = nxt[j];
            }
        }
        __syncthreads();
        // A3: words[p] = the token at p
        for (uint32_t p = tid; p < n; p += DFL_THREADS) {
            const uint32_t c = p + 4u <= n ? words[p] : 0u;
            uint32_t len = 0, dist = 0;
            if (c && p - (c - 1u) <= bgzf::DEFLATE_MAX_DIST) {
                const uint32_t q = c - 1u, cap = min(n - p, bgzf::DEFLATE_MAX_MATCH);
                dist = p - q;
                // four bytes a step from aligned dwords of the payload: the dword read ahead lies inside the region (n + 7 < DFL_REGION) and no byte
                // behind n is compared (len + 4 <= cap)
                const uint32_t* const w0 = (const uint32_t*)r0;
                const uint32_t sp = (p & 3u) * 8u, sq = (q & 3u) * 8u;
                uint32_t ip = p >> 2, iq = q >> 2, pa = w0[ip], qa = w0[iq];
                bool differ = false;
                while (len + 4u <= cap) {
                    const uint32_t pb = w0[++ip], qb = w0[++iq];
                    const uint32_t d = __funnelshift_r(pa, pb, sp) ^ __funnelshift_r(qa, qb, sq);
                    if (d) { len += (uint32_t)(__ffs((int)d) - 1) >> 3; differ = true; break; }
                    len += 4u; pa = pb; qa = qb;
                }
                if (!differ) while (len < cap && r0[q + len] == r0[p + len]) ++len;
                if (len < bgzf::DEFLATE_MIN_MATCH) len = 0;
            }
            words[p] = bgzf::token_word(len, r0[p], dist);
        }
        __syncthreads();
        // ---- B: step bytes in r0; in r1 per position the last chain position of its segment, then the chain's marks
        for (uint32_t p = tid; p < n; p += DFL_THREADS) { const uint32_t len = bgzf::token_len(words[p]); r0[p] = (uint8_t)(len ? len - 3u : 0u); }
        const uint32_t segs = (n + DFL_SEG - 1u) / DFL_SEG;
        if ((uint32_t)tid < DFL_MAX_SEGS) L.entry[tid] = 0xffffffffu;
        __syncthreads();
        if ((uint32_t)tid < segs) {
            const int seg_start = (int)(DFL_SEG * (uint32_t)tid), seg_end = (int)min(n, DFL_SEG * (uint32_t)tid + DFL_SEG);
            for (int p = seg_end - 1; p >= seg_start; --p) {
                const int nx = p + (int)dfl_step(r0[p]);
                r1[p] = nx >= seg_end ? (uint8_t)(p - seg_start) : r1[nx];
            }
        }
        __syncthreads();
        if (tid == 0) {
            uint32_t e = 0;
            while (e < n) {                                                                             // (every hop leaves a segment: at most DFL_MAX_SEGS hops)
                const uint32_t sg = e / DFL_SEG;
                L.entry[sg] = e;
                const uint32_t q = DFL_SEG * sg + r1[e];
                e = q + dfl_step(r0[q]);
            }
        }
        __syncthreads();
        dfl_zero(r1, tid);
        __syncthreads();
        if ((uint32_t)tid < segs && L.entry[tid] != 0xffffffffu) {
            const uint32_t seg_end = min(n, DFL_SEG * (uint32_t)tid + DFL_SEG);
            for (uint32_t p = L.entry[tid]; p < seg_end; p += dfl_step(r0[p])) r1[p] = 1;
        }
        __syncthreads();
        // ---- C: positions 64 tid .. 64 tid + 63 are this thread's; output words in r0
        const uint32_t base = 64u * (uint32_t)tid;
        uint64_t mask = 0;
        if (base < n)
            for (uint32_t j = 0; j < 16; ++j) {
                const uint32_t w = ((const uint32_t*)r1)[base / 4u + j];                                // (bytes behind n are zero)
                mask |= (uint64_t)((w & 1u) | ((w >> 7) & 2u) | ((w >> 14) & 4u) | ((w >> 21) & 8u)) << (4u * j);
            }
        __syncthreads();
        dfl_zero(r0, tid);
        long long bits = 0;
        for (uint64_t m = mask; m; m &= m - 1) { int nb; bgzf::token_code(words[base + (uint32_t)(__ffsll((long long)m) - 1)], &nb); bits += nb; }
        const long long incl = wave_incl_scan(bits, lane);
        if (lane == 63) L.wave_sum[wave] = incl;
        __syncthreads();
        long long at = 3 + incl - bits, all = 0;
        for (int w = 0; w < DFL_WAVES; ++w) { if (w < wave) at += L.wave_sum[w]; all += L.wave_sum[w]; }
        body = bgzf::coded_bytes((uint64_t)all);
        stored = body >= n + 5u;
        if (stored) body = n + 5u;
        else {
            uint32_t* const out = (uint32_t*)r0;                                                        // (body < n + 5: the last word touched lies inside the region)
            if (tid == 0) atomicOr(&out[0], 3u);                                                        // BFINAL 1, BTYPE 01; end-of-block is seven zero bits
            for (uint64_t m = mask; m; m &= m - 1) {
                int nb;
                const uint32_t v = bgzf::token_code(words[base + (uint32_t)(__ffsll((long long)m) - 1)], &nb);
                const uint64_t vv = (uint64_t)v << (at & 31);
                atomicOr(&out[at >> 5], (uint32_t)vv);
                if (vv >> 32) atomicOr(&out[(at >> 5) + 1], (uint32_t)(vv >> 32));
                at += nb;
            }
        }
    }
    // the payload (again) in r1: the CRC32 and a stored block's bytes
    dfl_stage(r1, src, n, tid);
    __syncthreads();
    uint32_t crc = 0;
    {
        const uint32_t a = min(64u * (uint32_t)tid, n), b = min(a + 64u, n);
        if (b > a) crc = bgzf::crc_shift(bgzf::crc_bytes(L.crc, r1 + a, (int64_t)(b - a)), n - b);
        for (int d = 32; d >= 1; d >>= 1) crc ^= (uint32_t)__shfl_xor((int)crc, d, 64);
        if (lane == 0) L.wave_crc[wave] = crc;
        __syncthreads();
        crc = 0;
        for (int w = 0; w < DFL_WAVES; ++w) crc ^= L.wave_crc[w];
    }
    const uint32_t block_len = bgzf::BLOCK_HEADER_BYTES + body + bgzf::BLOCK_TRAILER_BYTES;
    if ((uint32_t)tid < bgzf::BLOCK_HEADER_BYTES) slot[tid] = bgzf::header_byte((uint32_t)tid, block_len);
    if (tid >= 64 && tid < 64 + (int)bgzf::BLOCK_TRAILER_BYTES) slot[block_len - bgzf::BLOCK_TRAILER_BYTES + (uint32_t)(tid - 64)] = bgzf::trailer_byte((uint32_t)(tid - 64), crc, n);
    uint8_t* const z = slot + bgzf::BLOCK_HEADER_BYTES;                                                 // (dword aligned: the slot's address is 2 mod 4)
    const uint32_t body_words = body >> 2;
    if (stored) {
        auto byte_at = [&](uint32_t k) -> uint32_t {
            return k >= 5u ? r1[k - 5u] : k == 0u ? 1u : k == 1u ? (n & 0xffu) : k == 2u ? (n >> 8) : k == 3u ? (~n & 0xffu) : ((~n >> 8) & 0xffu);
        };
        for (uint32_t w = tid; w < body_words; w += DFL_THREADS)
            ((uint32_t*)z)[w] = byte_at(4u * w) | (byte_at(4u * w + 1u) << 8) | (byte_at(4u * w + 2u) << 16) | (byte_at(4u * w + 3u) << 24);
        if (4u * body_words + (uint32_t)tid < body) z[4u * body_words + tid] = (uint8_t)byte_at(4u * body_words + (uint32_t)tid);
    } else {
        for (uint32_t w = tid; w < body_words; w += DFL_THREADS) ((uint32_t*)z)[w] = ((const uint32_t*)r0)[w];
        if (4u * body_words + (uint32_t)tid < body) z[4u * body_words + tid] = r0[4u * body_words + tid];
    }
    return block_len;
}

__global__ void __launch_bounds__(DFL_THREADS)
k_dfl_block(plat_bgzf_deflate_in in, DflScratch s)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t lds_raw[];
    DflLds& L = *reinterpret_cast<DflLds*>(lds_raw);
    const int tid = threadIdx.x;
    for (int k = tid; k < 256; k += DFL_THREADS) L.crc[k] = bgzf::crc_table_entry((uint32_t)k);
    const long long blocks = s.meta[0];
    uint32_t* const words = s.words + (size_t)blockIdx.x * DFL_REGION;
    for (long long b = blockIdx.x; b < blocks; b += gridDim.x) {
        long long lo = 0, hi = in.n_pieces;                                                             // piece_blk[lo] <= b < piece_blk[hi]
        while (hi - lo > 1) { const long long mid = (lo + hi) >> 1; if (s.piece_blk[mid] <= b) lo = mid; else hi = mid; }
        const long long t = in.piece_off[lo] + (b - s.piece_blk[lo]) * (long long)DFL_PAYLOAD;
        const uint32_t n = (uint32_t)min((long long)DFL_PAYLOAD, in.piece_off[lo + 1] - t);
        const long long slot = ((t + 3) & ~3ll) + DFL_SLOT_STEP * b + 2;
        __syncthreads();                                                                                // (the block before has left LDS; the CRC table stands)
        const uint32_t len = dfl_block(L, in.text + t, n, in.level, words, s.slots + slot);
        if (tid == 0) { s.blk_at[b] = len; s.blk_slot[b] = slot; }
    }
}

__global__ void __launch_bounds__(BLOCK_SCAN_THREADS)
k_dfl_scan(int n_pieces, DflScratch s, plat_bgzf_deflate_out o)
{
    __shared__ long long s_wave[BLOCK_SCAN_THREADS / 64];
    __shared__ long long s_first;
    const int tid = threadIdx.x;
    const long long blocks = s.meta[0];
    const bool bad = s.meta[1] != 0;
    if (tid == 0) s_first = INT64_MAX;
    const long long total = block_scan_inplace<BLOCK_SCAN_THREADS>(s.blk_at, blocks, s_wave);
    if (tid == 0) s.blk_at[blocks] = total;
    __syncthreads();
    for (long long i = tid; i <= n_pieces; i += BLOCK_SCAN_THREADS) {
        const long long at = s.blk_at[s.piece_blk[i]];
        if (i < n_pieces && s.blk_at[s.piece_blk[i + 1]] > o.cap_bytes) atomicMin((unsigned long long*)&s_first, (unsigned long long)i);
        o.piece_out_off[i] = min(at, o.cap_bytes);                                                    // (clamped: the offsets stay valid numbers)
    }
    __syncthreads();
    const bool fits = total <= o.cap_bytes;
    if (fits && tid < PLAT_BLOB_PAD) o.data[total + tid] = 0;
    if (tid == 0) {
        o.status[0] = bad ? PLAT_ERR_BAD_INPUT : fits ? 0 : PLAT_ERR_OVERFLOW;
        o.status[1] = fits ? -1 : s_first;
        o.status[2] = total; o.status[3] = blocks;
        s.meta[2] = fits && !bad ? 1 : 0;
    }
}

__global__ void __launch_bounds__(DFL_COPY_THREADS)
k_dfl_copy(DflScratch s, plat_bgzf_deflate_out o)
{
    if (s.meta[2] == 0) return;                                                                         // (on overflow no payload byte is written)
    const long long blocks = s.meta[0];
    const uint32_t tid = threadIdx.x;
    for (long long b = blockIdx.x; b < blocks; b += gridDim.x) {
        const uint8_t* __restrict__ src = s.slots + s.blk_slot[b];
        uint8_t* __restrict__ dst = o.data + s.blk_at[b];
        const uint32_t len = (uint32_t)(s.blk_at[b + 1] - s.blk_at[b]);
        // bytes up to the first aligned dword of the output, dwords, the bytes left
        const uint32_t lead = min((uint32_t)((4u - (uint32_t)((uintptr_t)dst & 3u)) & 3u), len);
        const uint32_t n_words = (len - lead) >> 2;
        if (tid < lead) dst[tid] = src[tid];
        for (uint32_t w = tid; w < n_words; w += DFL_COPY_THREADS) {
            const uint8_t* p = src + lead + 4u * w;
            *(uint32_t*)(dst + lead + 4u * w) = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
        }
        const uint32_t tail = lead + 4u * n_words;
        if (tail + tid < len) dst[tail + tid] = src[tail + tid];
    }
}
}  // namespace plat

PLAT_EXPORT int plat_bgzf_deflate_batch(plat_ctx* ctx, const plat_bgzf_deflate_in* in, const plat_bgzf_deflate_out* out, void* stream)
{
    if (!ctx || !in || !out || in->n_pieces < 0 || in->text_len < 0 || in->level < 0 || in->level > 1 || out->cap_bytes < 0) return PLAT_ERR_INVALID;
    const plat_bgzf_deflate_out& o = *out;
    if (!o.status || !o.piece_out_off || !o.data || ((uintptr_t)o.data & 15)) return PLAT_ERR_INVALID;
    if ((in->n_pieces > 0 && !in->piece_off) || (in->text_len > 0 && !in->text)) return PLAT_ERR_INVALID;
    PLAT_HIP(ctx, hipSetDevice(ctx->device));
    const hipStream_t st = (hipStream_t)stream;
    const long long max_blocks = in->text_len / (long long)plat::DFL_PAYLOAD + in->n_pieces;
    const int grid = (int)std::min<long long>(max_blocks, ctx->n_cu > 0 ? ctx->n_cu : 256);
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t b_piece = up(((size_t)in->n_pieces + 1) * 8), b_meta = up(4 * 8), b_at = up(((size_t)max_blocks + 1) * 8), b_slot = up(((size_t)max_blocks + 1) * 8);
    const size_t b_words = up((size_t)std::max(grid, 1) * plat::DFL_REGION * 4), b_slots = up((size_t)in->text_len + (size_t)plat::DFL_SLOT_STEP * (size_t)max_blocks + 16);
    const int rc = plat_reserve(ctx, ctx->deflate, b_piece + b_meta + b_at + b_slot + b_words + b_slots);
    if (rc != PLAT_OK) return rc;
    uint8_t* base = (uint8_t*)ctx->deflate.ptr;
    plat::DflScratch s;
    s.piece_blk = (long long*)base; base += b_piece;
    s.meta = (long long*)base; base += b_meta;
    s.blk_at = (long long*)base; base += b_at;
    s.blk_slot = (long long*)base; base += b_slot;
    s.words = (uint32_t*)base; base += b_words;
    s.slots = base;
    PLAT_LAUNCH(ctx, PLAT_KT_OTHER, st, plat::k_dfl_plan, dim3(1), dim3(plat::BLOCK_SCAN_THREADS), 0, *in, s);
    if (max_blocks > 0) {
        PLAT_HIP(ctx, hipFuncSetAttribute((const void*)plat::k_dfl_block, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(plat::DflLds)));
        PLAT_LAUNCH(ctx, PLAT_KT_OTHER, st, plat::k_dfl_block, dim3((unsigned)grid), dim3(plat::DFL_THREADS), sizeof(plat::DflLds), *in, s);
    }
    PLAT_LAUNCH(ctx, PLAT_KT_OTHER, st, plat::k_dfl_scan, dim3(1), dim3(plat::BLOCK_SCAN_THREADS), 0, in->n_pieces, s, o);
    if (max_blocks > 0)
        PLAT_LAUNCH(ctx, PLAT_KT_OTHER, st, plat::k_dfl_copy, dim3((unsigned)std::min<long long>(max_blocks, plat::DFL_COPY_GRID_CAP)), dim3(plat::DFL_COPY_THREADS), 0, s, o);
    PLAT_HIP(ctx, hipGetLastError());
    return PLAT_OK;
}
