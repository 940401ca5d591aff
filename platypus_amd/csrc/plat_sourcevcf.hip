// plat_sourcevcf.hip -- candidate alleles from source VCF lines (plat_source_variants_batch, include/platypus_mi355x.h):
// variantutils.VariantCandidateReader.Variants (variantutils.py:72-159) and isValidVcfLine (:168-197) for the lines the tabix fetches of
// a chunk of regions returned, parsed where they lie: the text goes to the device as it is, and what comes back are the few alleles as
// offsets into it.  The rule of one line is source_rule.hpp (compiled for the host too and tested there); this file finds the lines,
// hands them to lanes, scans and reports.  The text is cut into tiles of TILE_BYTES = 64 aligned 16-byte words, one word per lane of a
// wave; the tile geometry, the newline mask of a word, the workgroup scan and the hand-out of a tile's lines to lanes are wave_tiles.hpp's
// (shared with plat_tabix.hip).  Seven launches:
//   k_src_check   one workgroup: text_off checked (ascending inside [0, text_len]), the status block and the per-region counters reset
//   k_src_mark    one wave per tile: each lane loads its word (one aligned 16-byte load), compares 16 bytes with '\n' and turns that
//                 into the mask of LINE STARTS of its word -- the byte behind a newline (the carry from the word before comes over a
//                 lane shuffle; lane 0 reads one byte) and the first byte of every region that is not empty; marks [word] (16 bits), and
//                 the tile's number of line starts
//   k_src_scan    one workgroup: tile counts to running counts in place (lines), the total
//   k_src_regions one lane per region: the index of its first line (rank of text_off[k] among the marks)
//   k_src_lines<false>  one wave per tile that holds a line start: one lane per line (64 per round) finds its start in the marks (the j-th set
//                 bit of the tile: a search over the lanes' running popcounts by shuffles), parses the five columns, counts its alleles,
//                 reports its verdict (the regions' counters summed over the wave first); the tile's allele count
//   k_src_scan2   one workgroup: tile allele counts and region allele counts to running counts, region_begin, the status block
//   k_src_lines<true>   as the count pass, each lane writing its alleles at tile base + the wave's running count
// A line belongs to the tile its first byte lies in, however long it is: a lane reads its line's first five columns and nothing behind
// them, so a line of megabytes of sample columns costs its marks and one short parse.  Errors go to the status block; nothing traps.
#include <algorithm>

#include "plat_internal.hpp"
#include "source_rule.hpp"
#include "wave_tiles.hpp"

namespace plat {
constexpr unsigned long long SRC_NO_ERROR = ~0ull;

struct SrcScratch {
    uint16_t* marks;                                      // [tiles * 64] line starts of every 16-byte word
    long long* tile_line;                                 // [tiles + 1] lines in front of each tile
    long long* tile_var;                                  // [tiles + 1] alleles in front of each tile
    long long* reg_line0;                                 // [n_regions + 1] index of each region's first line
    long long* reg_var;                                   // [n_regions + 1] alleles of each region, then in front of each region
    long long tiles;
};

// the first k in [0, n] with off[k] >= x (off ascending, n + 1 entries are NOT assumed: k = n means none)
__device__ __forceinline__ int src_lower_bound(const int64_t* __restrict__ off, int n, int64_t x)
{
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (off[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ void __launch_bounds__(BLOCK_SCAN_THREADS)
k_src_check(plat_source_variants_in in, plat_source_variants_out o, SrcScratch z)
{
    __shared__ int s_bad;
    const int tid = threadIdx.x;
    if (tid == 0) s_bad = 0;
    __syncthreads();
    bool bad = false;
    for (int k = tid; k < in.n_regions; k += BLOCK_SCAN_THREADS) {
        const int64_t a = in.text_off[k], b = in.text_off[k + 1];
        if (a < 0 || b < a || b > in.text_len) bad = true;
        z.reg_var[k] = 0;
    }
    if (bad) s_bad = 1;
    __syncthreads();
    if (!s_bad)                                                         // (refused as invalid: the status block is all that is written)
        for (int k = tid; k < 4 * in.n_regions; k += BLOCK_SCAN_THREADS) o.region_stats[k] = 0;
    if (tid == 0) {
        z.reg_var[in.n_regions] = 0;
        o.status[0] = s_bad ? PLAT_ERR_INVALID : 0;
        o.status[1] = s_bad ? -1 : (int64_t)SRC_NO_ERROR;
        o.status[2] = 0; o.status[3] = 0;
    }
}

__global__ void __launch_bounds__(TILE_WAVES * 64)
k_src_mark(plat_source_variants_in in, plat_source_variants_out o, SrcScratch z)
{
    if (o.status[0] == PLAT_ERR_INVALID) return;
    const int lane = threadIdx.x & 63;
    const int64_t lo = in.n_regions ? in.text_off[0] : 0, hi = in.n_regions ? in.text_off[in.n_regions] : 0;      // the regions' bytes: [lo, hi)
    for (long long tile = (long long)blockIdx.x * TILE_WAVES + (threadIdx.x >> 6); tile < z.tiles; tile += (long long)gridDim.x * TILE_WAVES) {
        const int64_t tileAt = tile * TILE_BYTES, at = tileAt + 16 * lane;
        const unsigned nl = word_newlines(in.text, at, lo, hi);
        // line starts: the byte behind a newline, while it still lies in a region
        unsigned before = 0;                                                // (lane 0 reads one byte: is the byte in front of the tile a newline?)
        if (lane == 0) before = (tileAt > lo && tileAt - 1 < hi && in.text[tileAt - 1] == '\n') ? 1u : 0u;
        unsigned m = behind_newlines(nl, lane, before);
#pragma unroll
        for (int j = 0; j < 16; ++j) if (at + j >= hi) m &= ~(1u << j);
        // ... and the first byte of every region that holds one (a region's last line may lack its newline)
        for (int k = src_lower_bound(in.text_off, in.n_regions, tileAt); k < in.n_regions; ++k) {
            const int64_t s = in.text_off[k];
            if (s >= tileAt + TILE_BYTES) break;
            if (in.text_off[k + 1] > s && s >= at && s < at + 16) m |= 1u << (int)(s - at);
        }
        z.marks[tile * 64 + lane] = (uint16_t)m;
        int c = __popc(m);
        for (int d = 32; d > 0; d >>= 1) c += __shfl_xor(c, d, 64);
        if (lane == 0) z.tile_line[tile] = c;
    }
}

__global__ void __launch_bounds__(BLOCK_SCAN_THREADS)
k_src_scan(plat_source_variants_out o, SrcScratch z)
{
    __shared__ long long s_wave[BLOCK_SCAN_THREADS / 64];
    if (o.status[0] == PLAT_ERR_INVALID) return;
    const long long total = block_scan_inplace<BLOCK_SCAN_THREADS>(z.tile_line, z.tiles, s_wave);
    if (threadIdx.x == 0) { z.tile_line[z.tiles] = total; o.status[3] = total; }
}

__global__ void __launch_bounds__(256)
k_src_regions(plat_source_variants_in in, plat_source_variants_out o, SrcScratch z)
{
    if (o.status[0] == PLAT_ERR_INVALID) return;
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k > in.n_regions) return;
    z.reg_line0[k] = marks_rank(z.marks, z.tile_line, z.tiles, in.text_off[k]);      // the line starts in front of its first byte
}

// the region of the line that starts at byte s: the last one that begins at or before it (the empty regions in front of it share its offset)
__device__ __forceinline__ int src_region_of(const plat_source_variants_in& in, int64_t s)
{
    int k = src_lower_bound(in.text_off, in.n_regions + 1, s + 1) - 1;
    if (k < 0) k = 0;
    if (k >= in.n_regions) k = in.n_regions - 1;
    return k;
}

template <bool WRITE>
__global__ void __launch_bounds__(TILE_WAVES * 64)
k_src_lines(plat_source_variants_in in, plat_source_variants_out o, SrcScratch z)
{
    if (o.status[0] == PLAT_ERR_INVALID) return;
    const int lane = threadIdx.x & 63;
    for (long long tile = (long long)blockIdx.x * TILE_WAVES + (threadIdx.x >> 6); tile < z.tiles; tile += (long long)gridDim.x * TILE_WAVES) {
        const long long line0 = z.tile_line[tile];
        if (z.tile_line[tile + 1] == line0) {                              // (wave-uniform: most tiles of wide lines hold no line start)
            if (!WRITE && lane == 0) z.tile_var[tile] = 0;
            continue;
        }
        TileLines L;
        L.open(z.marks, tile, lane);
        long long run = WRITE ? z.tile_var[tile] : 0;                    // alleles in front of this round's lines
        for (int done = 0; done < L.total; done += 64) {
            int j;
            const int64_t s = L.next(lane, &j);
            int n = 0;
            int k = 0;
            int32_t lineNo = 0;
            int nSkipped = 0, nInvalid = 0, nOver = 0;
            if (s >= 0) {
                k = src_region_of(in, s);
                lineNo = (int32_t)(line0 + j - z.reg_line0[k]);
                const srcrule::LineResult r = srcrule::parse_line(in.text, s, in.text_off[k + 1], in.maxSize, in.longHaps, srcrule::NoEmit());
                if (r.verdict == srcrule::LINE_OK) n = r.emitted;
                nSkipped = r.verdict == srcrule::LINE_SKIPPED; nInvalid = r.verdict == srcrule::LINE_INVALID; nOver = r.oversize;
                if (!WRITE && r.verdict == srcrule::LINE_BAD)
                    atomicMin((unsigned long long*)&o.status[1], ((unsigned long long)(unsigned)k << 32) | (unsigned long long)(unsigned)lineNo);
            }
            if (!WRITE) {
                // the round's counts per region: summed over the wave's lanes of one region first (a region's thousands of lines would
                // otherwise meet at one address), one round per distinct region of the wave -- nearly always one
                wave_groups(s >= 0, k, [&](int leader, int kk, bool mine) {
                    int v0 = mine ? n : 0, v1 = mine ? nSkipped : 0, v2 = mine ? nInvalid : 0, v3 = mine ? nOver : 0;
                    for (int d = 32; d > 0; d >>= 1) {
                        v0 += __shfl_xor(v0, d, 64); v1 += __shfl_xor(v1, d, 64); v2 += __shfl_xor(v2, d, 64); v3 += __shfl_xor(v3, d, 64);
                    }
                    if (lane == leader) {
                        if (v0) atomicAdd((unsigned long long*)&z.reg_var[kk], (unsigned long long)v0);
                        if (v1) atomicAdd(&o.region_stats[4 * kk + 1], v1);
                        if (v2) atomicAdd(&o.region_stats[4 * kk + 2], v2);
                        if (v3) atomicAdd(&o.region_stats[4 * kk + 3], v3);
                    }
                });
            }
            const int incl = wave_incl_scan(n, lane);
            if (WRITE && n) {
                long long at = run + incl - n;
                const uint64_t nameHash = (uint64_t)in.name_hash[k];
                const uint8_t* text = in.text;
                const int64_t cap = o.cap_variants;
                srcrule::parse_line(in.text, s, in.text_off[k + 1], in.maxSize, in.longHaps,
                                    [&](int32_t pos, int64_t remOff, int32_t nRem, int64_t addOff, int32_t nAdd) {
                                        if (at < cap) {
                                            o.pos[at] = pos; o.rem_off[at] = remOff; o.n_rem[at] = nRem; o.add_off[at] = addOff; o.n_add[at] = nAdd;
                                            o.hash[at] = srcrule::py2_variant_hash32(nameHash, pos, text + remOff, nRem, text + addOff, nAdd);
                                            o.line[at] = lineNo;
                                        }
                                        ++at;
                                    });
            }
            run += __shfl(incl, 63, 64);
        }
        if (!WRITE && lane == 0) z.tile_var[tile] = run;
    }
}

__global__ void __launch_bounds__(BLOCK_SCAN_THREADS)
k_src_scan2(plat_source_variants_in in, plat_source_variants_out o, SrcScratch z)
{
    __shared__ long long s_wave[BLOCK_SCAN_THREADS / 64];
    if (o.status[0] == PLAT_ERR_INVALID) return;
    const long long total = block_scan_inplace<BLOCK_SCAN_THREADS>(z.tile_var, z.tiles, s_wave);
    __syncthreads();
    block_scan_inplace<BLOCK_SCAN_THREADS>(z.reg_var, in.n_regions, s_wave);
    __syncthreads();
    const long long cap = o.cap_variants;
    for (int k = threadIdx.x; k <= in.n_regions; k += BLOCK_SCAN_THREADS) {
        const long long b = k < in.n_regions ? z.reg_var[k] : total;
        o.region_begin[k] = (int32_t)(b < cap ? b : cap);                // (PLAT_ERR_OVERFLOW: clamped, nothing lies behind the capacity)
        if (k < in.n_regions) o.region_stats[4 * k] = (int32_t)(z.reg_line0[k + 1] - z.reg_line0[k]);
    }
    if (threadIdx.x == 0) {
        z.tile_var[z.tiles] = total;
        const unsigned long long key = (unsigned long long)o.status[1];
        const bool refused = key != SRC_NO_ERROR;
        o.status[0] = refused ? PLAT_ERR_BAD_INPUT : total > cap ? PLAT_ERR_OVERFLOW : 0;
        o.status[1] = refused ? (int64_t)key : -1;
        o.status[2] = total;
    }
}
}  // namespace plat

PLAT_EXPORT int plat_source_variants_batch(plat_ctx* ctx, const plat_source_variants_in* in, const plat_source_variants_out* out, void* stream)
{
    if (!ctx || !in || !out) return PLAT_ERR_INVALID;
    const plat_source_variants_in& q = *in;
    const plat_source_variants_out& o = *out;
    if (q.n_regions < 0 || q.text_len < 0 || q.maxSize < 0 || o.cap_variants < 0) return PLAT_ERR_INVALID;
    if (!q.text_off || !o.status || !o.region_begin) return PLAT_ERR_INVALID;
    if (q.n_regions > 0 && (!q.name_hash || !o.region_stats)) return PLAT_ERR_INVALID;
    if (q.text_len > 0 && (!q.text || ((uintptr_t)q.text & 15))) return PLAT_ERR_INVALID;
    if (o.cap_variants > 0 && (!o.pos || !o.rem_off || !o.n_rem || !o.add_off || !o.n_add || !o.hash || !o.line)) return PLAT_ERR_INVALID;
    if (q.text_len > (int64_t)INT32_MAX - plat::TILE_BYTES || o.cap_variants > INT32_MAX) return PLAT_ERR_OVERFLOW;      // (line numbers and region_begin are 32-bit)
    PLAT_HIP(ctx, hipSetDevice(ctx->device));
    const hipStream_t st = (hipStream_t)stream;
    plat::SrcScratch z;
    z.tiles = (q.text_len + plat::TILE_BYTES - 1) / plat::TILE_BYTES;
    const size_t marksBytes = ((size_t)z.tiles * 64 * sizeof(uint16_t) + 15) & ~(size_t)15;
    const size_t perTile = ((size_t)z.tiles + 2) * sizeof(long long), perRegion = ((size_t)q.n_regions + 2) * sizeof(long long);
    const int rc = plat_reserve(ctx, ctx->srcvcf, marksBytes + 2 * perTile + 2 * perRegion);
    if (rc != PLAT_OK) return rc;
    uint8_t* base = (uint8_t*)ctx->srcvcf.ptr;
    z.marks = (uint16_t*)base;
    z.tile_line = (long long*)(base + marksBytes);
    z.tile_var = (long long*)(base + marksBytes + perTile);
    z.reg_line0 = (long long*)(base + marksBytes + 2 * perTile);
    z.reg_var = (long long*)(base + marksBytes + 2 * perTile + perRegion);
    const unsigned tileBlocks = (unsigned)std::max<long long>(1, std::min<long long>((z.tiles + plat::TILE_WAVES - 1) / plat::TILE_WAVES, plat::TILE_GRID_CAP));
    const dim3 tileThreads(plat::TILE_WAVES * 64);
    PLAT_LAUNCH(ctx, PLAT_KT_OTHER, st, plat::k_src_check, dim3(1), dim3(plat::BLOCK_SCAN_THREADS), 0, q, o, z);
    PLAT_LAUNCH(ctx, PLAT_KT_OTHER, st, plat::k_src_mark, dim3(tileBlocks), tileThreads, 0, q, o, z);
    PLAT_LAUNCH(ctx, PLAT_KT_OTHER, st, plat::k_src_scan, dim3(1), dim3(plat::BLOCK_SCAN_THREADS), 0, o, z);
    PLAT_LAUNCH(ctx, PLAT_KT_OTHER, st, plat::k_src_regions, dim3((unsigned)(q.n_regions / 256 + 1)), dim3(256), 0, q, o, z);
    PLAT_LAUNCH(ctx, PLAT_KT_OTHER, st, plat::k_src_lines<false>, dim3(tileBlocks), tileThreads, 0, q, o, z);
    PLAT_LAUNCH(ctx, PLAT_KT_OTHER, st, plat::k_src_scan2, dim3(1), dim3(plat::BLOCK_SCAN_THREADS), 0, q, o, z);
    PLAT_LAUNCH(ctx, PLAT_KT_OTHER, st, plat::k_src_lines<true>, dim3(tileBlocks), tileThreads, 0, q, o, z);
    PLAT_HIP(ctx, hipGetLastError());
    return PLAT_OK;
}
