// plat_tabix.hip -- tabix's iterator over inflated BGZF blocks (plat_tabix_fetch_batch, include/platypus_mi355x.h): ti_iter_read
// (src/tabix/index.c.pysam.c:872-911) for the streams of a chunk of regions, over the bytes plat_bgzf_inflate_batch left, without the host
// ever seeing an inflated byte but the kept lines.  The rule of one line is tabix_rule.hpp (compiled for the host too and tested there);
// this file finds the lines, hands them to lanes, finds each stream's stop, scans and copies.  The data is cut into tiles of TILE_BYTES
// = 64 aligned 16-byte words, one word per lane of a wave; the tile geometry, the newline mask of a word, the rank of a byte among the
// marks, the workgroup scan and the hand-out of a tile's lines to lanes are wave_tiles.hpp's (shared with plat_sourcevcf.hip).  Seven launches:
//   k_tbx_check    one workgroup: the geometry checked; per chunk its bytes [lo, hi), its first offset and its stop as offsets into data; the
//                  streams' keys, counters and the status block reset
//   k_tbx_mark     one wave per tile: each lane loads its word (one aligned 16-byte load), compares 16 bytes with '\n': nl [word] (16 bits, the
//                  newlines) and marks [word] (the LINE STARTS: a chunk's first offset and the byte behind a newline, while it lies in front
//                  of the chunk's stop; the carry from the word before comes over a lane shuffle, lane 0 reads one byte); the tile's counts
//   k_tbx_scan     one workgroup: both tile counts to running counts; one lane per chunk that holds no line and starts past its stop
//   k_tbx_verdict  one wave per tile that holds a line start, one lane per line (64 per round): the line's end is the r-th newline of the
//                  data, r the newlines in front of its start (a binary search over the tiles' running counts and one tile's marks: no lane
//                  walks the line); columns 1 to 8, the verdict; a stopping or refusing line, and a chunk's last line that runs past the stop
//                  of a chunk that is not its stream's last, lower the stream's key (atomicMin: the first of them in chunk order)
//   k_tbx_count    the same lanes: lines ahead of their stream's key count; walked / kept per stream (summed over the wave first), the tile's
//                  kept bytes
//   k_tbx_scan2    one workgroup: tile bytes and stream bytes to running counts, stream_text_off, the status block, the pad zeroed
//   k_tbx_copy     one wave per tile with kept bytes: one lane per line finds its place, then the WAVE copies each kept line, 16 bytes per
//                  lane with aligned stores, and ends it with '\n'
// A line belongs to the tile its first byte lies in, however long it is.  Errors go to the status block; nothing traps.
#include <algorithm>

#include "plat_internal.hpp"
#include "tabix_rule.hpp"
#include "wave_tiles.hpp"

namespace plat {
constexpr unsigned long long TBX_NO_KEY = ~0ull - 1;      // (even: an odd key is a refusal)
// a stream's key: 8 * (index of a line among the call's lines) + what happens there; line j counts while 8 j + 4 <= key
constexpr int TBX_AT_CHUNK = 1, TBX_AT_STOP = 2, TBX_AT_REFUSE = 3, TBX_BEHIND = 7;

struct TbxScratch {
    uint16_t* marks;                                      // [tiles * 64] line starts of every 16-byte word
    uint16_t* nl;                                         // [tiles * 64] its newlines
    long long* tile_line;                                 // [tiles + 1] lines in front of each tile
    long long* tile_nl;                                   // [tiles + 1] newlines in front of each tile
    long long* tile_bytes;                                // [tiles + 1] kept bytes in front of each tile
    long long* c_lo; long long* c_hi; long long* c_first; long long* c_stop;      // [n_chunks] offsets into data; lo <= stop <= hi
    unsigned long long* key;                              // [n_streams]
    long long* stream_bytes;                              // [n_streams + 1]
    long long tiles;
};

// the last k in [0, n) with a[k] <= x (a ascending), or -1
template <class T> __device__ __forceinline__ int tbx_last_le(const T* __restrict__ a, int n, long long x)
{
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if ((long long)a[mid] <= x) lo = mid + 1; else hi = mid;
    }
    return lo - 1;
}

__device__ __forceinline__ void tbx_lower(unsigned long long* key, unsigned long long k) { if (*key > k) atomicMin(key, k); }

__global__ void __launch_bounds__(BLOCK_SCAN_THREADS)
k_tbx_check(plat_tabix_fetch_in in, plat_tabix_fetch_out o, TbxScratch z)
{
    __shared__ int s_bad;
    const int tid = threadIdx.x;
    if (tid == 0) s_bad = 0;
    __syncthreads();
    bool bad = false;
    const long long total = in.n_blocks ? in.out_off[in.n_blocks] : 0;
    if (total < 0 || total > in.data_len) bad = true;
    for (int s = tid; s <= in.n_streams; s += BLOCK_SCAN_THREADS) {
        const int a = in.stream_chunk_begin[s];
        if (a < 0 || a > in.n_chunks || (s == 0 && a != 0) || (s == in.n_streams && a != in.n_chunks)) bad = true;
        if (s < in.n_streams) {
            if (in.stream_chunk_begin[s + 1] < a || in.name_off[s] < 0 || in.name_off[s + 1] < in.name_off[s]) bad = true;
            z.key[s] = TBX_NO_KEY;
            z.stream_bytes[s] = 0;
        }
    }
    for (int c = tid; c < in.n_chunks && !bad; c += BLOCK_SCAN_THREADS) {
        const int b0 = in.chunk_blk_first[c], b1 = in.chunk_blk_end[c], sb = in.chunk_stop_blk[c];
        if (b0 < 0 || b1 < b0 || b1 > in.n_blocks || sb < -1 || sb >= in.n_blocks || in.chunk_first_uoffset[c] < 0 || in.chunk_stop_uoffset[c] < 0 ||
            (c > 0 && b0 < in.chunk_blk_end[c - 1])) { bad = true; break; }
        const long long lo = in.out_off[b0], hi = in.out_off[b1];
        if (lo < 0 || hi < lo || hi > total) { bad = true; break; }
        const long long stop = sb < 0 ? hi : in.out_off[sb] + (long long)in.chunk_stop_uoffset[c];
        z.c_lo[c] = lo; z.c_hi[c] = hi; z.c_first[c] = lo + in.chunk_first_uoffset[c];
        z.c_stop[c] = stop < lo ? lo : stop > hi ? hi : stop;
    }
    if (bad) s_bad = 1;
    __syncthreads();
    if (!s_bad)                                                         // (refused as invalid: the status block is all that is written)
        for (int k = tid; k < 2 * in.n_streams; k += BLOCK_SCAN_THREADS) o.stream_counts[k] = 0;
    if (tid == 0) {
        o.status[0] = s_bad ? PLAT_ERR_INVALID : 0;
        o.status[1] = -1; o.status[2] = 0; o.status[3] = 0;
    }
}

__global__ void __launch_bounds__(TILE_WAVES * 64)
k_tbx_mark(plat_tabix_fetch_in in, plat_tabix_fetch_out o, TbxScratch z)
{
    if (o.status[0] == PLAT_ERR_INVALID) return;
    const int lane = threadIdx.x & 63;
    const long long total = in.n_blocks ? in.out_off[in.n_blocks] : 0;
    for (long long tile = (long long)blockIdx.x * TILE_WAVES + (threadIdx.x >> 6); tile < z.tiles; tile += (long long)gridDim.x * TILE_WAVES) {
        const long long tileAt = tile * TILE_BYTES, at = tileAt + 16 * lane;
        const unsigned nl = word_newlines(in.data, at, 0, total);
        const unsigned behind = behind_newlines(nl, lane, (lane == 0 && tileAt > 0 && tileAt - 1 < total && in.data[tileAt - 1] == '\n') ? 1u : 0u);
        // line starts: per chunk that meets this word, its first offset and the bytes behind its newlines, in front of its stop
        unsigned m = 0;
        if (at < total) {
            int c = tbx_last_le(z.c_lo, in.n_chunks, at);
            if (c < 0) c = 0;
            for (; c < in.n_chunks && z.c_lo[c] < at + 16; ++c) {
                const long long f = z.c_first[c], lim = z.c_stop[c];
                const long long a0 = f + 1 > at ? f + 1 : at, a1 = lim < at + 16 ? lim : at + 16;
                if (a0 < a1) m |= behind & ((1u << (int)(a1 - at)) - (1u << (int)(a0 - at)));
                if (f >= at && f < at + 16 && f < lim) m |= 1u << (int)(f - at);
            }
        }
        z.marks[tile * 64 + lane] = (uint16_t)m;
        z.nl[tile * 64 + lane] = (uint16_t)nl;
        int cm = __popc(m), cn = __popc(nl);
        for (int d = 32; d > 0; d >>= 1) { cm += __shfl_xor(cm, d, 64); cn += __shfl_xor(cn, d, 64); }
        if (lane == 0) { z.tile_line[tile] = cm; z.tile_nl[tile] = cn; }
    }
}

__global__ void __launch_bounds__(BLOCK_SCAN_THREADS)
k_tbx_scan(plat_tabix_fetch_in in, plat_tabix_fetch_out o, TbxScratch z)
{
    __shared__ long long s_wave[BLOCK_SCAN_THREADS / 64];
    if (o.status[0] == PLAT_ERR_INVALID) return;
    const long long lines = block_scan_inplace<BLOCK_SCAN_THREADS>(z.tile_line, z.tiles, s_wave);
    __syncthreads();
    const long long nls = block_scan_inplace<BLOCK_SCAN_THREADS>(z.tile_nl, z.tiles, s_wave);
    if (threadIdx.x == 0) { z.tile_line[z.tiles] = lines; z.tile_nl[z.tiles] = nls; }
    __syncthreads();
    // a chunk without a line whose first offset lies past its stop, and which is not its stream's last: the stream is refused there
    for (int c = threadIdx.x; c < in.n_chunks; c += BLOCK_SCAN_THREADS) {
        const long long f = z.c_first[c];
        if (f <= z.c_stop[c]) continue;
        const int s = tbx_last_le(in.stream_chunk_begin, in.n_streams, c);
        if (c + 1 < in.stream_chunk_begin[s + 1]) tbx_lower(&z.key[s], 8ull * (unsigned long long)marks_rank(z.marks, z.tile_line, z.tiles, f) + TBX_AT_CHUNK);
    }
}

// the line that starts at byte s: its chunk, its stream, its end (its newline, or the end of its chunk's bytes) and the offset behind it
struct TbxLine { int chunk, stream; long long end, behind; bool lastOfChunk; };

__device__ __forceinline__ TbxLine tbx_line_at(const plat_tabix_fetch_in& in, const TbxScratch& z, long long s)
{
    TbxLine L;
    L.chunk = max(tbx_last_le(z.c_lo, in.n_chunks, s), 0);               // (a line start lies in a chunk; the clamps are for offsets that do not ascend)
    L.stream = max(tbx_last_le(in.stream_chunk_begin, in.n_streams, L.chunk), 0);
    const long long hi = z.c_hi[L.chunk];
    // the newline that ends it is newline number r of the data, r = the newlines in front of s
    const long long r = marks_rank(z.nl, z.tile_nl, z.tiles, s);
    long long e = hi;
    if (r < z.tile_nl[z.tiles]) {
        long long t = s / TILE_BYTES;
        if (r >= z.tile_nl[t + 1]) {                                        // not in the line's own tile: the last tile with tile_nl <= r
            long long lo = t + 1, up = z.tiles;
            while (lo < up) {
                const long long mid = lo + (up - lo) / 2;
                if (z.tile_nl[mid] <= r) lo = mid + 1; else up = mid;
            }
            t = lo - 1;
        }
        if (t * TILE_BYTES < hi) {
            int want = (int)(r - z.tile_nl[t]);
            for (int w = 0; w < 64; ++w) {
                unsigned mw = z.nl[t * 64 + w];
                const int c = __popc(mw);
                if (want >= c) { want -= c; continue; }
                for (; want > 0; --want) mw &= mw - 1;
                const long long at = t * TILE_BYTES + 16 * w + (__ffs((int)mw) - 1);
                if (at < hi) e = at;
                break;
            }
        }
    }
    L.end = e;
    L.behind = e < hi ? e + 1 : hi;
    L.lastOfChunk = L.behind >= z.c_stop[L.chunk];
    return L;
}

__device__ __forceinline__ int tbx_verdict(const plat_tabix_fetch_in& in, const TbxLine& L, long long s)
{
    const int32_t n0 = in.name_off[L.stream];
    return tbxrule::line_verdict(in.data, s, L.end, in.names + n0, in.name_off[L.stream + 1] - n0, in.beg[L.stream], in.end[L.stream]);
}

__global__ void __launch_bounds__(TILE_WAVES * 64)
k_tbx_verdict(plat_tabix_fetch_in in, plat_tabix_fetch_out o, TbxScratch z)
{
    if (o.status[0] == PLAT_ERR_INVALID) return;
    const int lane = threadIdx.x & 63;
    for (long long tile = (long long)blockIdx.x * TILE_WAVES + (threadIdx.x >> 6); tile < z.tiles; tile += (long long)gridDim.x * TILE_WAVES) {
        const long long line0 = z.tile_line[tile];
        if (z.tile_line[tile + 1] == line0) continue;                      // (wave-uniform: most tiles of wide lines hold no line start)
        TileLines T;
        T.open(z.marks, tile, lane);
        for (int done = 0; done < T.total; done += 64) {
            int j;
            const long long s = T.next(lane, &j);
            if (s >= 0) {                                                  // (no lane leaves the round early: next() shuffles)
                const TbxLine L = tbx_line_at(in, z, s);
                const unsigned long long at = 8ull * (unsigned long long)(line0 + j);
                if (at + 4 <= z.key[L.stream]) {                           // (behind a stop already found, nothing it says can lower the key)
                    const int v = tbx_verdict(in, L, s);
                    if (v == tbxrule::LINE_STOP) tbx_lower(&z.key[L.stream], at + TBX_AT_STOP);
                    else if (v == tbxrule::LINE_REFUSE) tbx_lower(&z.key[L.stream], at + TBX_AT_REFUSE);
                    else if (L.lastOfChunk && L.behind > z.c_stop[L.chunk] && L.chunk + 1 < in.stream_chunk_begin[L.stream + 1])
                        tbx_lower(&z.key[L.stream], at + TBX_BEHIND);
                }
            }
        }
    }
}

// what line j of the call is worth once the keys stand: walked, kept, and its bytes in the text (the line and one '\n')
struct TbxWorth { int walked, kept; long long bytes; };

__device__ __forceinline__ TbxWorth tbx_worth(const plat_tabix_fetch_in& in, const TbxScratch& z, const TbxLine& L, long long s, long long index)
{
    TbxWorth w = {0, 0, 0};
    const unsigned long long key = z.key[L.stream];
    if (8ull * (unsigned long long)index + 4 > key) return w;
    w.walked = 1;
    if ((key & 1ull) || tbx_verdict(in, L, s) != tbxrule::LINE_KEEP) return w;      // (a refused stream keeps nothing)
    w.kept = 1; w.bytes = L.end - s + 1;
    return w;
}

__global__ void __launch_bounds__(TILE_WAVES * 64)
k_tbx_count(plat_tabix_fetch_in in, plat_tabix_fetch_out o, TbxScratch z)
{
    if (o.status[0] == PLAT_ERR_INVALID) return;
    const int lane = threadIdx.x & 63;
    for (long long tile = (long long)blockIdx.x * TILE_WAVES + (threadIdx.x >> 6); tile < z.tiles; tile += (long long)gridDim.x * TILE_WAVES) {
        const long long line0 = z.tile_line[tile];
        long long tileBytes = 0;
        if (z.tile_line[tile + 1] != line0) {
            TileLines T;
            T.open(z.marks, tile, lane);
            for (int done = 0; done < T.total; done += 64) {
                int j;
                const long long s = T.next(lane, &j);
                TbxWorth w = {0, 0, 0};
                int k = 0;
                if (s >= 0) {
                    const TbxLine L = tbx_line_at(in, z, s);
                    k = L.stream;
                    w = tbx_worth(in, z, L, s, line0 + j);
                }
                // the round's counts per stream: summed over the wave's lanes of one stream first, one round per distinct stream of the wave
                wave_groups(s >= 0 && w.walked, k, [&](int leader, int kk, bool mine) {
                    int v0 = mine ? w.walked : 0, v1 = mine ? w.kept : 0;
                    long long v2 = mine ? w.bytes : 0;
                    for (int d = 32; d > 0; d >>= 1) { v0 += __shfl_xor(v0, d, 64); v1 += __shfl_xor(v1, d, 64); v2 += __shfl_xor(v2, d, 64); }
                    if (lane == leader) {
                        atomicAdd((unsigned long long*)&o.stream_counts[2 * kk], (unsigned long long)v0);
                        if (v1) atomicAdd((unsigned long long*)&o.stream_counts[2 * kk + 1], (unsigned long long)v1);
                        if (v2) atomicAdd((unsigned long long*)&z.stream_bytes[kk], (unsigned long long)v2);
                    }
                    tileBytes += v2;
                });
            }
        }
        if (lane == 0) z.tile_bytes[tile] = tileBytes;
    }
}

__global__ void __launch_bounds__(BLOCK_SCAN_THREADS)
k_tbx_scan2(plat_tabix_fetch_in in, plat_tabix_fetch_out o, TbxScratch z)
{
    __shared__ long long s_wave[BLOCK_SCAN_THREADS / 64];
    __shared__ int s_refused;
    __shared__ unsigned long long s_kept;
    if (o.status[0] == PLAT_ERR_INVALID) return;
    if (threadIdx.x == 0) { s_refused = INT32_MAX; s_kept = 0; }
    const long long total = block_scan_inplace<BLOCK_SCAN_THREADS>(z.tile_bytes, z.tiles, s_wave);
    __syncthreads();
    block_scan_inplace<BLOCK_SCAN_THREADS>(z.stream_bytes, in.n_streams, s_wave);
    __syncthreads();
    const long long cap = o.cap_text;
    unsigned long long kept = 0;
    for (int s = threadIdx.x; s <= in.n_streams; s += BLOCK_SCAN_THREADS) {
        const long long b = s < in.n_streams ? z.stream_bytes[s] : total;
        o.stream_text_off[s] = b < cap ? b : cap;                        // (PLAT_ERR_OVERFLOW: clamped, nothing lies behind the capacity)
        if (s < in.n_streams) {
            if (z.key[s] & 1ull) atomicMin(&s_refused, s);
            kept += (unsigned long long)o.stream_counts[2 * s + 1];
        }
    }
    if (kept) atomicAdd(&s_kept, kept);
    const long long used = total < cap ? total : cap;
    if (threadIdx.x < PLAT_BLOB_PAD) o.text[used + threadIdx.x] = 0;
    __syncthreads();
    if (threadIdx.x == 0) {
        z.tile_bytes[z.tiles] = total;
        const bool refused = s_refused != INT32_MAX;
        o.status[0] = refused ? PLAT_ERR_BAD_INPUT : total > cap ? PLAT_ERR_OVERFLOW : 0;
        o.status[1] = refused ? s_refused : -1;
        o.status[2] = (long long)s_kept;
        o.status[3] = total;
    }
}

// n bytes from src to dst by the whole wave: bytes up to dst's first aligned 16-byte word, words (the source read as it lies), the bytes left
__device__ __forceinline__ void tbx_wave_copy(uint8_t* __restrict__ dst, const uint8_t* __restrict__ src, long long n, int lane)
{
    const long long lead = std::min<long long>((16 - (long long)((uintptr_t)dst & 15)) & 15, n);
    if (lane < lead) dst[lane] = src[lane];
    const long long words = (n - lead) >> 4;
    for (long long w = lane; w < words; w += 64) {
        uint4 v;
        __builtin_memcpy(&v, src + lead + 16 * w, 16);
        *reinterpret_cast<uint4*>(dst + lead + 16 * w) = v;
    }
    const long long tail = lead + 16 * words;
    if (tail + lane < n) dst[tail + lane] = src[tail + lane];
}

__global__ void __launch_bounds__(TILE_WAVES * 64)
k_tbx_copy(plat_tabix_fetch_in in, plat_tabix_fetch_out o, TbxScratch z)
{
    if (o.status[0] == PLAT_ERR_INVALID) return;
    const int lane = threadIdx.x & 63;
    const long long cap = o.cap_text;
    for (long long tile = (long long)blockIdx.x * TILE_WAVES + (threadIdx.x >> 6); tile < z.tiles; tile += (long long)gridDim.x * TILE_WAVES) {
        long long run = z.tile_bytes[tile];
        if (z.tile_bytes[tile + 1] == run) continue;                       // (wave-uniform: no kept line starts here)
        const long long line0 = z.tile_line[tile];
        TileLines T;
        T.open(z.marks, tile, lane);
        for (int done = 0; done < T.total; done += 64) {
            int j;
            const long long s = T.next(lane, &j);
            long long n = 0;
            if (s >= 0) n = tbx_worth(in, z, tbx_line_at(in, z, s), s, line0 + j).bytes;
            const long long incl = wave_incl_scan(n, lane);
            const long long at = run + incl - n;
            unsigned long long todo = __ballot(n > 0);
            while (todo) {                                                // one kept line per round, copied by the whole wave
                const int src = __ffsll((long long)todo) - 1;
                todo &= todo - 1;
                const long long ls = __shfl(s, src, 64), ln = __shfl(n, src, 64) - 1, ld = __shfl(at, src, 64);
                if (ld + ln + 1 <= cap) {
                    tbx_wave_copy(o.text + ld, in.data + ls, ln, lane);
                    if (lane == 0) o.text[ld + ln] = '\n';
                } else {                                                  // (the line that crosses the capacity, and those behind it: bytes in front of it only)
                    for (long long k = lane; k <= ln && ld + k < cap; k += 64) o.text[ld + k] = k < ln ? in.data[ls + k] : (uint8_t)'\n';
                }
            }
            run += __shfl(incl, 63, 64);
        }
    }
}
}  // namespace plat

PLAT_EXPORT int plat_tabix_fetch_batch(plat_ctx* ctx, const plat_tabix_fetch_in* in, const plat_tabix_fetch_out* out, void* stream)
{
    if (!ctx || !in || !out) return PLAT_ERR_INVALID;
    const plat_tabix_fetch_in& q = *in;
    const plat_tabix_fetch_out& o = *out;
    if (q.n_streams < 0 || q.n_chunks < 0 || q.n_blocks < 0 || q.data_len < 0 || o.cap_text < 0) return PLAT_ERR_INVALID;
    if (!o.status || !o.stream_text_off || !o.text || ((uintptr_t)o.text & 15) || !q.stream_chunk_begin) return PLAT_ERR_INVALID;
    if (q.n_streams > 0 && (!q.name_off || !q.beg || !q.end || !o.stream_counts)) return PLAT_ERR_INVALID;
    if (q.n_blocks > 0 && (!q.out_off || !q.data || ((uintptr_t)q.data & 15))) return PLAT_ERR_INVALID;
    if (q.n_chunks > 0 && (!q.chunk_blk_first || !q.chunk_blk_end || !q.chunk_first_uoffset || !q.chunk_stop_blk || !q.chunk_stop_uoffset)) return PLAT_ERR_INVALID;
    if (q.n_chunks > 0 && (q.n_streams == 0 || !q.out_off)) return PLAT_ERR_INVALID;
    PLAT_HIP(ctx, hipSetDevice(ctx->device));
    const hipStream_t st = (hipStream_t)stream;
    plat::TbxScratch z;
    z.tiles = q.n_blocks ? (q.data_len + plat::TILE_BYTES - 1) / plat::TILE_BYTES : 0;
    const size_t marksBytes = ((size_t)z.tiles * 64 * sizeof(uint16_t) + 15) & ~(size_t)15;
    const size_t perTile = ((size_t)z.tiles + 2) * sizeof(long long), perChunk = ((size_t)q.n_chunks + 2) * sizeof(long long);
    const size_t perStream = ((size_t)q.n_streams + 2) * sizeof(long long);
    const int rc = plat_reserve(ctx, ctx->tabix, 2 * marksBytes + 3 * perTile + 4 * perChunk + 2 * perStream);
    if (rc != PLAT_OK) return rc;
    uint8_t* base = (uint8_t*)ctx->tabix.ptr;
    z.marks = (uint16_t*)base; base += marksBytes;
    z.nl = (uint16_t*)base; base += marksBytes;
    z.tile_line = (long long*)base; base += perTile;
    z.tile_nl = (long long*)base; base += perTile;
    z.tile_bytes = (long long*)base; base += perTile;
    z.c_lo = (long long*)base; base += perChunk;
    z.c_hi = (long long*)base; base += perChunk;
    z.c_first = (long long*)base; base += perChunk;
    z.c_stop = (long long*)base; base += perChunk;
    z.key = (unsigned long long*)base; base += perStream;
    z.stream_bytes = (long long*)base;
    const unsigned tileBlocks = (unsigned)std::max<long long>(1, std::min<long long>((z.tiles + plat::TILE_WAVES - 1) / plat::TILE_WAVES, plat::TILE_GRID_CAP));
    const dim3 tileThreads(plat::TILE_WAVES * 64);
    PLAT_LAUNCH(ctx, PLAT_KT_OTHER, st, plat::k_tbx_check, dim3(1), dim3(plat::BLOCK_SCAN_THREADS), 0, q, o, z);
    PLAT_LAUNCH(ctx, PLAT_KT_OTHER, st, plat::k_tbx_mark, dim3(tileBlocks), tileThreads, 0, q, o, z);
    PLAT_LAUNCH(ctx, PLAT_KT_OTHER, st, plat::k_tbx_scan, dim3(1), dim3(plat::BLOCK_SCAN_THREADS), 0, q, o, z);
    PLAT_LAUNCH(ctx, PLAT_KT_OTHER, st, plat::k_tbx_verdict, dim3(tileBlocks), tileThreads, 0, q, o, z);
    PLAT_LAUNCH(ctx, PLAT_KT_OTHER, st, plat::k_tbx_count, dim3(tileBlocks), tileThreads, 0, q, o, z);
    PLAT_LAUNCH(ctx, PLAT_KT_OTHER, st, plat::k_tbx_scan2, dim3(1), dim3(plat::BLOCK_SCAN_THREADS), 0, q, o, z);
    PLAT_LAUNCH(ctx, PLAT_KT_OTHER, st, plat::k_tbx_copy, dim3(tileBlocks), tileThreads, 0, q, o, z);
    PLAT_HIP(ctx, hipGetLastError());
    return PLAT_OK;
}
