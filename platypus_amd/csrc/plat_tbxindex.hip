// plat_tbxindex.hip -- the tabix index of a bgzipped VCF built on the device (plat_tabix_index_batch, include/platypus_mi355x.h has the rule):
// ti_index_core (src/tabix/index.c.pysam.c:320-393) over the bytes plat_bgzf_inflate_batch left.  The rule of one record and the host twin
// are tabix_index.hpp; this file finds the records, hands them to lanes, links each to the record in front of it, numbers contigs and runs
// by scans, and reduces the windows' first offsets.  The tile geometry, the rank of a byte among a table's marks, the workgroup scan and
// the hand-out of a tile's marked bytes to lanes are wave_tiles.hpp's.  Nothing is kept per record: three tables of marks (16 bits per
// 16-byte word: record starts, contig heads, run heads) and the tiles' running counts say everything a later kernel asks.  Eleven launches:
//   k_tix_check    one workgroup: out_off and blk_addr checked entry by entry; the verdict key, the per-contig window counts and the
//                  status block reset
//   k_tix_mark     one wave per tile, one aligned 16-byte load per lane: nl (newlines) and marks (RECORD starts: the byte behind a newline,
//                  or byte 0, that is no '#'); the head tables zeroed; the tile's counts
//   k_tix_scan     one workgroup: both tile counts to running counts
//   k_tix_link     one lane per record: its line's end (the r-th newline, by rank and select: r + 1 is its line number), its columns;
//                  the record in front of it over a lane shuffle (the first of a tile looks its own up: a search over the running counts
//                  and one tile's marks); contig heads (the name differs in length or in a byte) and run heads (or the bin differs) set
//                  in their tables; a line that cannot be parsed or lies out of order lowers the verdict key (atomicMin: line * 8 + kind)
//   k_tix_scan2    one workgroup: head counts to running counts -- a record's tid and a run's index are ranks in those tables
//   k_tix_emit     one lane per record: its virtual offset (a bisection of out_off); run heads write (tid, bin, u) at their rank, contig
//                  heads their name's place, length, hash and line; every record raises its contig's window count (atomicMax)
//   k_tix_lin      one workgroup: window counts to lin_first, name lengths to the names' places in name_bytes
//   k_tix_winit    the window table set to `unset`
//   k_tix_windows  one lane per record: atomicMin of its offset into its windows (at most 2^17, what a 32-bit END spans)
//   k_tix_names    one wave per contig: its name against every earlier contig's, lanes striding over them (hash and length first); its name's bytes copied
//   k_tix_final    `unset` back to 0; the status block
// A record belongs to the tile its first byte lies in.  No lane walks a contig or the file.  Errors go to the status block; nothing traps.
#include <algorithm>

#include "plat_internal.hpp"
#include "tabix_index.hpp"
#include "wave_tiles.hpp"

namespace plat {
constexpr unsigned long long TIX_NO_KEY = ~0ull;
constexpr long long TIX_UNSET = INT64_MAX;

struct TixScratch {
    uint16_t* marks;                                      // [tiles * 64] record starts of every 16-byte word
    uint16_t* nl;                                         // [tiles * 64] its newlines
    uint16_t* chg;                                        // [tiles * 64] records that open a contig
    uint16_t* head;                                       // [tiles * 64] records that open a run
    long long* tile_rec; long long* tile_nl; long long* tile_chg; long long* tile_run;       // [tiles + 1] running counts
    unsigned long long* key;                              // [1] the verdict
    long long* c_off; int32_t* c_len; unsigned long long* c_hash; long long* c_line; int32_t* c_nwin;      // [MAX_REF] per contig
    long long* c_first;                                   // [MAX_REF + 1] its windows in lin
    long long* c_npos;                                    // [MAX_REF + 1] its name in name_bytes
    long long tiles;
};

__device__ __forceinline__ long long tix_total(const plat_tabix_index_in& in) { return in.n_blocks ? in.out_off[in.n_blocks] : 0; }
__device__ __forceinline__ void tix_lower(unsigned long long* key, unsigned long long k) { if (*key > k) atomicMin(key, k); }
__device__ __forceinline__ bool tix_refused(const plat_tabix_index_out& o) { return o.status[tbxindex::ST_VERDICT] == PLAT_ERR_INVALID; }

// a bit of a 16-bit-per-word table set by whichever lane finds it: the table is written as aligned 32-bit words
__device__ __forceinline__ void tix_set(uint16_t* table, long long s)
{
    const long long word = s >> 4;
    atomicOr(reinterpret_cast<unsigned*>(table) + (word >> 1), (1u << (int)(s & 15)) << (16 * (int)(word & 1)));
}

__global__ void __launch_bounds__(BLOCK_SCAN_THREADS)
k_tix_check(plat_tabix_index_in in, plat_tabix_index_out o, TixScratch z)
{
    __shared__ int s_bad;
    const int tid = threadIdx.x;
    if (tid == 0) s_bad = 0;
    __syncthreads();
    bool bad = false;
    if (in.n_blocks == 0) bad = in.blk_addr[0] < 0 || in.blk_addr[0] >= tbxindex::MAX_ADDR;
    else for (int b = tid; b <= in.n_blocks; b += BLOCK_SCAN_THREADS)
        if (!tbxindex::geometry_ok(in.out_off, in.blk_addr, in.n_blocks, in.data_len, b)) { bad = true; break; }
    if (bad) s_bad = 1;
    for (int k = tid; k < tbxindex::MAX_REF; k += BLOCK_SCAN_THREADS) z.c_nwin[k] = 0;
    __syncthreads();
    if (tid < tbxindex::ST_WORDS) o.status[tid] = tid == tbxindex::ST_VERDICT && s_bad ? PLAT_ERR_INVALID : tid == tbxindex::ST_LINE ? -1 : 0;
    if (tid == 0) *z.key = TIX_NO_KEY;
}

__global__ void __launch_bounds__(TILE_WAVES * 64)
k_tix_mark(plat_tabix_index_in in, plat_tabix_index_out o, TixScratch z)
{
    if (tix_refused(o)) return;
    const int lane = threadIdx.x & 63;
    const long long total = tix_total(in);
    for (long long tile = (long long)blockIdx.x * TILE_WAVES + (threadIdx.x >> 6); tile < z.tiles; tile += (long long)gridDim.x * TILE_WAVES) {
        const long long tileAt = tile * TILE_BYTES, at = tileAt + 16 * lane;
        unsigned nl = 0, meta = 0, inside = 0;
        if (at < total) {
            const uint4 w = *reinterpret_cast<const uint4*>(in.data + at);      // (may run up to 15 bytes past total, inside PLAT_BLOB_PAD)
            const unsigned v[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const unsigned c = (v[j >> 2] >> (8 * (j & 3))) & 0xffu;
                if (at + j < total) { inside |= 1u << j; if (c == '\n') nl |= 1u << j; if (c == '#') meta |= 1u << j; }
            }
        }
        const unsigned carry0 = lane == 0 && tileAt < total && (tileAt == 0 || in.data[tileAt - 1] == '\n') ? 1u : 0u;
        const unsigned m = behind_newlines(nl, lane, carry0) & inside & ~meta;
        z.marks[tile * 64 + lane] = (uint16_t)m;
        z.nl[tile * 64 + lane] = (uint16_t)nl;
        z.chg[tile * 64 + lane] = 0;
        z.head[tile * 64 + lane] = 0;
        int cm = __popc(m), cn = __popc(nl);
        for (int d = 32; d > 0; d >>= 1) { cm += __shfl_xor(cm, d, 64); cn += __shfl_xor(cn, d, 64); }
        if (lane == 0) { z.tile_rec[tile] = cm; z.tile_nl[tile] = cn; }
    }
}

__global__ void __launch_bounds__(BLOCK_SCAN_THREADS)
k_tix_scan(plat_tabix_index_in in, plat_tabix_index_out o, TixScratch z)
{
    __shared__ long long s_wave[BLOCK_SCAN_THREADS / 64];
    if (tix_refused(o)) return;
    const long long recs = block_scan_inplace<BLOCK_SCAN_THREADS>(z.tile_rec, z.tiles, s_wave);
    __syncthreads();
    const long long nls = block_scan_inplace<BLOCK_SCAN_THREADS>(z.tile_nl, z.tiles, s_wave);
    if (threadIdx.x == 0) { z.tile_rec[z.tiles] = recs; z.tile_nl[z.tiles] = nls; }
}

// the end of the line that starts at s (its newline, or the end of the data) and its number from 1: the newline is number r of the data,
// r the newlines in front of s -- a binary search over the tiles' running counts and one tile's marks, no walk along the line
__device__ __forceinline__ long long tix_line_end(const TixScratch& z, long long s, long long total, long long* lineNo)
{
    const long long r = marks_rank(z.nl, z.tile_nl, z.tiles, s);
    *lineNo = r + 1;
    if (r >= z.tile_nl[z.tiles]) return total;
    long long t = s / TILE_BYTES;
    if (r >= z.tile_nl[t + 1]) {                                            // not in the line's own tile: the last tile with tile_nl <= r
        long long lo = t + 1, up = z.tiles;
        while (lo < up) {
            const long long mid = lo + (up - lo) / 2;
            if (z.tile_nl[mid] <= r) lo = mid + 1; else up = mid;
        }
        t = lo - 1;
    }
    int want = (int)(r - z.tile_nl[t]);
    for (int w = 0; w < 64; ++w) {
        unsigned mw = z.nl[t * 64 + w];
        const int c = __popc(mw);
        if (want >= c) { want -= c; continue; }
        for (; want > 0; --want) mw &= mw - 1;
        return t * TILE_BYTES + 16 * w + (__ffs((int)mw) - 1);
    }
    return total;
}

// the start of record number r (r < tile_rec[tile]: it lies in a tile in front of `tile`), found as the last mark of its tile
__device__ __forceinline__ long long tix_record_in_front(const TixScratch& z, long long tile, long long r)
{
    long long lo = 0, up = tile;                                            // the last tile with tile_rec <= r
    while (lo < up) {
        const long long mid = lo + (up - lo) / 2;
        if (z.tile_rec[mid] <= r) lo = mid + 1; else up = mid;
    }
    const long long t = lo > 0 ? lo - 1 : 0;
    for (int w = 63; w >= 0; --w) {
        const unsigned mw = z.marks[t * 64 + w];
        if (mw) return t * TILE_BYTES + 16 * w + (31 - __clz((int)mw));
    }
    return -1;
}

// a record as the kernels see it: its columns, its bin, its line
struct TixRec { tbxindex::Record r; int32_t bin; long long line; };

__device__ __forceinline__ TixRec tix_record(const plat_tabix_index_in& in, const TixScratch& z, long long s, long long total)
{
    TixRec x;
    const long long e = tix_line_end(z, s, total, &x.line);
    x.r = tbxindex::parse_record(in.data, s, e);
    x.bin = tbxindex::reg2bin(x.r.beg, x.r.end);
    return x;
}

__global__ void __launch_bounds__(TILE_WAVES * 64)
k_tix_link(plat_tabix_index_in in, plat_tabix_index_out o, TixScratch z)
{
    if (tix_refused(o)) return;
    const int lane = threadIdx.x & 63;
    const long long total = tix_total(in);
    for (long long tile = (long long)blockIdx.x * TILE_WAVES + (threadIdx.x >> 6); tile < z.tiles; tile += (long long)gridDim.x * TILE_WAVES) {
        const long long rec0 = z.tile_rec[tile];
        int nChg = 0, nHead = 0;
        if (z.tile_rec[tile + 1] != rec0) {                                 // (wave-uniform)
            // what lane 0 of a round takes for the record in front of its own: every lane holds the same values
            long long cS = -1, cLen = 0;
            int32_t cBeg = 0, cBin = -1;
            if (rec0 > 0) {
                cS = tix_record_in_front(z, tile, rec0 - 1);
                if (cS >= 0) { const TixRec p = tix_record(in, z, cS, total); cLen = p.r.nameLen; cBeg = p.r.beg; cBin = p.bin; }
            }
            TileLines T;
            T.open(z.marks, tile, lane);
            for (int done = 0; done < T.total; done += 64) {
                int j;
                const long long s = T.next(lane, &j);
                TixRec x;
                x.r.nameLen = 0; x.r.beg = 0; x.r.end = 0; x.r.kind = 0; x.bin = -1; x.line = 0;
                if (s >= 0) x = tix_record(in, z, s, total);
                long long pS = __shfl_up(s, 1, 64), pLen = __shfl_up((long long)x.r.nameLen, 1, 64);
                int32_t pBeg = __shfl_up(x.r.beg, 1, 64), pBin = __shfl_up(x.bin, 1, 64);
                if (lane == 0) { pS = cS; pLen = cLen; pBeg = cBeg; pBin = cBin; }
                bool change = false, head = false;
                if (s >= 0) {
                    change = pS < 0 || x.r.nameLen != pLen;
                    for (long long k = 0; !change && k < pLen; ++k) change = in.data[s + k] != in.data[pS + k];      // (bounded by the name's length)
                    head = change || x.bin != pBin;
                    if (x.r.kind) tix_lower(z.key, 8ull * (unsigned long long)x.line + (unsigned)x.r.kind);
                    else if (!change && pBeg > x.r.beg) tix_lower(z.key, 8ull * (unsigned long long)x.line + tbxindex::KIND_ORDER);
                    if (change) tix_set(z.chg, s);
                    if (head) tix_set(z.head, s);
                }
                nChg += __popcll(__ballot(change));
                nHead += __popcll(__ballot(head));
                cS = __shfl(s, 63, 64); cLen = __shfl((long long)x.r.nameLen, 63, 64); cBeg = __shfl(x.r.beg, 63, 64); cBin = __shfl(x.bin, 63, 64);
            }
        }
        if (lane == 0) { z.tile_chg[tile] = nChg; z.tile_run[tile] = nHead; }
    }
}

__global__ void __launch_bounds__(BLOCK_SCAN_THREADS)
k_tix_scan2(plat_tabix_index_in in, plat_tabix_index_out o, TixScratch z)
{
    __shared__ long long s_wave[BLOCK_SCAN_THREADS / 64];
    if (tix_refused(o)) return;
    const long long refs = block_scan_inplace<BLOCK_SCAN_THREADS>(z.tile_chg, z.tiles, s_wave);
    __syncthreads();
    const long long runs = block_scan_inplace<BLOCK_SCAN_THREADS>(z.tile_run, z.tiles, s_wave);
    if (threadIdx.x == 0) { z.tile_chg[z.tiles] = refs; z.tile_run[z.tiles] = runs; }
}

__global__ void __launch_bounds__(TILE_WAVES * 64)
k_tix_emit(plat_tabix_index_in in, plat_tabix_index_out o, TixScratch z)
{
    if (tix_refused(o)) return;
    const int lane = threadIdx.x & 63;
    const long long total = tix_total(in);
    for (long long tile = (long long)blockIdx.x * TILE_WAVES + (threadIdx.x >> 6); tile < z.tiles; tile += (long long)gridDim.x * TILE_WAVES) {
        const long long rec0 = z.tile_rec[tile];
        if (z.tile_rec[tile + 1] == rec0) continue;                         // (wave-uniform)
        TileLines T;
        T.open(z.marks, tile, lane);
        for (int done = 0; done < T.total; done += 64) {
            int j;
            const long long s = T.next(lane, &j);
            if (s >= 0) {                                                   // (no lane leaves the round early: next() shuffles)
                const TixRec x = tix_record(in, z, s, total);
                const long long tid = marks_rank(z.chg, z.tile_chg, z.tiles, s + 1) - 1;
                const long long u = tbxindex::virtual_offset(in.out_off, in.blk_addr, in.n_blocks, s);
                const unsigned at = 1u << (int)(s & 15);
                const bool change = (z.chg[s >> 4] & at) != 0, head = (z.head[s >> 4] & at) != 0;
                const int32_t w0 = tbxindex::first_window(x.r.beg), w1 = tbxindex::last_window(x.r.end);
                if (head) {
                    const long long k = marks_rank(z.head, z.tile_run, z.tiles, s);
                    if (k < o.cap_runs) { o.run_tid[k] = (int32_t)tid; o.run_bin[k] = x.bin; o.run_u[k] = u; }
                }
                if (tid >= 0 && tid < tbxindex::MAX_REF) {
                    if (change) {
                        unsigned long long h = 1469598103934665603ull;            // FNV-1a over the name
                        for (long long k = 0; k < x.r.nameLen; ++k) h = (h ^ in.data[s + k]) * 1099511628211ull;
                        z.c_off[tid] = s; z.c_len[tid] = (int32_t)x.r.nameLen; z.c_hash[tid] = h; z.c_line[tid] = x.line;
                        if (tid < o.cap_names) { o.name_off[tid] = s; o.name_len[tid] = (int32_t)x.r.nameLen; }
                    }
                    if (w1 + 1 > z.c_nwin[tid]) atomicMax(&z.c_nwin[tid], w1 + 1);
                }
                if (rec0 + j == 0 && u == 0) { o.status[tbxindex::ST_FIRST0] = 1; o.status[tbxindex::ST_FIRST_BEG] = w0; o.status[tbxindex::ST_FIRST_END] = w1; }
            }
        }
    }
}

__global__ void __launch_bounds__(BLOCK_SCAN_THREADS)
k_tix_lin(plat_tabix_index_in in, plat_tabix_index_out o, TixScratch z)
{
    __shared__ long long s_wave[BLOCK_SCAN_THREADS / 64];
    if (tix_refused(o)) return;
    const long long nRef = std::min<long long>(z.tile_chg[z.tiles], tbxindex::MAX_REF);
    for (long long t = threadIdx.x; t < nRef; t += BLOCK_SCAN_THREADS) z.c_first[t] = z.c_nwin[t];
    __syncthreads();
    const long long windows = block_scan_inplace<BLOCK_SCAN_THREADS>(z.c_first, nRef, s_wave);
    if (threadIdx.x == 0) z.c_first[nRef] = windows;
    __syncthreads();
    for (long long t = threadIdx.x; t <= nRef && t <= o.cap_names; t += BLOCK_SCAN_THREADS) o.lin_first[t] = z.c_first[t];
    for (long long t = threadIdx.x; t < nRef; t += BLOCK_SCAN_THREADS) z.c_npos[t] = z.c_len[t];
    __syncthreads();
    const long long nameBytes = block_scan_inplace<BLOCK_SCAN_THREADS>(z.c_npos, nRef, s_wave);
    if (threadIdx.x == 0) z.c_npos[nRef] = nameBytes;
}

// the windows are written when all of them fit, or not at all
__device__ __forceinline__ long long tix_windows(const plat_tabix_index_out& o, const TixScratch& z)
{
    const long long nRef = std::min<long long>(z.tile_chg[z.tiles], tbxindex::MAX_REF), windows = z.c_first[nRef];
    return windows <= o.cap_windows ? windows : 0;
}

__global__ void __launch_bounds__(256)
k_tix_winit(plat_tabix_index_in in, plat_tabix_index_out o, TixScratch z)
{
    if (tix_refused(o)) return;
    const long long n = tix_windows(o, z);
    for (long long w = (long long)blockIdx.x * 256 + threadIdx.x; w < n; w += (long long)gridDim.x * 256) o.lin[w] = TIX_UNSET;
}

__global__ void __launch_bounds__(TILE_WAVES * 64)
k_tix_windows(plat_tabix_index_in in, plat_tabix_index_out o, TixScratch z)
{
    if (tix_refused(o)) return;
    if (tix_windows(o, z) == 0) return;
    const int lane = threadIdx.x & 63;
    const long long total = tix_total(in);
    for (long long tile = (long long)blockIdx.x * TILE_WAVES + (threadIdx.x >> 6); tile < z.tiles; tile += (long long)gridDim.x * TILE_WAVES) {
        if (z.tile_rec[tile + 1] == z.tile_rec[tile]) continue;             // (wave-uniform)
        TileLines T;
        T.open(z.marks, tile, lane);
        for (int done = 0; done < T.total; done += 64) {
            int j;
            const long long s = T.next(lane, &j);
            if (s >= 0) {                                                   // (no lane leaves the round early: next() shuffles)
                const TixRec x = tix_record(in, z, s, total);
                const long long tid = marks_rank(z.chg, z.tile_chg, z.tiles, s + 1) - 1;
                const long long u = tbxindex::virtual_offset(in.out_off, in.blk_addr, in.n_blocks, s);
                if (u != 0 && tid >= 0 && tid < tbxindex::MAX_REF) {        // (offset 0 is `unset` in the reference: it never holds a window)
                    const int32_t w0 = tbxindex::first_window(x.r.beg);
                    const int32_t w1 = std::min<int32_t>(tbxindex::last_window(x.r.end), z.c_nwin[tid] - 1);       // (its own atomicMax holds: at most 2^17 windows)
                    long long* lin = reinterpret_cast<long long*>(o.lin) + z.c_first[tid];
                    for (int32_t w = w0 < 0 ? 0 : w0; w <= w1; ++w) if (lin[w] > u) atomicMin(&lin[w], u);
                }
            }
        }
    }
}

__global__ void __launch_bounds__(TILE_WAVES * 64)
k_tix_names(plat_tabix_index_in in, plat_tabix_index_out o, TixScratch z)
{
    if (tix_refused(o)) return;
    const int lane = threadIdx.x & 63;
    const long long nRef = std::min<long long>(z.tile_chg[z.tiles], tbxindex::MAX_REF);
    for (long long i = (long long)blockIdx.x * TILE_WAVES + (threadIdx.x >> 6); i < nRef; i += (long long)gridDim.x * TILE_WAVES) {
        const unsigned long long h = z.c_hash[i];
        const int32_t n = z.c_len[i];
        const long long at = z.c_off[i];
        bool again = false;
        for (long long k = lane; k < i && !again; k += 64) {                // (at most MAX_REF / 64 rounds)
            if (z.c_hash[k] != h || z.c_len[k] != n) continue;
            const long long other = z.c_off[k];
            bool same = true;
            for (int32_t b = 0; same && b < n; ++b) same = in.data[at + b] == in.data[other + b];
            again = same;
        }
        if (again) tix_lower(z.key, 8ull * (unsigned long long)z.c_line[i] + tbxindex::KIND_NAME_AGAIN);
        if (z.c_npos[nRef] <= o.cap_name_bytes)                             // (the names' bytes: all of them or none)
            for (int32_t b = lane; b < n; b += 64) o.name_bytes[z.c_npos[i] + b] = in.data[at + b];
    }
}

__global__ void __launch_bounds__(256)
k_tix_final(plat_tabix_index_in in, plat_tabix_index_out o, TixScratch z)
{
    if (tix_refused(o)) return;
    const long long n = tix_windows(o, z);
    for (long long w = (long long)blockIdx.x * 256 + threadIdx.x; w < n; w += (long long)gridDim.x * 256) if (o.lin[w] == TIX_UNSET) o.lin[w] = 0;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const unsigned long long key = *z.key;
        const long long refs = z.tile_chg[z.tiles], runs = z.tile_run[z.tiles];
        const long long windows = z.c_first[std::min<long long>(refs, tbxindex::MAX_REF)], nameBytes = z.c_npos[std::min<long long>(refs, tbxindex::MAX_REF)];
        int64_t* st = o.status;
        if (key != TIX_NO_KEY) { st[tbxindex::ST_VERDICT] = PLAT_ERR_BAD_INPUT; st[tbxindex::ST_LINE] = (int64_t)(key >> 3); st[tbxindex::ST_KIND] = (int64_t)(key & 7); }
        else if (refs > tbxindex::MAX_REF) st[tbxindex::ST_VERDICT] = PLAT_ERR_UNSUPPORTED;
        else if (runs > o.cap_runs || refs > o.cap_names || windows > o.cap_windows || nameBytes > o.cap_name_bytes) st[tbxindex::ST_VERDICT] = PLAT_ERR_OVERFLOW;
        st[tbxindex::ST_RECORDS] = z.tile_rec[z.tiles]; st[tbxindex::ST_RUNS] = runs; st[tbxindex::ST_CONTIGS] = refs; st[tbxindex::ST_WINDOWS] = windows; st[tbxindex::ST_NAME_BYTES] = nameBytes;
        st[tbxindex::ST_END] = (int64_t)((uint64_t)in.blk_addr[in.n_blocks] << 16);
        const long long total = tix_total(in);
        st[tbxindex::ST_LINES] = z.tile_nl[z.tiles] + (total > 0 && in.data[total - 1] != '\n' ? 1 : 0);
    }
}
}  // namespace plat

PLAT_EXPORT int plat_tabix_index_batch(plat_ctx* ctx, const plat_tabix_index_in* in, const plat_tabix_index_out* out, void* stream)
{
    if (!ctx || !in || !out) return PLAT_ERR_INVALID;
    const plat_tabix_index_in& q = *in;
    const plat_tabix_index_out& o = *out;
    if (q.n_blocks < 0 || q.data_len < 0 || !q.blk_addr || o.cap_runs < 0 || o.cap_names < 0 || o.cap_windows < 0 || o.cap_name_bytes < 0 || !o.name_bytes) return PLAT_ERR_INVALID;
    if (!o.status || !o.lin_first || !o.run_tid || !o.run_bin || !o.run_u || !o.name_off || !o.name_len || !o.lin) return PLAT_ERR_INVALID;
    if (q.n_blocks > 0 && (!q.out_off || !q.data || ((uintptr_t)q.data & 15))) return PLAT_ERR_INVALID;
    PLAT_HIP(ctx, hipSetDevice(ctx->device));
    const hipStream_t st = (hipStream_t)stream;
    plat::TixScratch z;
    z.tiles = q.n_blocks ? (q.data_len + plat::TILE_BYTES - 1) / plat::TILE_BYTES : 0;
    const size_t marksBytes = ((size_t)z.tiles * 64 * sizeof(uint16_t) + 15) & ~(size_t)15;
    const size_t perTile = ((size_t)z.tiles + 2) * sizeof(long long), perRef = ((size_t)tbxindex::MAX_REF + 2) * sizeof(long long);
    const int rc = plat_reserve(ctx, ctx->tabix, 4 * marksBytes + 4 * perTile + 7 * perRef + 16);      // (the fetch's scratch: one call at a time per context)
    if (rc != PLAT_OK) return rc;
    uint8_t* base = (uint8_t*)ctx->tabix.ptr;
    z.marks = (uint16_t*)base; base += marksBytes;
    z.nl = (uint16_t*)base; base += marksBytes;
    z.chg = (uint16_t*)base; base += marksBytes;
    z.head = (uint16_t*)base; base += marksBytes;
    z.tile_rec = (long long*)base; base += perTile;
    z.tile_nl = (long long*)base; base += perTile;
    z.tile_chg = (long long*)base; base += perTile;
    z.tile_run = (long long*)base; base += perTile;
    z.c_off = (long long*)base; base += perRef;
    z.c_hash = (unsigned long long*)base; base += perRef;
    z.c_line = (long long*)base; base += perRef;
    z.c_first = (long long*)base; base += perRef;
    z.c_npos = (long long*)base; base += perRef;
    z.c_len = (int32_t*)base; base += perRef;
    z.c_nwin = (int32_t*)base; base += perRef;
    z.key = (unsigned long long*)base;
    const unsigned tileBlocks = (unsigned)std::max<long long>(1, std::min<long long>((z.tiles + plat::TILE_WAVES - 1) / plat::TILE_WAVES, plat::TILE_GRID_CAP));
    const unsigned flatBlocks = (unsigned)std::max<long long>(1, std::min<long long>((o.cap_windows + 255) / 256, plat::TILE_GRID_CAP));
    const unsigned nameBlocks = (unsigned)std::max<long long>(1, std::min<long long>((o.cap_names + plat::TILE_WAVES - 1) / plat::TILE_WAVES, plat::TILE_GRID_CAP));
    const dim3 tileThreads(plat::TILE_WAVES * 64);
    PLAT_LAUNCH(ctx, PLAT_KT_OTHER, st, plat::k_tix_check, dim3(1), dim3(plat::BLOCK_SCAN_THREADS), 0, q, o, z);
    PLAT_LAUNCH(ctx, PLAT_KT_OTHER, st, plat::k_tix_mark, dim3(tileBlocks), tileThreads, 0, q, o, z);
    PLAT_LAUNCH(ctx, PLAT_KT_OTHER, st, plat::k_tix_scan, dim3(1), dim3(plat::BLOCK_SCAN_THREADS), 0, q, o, z);
    PLAT_LAUNCH(ctx, PLAT_KT_OTHER, st, plat::k_tix_link, dim3(tileBlocks), tileThreads, 0, q, o, z);
    PLAT_LAUNCH(ctx, PLAT_KT_OTHER, st, plat::k_tix_scan2, dim3(1), dim3(plat::BLOCK_SCAN_THREADS), 0, q, o, z);
    PLAT_LAUNCH(ctx, PLAT_KT_OTHER, st, plat::k_tix_emit, dim3(tileBlocks), tileThreads, 0, q, o, z);
    PLAT_LAUNCH(ctx, PLAT_KT_OTHER, st, plat::k_tix_lin, dim3(1), dim3(plat::BLOCK_SCAN_THREADS), 0, q, o, z);
    PLAT_LAUNCH(ctx, PLAT_KT_OTHER, st, plat::k_tix_winit, dim3(flatBlocks), dim3(256), 0, q, o, z);
    PLAT_LAUNCH(ctx, PLAT_KT_OTHER, st, plat::k_tix_windows, dim3(tileBlocks), tileThreads, 0, q, o, z);
    PLAT_LAUNCH(ctx, PLAT_KT_OTHER, st, plat::k_tix_names, dim3(nameBlocks), tileThreads, 0, q, o, z);
    PLAT_LAUNCH(ctx, PLAT_KT_OTHER, st, plat::k_tix_final, dim3(flatBlocks), dim3(256), 0, q, o, z);
    PLAT_HIP(ctx, hipGetLastError());
    return PLAT_OK;
}
