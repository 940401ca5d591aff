// plat_bamroute.hip -- records routed to samples by read group (plat_bam_route_batch, include/platypus_mi355x.h): the second branch of
// loadBAMData (platypusutils.pyx:573-666) for whole fetches of a merged BAM file.  Everything that indexes memory from a record's bytes
// is bam_aux.hpp (compiled for the host too and tested there); this file stages the table, partitions and reports.  Six launches:
//   k_route_check       one workgroup: group_sample / group_off / stream_begin checked, the streams cut into tiles of ROUTE_TILE records
//                       (a tile never spans two streams): tile_begin [n_streams + 1] by a scan
//   k_route_tag         one lane per record: the group table staged once per workgroup in LDS -- an open-addressed table of (32-bit hash,
//                       group) and, while they fit, the IDs' bytes -- then per record the aux walk, the value hashed while its NUL is
//                       searched, the probe, and the byte comparison that decides; rec_sample, the refusals
//   k_route_hist        one workgroup per tile: its records per sample (LDS histogram) -> hist [tile][sample]
//   k_route_scan_tiles  one lane per (stream, sample): hist to running counts over the stream's tiles in place; the total to out_begin
//   k_route_scan_out    one workgroup: out_begin to offsets in place, the status block
//   k_route_place       one workgroup per tile: a record's rank among its tile's records of its own sample from wave ballots (a loop
//                       over the wave's distinct samples: __ballot(sample == k), popcount below the lane) plus the waves before it
//                       (per-wave per-sample counts in LDS); its place = out_begin + the tiles before + that rank
// Errors go to the status block; nothing traps.
#include <algorithm>

#include "plat_internal.hpp"
#include "bam_aux.hpp"
#include "wave_tiles.hpp"

namespace plat {
constexpr int ROUTE_TILE = 256;                           // records per tile = threads per workgroup of the tile kernels
constexpr int ROUTE_WAVES = ROUTE_TILE / 64;
constexpr int ROUTE_SLOTS = 2 * PLAT_ROUTE_MAX_GROUPS;    // the largest table: a power of two >= 2 * n_groups
constexpr int ROUTE_TAG_BLOCKS = 2048;                    // the tag kernel's grid is capped: a workgroup stages the table once for many records
constexpr unsigned long long ROUTE_NO_ERROR = ~0ull;

static_assert((ROUTE_SLOTS & (ROUTE_SLOTS - 1)) == 0, "the table size is a power of two");
static_assert(ROUTE_SLOTS * 8 + PLAT_ROUTE_LDS_ID_BYTES <= 60 * 1024, "table and IDs fit the 64 KiB of static LDS");

struct RouteBytes {
    const uint8_t* p;
    __device__ __forceinline__ uint8_t operator[](int64_t at) const { return p[at]; }
};

__global__ void __launch_bounds__(BLOCK_SCAN_THREADS)
k_route_check(plat_bam_route_in in, plat_bam_route_out o, int32_t* __restrict__ tile_begin)
{
    __shared__ long long s_wave[BLOCK_SCAN_THREADS / 64];
    __shared__ int s_bad;
    const int tid = threadIdx.x;
    if (tid == 0) s_bad = 0;
    __syncthreads();
    bool bad = false;
    for (int g = tid; g < in.n_groups; g += BLOCK_SCAN_THREADS) {
        const int32_t m = in.group_sample[g], a = in.group_off[g], b = in.group_off[g + 1];
        if (m < 0 || m >= in.n_samples || b < a || (g == 0 && a != 0)) bad = true;
    }
    if (tid == 0 && in.stream_begin[0] != 0) bad = true;
    for (int s = tid; s < in.n_streams; s += BLOCK_SCAN_THREADS) {
        const int32_t b = in.stream_begin[s], e = in.stream_begin[s + 1];
        const bool ok = b >= 0 && e >= b && e <= in.n_records;
        if (!ok) bad = true;
        tile_begin[s] = ok ? (e - b + ROUTE_TILE - 1) / ROUTE_TILE : 0;
    }
    if (bad) s_bad = 1;
    __syncthreads();
    if (s_bad) {                                                        // (the later kernels see PLAT_ERR_INVALID and write nothing)
        if (tid == 0) { o.status[0] = PLAT_ERR_INVALID; o.status[1] = -1; o.status[2] = 0; o.status[3] = 0; }
        return;
    }
    const long long tiles = block_scan_inplace<BLOCK_SCAN_THREADS>(tile_begin, in.n_streams, s_wave);
    if (tid == 0) {
        tile_begin[in.n_streams] = (int32_t)tiles;
        o.status[0] = 0; o.status[1] = (int64_t)ROUTE_NO_ERROR; o.status[2] = 0; o.status[3] = 0;
    }
}

__global__ void __launch_bounds__(ROUTE_TILE)
k_route_tag(plat_bam_route_in in, plat_bam_route_out o)
{
    __shared__ uint32_t s_hash[ROUTE_SLOTS];
    __shared__ int32_t s_group[ROUTE_SLOTS];
    __shared__ uint8_t s_ids[PLAT_ROUTE_LDS_ID_BYTES];
    if (o.status[0] == PLAT_ERR_INVALID) return;
    const int tid = threadIdx.x;
    const uint32_t slots = bamaux::table_slots(in.n_groups), mask = slots - 1;
    const int32_t idBytes = in.n_groups ? in.group_off[in.n_groups] : 0;
    const bool idsInLds = idBytes <= PLAT_ROUTE_LDS_ID_BYTES;
    for (uint32_t s = tid; s < slots; s += ROUTE_TILE) s_group[s] = -1;
    if (idsInLds) for (int32_t k = tid; k < idBytes; k += ROUTE_TILE) s_ids[k] = in.group_ids[k];
    __syncthreads();
    for (int g = tid; g < in.n_groups; g += ROUTE_TILE) {
        const int32_t a = in.group_off[g];
        const uint32_t h = bamaux::hash_id(in.group_ids + a, in.group_off[g + 1] - a);
        uint32_t s = h & mask;
        for (uint32_t probe = 0; probe < slots; ++probe) {              // (n_groups <= slots / 2: a free slot is met)
            if (atomicCAS(&s_group[s], -1, g) == -1) { s_hash[s] = h; break; }
            s = (s + 1) & mask;
        }
    }
    __syncthreads();
    const bamaux::GroupTable table{s_hash, s_group, mask, idsInLds ? s_ids : in.group_ids, in.group_off};
    const RouteBytes m{in.blob};
    const long long used = in.stream_begin[in.n_streams];
    for (long long i = blockIdx.x * (long long)ROUTE_TILE + tid; i < used; i += (long long)gridDim.x * ROUTE_TILE) {
        const int64_t off = in.rec_off[i], end = in.rec_end[i];
        int32_t g = -1;
        const int v = off < 0 || end < off || end > in.blob_len ? bamaux::FIXED_OVERRUN : bamaux::route(m, off, end, table, &g);
        o.rec_sample[i] = v == bamaux::ROUTED ? in.group_sample[g] : -1;
        if (v != bamaux::ROUTED) {
            atomicMin((unsigned long long*)&o.status[1], ((unsigned long long)i << 8) | (unsigned long long)v);
            atomicAdd((unsigned long long*)&o.status[3], 1ull);
        }
    }
}

// the tile's stream and records: [*first, *last) of the record list; false for a tile behind the last one
__device__ __forceinline__ bool route_tile_at(const plat_bam_route_in& in, const int32_t* __restrict__ tile_begin, int tile, int* stream, int* first, int* last)
{
    if (tile >= tile_begin[in.n_streams]) return false;
    int lo = 0, hi = in.n_streams;                                      // the last stream with tile_begin[s] <= tile (the one that is not empty)
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if (tile_begin[mid] <= tile) lo = mid; else hi = mid;
    }
    *stream = lo;
    const long long b = (long long)in.stream_begin[lo] + (long long)(tile - tile_begin[lo]) * ROUTE_TILE, e = in.stream_begin[lo + 1];
    *first = (int)b;
    *last = (int)(b + ROUTE_TILE < e ? b + ROUTE_TILE : e);
    return true;
}

__global__ void __launch_bounds__(ROUTE_TILE)
k_route_hist(plat_bam_route_in in, plat_bam_route_out o, const int32_t* __restrict__ tile_begin, int32_t* __restrict__ hist)
{
    __shared__ int32_t s_hist[PLAT_ROUTE_MAX_SAMPLES];
    __shared__ int s_at[3];
    if (o.status[0] == PLAT_ERR_INVALID) return;
    const int tid = threadIdx.x, tile = blockIdx.x;
    if (tid == 0) { int s = -1, a = 0, b = 0; if (!route_tile_at(in, tile_begin, tile, &s, &a, &b)) s = -1; s_at[0] = s; s_at[1] = a; s_at[2] = b; }
    for (int m = tid; m < in.n_samples; m += ROUTE_TILE) s_hist[m] = 0;
    __syncthreads();
    if (s_at[0] < 0) return;
    const int i = s_at[1] + tid;
    const int32_t key = i < s_at[2] ? o.rec_sample[i] : -1;
    if (key >= 0) atomicAdd(&s_hist[key], 1);
    __syncthreads();
    for (int m = tid; m < in.n_samples; m += ROUTE_TILE) hist[(size_t)tile * in.n_samples + m] = s_hist[m];
}

__global__ void __launch_bounds__(256)
k_route_scan_tiles(plat_bam_route_in in, plat_bam_route_out o, const int32_t* __restrict__ tile_begin, int32_t* __restrict__ hist)
{
    if (o.status[0] == PLAT_ERR_INVALID) return;
    const long long k = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (k >= (long long)in.n_streams * in.n_samples) return;
    const int s = (int)(k / in.n_samples), m = (int)(k % in.n_samples);
    int32_t run = 0;
    for (int t = tile_begin[s]; t < tile_begin[s + 1]; ++t) {
        const size_t at = (size_t)t * in.n_samples + m;
        const int32_t c = hist[at];
        hist[at] = run;
        run += c;
    }
    o.out_begin[k] = run;
}

__global__ void __launch_bounds__(BLOCK_SCAN_THREADS)
k_route_scan_out(plat_bam_route_in in, plat_bam_route_out o)
{
    __shared__ long long s_wave[BLOCK_SCAN_THREADS / 64];
    if (o.status[0] == PLAT_ERR_INVALID) {
        if (threadIdx.x == 0 && o.why) o.why[0] = 0;
        return;
    }
    const long long K = (long long)in.n_streams * in.n_samples;
    const long long total = block_scan_inplace<BLOCK_SCAN_THREADS>(o.out_begin, K, s_wave);
    if (threadIdx.x == 0) {
        o.out_begin[K] = (int32_t)total;
        const unsigned long long key = (unsigned long long)o.status[1];
        const bool refused = key != ROUTE_NO_ERROR;
        o.status[0] = refused ? PLAT_ERR_BAD_INPUT : 0;
        o.status[1] = refused ? (int64_t)(key >> 8) : -1;
        o.status[2] = total;
        if (o.why) o.why[0] = refused ? (int32_t)(key & 0xffull) : 0;
    }
}

__global__ void __launch_bounds__(ROUTE_TILE)
k_route_place(plat_bam_route_in in, plat_bam_route_out o, const int32_t* __restrict__ tile_begin, const int32_t* __restrict__ hist)
{
    __shared__ int32_t s_cnt[ROUTE_WAVES][PLAT_ROUTE_MAX_SAMPLES];
    __shared__ int s_at[3];
    if (o.status[0] == PLAT_ERR_INVALID) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, tile = blockIdx.x;
    if (tid == 0) { int s = -1, a = 0, b = 0; if (!route_tile_at(in, tile_begin, tile, &s, &a, &b)) s = -1; s_at[0] = s; s_at[1] = a; s_at[2] = b; }
    for (int m = tid; m < ROUTE_WAVES * in.n_samples; m += ROUTE_TILE) s_cnt[m / in.n_samples][m % in.n_samples] = 0;
    __syncthreads();
    if (s_at[0] < 0) return;
    const int i = s_at[1] + tid;
    const int32_t key = i < s_at[2] ? o.rec_sample[i] : -1;
    // the rank inside the wave, one round per distinct sample of the wave
    const unsigned long long below = lane ? (~0ull >> (64 - lane)) : 0ull;
    unsigned long long todo = __ballot(key >= 0);
    int rank = 0;
    while (todo) {                                                      // (todo is the same in every lane; each round clears at least one bit)
        const int leader = __ffsll((long long)todo) - 1;
        const int32_t k = __shfl(key, leader, 64);
        const unsigned long long same = __ballot(key == k);
        if (key == k) rank = __popcll(same & below);
        if (lane == leader) s_cnt[wave][k] = __popcll(same);
        todo &= ~same;
    }
    __syncthreads();
    if (key < 0) return;
    for (int w = 0; w < wave; ++w) rank += s_cnt[w][key];
    const long long dst = (long long)o.out_begin[(long long)s_at[0] * in.n_samples + key] + hist[(size_t)tile * in.n_samples + key] + rank;
    o.rec_off[dst] = in.rec_off[i];
    o.rec_limit[dst] = in.rec_end[i];
}
}  // namespace plat

PLAT_EXPORT int plat_bam_route_batch(plat_ctx* ctx, const plat_bam_route_in* in, const plat_bam_route_out* out, void* stream)
{
    if (!ctx || !in || !out) return PLAT_ERR_INVALID;
    const plat_bam_route_in& q = *in;
    const plat_bam_route_out& o = *out;
    if (q.n_records < 0 || q.n_streams < 0 || q.n_groups < 0 || q.n_samples < 1 || q.blob_len < 0) return PLAT_ERR_INVALID;
    if (!q.stream_begin || !o.status || !o.out_begin) return PLAT_ERR_INVALID;
    if (q.n_groups > 0 && (!q.group_ids || !q.group_off || !q.group_sample)) return PLAT_ERR_INVALID;
    if (q.n_records > 0 && (!q.blob || !q.rec_off || !q.rec_end || !o.rec_off || !o.rec_limit || !o.rec_sample)) return PLAT_ERR_INVALID;
    if (q.n_groups > PLAT_ROUTE_MAX_GROUPS || q.n_samples > PLAT_ROUTE_MAX_SAMPLES) return PLAT_ERR_UNSUPPORTED;
    const long long keys = (long long)q.n_streams * q.n_samples;
    // a tile never spans two streams: at most one short tile per stream that holds a record
    const long long tiles = q.n_records / plat::ROUTE_TILE + (q.n_streams < q.n_records ? q.n_streams : q.n_records) + 1;
    if (keys >= INT32_MAX || tiles >= INT32_MAX) return PLAT_ERR_OVERFLOW;
    PLAT_HIP(ctx, hipSetDevice(ctx->device));
    const hipStream_t st = (hipStream_t)stream;
    const size_t histInts = q.n_records ? (size_t)tiles * (size_t)q.n_samples : 0;
    const int rc = plat_reserve(ctx, ctx->route, ((size_t)q.n_streams + 1 + histInts) * sizeof(int32_t));
    if (rc != PLAT_OK) return rc;
    int32_t* tileBegin = (int32_t*)ctx->route.ptr;
    int32_t* hist = tileBegin + q.n_streams + 1;
    PLAT_LAUNCH(ctx, PLAT_KT_OTHER, st, plat::k_route_check, dim3(1), dim3(plat::BLOCK_SCAN_THREADS), 0, q, o, tileBegin);
    if (q.n_records > 0 && q.n_streams > 0) {
        const unsigned tagBlocks = (unsigned)std::min<long long>(((long long)q.n_records + plat::ROUTE_TILE - 1) / plat::ROUTE_TILE, plat::ROUTE_TAG_BLOCKS);
        PLAT_LAUNCH(ctx, PLAT_KT_OTHER, st, plat::k_route_tag, dim3(tagBlocks), dim3(plat::ROUTE_TILE), 0, q, o);
        PLAT_LAUNCH(ctx, PLAT_KT_OTHER, st, plat::k_route_hist, dim3((unsigned)tiles), dim3(plat::ROUTE_TILE), 0, q, o, tileBegin, hist);
    }
    if (keys > 0) PLAT_LAUNCH(ctx, PLAT_KT_OTHER, st, plat::k_route_scan_tiles, dim3((unsigned)((keys + 255) / 256)), dim3(256), 0, q, o, tileBegin, hist);
    PLAT_LAUNCH(ctx, PLAT_KT_OTHER, st, plat::k_route_scan_out, dim3(1), dim3(plat::BLOCK_SCAN_THREADS), 0, q, o);
    if (q.n_records > 0 && q.n_streams > 0)
        PLAT_LAUNCH(ctx, PLAT_KT_OTHER, st, plat::k_route_place, dim3((unsigned)tiles), dim3(plat::ROUTE_TILE), 0, q, o, tileBegin, hist);
    PLAT_HIP(ctx, hipGetLastError());
    return PLAT_OK;
}
