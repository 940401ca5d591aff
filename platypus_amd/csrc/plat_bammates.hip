// plat_bammates.hip -- the device pass of the broken-mate fetch (plat_bam_mates_batch, include/platypus_mi355x.h): over the records
// plat_bam_find_records kept, either the mate coordinates of the records that give one (PLAT_MATES_COORDS) or the records of a second-round
// fetch whose mate lies in the region, copied back to back (PLAT_MATES_FETCH).  The rule is csrc/mate_rule.hpp's.
// Three kernels: count (a lane per record, a workgroup per tile of MATES_THREADS records: the tile's kept records and bytes), scan (one
// workgroup: the tiles' running sums, the check of the stream partition, the capacities, the status block), write (the same tiles again:
// every kept record's slot from the tile's sum and a workgroup scan, its fields written by its lane, its bytes copied by the whole wave).
// Nothing indexes memory from a record's own fields: a record is [rec_off, rec_limit) and both are checked against data_len first.
#include "plat_internal.hpp"
#include "mate_rule.hpp"
#include "read_source.hpp"
#include "wave_tiles.hpp"

namespace plat {
constexpr int MATES_THREADS = 256;                                         // records per tile = threads per workgroup of the tile kernels
constexpr int MATES_GRID_CAP = 2048;                                       // ... whose grids are capped (grid-stride over tiles)
constexpr unsigned long long MATES_NO_STREAM = ~0ull;                      // status[1] while no stream has been named (-1 as the caller reads it)

// the records of the call: stream_begin[n_streams], held inside the arrays whatever it says
__device__ __forceinline__ long long mates_n(const plat_bam_mates_in& in)
{
    if (in.n_streams <= 0) return 0;
    const long long n = in.stream_begin[in.n_streams];
    return n < 0 ? 0 : n > in.n_records ? in.n_records : n;
}
// the stream of record i: the last s in [0, n_streams) with stream_begin[s] <= i (any table gives an index inside the arrays)
__device__ __forceinline__ int mates_stream_of(const plat_bam_mates_in& in, long long i)
{
    int lo = 0, hi = in.n_streams - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if ((long long)in.stream_begin[mid] <= i) lo = mid; else hi = mid - 1;
    }
    return lo;
}

struct MatesRecord { long long off, len; mate::Fields f; bool bad, keep; };

// record i of stream s: where it lies, its fixed fields (the mate's contig and position in one unaligned 8-byte load) and what the mode's rule says
__device__ __forceinline__ MatesRecord mates_record(const plat_bam_mates_in& in, long long i, int s)
{
    MatesRecord r;
    r.off = in.rec_off[i];
    const long long lim = in.rec_limit[i];
    r.bad = r.off < 0 || lim < 0 || lim > in.data_len || lim - r.off < mate::FIXED_BYTES || lim - r.off > (long long)INT32_MAX;
    r.len = r.bad ? 0 : lim - r.off;
    r.keep = false;
    r.f = mate::Fields{0, -1, -1};
    if (r.bad) return r;
    const uint8_t* p = in.data + r.off;
    const unsigned long long m = load_u64_bytes(p + mate::OFF_MTID);
    static_assert(mate::OFF_MPOS == mate::OFF_MTID + 4, "next_refID and next_pos are neighbours");
    r.f.flag = (uint16_t)((unsigned)p[mate::OFF_FLAG] | ((unsigned)p[mate::OFF_FLAG + 1] << 8));
    r.f.mtid = (int32_t)(uint32_t)m;
    r.f.mpos = (int32_t)(uint32_t)(m >> 32);
    r.keep = in.mode == PLAT_MATES_COORDS ? mate::gives_coord(r.f) : mate::is_mate(r.f, in.want_tid[s], in.lo[s], in.hi[s]);
    if (!r.keep) r.len = 0;
    return r;
}

__global__ void __launch_bounds__(MATES_THREADS)
k_bam_mates_count(plat_bam_mates_in in, plat_bam_mates_out o, long long* __restrict__ tile_n, long long* __restrict__ tile_bytes)
{
    __shared__ long long s_wave[MATES_THREADS / 64];
    const long long N = mates_n(in), tiles = (N + MATES_THREADS - 1) / MATES_THREADS;
    for (long long t = blockIdx.x; t < tiles; t += gridDim.x) {
        const long long i = t * MATES_THREADS + threadIdx.x;
        long long keep = 0, len = 0;
        if (i < N) {
            const int s = mates_stream_of(in, i);
            const MatesRecord r = mates_record(in, i, s);
            if (r.bad) atomicMin((unsigned long long*)&o.status[1], (unsigned long long)s);
            keep = r.keep ? 1 : 0; len = r.len;
        }
        long long all_n, all_bytes;
        block_excl_scan<MATES_THREADS>(keep, s_wave, all_n);
        block_excl_scan<MATES_THREADS>(len, s_wave, all_bytes);
        if (threadIdx.x == 0) { tile_n[t] = all_n; tile_bytes[t] = all_bytes; }
    }
}

// the tiles' sums to running sums, the partition check, the streams that begin behind the last record, the capacities and the status block
__global__ void __launch_bounds__(BLOCK_SCAN_THREADS)
k_bam_mates_scan(plat_bam_mates_in in, plat_bam_mates_out o, long long* __restrict__ tile_n, long long* __restrict__ tile_bytes)
{
    __shared__ long long s_wave[BLOCK_SCAN_THREADS / 64];
    __shared__ int s_broken;
    const int tid = threadIdx.x;
    if (tid == 0) s_broken = 0;
    __syncthreads();
    const long long N = mates_n(in), tiles = (N + MATES_THREADS - 1) / MATES_THREADS;
    long long run_n = 0, run_bytes = 0;
    for (long long t0 = 0; t0 < tiles; t0 += BLOCK_SCAN_THREADS) {
        const long long t = t0 + tid;
        const long long vn = t < tiles ? tile_n[t] : 0, vb = t < tiles ? tile_bytes[t] : 0;
        long long all_n, all_bytes;
        const long long en = block_excl_scan<BLOCK_SCAN_THREADS>(vn, s_wave, all_n);
        const long long eb = block_excl_scan<BLOCK_SCAN_THREADS>(vb, s_wave, all_bytes);
        if (t < tiles) { tile_n[t] = run_n + en; tile_bytes[t] = run_bytes + eb; }
        run_n += all_n; run_bytes += all_bytes;
    }
    // stream_begin has to be a partition of [0, n_records]: from 0, ascending, ending inside the arrays
    bool broken = false;
    for (int s = tid; s <= in.n_streams; s += BLOCK_SCAN_THREADS) {
        const long long b = in.stream_begin[s];
        if ((s == 0 && b != 0) || b < 0 || b > in.n_records || (s < in.n_streams && b > (long long)in.stream_begin[s + 1])) broken = true;
    }
    if (broken) s_broken = 1;
    __syncthreads();
    int32_t* begin = in.mode == PLAT_MATES_COORDS ? o.coord_begin : o.out_begin;
    if (s_broken) {
        if (tid == 0) { o.status[0] = PLAT_ERR_INVALID; o.status[1] = -1; o.status[2] = 0; o.status[3] = 0; if (o.need_bytes) *o.need_bytes = 0; }
        for (int s = tid; s <= in.n_streams; s += BLOCK_SCAN_THREADS) begin[s] = 0;
        return;
    }
    const long long shown = run_n < o.cap_records ? run_n : o.cap_records;
    for (int s = tid; s <= in.n_streams; s += BLOCK_SCAN_THREADS)
        if ((long long)in.stream_begin[s] >= N) begin[s] = (int32_t)shown;           // (the others are written where their first record gets its slot)
    const bool over = run_n > o.cap_records || (in.mode == PLAT_MATES_FETCH && run_bytes > o.cap_bytes);
    if (in.mode == PLAT_MATES_FETCH && !over && tid < PLAT_BLOB_PAD) o.out_data[run_bytes + tid] = 0;
    if (tid == 0) {
        const unsigned long long key = (unsigned long long)o.status[1];
        // (an overflow leaves status[1] at "none": the write pass names the lowest stream with a record that does not fit)
        o.status[0] = key != MATES_NO_STREAM ? PLAT_ERR_BAD_INPUT : over ? PLAT_ERR_OVERFLOW : 0;
        o.status[2] = run_n; o.status[3] = N;
        if (o.need_bytes) *o.need_bytes = run_bytes;
    }
}

// len bytes from src to dst by the 64 lanes of one wave: the bytes in front of dst's first 16-byte boundary, aligned 16-byte stores (from
// one 16-byte load where src is aligned there too, else from two 8-byte loads at src's own alignment), the bytes behind the last whole word
__device__ __forceinline__ void mates_wave_copy(uint8_t* __restrict__ dst, const uint8_t* __restrict__ src, long long len, int lane)
{
    long long head = (long long)((16 - ((uintptr_t)dst & 15)) & 15);
    if (head > len) head = len;
    if (lane < head) dst[lane] = src[lane];
    const long long words = (len - head) >> 4;
    const uint8_t* s16 = src + head;
    uint8_t* d16 = dst + head;
    if ((((uintptr_t)s16) & 15) == 0) {
        for (long long w = lane; w < words; w += 64) *reinterpret_cast<uint4*>(d16 + 16 * w) = *reinterpret_cast<const uint4*>(s16 + 16 * w);
    } else {
        for (long long w = lane; w < words; w += 64) {
            const unsigned long long a = load_u64_bytes(s16 + 16 * w), b = load_u64_bytes(s16 + 16 * w + 8);
            *reinterpret_cast<uint4*>(d16 + 16 * w) = make_uint4((unsigned)a, (unsigned)(a >> 32), (unsigned)b, (unsigned)(b >> 32));
        }
    }
    const long long tail = head + 16 * words;                              // (fewer than 16 bytes are left)
    if (tail + lane < len) dst[tail + lane] = src[tail + lane];
}

__global__ void __launch_bounds__(MATES_THREADS)
k_bam_mates_write(plat_bam_mates_in in, plat_bam_mates_out o, const long long* __restrict__ tile_n, const long long* __restrict__ tile_bytes)
{
    __shared__ long long s_wave[MATES_THREADS / 64];
    if (o.status[0] == PLAT_ERR_INVALID) return;
    const bool over = o.status[0] == PLAT_ERR_OVERFLOW;
    const bool fetch = in.mode == PLAT_MATES_FETCH;
    int32_t* begin = fetch ? o.out_begin : o.coord_begin;
    const int lane = threadIdx.x & 63;
    const long long N = mates_n(in), tiles = (N + MATES_THREADS - 1) / MATES_THREADS;
    for (long long t = blockIdx.x; t < tiles; t += gridDim.x) {
        const long long i = t * MATES_THREADS + threadIdx.x;
        int s = 0;
        MatesRecord r;
        r.off = 0; r.len = 0; r.bad = false; r.keep = false; r.f = mate::Fields{0, -1, -1};
        if (i < N) { s = mates_stream_of(in, i); r = mates_record(in, i, s); }
        long long all_n, all_bytes;
        const long long slot = tile_n[t] + block_excl_scan<MATES_THREADS>((long long)(r.keep ? 1 : 0), s_wave, all_n);
        const long long at = tile_bytes[t] + block_excl_scan<MATES_THREADS>(r.len, s_wave, all_bytes);
        const bool fits = r.keep && slot < o.cap_records && (!fetch || at + r.len <= o.cap_bytes);
        if (r.keep && !fits && over) atomicMin((unsigned long long*)&o.status[1], (unsigned long long)s);
        if (i < N && i == (long long)in.stream_begin[s]) {                 // the first record of its stream, and of the empty streams in front of it
            const int32_t b = (int32_t)(slot < o.cap_records ? slot : o.cap_records);
            begin[s] = b;
            for (int e = s - 1; e >= 0 && (long long)in.stream_begin[e] == i; --e) begin[e] = b;
        }
        if (fits && !fetch) { o.coords[2 * slot] = r.f.mtid; o.coords[2 * slot + 1] = r.f.mpos; }
        if (fits && fetch) { o.out_rec_off[slot] = at; o.out_rec_len[slot] = (int32_t)r.len; o.out_mpos[slot] = r.f.mpos; }
        if (fetch) {                                                       // a wave per record: the lanes that hold one take turns
            unsigned long long todo = __ballot(fits);
            while (todo) {
                const int src_lane = __ffsll((long long)todo) - 1;
                todo &= todo - 1;
                const long long off = __shfl(r.off, src_lane, 64), len = __shfl(r.len, src_lane, 64), to = __shfl(at, src_lane, 64);
                mates_wave_copy(o.out_data + to, in.data + off, len, lane);
            }
        }
    }
}
}  // namespace plat

PLAT_EXPORT int plat_bam_mates_batch(plat_ctx* ctx, const plat_bam_mates_in* in, const plat_bam_mates_out* out, void* stream)
{
    if (!ctx || !in || !out || in->n_streams < 0 || in->n_records < 0 || in->data_len < 0 || out->cap_records < 0 || out->cap_bytes < 0) return PLAT_ERR_INVALID;
    if (in->mode != PLAT_MATES_COORDS && in->mode != PLAT_MATES_FETCH) return PLAT_ERR_INVALID;
    const plat_bam_mates_out& o = *out;
    const bool fetch = in->mode == PLAT_MATES_FETCH;
    if (!o.status || !in->stream_begin || (fetch ? !o.out_begin : !o.coord_begin)) return PLAT_ERR_INVALID;
    if (in->n_records > 0 && (!in->data || !in->rec_off || !in->rec_limit)) return PLAT_ERR_INVALID;
    if (fetch && in->n_streams > 0 && (!in->want_tid || !in->lo || !in->hi)) return PLAT_ERR_INVALID;
    if (fetch && (!o.out_data || ((uintptr_t)o.out_data & 15))) return PLAT_ERR_INVALID;
    if (o.cap_records > 0 && (fetch ? (!o.out_rec_off || !o.out_rec_len || !o.out_mpos) : !o.coords)) return PLAT_ERR_INVALID;
    PLAT_HIP(ctx, hipSetDevice(ctx->device));
    const hipStream_t st = (hipStream_t)stream;
    const long long tiles = ((long long)in->n_records + plat::MATES_THREADS - 1) / plat::MATES_THREADS;
    const int rc = plat_reserve(ctx, ctx->mates, (size_t)(2 * tiles + 2) * sizeof(long long));
    if (rc != PLAT_OK) return rc;
    long long* tile_n = (long long*)ctx->mates.ptr;
    long long* tile_bytes = tile_n + tiles + 1;
    PLAT_HIP(ctx, hipMemsetAsync(o.status, 0xff, 2 * sizeof(int64_t), st));
    PLAT_HIP(ctx, hipMemsetAsync(o.status + 2, 0, 2 * sizeof(int64_t), st));
    const unsigned grid = (unsigned)(tiles < plat::MATES_GRID_CAP ? tiles : plat::MATES_GRID_CAP);
    if (tiles > 0) PLAT_LAUNCH(ctx, PLAT_KT_OTHER, st, plat::k_bam_mates_count, dim3(grid), dim3(plat::MATES_THREADS), 0, *in, o, tile_n, tile_bytes);
    PLAT_LAUNCH(ctx, PLAT_KT_OTHER, st, plat::k_bam_mates_scan, dim3(1), dim3(plat::BLOCK_SCAN_THREADS), 0, *in, o, tile_n, tile_bytes);
    if (tiles > 0) PLAT_LAUNCH(ctx, PLAT_KT_OTHER, st, plat::k_bam_mates_write, dim3(grid), dim3(plat::MATES_THREADS), 0, *in, o, tile_n, tile_bytes);
    PLAT_HIP(ctx, hipGetLastError());
    return PLAT_OK;
}
