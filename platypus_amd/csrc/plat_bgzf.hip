// plat_bgzf.hip -- BGZF blocks of a BAM file inflated on the device (plat_bgzf_inflate_batch) and the iterator over the inflated bytes
// (plat_bam_find_records), include/platypus_mi355x.h.  Everything that indexes memory from input data is bgzf_inflate.hpp, which the CPU
// suite builds for the host and runs over a corrupt-input corpus.
//   k_bgzf_head     one lane per block: the header (magic, FLG, the BC subfield, the trailer's ISIZE) -> out_off[i + 1] = ISIZE
//   k_bgzf_scan     one workgroup: ISIZEs to offsets in place, the capacity check, the zeroed slack behind the last byte
//   k_bgzf_inflate  one wave per block.  Lane 0 decodes symbols (a 9-bit primary table in LDS, the canonical walk for longer codes) into a
//                   batch of up to 64 commands; the wave executes the batch on the block's 64 KiB output window IN LDS: the literals by one
//                   lane each, then every match by all lanes (byte k of a match is source byte k mod distance: the overlap rule).  LDS
//                   operations of one wave complete in order, so a match reads what the commands before it wrote without any global
//                   round trip.  The finished window's CRC32 is taken by the 64 lanes over disjoint slices and combined with x^(8n)
//                   multiplications; only a block that passes is copied out, as aligned dwords.  64 KiB + 4 KiB of LDS per wave: two waves
//                   per CU.
//   k_bgzf_status   one lane: the status block
//   k_bam_find      one workgroup per stream, twice (count, then write): the stream goes through LDS in 16 KiB windows, lane 0 follows the
//                   block_size chain there; a record whose CIGAR does not fit a window is walked in global memory.
// Errors go to the status blocks; nothing traps.
#include "plat_internal.hpp"
#include "bgzf_inflate.hpp"
#include "wave_tiles.hpp"

namespace plat {
constexpr int BGZF_SCAN_THREADS = 1024;
constexpr unsigned long long BGZF_NO_ERROR = ~0ull;
constexpr int FIND_THREADS = 256;
constexpr int FIND_WINDOW = 16384;

struct BgzfLds {
    uint8_t win[bgzf::MAX_ISIZE];
    bgzf::Tables t;
    uint64_t cmds[64];
    uint32_t crc[256];
    int n;
};

__device__ __forceinline__ void bgzf_fail(int64_t* status, long long i, int err) {
    atomicMin((unsigned long long*)&status[1], ((unsigned long long)i << 8) | (unsigned long long)(unsigned)(-err));
}

// LDS writes of this wave's lanes are visible to its other lanes behind this (the wave's LDS operations complete in order)
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

__global__ void __launch_bounds__(256)
k_bgzf_head(int n, const uint8_t* __restrict__ blob, long long blob_len, const int64_t* __restrict__ blk_off, const int64_t* __restrict__ blk_limit,
            plat_bgzf_inflate_out o)
{
    const int i = (int)(blockIdx.x * (long long)blockDim.x + threadIdx.x);
    if (i >= n) return;
    if (i == 0) o.out_off[0] = 0;
    if (blk_limit && blk_limit[i] < blob_len) blob_len = blk_limit[i];
    bgzf::BlockHead h;
    const int rc = bgzf::parse_header(blob, blob_len, blk_off[i], &h);
    o.out_off[i + 1] = rc == 0 ? (int64_t)h.isize : 0;
    if (rc != 0) bgzf_fail(o.status, i, PLAT_ERR_BAD_INPUT);
}

__global__ void __launch_bounds__(BGZF_SCAN_THREADS)
k_bgzf_scan(int n, plat_bgzf_inflate_out o)
{
    __shared__ long long s_wave[BGZF_SCAN_THREADS / 64];
    __shared__ int s_first;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) s_first = INT32_MAX;
    __syncthreads();
    long long run = 0;
    for (long long t0 = 0; t0 < n; t0 += BGZF_SCAN_THREADS) {
        const long long i = t0 + tid;
        const long long v = i < n ? o.out_off[i + 1] : 0;
        const long long inc = wave_incl_scan(v, lane);
        if (lane == 63) s_wave[wave] = inc;
        __syncthreads();
        long long at = run + inc, all = 0;
        for (int w = 0; w < BGZF_SCAN_THREADS / 64; ++w) {
            if (w < wave) at += s_wave[w];
            all += s_wave[w];
        }
        if (i < n) {
            if (at > o.cap_bytes) { atomicMin(&s_first, (int)i); at = o.cap_bytes; }      // (clamped: the offsets stay valid numbers)
            o.out_off[i + 1] = at;
        }
        run += all;
        __syncthreads();
    }
    const bool fits = s_first == INT32_MAX;
    if (fits && tid < PLAT_BLOB_PAD) o.data[run + tid] = 0;
    if (tid == 0) { o.status[0] = fits ? 0 : PLAT_ERR_OVERFLOW; o.status[2] = run; o.status[3] = fits ? -1 : s_first; }
}

__global__ void __launch_bounds__(64)
k_bgzf_inflate(int n, const uint8_t* __restrict__ blob, long long blob_len, const int64_t* __restrict__ blk_off, const int64_t* __restrict__ blk_limit,
               plat_bgzf_inflate_out o)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t lds_raw[];
    BgzfLds& L = *reinterpret_cast<BgzfLds*>(lds_raw);
    const int lane = threadIdx.x;
    const long long i = blockIdx.x;
    for (int k = lane; k < 256; k += 64) L.crc[k] = bgzf::crc_table_entry((uint32_t)k);
    if (blk_limit && blk_limit[i] < blob_len) blob_len = blk_limit[i];
    bgzf::BlockHead h;
    if (bgzf::parse_header(blob, blob_len, blk_off[i], &h) != 0) return;              // (refused by k_bgzf_head)
    const bool fits = o.status[0] == 0;
    const long long base = o.out_off[i];
    bgzf::Inflate s;
    bgzf::inflate_begin(s, blob + h.payload, h.payload_len, h.isize);
    bool done = false;
    // every round consumes input bits or ends the block: at most 8 * payload_len + 1 rounds
    while (!done) {
        wave_lds_sync();                                                              // (the batch before this one has been read)
        if (lane == 0) {
            const int n_cmd = bgzf::inflate_step(s, L.t, L.cmds, 64);
            L.n = n_cmd < 0 ? n_cmd : (n_cmd | (s.phase == bgzf::DONE ? 0x100 : 0));
        }
        wave_lds_sync();
        const int word = L.n;
        if (word < 0) { if (lane == 0) bgzf_fail(o.status, i, PLAT_ERR_BAD_INPUT); return; }
        const int n_cmd = word & 0xff;
        done = (word & 0x100) != 0;
        if (lane < n_cmd) {
            const uint64_t c = L.cmds[lane];
            if (!bgzf::cmd_len(c)) L.win[bgzf::cmd_dst(c)] = (uint8_t)bgzf::cmd_low(c);
        }
        wave_lds_sync();
        for (int j = 0; j < n_cmd; ++j) {
            const uint64_t c = L.cmds[j];
            const uint32_t len = bgzf::cmd_len(c);
            if (!len) continue;
            const uint32_t dst = bgzf::cmd_dst(c), dist = bgzf::cmd_low(c) + 1u;       // (dst + len <= ISIZE and dist <= dst: inflate_step)
            for (uint32_t k = lane; k < len; k += 64) L.win[dst + k] = L.win[dst - dist + (dist >= len ? k : k % dist)];
            wave_lds_sync();
        }
    }
    const uint32_t isize = h.isize;
    const uint32_t out_len = (uint32_t)__shfl((int)s.out, 0, 64);
    if (out_len != isize) { if (lane == 0) bgzf_fail(o.status, i, PLAT_ERR_BAD_INPUT); return; }
    // CRC32: 64 slices, combined
    const uint32_t per = (isize + 63u) / 64u;
    const uint32_t a = min((uint32_t)lane * per, isize), b = min(a + per, isize);
    uint32_t crc = bgzf::crc_shift(bgzf::crc_bytes(L.crc, L.win + a, (int64_t)(b - a)), isize - b);
    for (int d = 32; d >= 1; d >>= 1) crc ^= (uint32_t)__shfl_xor((int)crc, d, 64);
    if (crc != h.crc) { if (lane == 0) bgzf_fail(o.status, i, PLAT_ERR_BAD_INPUT); return; }
    if (!fits || base < 0 || base + (long long)isize > o.cap_bytes) return;          // (on overflow no payload byte is written)
    // copy out: bytes up to the first aligned dword of the output, dwords, the bytes left
    uint8_t* dst = o.data + base;
    const uint32_t lead = min((uint32_t)((4u - (uint32_t)((uintptr_t)dst & 3u)) & 3u), isize);
    const uint32_t words = (isize - lead) >> 2;
    if ((uint32_t)lane < lead) dst[lane] = L.win[lane];
    for (uint32_t w = lane; w < words; w += 64) {
        const uint8_t* p = L.win + lead + 4u * w;
        *(uint32_t*)(dst + lead + 4u * w) = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
    }
    const uint32_t tail = lead + 4u * words;
    if (tail + (uint32_t)lane < isize) dst[tail + lane] = L.win[tail + lane];
}

__global__ void k_bgzf_status(plat_bgzf_inflate_out o)
{
    const unsigned long long key = (unsigned long long)o.status[1];
    long long err = o.status[0], who = o.status[3];
    if (key != BGZF_NO_ERROR) { err = -(long long)(key & 0xffull); who = (long long)(key >> 8); }
    o.status[0] = err; o.status[1] = who; o.status[3] = 0;
}

// ---- the record walk ---------------------------------------------------------------------------------------------------------------
struct WindowBytes {                                                                  // bytes [base, base + FIND_WINDOW) of the data, in LDS
    const uint8_t* w; long long base;
    __device__ uint8_t operator[](long long at) const { return w[at - base]; }
};
struct GlobalBytes {
    const uint8_t* p;
    __device__ uint8_t operator[](long long at) const { return p[at]; }
};

template <bool WRITE>
__global__ void __launch_bounds__(FIND_THREADS)
k_bam_find(plat_bam_find_in in, plat_bam_find_out o)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_win[FIND_WINDOW];
    __shared__ long long s_pos;
    __shared__ int s_state;                                                           // 0 walking, 1 chunk ended, 2 stream ended, < 0 error
    __shared__ long long s_kept, s_walked;
    const int s = blockIdx.x, tid = threadIdx.x;
    const int32_t want_tid = in.tid[s], beg = in.beg[s], end = in.end[s];
    if (tid == 0) { s_kept = 0; s_walked = 0; s_state = 0; }
    long long at_out = WRITE ? (long long)o.stream_begin[s] : 0;
    const long long out_end = WRITE ? (long long)o.stream_begin[s + 1] : 0;
    int c = in.stream_chunk_begin[s];
    const int c_end = in.stream_chunk_begin[s + 1];
    bool bad = c < 0 || c_end > in.n_chunks || c > c_end;
    for (; !bad && c < c_end; ++c) {
        const int b0 = in.chunk_blk_first[c], b1 = in.chunk_blk_end[c], sb = in.chunk_stop_blk[c];
        if (b0 < 0 || b1 < b0 || b1 > in.n_blocks || sb >= in.n_blocks || sb < -1 || in.chunk_first_uoffset[c] < 0 || in.chunk_stop_uoffset[c] < 0) { bad = true; break; }
        const long long lo = in.out_off[b0], hi = in.out_off[b1];
        const long long stop = sb < 0 ? hi : min(hi, in.out_off[sb] + (long long)in.chunk_stop_uoffset[c]);
        __syncthreads();
        if (tid == 0) { s_pos = lo + in.chunk_first_uoffset[c]; s_state = 0; }
        __syncthreads();
        // every round of the outer loop moves s_pos forward by at least one record or ends the chunk
        while (true) {
            const long long pos = s_pos;
            if (s_state != 0) break;
            if (pos >= stop || pos >= hi) { __syncthreads(); if (tid == 0) s_state = 1; __syncthreads(); break; }
            const long long base = pos & ~3ll;                                         // (data is 16-byte aligned: whole dwords)
            const long long n_load = min((long long)FIND_WINDOW, ((hi - base) + 3) & ~3ll);      // (behind hi: the next stream's bytes or the zeroed slack)
            for (long long k = 4ll * tid; k < n_load; k += 4ll * FIND_THREADS) *(uint32_t*)(s_win + k) = *(const uint32_t*)(in.data + base + k);
            __syncthreads();
            if (tid == 0) {
                const long long w_end = min(base + FIND_WINDOW, hi);
                const WindowBytes W{s_win, base};
                const GlobalBytes G{in.data};
                long long p = pos, kept = s_kept, walked = s_walked;
                int state = 0;
                while (p < stop && p < hi) {
                    // in the window: the 36 bytes every step reads, then the name's length and the CIGAR behind them
                    const bool head_in = p + 36 <= w_end;
                    const bool all_in = head_in && p + bgzf::walk_need(W, p) <= w_end;
                    if (!all_in && p != pos && w_end < hi) break;                      // (load the window again, from this record on)
                    long long next = p; bool keep = false;
                    // (a record at the window's start that still does not fit it -- or the stream's last bytes -- goes through global memory)
                    const int rc = all_in ? bgzf::walk_step(W, p, hi, want_tid, beg, end, (int64_t*)&next, &keep)
                                          : bgzf::walk_step(G, p, hi, want_tid, beg, end, (int64_t*)&next, &keep);
                    if (rc == bgzf::WALK_STOP) { state = 2; break; }
                    if (rc != bgzf::WALK_NEXT) { state = PLAT_ERR_BAD_INPUT; break; }
                    ++walked;
                    if (keep) {
                        if (WRITE && at_out + kept < out_end) { o.rec_off[at_out + kept] = p + 4; o.rec_limit[at_out + kept] = next; }
                        ++kept;
                    }
                    p = next;
                }
                s_pos = p; s_kept = kept; s_walked = walked; s_state = state;
            }
            __syncthreads();
        }
        if (s_state == 2 || s_state < 0) break;
    }
    __syncthreads();
    if (tid == 0) {
        if (!WRITE) {                                                                 // (the second pass finds the same and reports nothing)
            if (bad || s_state < 0) bgzf_fail(o.status, s, bad ? PLAT_ERR_INVALID : PLAT_ERR_BAD_INPUT);
            o.stream_begin[s + 1] = (int32_t)min(s_kept, (long long)INT32_MAX);
            atomicAdd((unsigned long long*)&o.status[3], (unsigned long long)s_walked);
        }
    }
}

// kept counts to offsets (one workgroup; the streams of a call are few against its records), the capacity check and the status block
__global__ void __launch_bounds__(64)
k_bam_find_scan(int n_streams, plat_bam_find_out o)
{
    if (threadIdx.x != 0) return;
    long long at = 0, all = 0, first = -1;
    o.stream_begin[0] = 0;
    for (int s = 0; s < n_streams; ++s) {
        at += o.stream_begin[s + 1]; all += o.stream_begin[s + 1];
        if (at > o.cap_records) { if (first < 0) first = s; at = o.cap_records; }      // (clamped: the second pass writes inside the capacity)
        o.stream_begin[s + 1] = (int32_t)at;
    }
    const unsigned long long key = (unsigned long long)o.status[1];
    long long err = 0, who = -1;
    if (key != BGZF_NO_ERROR) { err = -(long long)(key & 0xffull); who = (long long)(key >> 8); }
    else if (first >= 0) { err = PLAT_ERR_OVERFLOW; who = first; }
    o.status[0] = err; o.status[1] = who; o.status[2] = all;
}
}  // namespace plat

PLAT_EXPORT int plat_bgzf_inflate_batch(plat_ctx* ctx, int n_blocks, const uint8_t* blob, int64_t blob_len, const int64_t* blk_off,
                                        const int64_t* blk_limit, const plat_bgzf_inflate_out* out, void* stream)
{
    if (!ctx || !out || n_blocks < 0 || blob_len < 0 || out->cap_bytes < 0) return PLAT_ERR_INVALID;
    const plat_bgzf_inflate_out& o = *out;
    if (!o.status || !o.out_off || !o.data || ((uintptr_t)o.data & 15)) return PLAT_ERR_INVALID;
    if (n_blocks > 0 && (!blob || !blk_off)) return PLAT_ERR_INVALID;
    PLAT_HIP(ctx, hipSetDevice(ctx->device));
    const hipStream_t st = (hipStream_t)stream;
    PLAT_HIP(ctx, hipMemsetAsync(o.status, 0xff, 4 * sizeof(int64_t), st));
    if (n_blocks == 0) PLAT_HIP(ctx, hipMemsetAsync(o.out_off, 0, sizeof(int64_t), st));
    if (n_blocks > 0)
        PLAT_LAUNCH(ctx, PLAT_KT_OTHER, st, plat::k_bgzf_head, dim3((unsigned)((n_blocks + 255) / 256)), dim3(256), 0, n_blocks, blob, (long long)blob_len, blk_off, blk_limit, o);
    PLAT_LAUNCH(ctx, PLAT_KT_OTHER, st, plat::k_bgzf_scan, dim3(1), dim3(plat::BGZF_SCAN_THREADS), 0, n_blocks, o);
    if (n_blocks > 0) {
        PLAT_HIP(ctx, hipFuncSetAttribute((const void*)plat::k_bgzf_inflate, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(plat::BgzfLds)));
        PLAT_LAUNCH(ctx, PLAT_KT_OTHER, st, plat::k_bgzf_inflate, dim3((unsigned)n_blocks), dim3(64), sizeof(plat::BgzfLds), n_blocks, blob, (long long)blob_len, blk_off, blk_limit, o);
    }
    hipLaunchKernelGGL(plat::k_bgzf_status, dim3(1), dim3(1), 0, st, o);
    PLAT_HIP(ctx, hipGetLastError());
    return PLAT_OK;
}

PLAT_EXPORT int plat_bam_find_records(plat_ctx* ctx, const plat_bam_find_in* in, const plat_bam_find_out* out, void* stream)
{
    if (!ctx || !in || !out || in->n_streams < 0 || in->n_chunks < 0 || in->n_blocks < 0 || out->cap_records < 0) return PLAT_ERR_INVALID;
    const plat_bam_find_out& o = *out;
    if (!o.status || !o.stream_begin) return PLAT_ERR_INVALID;
    if (in->n_streams > 0 && (!in->data || ((uintptr_t)in->data & 15) || !in->out_off || !in->stream_chunk_begin || !in->tid || !in->beg || !in->end)) return PLAT_ERR_INVALID;
    if (in->n_chunks > 0 && (!in->chunk_blk_first || !in->chunk_blk_end || !in->chunk_first_uoffset || !in->chunk_stop_blk || !in->chunk_stop_uoffset))
        return PLAT_ERR_INVALID;
    if (out->cap_records > 0 && (!o.rec_off || !o.rec_limit)) return PLAT_ERR_INVALID;
    PLAT_HIP(ctx, hipSetDevice(ctx->device));
    const hipStream_t st = (hipStream_t)stream;
    PLAT_HIP(ctx, hipMemsetAsync(o.status, 0xff, 2 * sizeof(int64_t), st));
    PLAT_HIP(ctx, hipMemsetAsync(o.status + 2, 0, 2 * sizeof(int64_t), st));
    if (in->n_streams > 0) PLAT_LAUNCH(ctx, PLAT_KT_OTHER, st, plat::k_bam_find<false>, dim3((unsigned)in->n_streams), dim3(plat::FIND_THREADS), 0, *in, o);
    hipLaunchKernelGGL(plat::k_bam_find_scan, dim3(1), dim3(64), 0, st, in->n_streams, o);
    if (in->n_streams > 0 && out->cap_records > 0)
        PLAT_LAUNCH(ctx, PLAT_KT_OTHER, st, plat::k_bam_find<true>, dim3((unsigned)in->n_streams), dim3(plat::FIND_THREADS), 0, *in, o);
    PLAT_HIP(ctx, hipGetLastError());
    return PLAT_OK;
}
