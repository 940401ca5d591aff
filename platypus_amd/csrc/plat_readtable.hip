// plat_readtable.hip -- read tables on the device: window read slices gathered out of a resident table, packed tables unpacked (whole, by
// pieces, the 2-bit codes alone), a chunk's table concatenated from resident tables, pieces of device memory copied into one blob.
#include "plat_internal.hpp"
#include "read_source.hpp"

// ---- window read slices out of a resident read table (plat_gather_reads) --------------------------------------------------
namespace plat {
// Four destination reads per wave, sixteen lanes each: lanes 0-7 of the sixteen move the bases, 8-15 the qualities, 16 bytes at a time
// from and to any address (global memory takes unaligned 64-bit loads and stores).  A read's copy is a chain of three dependent loads
// (index -> offsets -> bytes) that a wave waits out whatever its width: with one read per wave (rounds 3-4) the 230 k reads of a chunk of
// 64 regions were 28 rounds of waves on the chip, 76-85 us for 86 MB; four per wave share each wait.
__global__ void __launch_bounds__(256)
k_gather_reads(long long n_dst, const int32_t* __restrict__ src_index, const int64_t* __restrict__ dst_off,
               const uint8_t* __restrict__ src_seq, const uint8_t* __restrict__ src_qual, const int64_t* __restrict__ src_off,
               const int32_t* __restrict__ src_pos, const int32_t* __restrict__ src_end, const uint8_t* __restrict__ src_mapq,
               const int32_t* __restrict__ src_flags, uint8_t* __restrict__ dst_seq, uint8_t* __restrict__ dst_qual,
               int32_t* __restrict__ dst_pos, int32_t* __restrict__ dst_end, uint8_t* __restrict__ dst_mapq, int32_t* __restrict__ dst_flags)
{
    typedef unsigned long long __attribute__((aligned(1))) u64u;
    const int l16 = threadIdx.x & 15, l8 = l16 & 7;
    const long long ng = ((long long)gridDim.x * blockDim.x) >> 4;
    for (long long d = (((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 4); d < n_dst; d += ng) {
        const int s = src_index[d];
        const long long so = src_off[s], n = src_off[s + 1] - so, to = dst_off[d];
        const uint8_t* src = l16 < 8 ? src_seq + so : src_qual + so;
        uint8_t* dst = l16 < 8 ? dst_seq + to : dst_qual + to;
        if (n >= 16) {                                                  // pieces of 16 bytes; the last one ends AT the read's end (it may overlap the one before)
            const long long np = (n + 15) >> 4;
            for (long long k = l8; k < np; k += 8) {
                const long long i = k + 1 < np ? 16 * k : n - 16;
                const unsigned long long a = *(const u64u*)(src + i), c = *(const u64u*)(src + i + 8);
                *(u64u*)(dst + i) = a; *(u64u*)(dst + i + 8) = c;
            }
        } else for (long long i = l8; i < n; i += 8) dst[i] = src[i];
        if (l16 == 0) { dst_pos[d] = src_pos[s]; dst_end[d] = src_end[s]; dst_mapq[d] = src_mapq[s]; dst_flags[d] = src_flags[s]; }
    }
}

// The same from packed sources (plat_gather_reads_packed): sixteen lanes per destination read, each turns 16 packed bytes into the base line
// AND the quality line (half the bytes in for the same bytes out).  A read with exceptions -- rare -- goes byte by byte through the accessor.
__global__ void __launch_bounds__(256)
k_gather_reads_packed(long long n_dst, const int32_t* __restrict__ src_index, const int64_t* __restrict__ dst_off, plat_packed_reads pk,
                      const int64_t* __restrict__ src_off, const int32_t* __restrict__ src_pos, const int32_t* __restrict__ src_end,
                      const uint8_t* __restrict__ src_mapq, const int32_t* __restrict__ src_flags, uint8_t* __restrict__ dst_seq,
                      uint8_t* __restrict__ dst_qual, int32_t* __restrict__ dst_pos, int32_t* __restrict__ dst_end, uint8_t* __restrict__ dst_mapq,
                      int32_t* __restrict__ dst_flags)
{
    typedef unsigned long long __attribute__((aligned(1))) u64u;
    const int l16 = threadIdx.x & 15;
    const long long ng = ((long long)gridDim.x * blockDim.x) >> 4;
    const SrcPacked sp{pk};
    for (long long d = (((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 4); d < n_dst; d += ng) {
        const int s = src_index[d];
        const long long so = src_off[s], n = src_off[s + 1] - so, to = dst_off[d];
        const ReadPacked rd = sp.read(s, so, n);
        uint8_t* dseq = dst_seq + to;
        uint8_t* dqual = dst_qual + to;
        if (n >= 16 && rd.e0 == rd.e1) {                                // pieces of 16 bytes; the last one ends AT the read's end (it may overlap the one before)
            const long long np = (n + 15) >> 4;
            for (long long k = l16; k < np; k += 16) {
                const long long i = k + 1 < np ? 16 * k : n - 16;
                const unsigned long long a = *(const u64u*)(rd.p + i), c = *(const u64u*)(rd.p + i + 8);
                const uint32_t w[4] = {(uint32_t)a, (uint32_t)(a >> 32), (uint32_t)c, (uint32_t)(c >> 32)};
                uint32_t sq[4], ql[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    sq[q] = __builtin_amdgcn_perm(0u, 0x47544341u, w[q] & 0x03030303u);       // byte selector 0..3 -> 'A' 'C' 'T' 'G'
                    ql[q] = (w[q] >> 2) & 0x3F3F3F3Fu;
                }
                *(u64u*)(dseq + i) = (unsigned long long)sq[0] | ((unsigned long long)sq[1] << 32);
                *(u64u*)(dseq + i + 8) = (unsigned long long)sq[2] | ((unsigned long long)sq[3] << 32);
                *(u64u*)(dqual + i) = (unsigned long long)ql[0] | ((unsigned long long)ql[1] << 32);
                *(u64u*)(dqual + i + 8) = (unsigned long long)ql[2] | ((unsigned long long)ql[3] << 32);
            }
        } else for (long long i = l16; i < n; i += 16) { dseq[i] = rd.base((int)i); dqual[i] = rd.qual((int)i); }
        if (l16 == 0) { dst_pos[d] = src_pos[s]; dst_end[d] = src_end[s]; dst_mapq[d] = src_mapq[s]; dst_flags[d] = src_flags[s]; }
    }
}
}  // namespace plat

PLAT_EXPORT int plat_gather_reads_packed(plat_ctx* ctx, int64_t n_dst, const int32_t* src_index, const int64_t* dst_off, const plat_packed_reads* packed,
                                         const int64_t* src_off, const int32_t* src_pos, const int32_t* src_end, const uint8_t* src_mapq,
                                         const int32_t* src_flags, uint8_t* dst_seq, uint8_t* dst_qual, int32_t* dst_pos, int32_t* dst_end,
                                         uint8_t* dst_mapq, int32_t* dst_flags, void* stream)
{
    if (!ctx || n_dst < 0 || !packed || packed->n_exc < 0) return PLAT_ERR_INVALID;
    if (n_dst == 0) return PLAT_OK;
    const plat_packed_reads pk = *packed;
    if (!src_index || !dst_off || !pk.read_src || (pk.n_exc > 0 && (!pk.exc_index || !pk.exc_base || !pk.exc_qual)) || !src_off || !src_pos || !src_end ||
        !src_mapq || !src_flags || !dst_seq || !dst_qual || !dst_pos || !dst_end || !dst_mapq || !dst_flags)
        return PLAT_ERR_INVALID;
    PLAT_HIP(ctx, hipSetDevice(ctx->device));
    const long long nblk = (n_dst + 15) / 16;                         // 256 threads = 16 reads
    PLAT_LAUNCH(ctx, PLAT_KT_GATHER_READS, stream, plat::k_gather_reads_packed, dim3((unsigned)(nblk < 65535 * 8 ? nblk : 65535 * 8)), dim3(256), 0,
                       (long long)n_dst, src_index, dst_off, pk, src_off, src_pos, src_end, src_mapq, src_flags, dst_seq, dst_qual, dst_pos, dst_end, dst_mapq,
                       dst_flags);
    PLAT_HIP(ctx, hipGetLastError());
    return PLAT_OK;
}

PLAT_EXPORT int plat_gather_reads(plat_ctx* ctx, int64_t n_dst, const int32_t* src_index, const int64_t* dst_off,
                                  const uint8_t* src_seq, const uint8_t* src_qual, const int64_t* src_off, const int32_t* src_pos,
                                  const int32_t* src_end, const uint8_t* src_mapq, const int32_t* src_flags, uint8_t* dst_seq,
                                  uint8_t* dst_qual, int32_t* dst_pos, int32_t* dst_end, uint8_t* dst_mapq, int32_t* dst_flags,
                                  void* stream)
{
    if (!ctx || n_dst < 0) return PLAT_ERR_INVALID;
    if (n_dst == 0) return PLAT_OK;
    if (!src_index || !dst_off || !src_seq || !src_qual || !src_off || !src_pos || !src_end || !src_mapq || !src_flags || !dst_seq ||
        !dst_qual || !dst_pos || !dst_end || !dst_mapq || !dst_flags)
        return PLAT_ERR_INVALID;
    PLAT_HIP(ctx, hipSetDevice(ctx->device));
    const long long nblk = (n_dst + 15) / 16;                         // 256 threads = 16 reads
    PLAT_LAUNCH(ctx, PLAT_KT_GATHER_READS, stream, plat::k_gather_reads, dim3((unsigned)(nblk < 65535 * 8 ? nblk : 65535 * 8)), dim3(256), 0, (long long)n_dst,
                       src_index, dst_off, src_seq, src_qual, src_off, src_pos, src_end, src_mapq, src_flags, dst_seq, dst_qual, dst_pos,
                       dst_end, dst_mapq, dst_flags);
    PLAT_HIP(ctx, hipGetLastError());
    return PLAT_OK;
}


// ---- read tables packed at one byte per base (plat_unpack_reads) ----------------------------------------------------------
namespace plat {
// 16 packed bytes per thread: one 128-bit load (two 64-bit ones from any address when the source does not share the outputs' alignment:
// global memory takes unaligned loads), two 128-bit stores.  The two OUTPUT arrays may start anywhere as long as they share their
// misalignment `mis` (a read table inside a chunk's blob does): thread t takes the 16-byte line [16 t - mis, 16 t - mis + 16) of them,
// clipped to [0, n) at the two ends.
__global__ void __launch_bounds__(256)
k_unpack_reads(long long n, int mis, int vec, int src_aligned, const uint8_t* __restrict__ packed, uint8_t* __restrict__ out_seq, uint8_t* __restrict__ out_qual)
{
    const long long i0 = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 16 - mis;
    if (i0 >= n) return;
    if (vec && i0 >= 0 && i0 + 16 <= n) {
        uint32_t w[4];
        if (src_aligned) { const uint4 v = *(const uint4*)(packed + i0); w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w; }
        else {
            const unsigned long long lo = load_u64_bytes(packed + i0), hi = load_u64_bytes(packed + i0 + 8);
            w[0] = (uint32_t)lo; w[1] = (uint32_t)(lo >> 32); w[2] = (uint32_t)hi; w[3] = (uint32_t)(hi >> 32);
        }
        uint32_t sq[4], ql[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t code = w[k] & 0x03030303u;
            sq[k] = __builtin_amdgcn_perm(0u, 0x47544341u, code);           // byte selector 0..3 -> 'A' 'C' 'T' 'G'
            ql[k] = (w[k] >> 2) & 0x3F3F3F3Fu;
        }
        *(uint4*)(out_seq + i0) = make_uint4(sq[0], sq[1], sq[2], sq[3]);
        *(uint4*)(out_qual + i0) = make_uint4(ql[0], ql[1], ql[2], ql[3]);
    } else {
        for (long long i = i0 < 0 ? 0 : i0; i < n && i < i0 + 16; ++i) {
            const unsigned b = packed[i];
            out_seq[i] = (uint8_t)((0x47544341u >> (8u * (b & 3u))) & 0xFFu);
            out_qual[i] = (uint8_t)(b >> 2);
        }
    }
}
__global__ void __launch_bounds__(256)
k_unpack_exceptions(long long n_exc, long long n, const int64_t* __restrict__ idx, const uint8_t* __restrict__ eb, const uint8_t* __restrict__ eq,
                    uint8_t* __restrict__ out_seq, uint8_t* __restrict__ out_qual, uint32_t* __restrict__ codes = nullptr)
{
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_exc) return;
    const long long i = idx[k];
    if (i < 0 || i >= n) return;
    out_seq[i] = eb[k]; out_qual[i] = eq[k];
    if (codes) {                                                           // the base's code follows its byte: (ASCII >> 1) & 3
        const unsigned sh = 2u * (unsigned)(i & 15);
        atomicAnd(&codes[i >> 4], ~(3u << sh));
        atomicOr(&codes[i >> 4], (((unsigned)eb[k] >> 1) & 3u) << sh);
    }
}
}  // namespace plat

PLAT_EXPORT int plat_unpack_reads(plat_ctx* ctx, int64_t n_bytes, const uint8_t* packed, uint8_t* out_seq, uint8_t* out_qual,
                                  int64_t n_exc, const int64_t* exc_index, const uint8_t* exc_base, const uint8_t* exc_qual, void* stream)
{
    if (!ctx || n_bytes < 0 || n_exc < 0) return PLAT_ERR_INVALID;
    if (n_bytes == 0) return PLAT_OK;
    if (!packed || !out_seq || !out_qual || (n_exc > 0 && (!exc_index || !exc_base || !exc_qual))) return PLAT_ERR_INVALID;
    PLAT_HIP(ctx, hipSetDevice(ctx->device));
    // lanes work on 16-byte lines of the OUTPUT arrays: possible when the two share their misalignment (else byte by byte); a source
    // with another misalignment (a resident table expanded into its place in a chunk's blob) is read with unaligned loads
    const int m0 = (int)((uintptr_t)packed & 15), m1 = (int)((uintptr_t)out_seq & 15), m2 = (int)((uintptr_t)out_qual & 15);
    const int vec = m1 == m2, mis = vec ? m1 : 0;                          // (not shared: every thread walks its own 16 bytes)
    const long long nthr = (n_bytes + mis + 15) / 16;
    hipLaunchKernelGGL(plat::k_unpack_reads, dim3((unsigned)((nthr + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (long long)n_bytes,
                       mis, vec, (int)(m0 == mis), packed, out_seq, out_qual);
    if (n_exc > 0)
        hipLaunchKernelGGL(plat::k_unpack_exceptions, dim3((unsigned)((n_exc + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (long long)n_exc,
                           (long long)n_bytes, exc_index, exc_base, exc_qual, out_seq, out_qual);
    PLAT_HIP(ctx, hipGetLastError());
    return PLAT_OK;
}


namespace plat {
// k_unpack_reads for a list of pieces: blockIdx.y = piece; lanes work on 16-byte lines of the piece's place in the output
__global__ void __launch_bounds__(256)
k_unpack_pieces(const plat_unpack_piece* __restrict__ pieces, uint8_t* __restrict__ out_seq, uint8_t* __restrict__ out_qual, int same_base_alignment,
                uint32_t* __restrict__ codes)
{
    // codes (round 6, may be null): the bases again as 2 bits each (A 0, C 1, T 2, G 3 = the packed byte's low bits = (ASCII >> 1) & 3), base i of the
    // blob at bits 2 (i & 15) of dword i >> 4 -- what plat_candidates_batch_codes compares 32 bases per 64-bit word.  A whole line of 16 bases is one
    // plain store; the bases of a partial line (a piece's first and last) are OR-ed in, the buffer having been zeroed by the caller.
    const plat_unpack_piece pc = pieces[blockIdx.y];
    const uint8_t* packed = pc.src;
    uint8_t* oseq = out_seq + pc.dst;
    uint8_t* oqual = out_qual + pc.dst;
    const long long n = pc.n;
    const int mis = same_base_alignment ? (int)((uintptr_t)oseq & 15) : 0;
    const bool srcAligned = (((uintptr_t)packed - (uintptr_t)mis) & 15) == 0 || (((uintptr_t)packed & 15) == (unsigned)mis);
    const long long lines = (n + mis + 15) / 16;
    for (long long ln = (long long)blockIdx.x * blockDim.x + threadIdx.x; ln < lines; ln += (long long)gridDim.x * blockDim.x) {
        const long long i0 = ln * 16 - mis;
        if (same_base_alignment && i0 >= 0 && i0 + 16 <= n) {
            uint32_t w[4];
            if (srcAligned) { const uint4 v = *(const uint4*)(packed + i0); w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w; }
            else {
                const unsigned long long lo = load_u64_bytes(packed + i0), hi = load_u64_bytes(packed + i0 + 8);
                w[0] = (uint32_t)lo; w[1] = (uint32_t)(lo >> 32); w[2] = (uint32_t)hi; w[3] = (uint32_t)(hi >> 32);
            }
            uint32_t sq[4], ql[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t code = w[k] & 0x03030303u;
                sq[k] = __builtin_amdgcn_perm(0u, 0x47544341u, code);
                ql[k] = (w[k] >> 2) & 0x3F3F3F3Fu;
            }
            *(uint4*)(oseq + i0) = make_uint4(sq[0], sq[1], sq[2], sq[3]);
            *(uint4*)(oqual + i0) = make_uint4(ql[0], ql[1], ql[2], ql[3]);
            if (codes) {
                uint32_t cw = 0;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    uint32_t t = w[k] & 0x03030303u;
                    t = (t | (t >> 6)) & 0x000F000Fu;
                    cw |= ((t | (t >> 12)) & 0xFFu) << (8 * k);
                }
                const long long at = pc.dst + i0;                          // blob index of the line's first base
                if ((at & 15) == 0) codes[at >> 4] = cw;
                else for (int k = 0; k < 16; ++k) atomicOr(&codes[(at + k) >> 4], ((cw >> (2 * k)) & 3u) << (2 * ((at + k) & 15)));
            }
        } else {
            for (long long i = i0 < 0 ? 0 : i0; i < n && i < i0 + 16; ++i) {
                const unsigned bb = packed[i];
                oseq[i] = (uint8_t)((0x47544341u >> (8u * (bb & 3u))) & 0xFFu);
                oqual[i] = (uint8_t)(bb >> 2);
                if (codes) atomicOr(&codes[(pc.dst + i) >> 4], (bb & 3u) << (2 * ((pc.dst + i) & 15)));
            }
        }
    }
}
}  // namespace plat

static int unpack_pieces(plat_ctx* ctx, int n_pieces, int64_t max_piece_bytes, const plat_unpack_piece* pieces, uint8_t* out_seq, uint8_t* out_qual, uint32_t* out_codes,
                         int64_t total_bytes, int64_t n_exc, const int64_t* exc_index, const uint8_t* exc_base, const uint8_t* exc_qual, void* stream);

PLAT_EXPORT int plat_unpack_reads_pieces(plat_ctx* ctx, int n_pieces, int64_t max_piece_bytes, const plat_unpack_piece* pieces, uint8_t* out_seq, uint8_t* out_qual,
                                         int64_t total_bytes, int64_t n_exc, const int64_t* exc_index, const uint8_t* exc_base, const uint8_t* exc_qual, void* stream)
{
    return unpack_pieces(ctx, n_pieces, max_piece_bytes, pieces, out_seq, out_qual, nullptr, total_bytes, n_exc, exc_index, exc_base, exc_qual, stream);
}

PLAT_EXPORT int plat_unpack_reads_pieces_codes(plat_ctx* ctx, int n_pieces, int64_t max_piece_bytes, const plat_unpack_piece* pieces, uint8_t* out_seq, uint8_t* out_qual,
                                               uint32_t* out_codes, int64_t total_bytes, int64_t n_exc, const int64_t* exc_index, const uint8_t* exc_base,
                                               const uint8_t* exc_qual, void* stream)
{
    if (!out_codes) return PLAT_ERR_INVALID;
    return unpack_pieces(ctx, n_pieces, max_piece_bytes, pieces, out_seq, out_qual, out_codes, total_bytes, n_exc, exc_index, exc_base, exc_qual, stream);
}

static int unpack_pieces(plat_ctx* ctx, int n_pieces, int64_t max_piece_bytes, const plat_unpack_piece* pieces, uint8_t* out_seq, uint8_t* out_qual, uint32_t* out_codes,
                         int64_t total_bytes, int64_t n_exc, const int64_t* exc_index, const uint8_t* exc_base, const uint8_t* exc_qual, void* stream)
{
    if (!ctx || n_pieces < 0 || max_piece_bytes < 0 || total_bytes < 0 || n_exc < 0) return PLAT_ERR_INVALID;
    if (n_pieces == 0) return PLAT_OK;
    if (!pieces || !out_seq || !out_qual || (n_exc > 0 && (!exc_index || !exc_base || !exc_qual))) return PLAT_ERR_INVALID;
    PLAT_HIP(ctx, hipSetDevice(ctx->device));
    // (the code words of partial lines are OR-ed in: the buffer starts as zeros; + 8 words: plat_candidates_batch_codes reads a 64-bit word past the last base)
    if (out_codes) PLAT_HIP(ctx, hipMemsetAsync(out_codes, 0, ((size_t)(total_bytes + 15) / 16 + 8) * sizeof(uint32_t), (hipStream_t)stream));
    const int same = ((uintptr_t)out_seq & 15) == ((uintptr_t)out_qual & 15);
    long long gx = (max_piece_bytes / 16 + 256) / 256;
    gx = gx < 1 ? 1 : (gx > 1024 ? 1024 : gx);
    PLAT_EV_TAB(ctx, 0, (hipStream_t)stream);
    for (int p0 = 0; p0 < n_pieces; p0 += PLAT_GRID_Y_MAX) {      // (gridDim.y holds at most 65 535 pieces: one launch per batch of them)
        const int np = n_pieces - p0 < PLAT_GRID_Y_MAX ? n_pieces - p0 : PLAT_GRID_Y_MAX;
        PLAT_LAUNCH(ctx, PLAT_KT_UNPACK_PIECES, stream, plat::k_unpack_pieces, dim3((unsigned)gx, (unsigned)np), dim3(256), 0, pieces + p0, out_seq, out_qual, same, out_codes);
    }
    PLAT_EV_TAB(ctx, 1, (hipStream_t)stream);
    ctx->ev_valid_unpack = ctx->profile;
    if (n_exc > 0)
        hipLaunchKernelGGL(plat::k_unpack_exceptions, dim3((unsigned)((n_exc + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (long long)n_exc,
                           (long long)total_bytes, exc_index, exc_base, exc_qual, out_seq, out_qual, out_codes);
    PLAT_HIP(ctx, hipGetLastError());
    return PLAT_OK;
}

// ---- the codes alone, the packed bytes staying where they are (plat_pack_codes_pieces) ------------------------------------------------------
namespace plat {
// Before the pass: the code dwords a piece does not fill by itself -- the one holding its first base and the one behind its last, where they are
// shared with a neighbouring piece or with nothing -- and the 8 words behind the blob's last base start as zeros; everything else is stored whole.
// (The whole-buffer memset of plat_unpack_reads_pieces_codes was a quarter byte per base written twice.)
__global__ void __launch_bounds__(256)
k_codes_edges(const plat_unpack_piece* __restrict__ pieces, int n_pieces, long long total_bytes, uint32_t* __restrict__ codes)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n_pieces) {
        const plat_unpack_piece pc = pieces[k];
        if (pc.n > 0) {
            if (pc.dst & 15) codes[pc.dst >> 4] = 0u;
            if ((pc.dst + pc.n) & 15) codes[(pc.dst + pc.n) >> 4] = 0u;
        }
    } else if (k < n_pieces + 8) codes[(total_bytes + 15) / 16 + (k - n_pieces)] = 0u;
}

// blockIdx.y = piece; one thread per code dword of the piece's place in the blob (16 bases: one 128-bit load, or two 64-bit ones from a source of
// another alignment, and one 32-bit store); a dword the piece shares is OR-ed in, once
__global__ void __launch_bounds__(256)
k_unpack_pieces_codes(const plat_unpack_piece* __restrict__ pieces, uint32_t* __restrict__ codes)
{
    const plat_unpack_piece pc = pieces[blockIdx.y];
    const uint8_t* packed = pc.src;
    const long long n = pc.n;
    if (n <= 0) return;
    const long long d0 = pc.dst >> 4, d1 = (pc.dst + n + 15) >> 4;
    const bool srcAligned = (((uintptr_t)packed - (uintptr_t)(pc.dst & 15)) & 15) == 0;
    for (long long d = d0 + (long long)blockIdx.x * blockDim.x + threadIdx.x; d < d1; d += (long long)gridDim.x * blockDim.x) {
        const long long i0 = 16 * d - pc.dst;                              // the dword's first base, counted from the piece's
        if (i0 >= 0 && i0 + 16 <= n) {
            uint32_t w[4];
            if (srcAligned) { const uint4 v = *(const uint4*)(packed + i0); w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w; }
            else {
                const unsigned long long lo = load_u64_bytes(packed + i0), hi = load_u64_bytes(packed + i0 + 8);
                w[0] = (uint32_t)lo; w[1] = (uint32_t)(lo >> 32); w[2] = (uint32_t)hi; w[3] = (uint32_t)(hi >> 32);
            }
            uint32_t cw = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                uint32_t t = w[k] & 0x03030303u;
                t = (t | (t >> 6)) & 0x000F000Fu;
                cw |= ((t | (t >> 12)) & 0xFFu) << (8 * k);
            }
            codes[d] = cw;
        } else {
            uint32_t cw = 0;
            for (long long i = i0 < 0 ? 0 : i0; i < n && i < i0 + 16; ++i) cw |= ((uint32_t)packed[i] & 3u) << (2 * (int)(i - i0));
            atomicOr(&codes[d], cw);
        }
    }
}

__global__ void __launch_bounds__(256)
k_codes_exceptions(long long n_exc, long long n, const int64_t* __restrict__ idx, const uint8_t* __restrict__ eb, uint32_t* __restrict__ codes)
{
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_exc) return;
    const long long i = idx[k];
    if (i < 0 || i >= n) return;
    const unsigned sh = 2u * (unsigned)(i & 15);                           // the base's code follows its byte: (ASCII >> 1) & 3
    atomicAnd(&codes[i >> 4], ~(3u << sh));
    atomicOr(&codes[i >> 4], (((unsigned)eb[k] >> 1) & 3u) << sh);
}
}  // namespace plat

PLAT_EXPORT int plat_pack_codes_pieces(plat_ctx* ctx, int n_pieces, int64_t max_piece_bytes, const plat_unpack_piece* pieces, uint32_t* out_codes,
                                       int64_t total_bytes, int64_t n_exc, const int64_t* exc_index, const uint8_t* exc_base, void* stream)
{
    if (!ctx || n_pieces < 0 || max_piece_bytes < 0 || total_bytes < 0 || n_exc < 0) return PLAT_ERR_INVALID;
    if (n_pieces == 0) return PLAT_OK;
    if (!pieces || !out_codes || (n_exc > 0 && (!exc_index || !exc_base))) return PLAT_ERR_INVALID;
    PLAT_HIP(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(plat::k_codes_edges, dim3((unsigned)((n_pieces + 8 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, pieces, n_pieces, (long long)total_bytes, out_codes);
    long long gx = (max_piece_bytes / 16 + 256) / 256;
    gx = gx < 1 ? 1 : (gx > 1024 ? 1024 : gx);
    PLAT_EV_TAB(ctx, 0, (hipStream_t)stream);
    for (int p0 = 0; p0 < n_pieces; p0 += PLAT_GRID_Y_MAX) {      // (gridDim.y holds at most 65 535 pieces: one launch per batch of them)
        const int np = n_pieces - p0 < PLAT_GRID_Y_MAX ? n_pieces - p0 : PLAT_GRID_Y_MAX;
        PLAT_LAUNCH(ctx, PLAT_KT_UNPACK_PIECES, stream, plat::k_unpack_pieces_codes, dim3((unsigned)gx, (unsigned)np), dim3(256), 0, pieces + p0, out_codes);
    }
    PLAT_EV_TAB(ctx, 1, (hipStream_t)stream);
    ctx->ev_valid_unpack = ctx->profile;
    if (n_exc > 0)
        hipLaunchKernelGGL(plat::k_codes_exceptions, dim3((unsigned)((n_exc + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (long long)n_exc, (long long)total_bytes,
                           exc_index, exc_base, out_codes);
    PLAT_HIP(ctx, hipGetLastError());
    return PLAT_OK;
}

// ---- a chunk's read table put together on the device from resident tables (plat_concat_read_tables) ----------------------------------
namespace plat {
__device__ __forceinline__ void concat_src(const plat_table_desc&, int, long long, const uint8_t**) {}
__device__ __forceinline__ void concat_src(const plat_table_src_desc& d, int i, long long r, const uint8_t** dst_src) { dst_src[r] = d.src + d.off[i]; }

// (D = plat_table_src_desc: + the per-read source pointer column of a chunk whose packed bytes are read where they lie)
template <class D>
__device__ __forceinline__ void concat_tables_one(const D* __restrict__ desc, int64_t* __restrict__ dst_off, int32_t* __restrict__ dst_pos, int32_t* __restrict__ dst_end,
                uint8_t* __restrict__ dst_mapq, int32_t* __restrict__ dst_flags, int32_t* __restrict__ dst_cig_off, int16_t* __restrict__ dst_cigar,
                int32_t* __restrict__ dst_region, const uint8_t** __restrict__ dst_src, long long n_total, long long total_bytes, long long total_pairs)
{
    const D d = desc[blockIdx.y];
    const int stride = gridDim.x * blockDim.x;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < d.n; i += stride) {
        const long long r = d.first_read + i;
        dst_off[r] = d.first_byte + d.off[i];
        concat_src(d, i, r, dst_src);
        dst_pos[r] = d.pos[i]; dst_end[r] = d.end[i]; dst_mapq[r] = d.mapq[i]; dst_flags[r] = d.flags[i];
        const int c0 = d.cig_off[i], c1 = d.cig_off[i + 1];
        dst_cig_off[r] = (int32_t)(d.first_pair + c0);
        for (int c = c0; c < c1; ++c) {
            dst_cigar[2 * (d.first_pair + c)] = d.cigar[2 * c];
            dst_cigar[2 * (d.first_pair + c) + 1] = d.cigar[2 * c + 1];
        }
        if (d.scan >= 0) dst_region[r] = d.scan;
    }
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
        dst_off[n_total] = total_bytes; dst_cig_off[n_total] = (int32_t)total_pairs;
        dst_cigar[2 * total_pairs] = 0; dst_cigar[2 * total_pairs + 1] = 0;
    }
}

__global__ void __launch_bounds__(256)
k_concat_tables(const plat_table_desc* __restrict__ desc, int64_t* __restrict__ dst_off, int32_t* __restrict__ dst_pos, int32_t* __restrict__ dst_end,
                uint8_t* __restrict__ dst_mapq, int32_t* __restrict__ dst_flags, int32_t* __restrict__ dst_cig_off, int16_t* __restrict__ dst_cigar,
                int32_t* __restrict__ dst_region, long long n_total, long long total_bytes, long long total_pairs)
{
    concat_tables_one(desc, dst_off, dst_pos, dst_end, dst_mapq, dst_flags, dst_cig_off, dst_cigar, dst_region, nullptr, n_total, total_bytes, total_pairs);
}

__global__ void __launch_bounds__(256)
k_concat_tables_src(const plat_table_src_desc* __restrict__ desc, int64_t* __restrict__ dst_off, int32_t* __restrict__ dst_pos, int32_t* __restrict__ dst_end,
                    uint8_t* __restrict__ dst_mapq, int32_t* __restrict__ dst_flags, int32_t* __restrict__ dst_cig_off, int16_t* __restrict__ dst_cigar,
                    int32_t* __restrict__ dst_region, const uint8_t** __restrict__ dst_src, long long n_total, long long total_bytes, long long total_pairs)
{
    concat_tables_one(desc, dst_off, dst_pos, dst_end, dst_mapq, dst_flags, dst_cig_off, dst_cigar, dst_region, dst_src, n_total, total_bytes, total_pairs);
}
}  // namespace plat

PLAT_EXPORT int plat_concat_read_tables_src(plat_ctx* ctx, int n_tables, int max_reads_per_table, const plat_table_src_desc* desc, int64_t* dst_off, int32_t* dst_pos,
                                            int32_t* dst_end, uint8_t* dst_mapq, int32_t* dst_flags, int32_t* dst_cig_off, int16_t* dst_cigar,
                                            int32_t* dst_region, const uint8_t** dst_src, int64_t n_total_reads, int64_t total_bytes, int64_t total_pairs, void* stream)
{
    if (!ctx || n_tables < 0 || max_reads_per_table < 0 || n_total_reads < 0) return PLAT_ERR_INVALID;
    if (!dst_off || !dst_pos || !dst_end || !dst_mapq || !dst_flags || !dst_cig_off || !dst_cigar || !dst_region || !dst_src) return PLAT_ERR_INVALID;
    if (n_tables < 1 || !desc) return PLAT_ERR_INVALID;
    PLAT_HIP(ctx, hipSetDevice(ctx->device));
    unsigned gx = (unsigned)((max_reads_per_table + 255) / 256);
    gx = gx < 1 ? 1 : (gx > 64 ? 64 : gx);
    for (int t0 = 0; t0 < n_tables; t0 += PLAT_GRID_Y_MAX) {      // (every batch's first block also writes the table's closing entries: the same values)
        const int nt = n_tables - t0 < PLAT_GRID_Y_MAX ? n_tables - t0 : PLAT_GRID_Y_MAX;
        PLAT_LAUNCH(ctx, PLAT_KT_CONCAT_TABLES, stream, plat::k_concat_tables_src, dim3(gx, (unsigned)nt), dim3(256), 0, desc + t0, dst_off, dst_pos, dst_end,
                           dst_mapq, dst_flags, dst_cig_off, dst_cigar, dst_region, dst_src, (long long)n_total_reads, (long long)total_bytes, (long long)total_pairs);
    }
    PLAT_HIP(ctx, hipGetLastError());
    return PLAT_OK;
}

PLAT_EXPORT int plat_concat_read_tables(plat_ctx* ctx, int n_tables, int max_reads_per_table, const plat_table_desc* desc, int64_t* dst_off, int32_t* dst_pos,
                                        int32_t* dst_end, uint8_t* dst_mapq, int32_t* dst_flags, int32_t* dst_cig_off, int16_t* dst_cigar,
                                        int32_t* dst_region, int64_t n_total_reads, int64_t total_bytes, int64_t total_pairs, void* stream)
{
    if (!ctx || n_tables < 0 || max_reads_per_table < 0 || n_total_reads < 0) return PLAT_ERR_INVALID;
    if (!dst_off || !dst_pos || !dst_end || !dst_mapq || !dst_flags || !dst_cig_off || !dst_cigar || !dst_region) return PLAT_ERR_INVALID;
    if (n_tables < 1 || !desc) return PLAT_ERR_INVALID;
    PLAT_HIP(ctx, hipSetDevice(ctx->device));
    unsigned gx = (unsigned)((max_reads_per_table + 255) / 256);
    gx = gx < 1 ? 1 : (gx > 64 ? 64 : gx);
    for (int t0 = 0; t0 < n_tables; t0 += PLAT_GRID_Y_MAX) {      // (every batch's first block also writes the table's closing entries: the same values)
        const int nt = n_tables - t0 < PLAT_GRID_Y_MAX ? n_tables - t0 : PLAT_GRID_Y_MAX;
        PLAT_LAUNCH(ctx, PLAT_KT_CONCAT_TABLES, stream, plat::k_concat_tables, dim3(gx, (unsigned)nt), dim3(256), 0, desc + t0, dst_off, dst_pos, dst_end,
                           dst_mapq, dst_flags, dst_cig_off, dst_cigar, dst_region, (long long)n_total_reads, (long long)total_bytes, (long long)total_pairs);
    }
    PLAT_HIP(ctx, hipGetLastError());
    return PLAT_OK;
}


// ---- pieces of device memory into one blob (plat_copy_pieces) -----------------------------------------------------------------------------
namespace plat {
__global__ void __launch_bounds__(256)
k_copy_pieces(const plat_unpack_piece* __restrict__ pieces, uint8_t* __restrict__ dst_blob)
{
    typedef unsigned long long __attribute__((aligned(1))) u64u;
    const plat_unpack_piece pc = pieces[blockIdx.y];
    const uint8_t* src = pc.src;
    uint8_t* dst = dst_blob + pc.dst;
    const long long n8 = pc.n & ~7ll;
    const long long stride = 8ll * gridDim.x * blockDim.x;
    for (long long i = 8ll * ((long long)blockIdx.x * blockDim.x + threadIdx.x); i < n8; i += stride) *(u64u*)(dst + i) = *(const u64u*)(src + i);
    if (blockIdx.x == 0) for (long long i = n8 + threadIdx.x; i < pc.n; i += blockDim.x) dst[i] = src[i];
}
}  // namespace plat

PLAT_EXPORT int plat_copy_pieces(plat_ctx* ctx, int n_pieces, int64_t max_piece_bytes, const plat_unpack_piece* pieces, uint8_t* dst_blob, void* stream)
{
    if (!ctx || n_pieces < 0 || max_piece_bytes < 0) return PLAT_ERR_INVALID;
    if (n_pieces == 0) return PLAT_OK;
    if (!pieces || !dst_blob) return PLAT_ERR_INVALID;
    PLAT_HIP(ctx, hipSetDevice(ctx->device));
    long long gx = (max_piece_bytes / 8 + 256) / 256;
    gx = gx < 1 ? 1 : (gx > 256 ? 256 : gx);
    for (int p0 = 0; p0 < n_pieces; p0 += PLAT_GRID_Y_MAX) {      // (a whole job's regions are one piece each in the exchange: more than gridDim.y holds)
        const int np = n_pieces - p0 < PLAT_GRID_Y_MAX ? n_pieces - p0 : PLAT_GRID_Y_MAX;
        PLAT_LAUNCH(ctx, PLAT_KT_COPY_PIECES, stream, plat::k_copy_pieces, dim3((unsigned)gx, (unsigned)np), dim3(256), 0, pieces + p0, dst_blob);
    }
    PLAT_HIP(ctx, hipGetLastError());
    return PLAT_OK;
}
