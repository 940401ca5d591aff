// plat_bamdecode.hip -- read tables from raw BAM alignment records (plat_bam_decode_batch, include/platypus_mi355x.h): ReadIterator.get
// (htslibWrapper.pyx:328-406) for a whole batch of records.  Three launches:
//   k_bam_core    one lane per record: the 32 fixed bytes and the CIGAR walk with byte loads and bounds checks; the per-read arrays, and
//                 the record's base and pair counts into read_off[i+1] / cig_off[i+1]
//   k_bam_scan    one workgroup: those counts to offsets in place, the capacity check, the status block, the blobs' zeroed slack
//   k_bam_expand  the hot path, 16 lanes per record and 16 bases per lane and step: the lane owns one 16-byte ALIGNED window of the output
//                 blobs, loads the 8-9 sequence bytes and 16 quality bytes behind it as the aligned words that cover them (shifted into
//                 place with v_alignbyte), turns the 16 codes into letters with v_perm, and stores 16 letters and 16 qualities as one
//                 16-byte store each.  Only a record's first and last window (shared with its neighbours) are stored byte by byte.
//                 1.5 bytes in and 2 bytes out per base: a streaming kernel.
// Errors go to the status block; nothing traps.
#include "plat_internal.hpp"
#include "wave_tiles.hpp"

namespace plat {
constexpr int SCAN_THREADS = 1024;
constexpr int SCAN_ITEMS = 4;                             // consecutive records per thread and tile
constexpr unsigned long long BAM_NO_ERROR = ~0ull;

__device__ __forceinline__ uint32_t ld_u16(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
__device__ __forceinline__ uint32_t ld_u32(const uint8_t* p) { return ld_u16(p) | (ld_u16(p + 2) << 16); }

__device__ __forceinline__ void bam_fail(int64_t* status, int i, int err) {
    atomicMin((unsigned long long*)&status[1], ((unsigned long long)(unsigned)i << 8) | (unsigned long long)(unsigned)(-err));
}

__global__ void __launch_bounds__(256)
k_bam_core(int n, const uint8_t* __restrict__ blob, long long blob_len, const int64_t* __restrict__ rec_off, const int64_t* __restrict__ rec_limit,
           plat_bam_decode_out o)
{
    const int i = (int)(blockIdx.x * (long long)blockDim.x + threadIdx.x);
    if (i >= n) return;
    if (i == 0) { o.read_off[0] = 0; o.cig_off[0] = 0; }
    o.read_off[i + 1] = 0; o.cig_off[i + 1] = 0;                        // (a refused record: an empty read)
    const long long off = rec_off[i];
    if (rec_limit && rec_limit[i] < blob_len) blob_len = rec_limit[i];
    if (off < 0 || off > blob_len - 32) { bam_fail(o.status, i, PLAT_ERR_BAD_INPUT); return; }
    const uint8_t* p = blob + off;
    const int32_t refID = (int32_t)ld_u32(p), pos = (int32_t)ld_u32(p + 4), lSeq = (int32_t)ld_u32(p + 16);
    const int32_t nextRef = (int32_t)ld_u32(p + 20), nextPos = (int32_t)ld_u32(p + 24), tlen = (int32_t)ld_u32(p + 28);
    const uint32_t lName = p[8], mapq = p[9], nCig = ld_u16(p + 12), flag = ld_u16(p + 14);
    bool bad = lSeq <= 0 || lSeq > 32767 || nCig > 32767 || refID > 32767 || refID < -32768 || nextRef > 32767 || nextRef < -32768;
    const long long cigAt = 32 + (long long)lName, seqAt = cigAt + 4ll * nCig, qualAt = seqAt + (bad ? 0 : (lSeq + 1) / 2);
    if (!bad && off + qualAt + lSeq > blob_len) bad = true;
    if (bad) { bam_fail(o.status, i, PLAT_ERR_BAD_INPUT); return; }
    if (p[qualAt] == 0xff) { bam_fail(o.status, i, PLAT_ERR_BAD_INPUT); return; }
    long long refLen = 0, clip = 0;
    for (uint32_t k = 0; k < nCig; ++k) {
        const uint32_t w = ld_u32(p + cigAt + 4ll * k), op = w & 15u, len = w >> 4;
        if (op > 8 || len > 32767) bad = true;
        if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) refLen += len;
        if (k == 0 && op == 4) clip = len;
    }
    const long long start = (long long)pos - clip;
    if (bad || start < INT32_MIN || start > INT32_MAX) { bam_fail(o.status, i, PLAT_ERR_BAD_INPUT); return; }
    o.pos[i] = (int32_t)start;
    o.end[i] = (int32_t)(uint32_t)((unsigned long long)(long long)pos + (unsigned long long)(((flag & 4u) || nCig == 0) ? 1ll : refLen));
    o.mapq[i] = (uint8_t)mapq; o.flags[i] = (int32_t)flag;
    o.chrom_id[i] = (int16_t)refID; o.mate_chrom_id[i] = (int16_t)nextRef; o.insert_size[i] = tlen; o.mate_pos[i] = nextPos;
    o.read_off[i + 1] = lSeq; o.cig_off[i + 1] = (int32_t)nCig;
}

__global__ void __launch_bounds__(SCAN_THREADS)
k_bam_scan(int n, plat_bam_decode_out o)
{
    __shared__ long long s_wave[2][SCAN_THREADS / 64];
    __shared__ int s_first;                                             // first record that does not fit
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) s_first = INT32_MAX;
    __syncthreads();
    const long long capPairs = o.cap_pairs < (long long)INT32_MAX ? o.cap_pairs : (long long)INT32_MAX;      // (cig_off is 32 bits wide)
    long long runB = 0, runP = 0;
    for (long long t0 = 0; t0 < n; t0 += SCAN_THREADS * SCAN_ITEMS) {
        const long long i0 = t0 + (long long)tid * SCAN_ITEMS;
        long long b[SCAN_ITEMS], c[SCAN_ITEMS], sb = 0, sc = 0;
        for (int k = 0; k < SCAN_ITEMS; ++k) {
            const bool in = i0 + k < n;
            b[k] = in ? o.read_off[i0 + k + 1] : 0; c[k] = in ? o.cig_off[i0 + k + 1] : 0;
            sb += b[k]; sc += c[k];
        }
        const long long ib = wave_incl_scan(sb, lane), ic = wave_incl_scan(sc, lane);
        if (lane == 63) { s_wave[0][wave] = ib; s_wave[1][wave] = ic; }
        __syncthreads();
        long long atB = runB + ib - sb, atP = runP + ic - sc, allB = 0, allP = 0;
        for (int w = 0; w < SCAN_THREADS / 64; ++w) {
            if (w < wave) { atB += s_wave[0][w]; atP += s_wave[1][w]; }
            allB += s_wave[0][w]; allP += s_wave[1][w];
        }
        for (int k = 0; k < SCAN_ITEMS; ++k) {
            if (i0 + k >= n) break;
            atB += b[k]; atP += c[k];
            if (atB > o.cap_bases || atP > capPairs) {                  // (offsets past a capacity are clamped: they stay valid numbers)
                atomicMin(&s_first, (int)(i0 + k));
                if (atB > o.cap_bases) atB = o.cap_bases;
                if (atP > capPairs) atP = capPairs;
            }
            o.read_off[i0 + k + 1] = atB; o.cig_off[i0 + k + 1] = (int32_t)atP;
        }
        runB += allB; runP += allP;
        __syncthreads();                                                // (s_wave is rewritten by the next tile)
    }
    const bool fits = s_first == INT32_MAX;
    if (fits && tid < PLAT_BLOB_PAD) { o.seq[runB + tid] = 0; o.qual[runB + tid] = 0; }
    if (tid == 0) {
        const unsigned long long key = (unsigned long long)o.status[1];
        long long err = 0, who = -1;
        if (key != BAM_NO_ERROR) { err = -(long long)(key & 0xffull); who = (long long)(key >> 8); }
        else if (!fits) { err = PLAT_ERR_OVERFLOW; who = s_first; }
        o.status[0] = err; o.status[1] = who; o.status[2] = runB; o.status[3] = runP;
    }
}

// n bytes (1..16) at p as four dwords, from the aligned dwords that cover them (a dword is loaded only when it holds one of the bytes)
__device__ __forceinline__ void ld_bytes16(const uint8_t* p, int n, uint32_t out[4]) {
    const uintptr_t a = (uintptr_t)p;
    const uint32_t* w = (const uint32_t*)(a & ~(uintptr_t)3);
    const uint32_t sh = (uint32_t)(a & 3);
    const int nd = (int)(sh + (uint32_t)n + 3) >> 2;                    // 1..5
    uint32_t v[5];
    for (int k = 0; k < 5; ++k) v[k] = k < nd ? w[k] : 0u;
    for (int k = 0; k < 4; ++k) out[k] = __builtin_amdgcn_alignbyte(v[k + 1], v[k], sh);
}

// four 4-bit codes (bits 0..15 of x, first code lowest) to four letters of "=ACMGRSVTWYHKDBN" (first letter lowest byte)
__device__ __forceinline__ uint32_t bam_letters4(uint32_t x) {
    uint32_t c = (x | (x << 8)) & 0x00ff00ffu;
    c = (c | (c << 4)) & 0x0f0f0f0fu;                                   // one code per byte
    const uint32_t sel = c & 0x07070707u;
    const uint32_t lo = __builtin_amdgcn_perm(0x56535247u, 0x4d43413du, sel);       // "=ACM" "GRSV"
    const uint32_t hi = __builtin_amdgcn_perm(0x4e42444bu, 0x48595754u, sel);       // "TWYH" "KDBN"
    const uint32_t m = ((c >> 3) & 0x01010101u) * 0xffu;
    return (lo & ~m) | (hi & m);
}

__global__ void __launch_bounds__(256)
k_bam_expand(int n, const uint8_t* __restrict__ blob, const int64_t* __restrict__ rec_off, plat_bam_decode_out o)
{
    const long long gid = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    const int r = (int)(gid >> 4), sub = (int)(gid & 15);
    if (r >= n || o.status[0] == PLAT_ERR_OVERFLOW) return;
    const long long d0 = o.read_off[r], len = o.read_off[r + 1] - d0;
    const long long c0 = o.cig_off[r], nc = o.cig_off[r + 1] - c0;
    if (len <= 0 || d0 < 0 || d0 + len > o.cap_bases || nc < 0 || c0 < 0 || c0 + nc > o.cap_pairs) return;        // (a refused record)
    const uint8_t* p = blob + rec_off[r];
    const uint8_t* cig = p + 32 + p[8];
    const uint8_t* seq = cig + 4 * nc;
    const uint8_t* qual = seq + (len + 1) / 2;
    for (long long k = sub; k < nc; k += 16) {
        const uint32_t w = ld_u32(cig + 4 * k);
        o.cigar[2 * (c0 + k)] = (int16_t)(w & 15u); o.cigar[2 * (c0 + k) + 1] = (int16_t)(w >> 4);
    }
    const long long w0 = d0 & ~15ll, nWin = ((d0 + len + 15) >> 4) - (d0 >> 4);
    for (long long w = sub; w < nWin; w += 16) {
        const long long ws = w0 + 16 * w;
        const long long lo = ws > d0 ? ws : d0, hi = ws + 16 < d0 + len ? ws + 16 : d0 + len;
        const long long j = lo - d0;                                    // first base of the window
        const int nb = (int)(hi - lo);
        uint32_t q[4], s[4], l[4];
        ld_bytes16(qual + j, nb, q);
        ld_bytes16(seq + (j >> 1), (int)(((j & 1) + nb + 1) >> 1), s);
        // high nibble first -> nibble k = code k; then drop the odd base in front
        for (int k = 0; k < 3; ++k) s[k] = ((s[k] & 0x0f0f0f0fu) << 4) | ((s[k] >> 4) & 0x0f0f0f0fu);
        unsigned long long codes = (unsigned long long)s[0] | ((unsigned long long)s[1] << 32);
        if (j & 1) codes = (codes >> 4) | ((unsigned long long)s[2] << 60);
        for (int k = 0; k < 4; ++k) l[k] = bam_letters4((uint32_t)(codes >> (16 * k)) & 0xffffu);
        if (nb == 16) {
            *(uint4*)(o.seq + ws) = make_uint4(l[0], l[1], l[2], l[3]);
            *(uint4*)(o.qual + ws) = make_uint4(q[0], q[1], q[2], q[3]);
        } else {
            for (int t = 0; t < 16; ++t) {
                if (t < nb) {
                    o.seq[lo + t] = (uint8_t)(l[t >> 2] >> (8 * (t & 3)));
                    o.qual[lo + t] = (uint8_t)(q[t >> 2] >> (8 * (t & 3)));
                }
            }
        }
    }
}
}  // namespace plat

PLAT_EXPORT int plat_bam_decode_batch(plat_ctx* ctx, int n_records, const uint8_t* blob, int64_t blob_len, const int64_t* rec_off,
                                      const int64_t* rec_limit, const plat_bam_decode_out* out, void* stream)
{
    if (!ctx || !out || n_records < 0 || blob_len < 0 || out->cap_bases < 0 || out->cap_pairs < 0) return PLAT_ERR_INVALID;
    const plat_bam_decode_out& o = *out;
    if (!o.status || !o.read_off || !o.cig_off || !o.seq || !o.qual) return PLAT_ERR_INVALID;
    if (((uintptr_t)o.seq | (uintptr_t)o.qual) & 15) return PLAT_ERR_INVALID;
    if (n_records > 0 && (!blob || !rec_off || !o.cigar || !o.pos || !o.end || !o.mapq || !o.flags || !o.chrom_id || !o.mate_chrom_id ||
                          !o.insert_size || !o.mate_pos))
        return PLAT_ERR_INVALID;
    if (n_records > (INT32_MAX >> 4)) return PLAT_ERR_OVERFLOW;         // (the expansion's grid: 16 lanes per record)
    PLAT_HIP(ctx, hipSetDevice(ctx->device));
    const hipStream_t st = (hipStream_t)stream;
    PLAT_HIP(ctx, hipMemsetAsync(o.status, 0xff, 4 * sizeof(int64_t), st));
    if (n_records == 0) PLAT_HIP(ctx, hipMemsetAsync(o.read_off, 0, sizeof(int64_t), st));
    if (n_records == 0) PLAT_HIP(ctx, hipMemsetAsync(o.cig_off, 0, sizeof(int32_t), st));
    if (n_records > 0)
        PLAT_LAUNCH(ctx, PLAT_KT_OTHER, st, plat::k_bam_core, dim3((unsigned)((n_records + 255) / 256)), dim3(256), 0, n_records, blob, (long long)blob_len, rec_off, rec_limit, o);
    PLAT_LAUNCH(ctx, PLAT_KT_OTHER, st, plat::k_bam_scan, dim3(1), dim3(plat::SCAN_THREADS), 0, n_records, o);
    if (n_records > 0)
        PLAT_LAUNCH(ctx, PLAT_KT_OTHER, st, plat::k_bam_expand, dim3((unsigned)(((long long)n_records * 16 + 255) / 256)), dim3(256), 0, n_records, blob, rec_off, o);
    PLAT_HIP(ctx, hipGetLastError());
    return PLAT_OK;
}
