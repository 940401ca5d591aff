// bgzf_inflate.hpp -- every part of plat_bgzf.hip that indexes memory from input data, as plain functions that compile for the host too:
// BGZF header parsing (RFC 1952 + SAM specification 4.1), the RFC 1951 decoder (code-length reading, table construction, symbol decode,
// the match-distance and output-length checks), the CRC32 pieces, and one step of the record walk (plat_bam_find_records).
//
// The decoder is a producer of COMMANDS: inflate_step() decodes up to `cap` symbols and writes one 64-bit command per literal or match,
// each with its destination offset inside the block's output.  A command is only produced after its checks passed (destination + length
// <= ISIZE, distance <= destination), so whoever executes them -- one lane after the other on the host (inflate_block below), the 64 lanes
// of a wave on the device -- writes inside [0, ISIZE) and reads inside what was written before.  Every loop consumes input bits or is
// bounded by a constant: no input can make it spin.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define BGZF_HD __host__ __device__ inline
#else
#define BGZF_HD inline
#endif

namespace bgzf {

constexpr int ERR_BAD_INPUT = -9;                         // PLAT_ERR_BAD_INPUT
constexpr uint32_t MAX_ISIZE = 65536;
constexpr int LBITS = 9, DBITS = 6;                       // primary table bits: literal/length, distance (and the code-length code)

BGZF_HD uint32_t ld16(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
BGZF_HD uint32_t ld32(const uint8_t* p) { return ld16(p) | (ld16(p + 2) << 16); }

// ---- the block header ------------------------------------------------------------------------------------------------------------
struct BlockHead {
    int64_t payload;                                      // offset of the deflate data in the blob
    int64_t payload_len;
    uint32_t crc, isize;
};

// blob_len: the end the block must not pass (the blob's, or the block's own limit when that is lower)
BGZF_HD int parse_header(const uint8_t* blob, int64_t blob_len, int64_t off, BlockHead* h)
{
    if (off < 0 || off > blob_len - 26) return ERR_BAD_INPUT;                      // 12 fixed bytes, the BC subfield (6) and the trailer (8)
    const uint8_t* p = blob + off;
    if (p[0] != 0x1f || p[1] != 0x8b || p[2] != 8 || p[3] != 4) return ERR_BAD_INPUT;
    const int64_t xlen = ld16(p + 10);
    if (off + 12 + xlen + 8 > blob_len) return ERR_BAD_INPUT;
    int64_t x = 0, bsize = -1;
    while (x + 4 <= xlen) {                                                         // (at most xlen / 4 rounds)
        const uint8_t* s = p + 12 + x;
        const int64_t slen = ld16(s + 2);
        if (x + 4 + slen > xlen) return ERR_BAD_INPUT;
        if (s[0] == 'B' && s[1] == 'C' && slen == 2 && bsize < 0) bsize = ld16(s + 4);
        x += 4 + slen;
    }
    if (x != xlen || bsize < 0) return ERR_BAD_INPUT;
    const int64_t total = bsize + 1;
    if (total < 12 + xlen + 8 || off + total > blob_len) return ERR_BAD_INPUT;
    h->payload = off + 12 + xlen;
    h->payload_len = total - 12 - xlen - 8;
    h->crc = ld32(p + total - 8);
    h->isize = ld32(p + total - 4);
    return h->isize > MAX_ISIZE ? ERR_BAD_INPUT : 0;
}

// ---- CRC32 (RFC 1952, reflected polynomial 0xedb88320) ---------------------------------------------------------------------------
BGZF_HD uint32_t crc_table_entry(uint32_t i) {
    for (int k = 0; k < 8; ++k) i = (i & 1u) ? (i >> 1) ^ 0xedb88320u : i >> 1;
    return i;
}
// a(x) * b(x) modulo the CRC polynomial; x^0 is bit 31
BGZF_HD uint32_t crc_mulmod(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (int k = 0; k < 32; ++k) {
        if (a & (0x80000000u >> k)) p ^= b;
        b = (b & 1u) ? (b >> 1) ^ 0xedb88320u : b >> 1;
    }
    return p;
}
// the CRC of A followed by n more bytes, from the CRC of A, is crc_shift(crc(A), n) ^ crc(those n bytes): x^(8n) by square and multiply
BGZF_HD uint32_t crc_shift(uint32_t crc, uint32_t n) {
    uint32_t f = 0x80000000u, sq = 0x00800000u;           // x^0, x^8
    for (int k = 0; k < 32 && n; ++k, n >>= 1) {
        if (n & 1u) f = crc_mulmod(sq, f);
        sq = crc_mulmod(sq, sq);
    }
    return crc_mulmod(f, crc);
}
BGZF_HD uint32_t crc_bytes(const uint32_t* table, const uint8_t* p, int64_t n) {
    uint32_t c = 0xffffffffu;
    for (int64_t i = 0; i < n; ++i) c = table[(c ^ p[i]) & 0xffu] ^ (c >> 8);
    return ~c;
}

// ---- RFC 1951 --------------------------------------------------------------------------------------------------------------------
struct Tables {                                           // one block's decode tables (LDS on the device: 2.2 KB)
    uint16_t lfast[1 << LBITS], dfast[1 << DBITS];        // (symbol << 4) | code length for the codes of up to LBITS / DBITS bits, else 0
    uint16_t lcount[16], dcount[16];                      // codes per length
    uint16_t lsym[288], dsym[32];                         // symbols in canonical order
    uint8_t lens[320];                                    // code lengths while they are read
};

struct Bits {
    const uint8_t* in;
    int64_t len, pos;                                     // bytes of input, next byte to load
    uint64_t buf;
    int n;                                                // valid bits in buf
};
BGZF_HD void refill(Bits& b) {
    while (b.n <= 56 && b.pos < b.len) { b.buf |= (uint64_t)b.in[b.pos++] << b.n; b.n += 8; }
}
// k bits (k <= 16), or -1 when the input has fewer left
BGZF_HD int take(Bits& b, int k) {
    if (b.n < k) { refill(b); if (b.n < k) return -1; }
    const int v = (int)(b.buf & ((1u << k) - 1u));
    b.buf >>= k; b.n -= k;
    return v;
}

// canonical Huffman tables from n code lengths.  0, or ERR_BAD_INPUT for an over-subscribed set or an incomplete one -- but for a single
// one-bit code where allowSingle says so (zlib's rule: the literal/length and distance sets may, the code-length set may not; a set
// without any code is valid: decoding a symbol from it fails)
BGZF_HD int build(const uint8_t* lens, int n, uint16_t* count, uint16_t* sym, uint16_t* fast, int fastBits, bool allowSingle)
{
    uint16_t offs[16], next[16];
    for (int l = 0; l < 16; ++l) count[l] = 0;
    for (int i = 0; i < n; ++i) ++count[lens[i] & 15];
    for (int i = 0; i < (1 << fastBits); ++i) fast[i] = 0;
    if (count[0] == n) return 0;
    int left = 1, maxLen = 0;
    for (int l = 1; l < 16; ++l) {
        left = (left << 1) - count[l];
        if (left < 0) return ERR_BAD_INPUT;
        if (count[l]) maxLen = l;
    }
    if (left > 0 && !(allowSingle && maxLen == 1)) return ERR_BAD_INPUT;
    offs[1] = 0; next[0] = next[1] = 0;
    for (int l = 1; l < 15; ++l) { offs[l + 1] = (uint16_t)(offs[l] + count[l]); next[l + 1] = (uint16_t)((next[l] + count[l]) << 1); }
    for (int i = 0; i < n; ++i) {
        const int l = lens[i] & 15;
        if (!l) continue;
        sym[offs[l]++] = (uint16_t)i;                     // (offs[l] < n: the lengths counted above)
        const uint32_t code = next[l]++;
        if (l <= fastBits) {
            uint32_t r = 0;
            for (int k = 0; k < l; ++k) r |= ((code >> k) & 1u) << (l - 1 - k);
            for (uint32_t at = r; at < (1u << fastBits); at += 1u << l) fast[at] = (uint16_t)((i << 4) | l);
        }
    }
    return 0;
}

// one symbol, or -1: no code matches or the input ends inside it
BGZF_HD int decode(Bits& b, const uint16_t* count, const uint16_t* sym, const uint16_t* fast, int fastBits)
{
    if (b.n < 15) refill(b);
    const uint32_t e = fast[b.buf & ((1u << fastBits) - 1u)];
    if (e) {
        const int l = (int)(e & 15u);
        if (l > b.n) return -1;
        b.buf >>= l; b.n -= l;
        return (int)(e >> 4);
    }
    int code = 0, first = 0, index = 0;
    const int have = b.n < 15 ? b.n : 15;
    for (int l = 1; l <= have; ++l) {                     // the canonical walk, a bit at a time, for the longer codes
        code |= (int)((b.buf >> (l - 1)) & 1u);
        const int c = count[l];
        if (code - c < first) { b.buf >>= l; b.n -= l; return sym[index + (code - first)]; }
        index += c; first = (first + c) << 1; code <<= 1;
    }
    return -1;
}

// a command: bits 0-15 the literal byte or distance - 1, bits 16-24 the match length (0: a literal), bits 32-47 the destination offset
BGZF_HD uint64_t cmd_literal(uint32_t dst, uint32_t byte) { return ((uint64_t)dst << 32) | byte; }
BGZF_HD uint64_t cmd_match(uint32_t dst, uint32_t len, uint32_t dist) { return ((uint64_t)dst << 32) | (len << 16) | (dist - 1u); }
BGZF_HD uint32_t cmd_dst(uint64_t c) { return (uint32_t)(c >> 32); }
BGZF_HD uint32_t cmd_len(uint64_t c) { return (uint32_t)(c >> 16) & 0x1ffu; }
BGZF_HD uint32_t cmd_low(uint64_t c) { return (uint32_t)c & 0xffffu; }

enum Phase { BLOCK_HEAD = 0, STORED = 1, CODED = 2, DONE = 3 };

struct Inflate {
    Bits b;
    uint32_t isize, out;                                  // output bytes the commands so far produce
    int phase, last;
    uint32_t stored_left;
};

BGZF_HD void inflate_begin(Inflate& s, const uint8_t* payload, int64_t payload_len, uint32_t isize) {
    s.b.in = payload; s.b.len = payload_len; s.b.pos = 0; s.b.buf = 0; s.b.n = 0;
    s.isize = isize; s.out = 0; s.phase = BLOCK_HEAD; s.last = 0; s.stored_left = 0;
}

BGZF_HD int read_block_head(Inflate& s, Tables& t)
{
    static const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    const int head = take(s.b, 3);
    if (head < 0) return ERR_BAD_INPUT;
    s.last = head & 1;
    const int type = head >> 1;
    if (type == 0) {
        const int drop = s.b.n & 7;                       // to the byte boundary: buf holds whole bytes behind the bits taken
        s.b.buf >>= drop; s.b.n -= drop;
        const int len = take(s.b, 16), nlen = take(s.b, 16);
        if (len < 0 || nlen < 0 || (len ^ 0xffff) != nlen) return ERR_BAD_INPUT;
        s.stored_left = (uint32_t)len;
        s.phase = STORED;
        return 0;
    }
    if (type == 3) return ERR_BAD_INPUT;
    int nl, nd;
    if (type == 1) {
        nl = 288; nd = 32;                                // (symbols 286 / 287 and 30 / 31 take part in the code and are refused when met)
        for (int i = 0; i < 288; ++i) t.lens[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8);
        for (int i = 0; i < 32; ++i) t.lens[288 + i] = 5;
    } else {
        const int hlit = take(s.b, 5), hdist = take(s.b, 5), hclen = take(s.b, 4);
        if (hlit < 0 || hdist < 0 || hclen < 0) return ERR_BAD_INPUT;
        nl = hlit + 257; nd = hdist + 1;
        if (nl > 286 || nd > 30) return ERR_BAD_INPUT;
        uint8_t cl[19];
        for (int i = 0; i < 19; ++i) cl[i] = 0;
        for (int i = 0; i < hclen + 4; ++i) {
            const int v = take(s.b, 3);
            if (v < 0) return ERR_BAD_INPUT;
            cl[order[i]] = (uint8_t)v;
        }
        if (build(cl, 19, t.dcount, t.dsym, t.dfast, DBITS, false) != 0) return ERR_BAD_INPUT;
        int at = 0;
        while (at < nl + nd) {                            // (every round reads a symbol: bounded by the input)
            const int sym = decode(s.b, t.dcount, t.dsym, t.dfast, DBITS);
            if (sym < 0) return ERR_BAD_INPUT;
            if (sym < 16) { t.lens[at++] = (uint8_t)sym; continue; }
            int rep, val = 0;
            if (sym == 16) {
                if (at == 0) return ERR_BAD_INPUT;        // nothing to repeat
                val = t.lens[at - 1];
                rep = take(s.b, 2); if (rep < 0) return ERR_BAD_INPUT; rep += 3;
            } else if (sym == 17) { rep = take(s.b, 3); if (rep < 0) return ERR_BAD_INPUT; rep += 3; }
            else { rep = take(s.b, 7); if (rep < 0) return ERR_BAD_INPUT; rep += 11; }
            if (at + rep > nl + nd) return ERR_BAD_INPUT; // more lengths than HLIT + HDIST
            while (rep--) t.lens[at++] = (uint8_t)val;
        }
        if (t.lens[256] == 0) return ERR_BAD_INPUT;       // no end-of-block code
    }
    if (build(t.lens, nl, t.lcount, t.lsym, t.lfast, LBITS, true) != 0) return ERR_BAD_INPUT;
    if (build(t.lens + nl, nd, t.dcount, t.dsym, t.dfast, DBITS, true) != 0) return ERR_BAD_INPUT;
    s.phase = CODED;
    return 0;
}

// Decode until `cap` commands are written or the last deflate block has ended (s.phase == DONE).  The number of commands written
// (0 .. cap), or ERR_BAD_INPUT.
BGZF_HD int inflate_step(Inflate& s, Tables& t, uint64_t* cmds, int cap)
{
    static const uint16_t lbase[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
    static const uint8_t lext[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
    static const uint16_t dbase[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
                                       12289, 16385, 24577};
    static const uint8_t dext[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
    int n = 0;
    while (n < cap && s.phase != DONE) {
        if (s.phase == BLOCK_HEAD) {
            if (read_block_head(s, t) != 0) return ERR_BAD_INPUT;
        } else if (s.phase == STORED) {
            if (s.stored_left == 0) { s.phase = s.last ? DONE : BLOCK_HEAD; continue; }
            const int v = take(s.b, 8);
            if (v < 0 || s.out >= s.isize) return ERR_BAD_INPUT;
            cmds[n++] = cmd_literal(s.out++, (uint32_t)v);
            --s.stored_left;
        } else {
            const int sym = decode(s.b, t.lcount, t.lsym, t.lfast, LBITS);
            if (sym < 0) return ERR_BAD_INPUT;
            if (sym < 256) {
                if (s.out >= s.isize) return ERR_BAD_INPUT;
                cmds[n++] = cmd_literal(s.out++, (uint32_t)sym);
            } else if (sym == 256) {
                s.phase = s.last ? DONE : BLOCK_HEAD;
            } else {
                if (sym > 285) return ERR_BAD_INPUT;
                const int le = take(s.b, lext[sym - 257]);
                if (le < 0) return ERR_BAD_INPUT;
                const uint32_t len = (uint32_t)lbase[sym - 257] + (uint32_t)le;
                const int ds = decode(s.b, t.dcount, t.dsym, t.dfast, DBITS);
                if (ds < 0 || ds > 29) return ERR_BAD_INPUT;
                const int de = take(s.b, dext[ds]);
                if (de < 0) return ERR_BAD_INPUT;
                const uint32_t dist = (uint32_t)dbase[ds] + (uint32_t)de;
                if (dist > s.out || len > s.isize - s.out) return ERR_BAD_INPUT;    // before the block's output / more than ISIZE
                cmds[n++] = cmd_match(s.out, len, dist);
                s.out += len;
            }
        }
    }
    return n;
}

// The scalar driver (the host build's, and the meaning of the commands): inflate one BGZF block at blob[off] into out[0 .. ISIZE) and
// check its CRC32 -- in 64 slices combined with crc_shift, as the device's lanes do.  Returns ISIZE or ERR_BAD_INPUT; out must hold
// out_cap >= ISIZE bytes (else ERR_BAD_INPUT: the caller sized it from the header).
inline int64_t inflate_block(const uint8_t* blob, int64_t blob_len, int64_t off, uint8_t* out, int64_t out_cap, Tables& t, const uint32_t* crcTable)
{
    BlockHead h;
    if (parse_header(blob, blob_len, off, &h) != 0 || (int64_t)h.isize > out_cap) return ERR_BAD_INPUT;
    Inflate s;
    inflate_begin(s, blob + h.payload, h.payload_len, h.isize);
    uint64_t cmds[64];
    while (s.phase != DONE) {
        const int n = inflate_step(s, t, cmds, 64);
        if (n < 0) return ERR_BAD_INPUT;
        for (int i = 0; i < n; ++i) {
            const uint32_t dst = cmd_dst(cmds[i]), len = cmd_len(cmds[i]), low = cmd_low(cmds[i]);
            if (!len) out[dst] = (uint8_t)low;
            else for (uint32_t k = 0; k < len; ++k) out[dst + k] = out[dst + k - (low + 1)];
        }
    }
    if (s.out != h.isize) return ERR_BAD_INPUT;
    const uint32_t per = (h.isize + 63) / 64;
    uint32_t crc = 0;
    for (uint32_t lane = 0; lane < 64; ++lane) {
        const uint32_t a = lane * per < h.isize ? lane * per : h.isize, b = a + per < h.isize ? a + per : h.isize;
        crc ^= crc_shift(crc_bytes(crcTable, out + a, b - a), h.isize - b);
    }
    return crc == h.crc ? (int64_t)h.isize : ERR_BAD_INPUT;
}

// ---- the record walk (plat_bam_find_records) ---------------------------------------------------------------------------------------
// One step of the rule at offset pos of a stream that ends at hi; `m[k]` is byte k of the inflated data.  The caller has checked
// pos < hi and pos < stop.  Returns WALK_NEXT (continue at *next; *keep says whether the record at pos + 4 is kept), WALK_STOP or
// ERR_BAD_INPUT.  walk_need(): how many bytes from pos on a step reads, once the 36 first are at hand.
enum { WALK_NEXT = 0, WALK_STOP = 1 };

template <class Bytes> BGZF_HD uint32_t walk_ld32(const Bytes& m, int64_t at) {
    return (uint32_t)m[at] | ((uint32_t)m[at + 1] << 8) | ((uint32_t)m[at + 2] << 16) | ((uint32_t)m[at + 3] << 24);
}

template <class Bytes> BGZF_HD int64_t walk_need(const Bytes& m, int64_t pos) {
    return 36 + (int64_t)m[pos + 12] + 4 * (int64_t)(walk_ld32(m, pos + 16) & 0xffffu);
}

template <class Bytes>
BGZF_HD int walk_step(const Bytes& m, int64_t pos, int64_t hi, int32_t tid, int32_t beg, int32_t end, int64_t* next, bool* keep)
{
    *keep = false;
    if (hi - pos < 4) return ERR_BAD_INPUT;
    const int64_t blockSize = (int32_t)walk_ld32(m, pos);
    if (blockSize < 32 || blockSize > hi - pos - 4) return ERR_BAD_INPUT;
    const int32_t t = (int32_t)walk_ld32(m, pos + 4), b = (int32_t)walk_ld32(m, pos + 8);
    if (t != tid || b >= end) return WALK_STOP;
    const int64_t nCig = walk_ld32(m, pos + 16) & 0xffffu, cigAt = pos + 36 + (int64_t)m[pos + 12];
    if (cigAt + 4 * nCig > pos + 4 + blockSize) return ERR_BAD_INPUT;             // (the CIGAR lies inside the record)
    int64_t refLen = nCig ? 0 : 1;
    for (int64_t k = 0; k < nCig; ++k) {
        const uint32_t w = walk_ld32(m, cigAt + 4 * k), op = w & 15u;
        if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) refLen += w >> 4;
    }
    *keep = (int64_t)b + refLen > (int64_t)beg && end > b;
    *next = pos + 4 + blockSize;
    return WALK_NEXT;
}

}  // namespace bgzf
