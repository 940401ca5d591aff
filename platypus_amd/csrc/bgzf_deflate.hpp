// bgzf_deflate.hpp -- the encoding rule of plat_bgzf_deflate_batch (include/platypus_mi355x.h has it in words), written from RFC 1951,
// RFC 1952 and SAM specification 4.1 as the inflate side was (bgzf_inflate.hpp).  Two parts:
//   what the device compiles too (BGZF_HD): the hash, the fixed-Huffman code of a literal and of a (length, distance) pair, the token word,
//   the block header and trailer;
//   the rule restated serially for the host (deflate_block, deflate_pieces): the twin of plat_bgzfout.hip, byte for byte.  The caller
//   library runs it under PLAT_CALLER_HOST_DEFLATE=1 (host/bgzf_out.hpp) and tests/bgzf_deflate_host_driver.cpp builds it alone.
// A block is never longer than MAX_BLOCK_BYTES: data that fixed Huffman codes would make n + 5 bytes or longer is stored.
#pragma once
#include <stdint.h>
#include "bgzf_inflate.hpp"
#if !defined(__HIP_DEVICE_COMPILE__)
#include <string.h>
#include <algorithm>
#include <vector>
#endif

namespace bgzf {

constexpr uint32_t DEFLATE_PAYLOAD = 0xff00;              // payload bytes of a full block
constexpr int DEFLATE_HASH_BITS = 15;
constexpr uint32_t DEFLATE_MIN_MATCH = 4, DEFLATE_MAX_MATCH = 258, DEFLATE_MAX_DIST = 32768;
constexpr uint32_t BLOCK_HEADER_BYTES = 18, BLOCK_TRAILER_BYTES = 8;
constexpr uint32_t BLOCK_OVERHEAD = BLOCK_HEADER_BYTES + 5 + BLOCK_TRAILER_BYTES;         // 31: what a stored block adds to its payload
constexpr uint32_t MAX_BLOCK_BYTES = DEFLATE_PAYLOAD + BLOCK_OVERHEAD;

BGZF_HD uint32_t deflate_hash(uint32_t le32) { return (le32 * 2654435761u) >> (32 - DEFLATE_HASH_BITS); }

// the low n bits of v in reverse order (Huffman codes go into the stream from their most significant bit)
BGZF_HD uint32_t rev_bits(uint32_t v, int n) {
    v = ((v >> 1) & 0x55555555u) | ((v & 0x55555555u) << 1);
    v = ((v >> 2) & 0x33333333u) | ((v & 0x33333333u) << 2);
    v = ((v >> 4) & 0x0f0f0f0fu) | ((v & 0x0f0f0f0fu) << 4);
    v = ((v >> 8) & 0x00ff00ffu) | ((v & 0x00ff00ffu) << 8);
    v = (v >> 16) | (v << 16);
    return v >> (32 - n);
}
BGZF_HD int floor_log2(uint32_t v) { return 31 - __builtin_clz(v); }                     // (v >= 1)

// RFC 1951 3.2.6: the fixed code of literal/length symbol s (0 .. 287), as the bits to put into the stream (least significant first)
BGZF_HD uint32_t fixed_code(uint32_t s, int* n) {
    if (s < 144) { *n = 8; return rev_bits(0x30u + s, 8); }
    if (s < 256) { *n = 9; return rev_bits(0x190u + (s - 144u), 9); }
    if (s < 280) { *n = 7; return rev_bits(s - 256u, 7); }
    *n = 8; return rev_bits(0xc0u + (s - 280u), 8);
}
// ... of a match: the length symbol, its extra bits, the 5-bit distance symbol, its extra bits (RFC 1951 3.2.5); at most 31 bits.
// len 3 .. 258, dist 1 .. 32768
BGZF_HD uint32_t match_code(uint32_t len, uint32_t dist, int* n) {
    uint32_t li, le = 0, lx = 0;
    const uint32_t l = len - 3u;
    if (len == 258u) li = 28;
    else if (l < 8u) li = l;
    else { le = (uint32_t)floor_log2(l) - 2u; li = 4u * le + 4u + ((l >> le) & 3u); lx = l & ((1u << le) - 1u); }
    uint32_t di, de = 0, dx = 0;
    const uint32_t d = dist - 1u;
    if (d < 4u) di = d;
    else { const uint32_t nb = (uint32_t)floor_log2(d); de = nb - 1u; di = 2u * nb + ((d >> de) & 1u); dx = d & ((1u << de) - 1u); }
    int at = 0;
    uint32_t v = fixed_code(257u + li, &at);
    v |= lx << at; at += (int)le;
    v |= rev_bits(di, 5) << at; at += 5;
    v |= dx << at; at += (int)de;
    *n = at;
    return v;
}

// a token: bits 0-8 the match length (0: a literal), bits 9-16 the byte at its position, bits 17-31 the distance - 1
BGZF_HD uint32_t token_word(uint32_t len, uint32_t byte, uint32_t dist) { return len | (byte << 9) | (len ? (dist - 1u) << 17 : 0u); }
BGZF_HD uint32_t token_len(uint32_t t) { return t & 0x1ffu; }
BGZF_HD uint32_t token_code(uint32_t t, int* n) {
    return token_len(t) ? match_code(token_len(t), (t >> 17) + 1u, n) : fixed_code((t >> 9) & 0xffu, n);
}
// bytes of the deflate data of a block whose tokens take token_bits bits: the 3 header bits, the tokens, end-of-block (7 bits), padding
BGZF_HD uint32_t coded_bytes(uint64_t token_bits) { return (uint32_t)((3u + token_bits + 7u + 7u) >> 3); }

// byte k of the header of a block of block_len bytes (k < 18), and of its trailer (k < 8)
BGZF_HD uint8_t header_byte(uint32_t k, uint32_t block_len) {
    const uint32_t bsize = block_len - 1u;
    switch (k) {
    case 0: return 0x1f; case 1: return 0x8b; case 2: return 8; case 3: return 4;
    case 9: return 0xff; case 10: return 6; case 12: return 'B'; case 13: return 'C'; case 14: return 2;
    case 16: return (uint8_t)(bsize & 0xffu); case 17: return (uint8_t)(bsize >> 8);
    default: return 0;                                    // MTIME, XFL, the high bytes of XLEN and SLEN
    }
}
BGZF_HD uint8_t trailer_byte(uint32_t k, uint32_t crc, uint32_t isize) { return (uint8_t)((k < 4 ? crc >> (8u * k) : isize >> (8u * (k - 4u))) & 0xffu); }

#if !defined(__HIP_DEVICE_COMPILE__)
// the EOF marker of SAM specification 4.1.2: an empty fixed-Huffman block
static const uint8_t EOF_BLOCK[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};

struct Deflater {                                         // the tables of the serial twin, reused from block to block
    std::vector<uint16_t> head;                           // per hash the last inserted position + 1
    std::vector<uint32_t> tokens;
    uint32_t crcTable[256];
    Deflater() : head((size_t)1 << DEFLATE_HASH_BITS) { for (uint32_t i = 0; i < 256; ++i) crcTable[i] = crc_table_entry(i); }
};

inline void write_frame(uint8_t* out, uint32_t block_len, uint32_t crc, uint32_t isize) {
    for (uint32_t k = 0; k < BLOCK_HEADER_BYTES; ++k) out[k] = header_byte(k, block_len);
    for (uint32_t k = 0; k < BLOCK_TRAILER_BYTES; ++k) out[block_len - BLOCK_TRAILER_BYTES + k] = trailer_byte(k, crc, isize);
}

// One block: in[0 .. n), 1 <= n <= DEFLATE_PAYLOAD, to out (room for n + BLOCK_OVERHEAD bytes).  Returns the block's length.
inline uint32_t deflate_block(Deflater& d, const uint8_t* in, uint32_t n, int level, uint8_t* out)
{
    uint64_t bits = 0;
    d.tokens.clear();
    if (level > 0) {
        std::fill(d.head.begin(), d.head.end(), (uint16_t)0);
        uint32_t inserted = 0;                            // positions < inserted are in the table
        for (uint32_t p = 0; p < n;) {
            for (; inserted < p; ++inserted) if (inserted + 4u <= n) d.head[deflate_hash(ld32(in + inserted))] = (uint16_t)(inserted + 1u);
            uint32_t len = 0, dist = 0;
            if (p + 4u <= n) {
                const uint32_t c = d.head[deflate_hash(ld32(in + p))];
                if (c && p - (c - 1u) <= DEFLATE_MAX_DIST) {
                    const uint32_t q = c - 1u, cap = n - p < DEFLATE_MAX_MATCH ? n - p : DEFLATE_MAX_MATCH;
                    while (len < cap && in[q + len] == in[p + len]) ++len;
                    if (len < DEFLATE_MIN_MATCH) len = 0;
                    dist = p - q;
                }
            }
            const uint32_t t = token_word(len, in[p], dist);
            int nb;
            token_code(t, &nb);
            bits += (uint64_t)nb;
            d.tokens.push_back(t);
            p += len ? len : 1u;
        }
    }
    const bool stored = level <= 0 || coded_bytes(bits) >= n + 5u;
    const uint32_t body = stored ? n + 5u : coded_bytes(bits);
    const uint32_t block_len = BLOCK_HEADER_BYTES + body + BLOCK_TRAILER_BYTES;
    uint8_t* z = out + BLOCK_HEADER_BYTES;
    if (stored) {
        z[0] = 1; z[1] = (uint8_t)(n & 0xffu); z[2] = (uint8_t)(n >> 8); z[3] = (uint8_t)(~n & 0xffu); z[4] = (uint8_t)((~n >> 8) & 0xffu);
        memcpy(z + 5, in, n);
    } else {
        uint64_t acc = 3;                                 // BFINAL 1, BTYPE 01
        int have = 3;
        uint32_t at = 0;
        auto put = [&](uint32_t v, int nb) {
            acc |= (uint64_t)v << have; have += nb;
            while (have >= 8) { z[at++] = (uint8_t)(acc & 0xffu); acc >>= 8; have -= 8; }
        };
        for (uint32_t t : d.tokens) { int nb; const uint32_t v = token_code(t, &nb); put(v, nb); }
        { int nb; const uint32_t v = fixed_code(256, &nb); put(v, nb); }
        if (have) z[at++] = (uint8_t)(acc & 0xffu);
    }
    write_frame(out, block_len, crc_bytes(d.crcTable, in, (int64_t)n), n);
    return block_len;
}
inline uint32_t deflate_block(const uint8_t* in, uint32_t n, int level, uint8_t* out) { Deflater d; return deflate_block(d, in, n, level, out); }

// The pieces text[piece_off[i] .. piece_off[i + 1]) of a text, each cut into blocks of DEFLATE_PAYLOAD bytes, appended to out;
// piece_out_off [n_pieces + 1] (may be null): where each piece's blocks begin in what was appended.  Returns the number of blocks.
inline int64_t deflate_pieces(Deflater& d, const uint8_t* text, const int64_t* piece_off, int64_t n_pieces, int level, std::vector<uint8_t>& out,
                              int64_t* piece_out_off)
{
    const size_t base = out.size();
    int64_t blocks = 0;
    for (int64_t i = 0; i < n_pieces; ++i) {
        if (piece_out_off) piece_out_off[i] = (int64_t)(out.size() - base);
        for (int64_t at = piece_off[i]; at < piece_off[i + 1]; at += DEFLATE_PAYLOAD, ++blocks) {
            const uint32_t n = (uint32_t)(piece_off[i + 1] - at < (int64_t)DEFLATE_PAYLOAD ? piece_off[i + 1] - at : (int64_t)DEFLATE_PAYLOAD);
            const size_t old = out.size();
            out.resize(old + n + BLOCK_OVERHEAD);
            out.resize(old + deflate_block(d, text + at, n, level, out.data() + old));
        }
    }
    if (piece_out_off) piece_out_off[n_pieces] = (int64_t)(out.size() - base);
    return blocks;
}
#endif

}  // namespace bgzf
