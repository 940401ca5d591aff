// The host twin of plat_bgzf_deflate_batch (csrc/bgzf_deflate.hpp) and the host build of the inflate side (csrc/bgzf_inflate.hpp) as a
// stand-alone program for tests/test_bgzf_deflate_cpu.py: built with -fsanitize=address,undefined where that links.
//   driver IN OUT
// IN:  u32 cases; per case  i32 level, i32 n_pieces, i64 text_len, the text, i64 piece_off[n_pieces + 1]
// OUT: the 28 bytes of the EOF block; per case  i64 out_len, the bytes, i64 piece_out_off[n_pieces + 1], i64 blocks,
//      i64 blocks that bgzf::inflate_block accepts and inflates to their payload
// Exit status 2: a malformed IN; 3: deflate_block wrote behind what it returned.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <memory>
#include <vector>

#include "bgzf_deflate.hpp"

static bool get(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }
static void put(FILE* f, const void* p, size_t n) { if (n && fwrite(p, 1, n, f) != n) { fprintf(stderr, "short write\n"); exit(2); } }

int main(int argc, char** argv)
{
    if (argc != 3) { fprintf(stderr, "usage: driver IN OUT\n"); return 2; }
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) { fprintf(stderr, "cannot open the files\n"); return 2; }
    put(out, bgzf::EOF_BLOCK, sizeof bgzf::EOF_BLOCK);
    uint32_t cases = 0;
    if (!get(in, &cases, 4)) return 2;
    bgzf::Deflater d;
    std::unique_ptr<bgzf::Tables> tables(new bgzf::Tables);
    for (uint32_t k = 0; k < cases; ++k) {
        int32_t level = 0, n_pieces = 0;
        int64_t text_len = 0;
        if (!get(in, &level, 4) || !get(in, &n_pieces, 4) || !get(in, &text_len, 8) || n_pieces < 0 || text_len < 0) return 2;
        std::vector<uint8_t> text((size_t)text_len);
        std::vector<int64_t> off((size_t)n_pieces + 1), out_off((size_t)n_pieces + 1);
        if (!get(in, text.data(), text.size()) || !get(in, off.data(), off.size() * 8)) return 2;
        for (int32_t i = 0; i < n_pieces; ++i) if (off[(size_t)i] < 0 || off[(size_t)i + 1] < off[(size_t)i] || off[(size_t)i + 1] > text_len) return 2;
        std::vector<uint8_t> z;
        const int64_t blocks = bgzf::deflate_pieces(d, text.data(), off.data(), n_pieces, level, z, out_off.data());
        // one block alone in an exact buffer with a guard band: nothing is written behind the length it returns
        if (n_pieces > 0 && off[1] > 0) {
            const uint32_t n = (uint32_t)(off[1] < (int64_t)bgzf::DEFLATE_PAYLOAD ? off[1] : (int64_t)bgzf::DEFLATE_PAYLOAD);
            std::vector<uint8_t> one((size_t)n + bgzf::BLOCK_OVERHEAD + 64, 0xee);
            const uint32_t len = bgzf::deflate_block(text.data(), n, level, one.data());
            if (len > n + bgzf::BLOCK_OVERHEAD) return 3;
            for (size_t j = (size_t)n + bgzf::BLOCK_OVERHEAD; j < one.size(); ++j) if (one[j] != 0xee) return 3;
            if (memcmp(one.data(), z.data(), len) != 0) return 3;
        }
        // every block through the inflate side
        int64_t accepted = 0, at = 0, text_at = 0;
        std::vector<uint8_t> back(bgzf::MAX_ISIZE);
        while (at < (int64_t)z.size()) {
            bgzf::BlockHead h;
            if (bgzf::parse_header(z.data(), (int64_t)z.size(), at, &h) != 0) break;
            const int64_t got = bgzf::inflate_block(z.data(), (int64_t)z.size(), at, back.data(), (int64_t)back.size(), *tables, d.crcTable);
            if (got == (int64_t)h.isize && text_at + got <= text_len && memcmp(back.data(), text.data() + text_at, (size_t)got) == 0) ++accepted;
            text_at += h.isize;
            at = h.payload + h.payload_len + 8;
        }
        const int64_t out_len = (int64_t)z.size();
        put(out, &out_len, 8); put(out, z.data(), z.size()); put(out, out_off.data(), out_off.size() * 8); put(out, &blocks, 8); put(out, &accepted, 8);
    }
    fclose(in);
    if (fclose(out) != 0) return 2;
    return 0;
}
