// The host build of platypus_amd/csrc/bgzf_inflate.hpp for tests/test_bgzf_cpu.py: the scalar driver over a file of cases, every output
// buffer allocated at exactly its size (the sanitizers see the first byte outside) between two guard bands that are checked here too.
//   bgzf_host_driver inflate CASES OUT    cases: u32 n, then per case u32 len + the block's bytes (one block, at offset 0)
//                                         out:   per case i64 rc (ISIZE or -9), then rc bytes
//   bgzf_host_driver walk CASES OUT       cases: u32 n, then per case u32 len + a BGZF stream, i32 first_uoffset, i32 stop_blk, i32 stop_uoffset,
//                                                i32 tid, i32 beg, i32 end
//                                         out:   per case i64 rc (0, -9 for the walk, -19 for a block), i64 kept, i64 walked, kept x i64 offsets
// Exit status 0; 3 when a guard band was written; 2 for a malformed case file.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "bgzf_inflate.hpp"

static const int GUARD = 64;
static uint32_t g_crc[256];

struct Checked {                                          // a byte accessor that refuses to leave its buffer
    const uint8_t* p; int64_t n;
    uint8_t operator[](int64_t at) const { if (at < 0 || at >= n) { fprintf(stderr, "walk read outside the stream: %lld of %lld\n", (long long)at, (long long)n); abort(); } return p[at]; }
};

static bool read_all(const char* path, std::vector<uint8_t>& v) {
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    fseek(f, 0, SEEK_END); const long n = ftell(f); fseek(f, 0, SEEK_SET);
    v.resize((size_t)n);
    const bool ok = n == 0 || fread(v.data(), 1, (size_t)n, f) == (size_t)n;
    fclose(f);
    return ok;
}

// The commands executed in the DEVICE's order (k_bgzf_inflate): per batch of 64 first every literal, then every match in turn, a match in
// strips of 64 bytes whose sources are all read before any of the strip is written (one vector load, one vector store).  Must give the
// bytes the scalar order gives.
static bool wave_order_matches(const uint8_t* in, int64_t len, const bgzf::BlockHead& h, const uint8_t* want) {
    std::vector<uint8_t> win(bgzf::MAX_ISIZE, 0);
    bgzf::Tables* t = new bgzf::Tables;
    bgzf::Inflate s;
    bgzf::inflate_begin(s, in + h.payload, h.payload_len, h.isize);
    uint64_t cmds[64];
    bool ok = true;
    while (ok && s.phase != bgzf::DONE) {
        const int n = bgzf::inflate_step(s, *t, cmds, 64);
        if (n < 0) { ok = false; break; }
        for (int i = 0; i < n; ++i) if (!bgzf::cmd_len(cmds[i])) win[bgzf::cmd_dst(cmds[i])] = (uint8_t)bgzf::cmd_low(cmds[i]);
        for (int i = 0; i < n; ++i) {
            const uint32_t l = bgzf::cmd_len(cmds[i]), dst = bgzf::cmd_dst(cmds[i]), dist = bgzf::cmd_low(cmds[i]) + 1;
            for (uint32_t k0 = 0; k0 < l; k0 += 64) {
                uint8_t strip[64];
                for (uint32_t k = k0; k < l && k < k0 + 64; ++k) strip[k - k0] = win[dst - dist + (dist >= l ? k : k % dist)];
                for (uint32_t k = k0; k < l && k < k0 + 64; ++k) win[dst + k] = strip[k - k0];
            }
        }
    }
    delete t;
    (void)len;
    return ok && s.out == h.isize && memcmp(win.data(), want, h.isize) == 0;
}

// one block into a fresh buffer of exactly ISIZE bytes (from a copy of the block of exactly its length); -9, or ISIZE
static int64_t inflate_one(const uint8_t* blk, int64_t len, std::vector<uint8_t>& out, bool* guard_hit) {
    uint8_t* in = (uint8_t*)malloc(len ? (size_t)len : 1);   // (an exact-size copy: a read past the block is a read past the allocation)
    if (len) memcpy(in, blk, (size_t)len);
    bgzf::BlockHead h;
    int64_t rc = bgzf::ERR_BAD_INPUT;
    out.clear();
    if (bgzf::parse_header(in, len, 0, &h) == 0) {
        uint8_t* buf = (uint8_t*)malloc((size_t)h.isize + 2 * GUARD);
        memset(buf, 0xEE, (size_t)h.isize + 2 * GUARD);
        bgzf::Tables* t = new bgzf::Tables;
        rc = bgzf::inflate_block(in, len, 0, buf + GUARD, h.isize, *t, g_crc);
        delete t;
        for (int k = 0; k < GUARD; ++k) if (buf[k] != 0xEE || buf[GUARD + h.isize + k] != 0xEE) *guard_hit = true;
        if (rc >= 0) out.assign(buf + GUARD, buf + GUARD + rc);
        if (rc >= 0 && !wave_order_matches(in, len, h, buf + GUARD)) { fprintf(stderr, "the device's order of execution gives other bytes\n"); abort(); }
        free(buf);
    }
    free(in);
    return rc;
}

int main(int argc, char** argv)
{
    if (argc != 4) return 2;
    for (uint32_t i = 0; i < 256; ++i) g_crc[i] = bgzf::crc_table_entry(i);
    std::vector<uint8_t> cases;
    if (!read_all(argv[2], cases)) return 2;
    FILE* fo = fopen(argv[3], "wb");
    if (!fo) return 2;
    size_t at = 0;
    auto u32 = [&]() -> uint32_t { if (at + 4 > cases.size()) exit(2); uint32_t v; memcpy(&v, &cases[at], 4); at += 4; return v; };
    const uint32_t n = u32();
    bool guard_hit = false;
    const bool walk = strcmp(argv[1], "walk") == 0;
    for (uint32_t c = 0; c < n; ++c) {
        const uint32_t len = u32();
        if (at + len > cases.size()) return 2;
        const uint8_t* blob = cases.data() + at;
        at += len;
        std::vector<uint8_t> out;
        if (!walk) {
            const int64_t rc = inflate_one(blob, len, out, &guard_hit);
            fwrite(&rc, 8, 1, fo);
            if (rc > 0) fwrite(out.data(), 1, (size_t)rc, fo);
            continue;
        }
        const int32_t first = (int32_t)u32(), stop_blk = (int32_t)u32(), stop_uoff = (int32_t)u32(), tid = (int32_t)u32(), beg = (int32_t)u32(), end = (int32_t)u32();
        // the BSIZE chain, every block inflated behind the one before
        std::vector<uint8_t> data;
        std::vector<int64_t> out_off(1, 0);
        int64_t rc = 0;
        for (int64_t off = 0; off < (int64_t)len && rc == 0;) {
            bgzf::BlockHead h;
            if (bgzf::parse_header(blob, len, off, &h) != 0) { rc = -19; break; }
            const int64_t total = h.payload + h.payload_len + 8 - off;
            if (inflate_one(blob + off, total, out, &guard_hit) < 0) { rc = -19; break; }
            data.insert(data.end(), out.begin(), out.end());
            out_off.push_back((int64_t)data.size());
            off += total;
        }
        std::vector<int64_t> kept;
        int64_t walked = 0;
        if (rc == 0) {
            uint8_t* exact = (uint8_t*)malloc(data.size() ? data.size() : 1);
            if (!data.empty()) memcpy(exact, data.data(), data.size());
            const Checked m{exact, (int64_t)data.size()};
            const int64_t hi = (int64_t)data.size();
            const int64_t stop = stop_blk < 0 ? hi : out_off[(size_t)stop_blk] + stop_uoff;
            for (int64_t pos = first; pos < stop && pos < hi;) {
                int64_t next = pos; bool keep = false;
                const int r = bgzf::walk_step(m, pos, hi, tid, beg, end, &next, &keep);
                if (r == bgzf::WALK_STOP) break;
                if (r != bgzf::WALK_NEXT) { rc = r; break; }
                if (next <= pos) abort();                 // (every step moves forward)
                ++walked;
                if (keep) kept.push_back(pos + 4);
                pos = next;
            }
            free(exact);
        }
        const int64_t nk = (int64_t)kept.size();
        fwrite(&rc, 8, 1, fo); fwrite(&nk, 8, 1, fo); fwrite(&walked, 8, 1, fo);
        if (nk) fwrite(kept.data(), 8, (size_t)nk, fo);
    }
    fclose(fo);
    return guard_hit ? 3 : 0;
}
