// The block list of the host's BGZF entry points (platypus_amd/csrc/host/bgzf_blocks.hpp over csrc/bgzf_inflate.hpp) alone, as a stand-alone
// program for tests/test_bgzf_blocks_cpu.py: built with -fsanitize=address,undefined where that links.  The walk parses bytes that come
// from outside the process; here it runs on them with every chunk allocated to the byte, so a read past a chunk is the sanitizer's to find.
//   driver IN        (the answers go to stdout)
// IN:  u32 n_cases; per case u32 data_len, data, i32 first_uoffset, i64 end_coffset, i32 end_uoffset, u32 refuse_empty
// OUT: per case a line "case K rc R", a line with the message (empty when there is none), and for rc 0 the tables, a line each:
//      "chunk blkFirst blkEnd firstU stopBlk stopU blobBytes inflated", "off ...", "limit ...", "inflated ...", "span first stop hi",
//      "inflate B" (the first block the host inflate refuses, or -1) with the message for B on the next line, and for -1 "data HEX".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#define PLAT_BGZF_BLOCKS_HOST_ONLY
#include "host/bgzf_blocks.hpp"

static std::vector<uint8_t> readAll(const char* path) {
    FILE* f = fopen(path, "rb");
    if (!f) { perror(path); exit(2); }
    std::vector<uint8_t> v;
    uint8_t buf[65536];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + n);
    fclose(f);
    return v;
}
struct In {
    const std::vector<uint8_t>& v; size_t at = 0;
    template <class T> T take() { T x; if (at + sizeof x > v.size()) { fprintf(stderr, "short input\n"); exit(2); } memcpy(&x, v.data() + at, sizeof x); at += sizeof x; return x; }
    const uint8_t* bytes(size_t n) { if (at + n > v.size()) { fprintf(stderr, "short input\n"); exit(2); } const uint8_t* p = v.data() + at; at += n; return p; }
};
static void row(const char* name, const std::vector<int64_t>& v) {
    printf("%s", name);
    for (int64_t x : v) printf(" %lld", (long long)x);
    printf("\n");
}

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: driver IN\n"); return 2; }
    const std::vector<uint8_t> raw = readAll(argv[1]);
    In in{raw};
    const uint32_t nCases = in.take<uint32_t>();
    for (uint32_t k = 0; k < nCases; ++k) {
        const uint32_t n = in.take<uint32_t>();
        const uint8_t* p = in.bytes(n);
        std::unique_ptr<uint8_t[]> data(n ? new uint8_t[n] : nullptr);                 // (to the byte; no bytes: a null pointer)
        if (n) memcpy(data.get(), p, n);
        plat_bgzf_chunk ch;
        memset(&ch, 0, sizeof ch);
        ch.data = data.get(); ch.data_len = n;
        ch.first_uoffset = in.take<int32_t>(); ch.end_coffset = in.take<int64_t>(); ch.end_uoffset = in.take<int32_t>();
        const bool refuseEmpty = in.take<uint32_t>() != 0;
        std::string error;
        plathost::BgzfBlockList L("driver", [](const plathost::BgzfChunkAt& a) { return "chunk " + std::to_string(a.chunk); }, refuseEmpty, error);
        const int rc = L.add(0, 0, 0, ch);
        printf("case %u rc %d\n%s\n", k, rc, error.c_str());
        if (rc != 0) continue;
        const plathost::BgzfChunkAt& a = L.chunkAt[0];
        printf("chunk %d %d %d %d %d %lld %lld\n", a.blkFirst, a.blkEnd, L.firstU[0], L.stopBlk[0], L.stopU[0], L.blobBytes, L.inflated);
        row("off", L.blkOff); row("limit", L.blkLimit); row("inflated", L.blkInflated);
        int64_t first, stop, hi;
        L.span(0, first, stop, hi);
        printf("span %lld %lld %lld\n", (long long)first, (long long)stop, (long long)hi);
        std::vector<uint8_t> out;
        const int64_t bad = L.inflateOnHost(out);
        error.clear();
        if (bad >= 0) L.blockRefused(bad, PLAT_ERR_BAD_INPUT);
        printf("inflate %lld\n%s\n", (long long)bad, error.c_str());
        if (bad >= 0) continue;
        printf("data ");
        for (uint8_t x : out) printf("%02x", x);
        printf("\n");
    }
    return 0;
}
