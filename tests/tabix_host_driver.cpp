// The host build of the tabix rule (platypus_amd/csrc/tabix_rule.hpp -- the text the device compiles) over blocks walked and inflated by the
// caller library's own block list (csrc/host/bgzf_blocks.hpp over csrc/bgzf_inflate.hpp), as a stand-alone program for
// tests/test_tabix_cpu.py: built with -fsanitize=address,undefined where that links.
//   driver IN OUT
// IN:  u32 n_cases; per case u32 n_streams; per stream u32 name_len, name, i32 beg, i32 end, u32 n_chunks; per chunk u32 data_len, data,
//      i32 first_uoffset, i64 end_coffset, i32 end_uoffset
// OUT: per case i64 status[4] {0 or -9, the lowest refused stream or -1, kept lines, kept bytes}, i64 off[n_streams + 1], i64 counts[2 n_streams]
//      (lines walked ahead of the stop or refusal; lines kept, 0 for a refused stream), then the text
// The inflated bytes lie between two guard bands that no read or write may touch (exit code 3 when a byte of them changed; a read is the
// sanitizer's to find: the buffer is allocated to the byte).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#define PLAT_BGZF_BLOCKS_HOST_ONLY
#include "host/bgzf_blocks.hpp"
#include "tabix_rule.hpp"

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
struct Chunk { std::vector<uint8_t> data; int32_t firstU, endU; int64_t endC; };
struct Stream { std::vector<uint8_t> name; int32_t beg, end; std::vector<Chunk> chunks; };

constexpr size_t GUARD = 64;
constexpr uint8_t GUARD_BYTE = 0xa5;

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: driver IN OUT\n"); return 2; }
    const std::vector<uint8_t> raw = readAll(argv[1]);
    In in{raw};
    FILE* out = fopen(argv[2], "wb");
    if (!out) { perror(argv[2]); return 2; }
    const uint32_t nCases = in.take<uint32_t>();
    for (uint32_t k = 0; k < nCases; ++k) {
        std::vector<Stream> streams(in.take<uint32_t>());
        for (Stream& s : streams) {
            const uint32_t nameLen = in.take<uint32_t>();
            const uint8_t* p = in.bytes(nameLen);
            s.name.assign(p, p + nameLen);
            s.beg = in.take<int32_t>(); s.end = in.take<int32_t>();
            s.chunks.resize(in.take<uint32_t>());
            for (Chunk& c : s.chunks) {
                const uint32_t n = in.take<uint32_t>();
                const uint8_t* d = in.bytes(n);
                c.data.assign(d, d + n);
                c.firstU = in.take<int32_t>(); c.endC = in.take<int64_t>(); c.endU = in.take<int32_t>();
            }
        }
        int64_t status[4] = {0, -1, 0, 0};
        std::vector<int64_t> off(1, 0), counts;
        std::string text;
        for (size_t si = 0; si < streams.size(); ++si) {
            const Stream& s = streams[si];
            // the chunks' blocks inflated back to back between the guard bands, the chunks' geometry as the caller library derives it
            std::string error;
            plathost::BgzfBlockList L("driver", [](const plathost::BgzfChunkAt& a) { return "chunk " + std::to_string(a.chunk); }, false, error);
            std::vector<plat_bgzf_chunk> chunks;
            for (const Chunk& c : s.chunks) chunks.push_back(plat_bgzf_chunk{c.data.data(), (int64_t)c.data.size(), c.firstU, c.endC, c.endU});
            for (size_t q = 0; q < chunks.size(); ++q)
                if (L.add((int)k, (int)si, (int)q, chunks[q]) != 0) { fprintf(stderr, "case %u: %s\n", k, error.c_str()); return 2; }
            const int64_t inflated = L.inflated;
            std::unique_ptr<uint8_t[]> buf(new uint8_t[(size_t)inflated + 2 * GUARD]);
            memset(buf.get(), GUARD_BYTE, (size_t)inflated + 2 * GUARD);
            uint8_t* data = buf.get() + GUARD;
            const int64_t bad = L.inflateOnHost(data);
            if (bad >= 0) { L.blockRefused(bad, -9); fprintf(stderr, "case %u: %s\n", k, error.c_str()); return 2; }
            std::vector<int64_t> first(chunks.size()), stop(chunks.size()), hi(chunks.size());
            for (size_t q = 0; q < chunks.size(); ++q) L.span(q, first[q], stop[q], hi[q]);
            int64_t walked = 0, kept = 0;
            const size_t before = text.size();
            const bool ok = tbxrule::walk_stream(data, (int)s.chunks.size(), first.data(), stop.data(), hi.data(), s.name.data(), (int32_t)s.name.size(), s.beg, s.end,
                                                 &walked, &kept, [&](int64_t a, int64_t e) { text.append((const char*)data + a, (size_t)(e - a)); text.push_back('\n'); });
            for (size_t g = 0; g < GUARD; ++g)
                if (buf[g] != GUARD_BYTE || buf[GUARD + (size_t)inflated + g] != GUARD_BYTE) { fprintf(stderr, "case %u: a guard band was written\n", k); return 3; }
            if (!ok) {
                text.resize(before); kept = 0;
                if (status[0] == 0) { status[0] = -9; status[1] = (int64_t)si; }
            }
            counts.push_back(walked); counts.push_back(kept);
            status[2] += kept;
            off.push_back((int64_t)text.size());
        }
        status[3] = (int64_t)text.size();
        fwrite(status, sizeof(int64_t), 4, out);
        fwrite(off.data(), sizeof(int64_t), off.size(), out);
        if (!counts.empty()) fwrite(counts.data(), sizeof(int64_t), counts.size(), out);
        if (!text.empty()) fwrite(text.data(), 1, text.size(), out);
    }
    fclose(out);
    return 0;
}
