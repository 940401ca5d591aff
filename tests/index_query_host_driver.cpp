// index_query_host_driver.cpp -- the host side of csrc/index_query.hpp alone, for tests/test_index_query_cpu.py: built with
// -fsanitize=address,undefined where that links.  Three modes:
//   driver cases IN OUT   IN: u32 n, then per index {i32 kind, i32 prefixes, i64 len, the bytes (a .tbi's already inflated), i32 n_queries,
//                         n_queries x (tid, beg, end) i32}.  OUT (text): per index "I rc n_ref no_coor", the seven tables as "T name values...",
//                         "N name" per reference name (hex), per query "Q rc count gathered" and count lines "u v"; and, where prefixes is
//                         set, "P" followed by every length L < len whose prefix raw[0, L) -- copied to a heap block of exactly L bytes, so
//                         that a read past it is the sanitizer's -- the flatten ACCEPTS
//   driver loops SEED N   N seeded random lists (ties and zero-length chunks included) through the reference's three sequential loops
//                         (resolve_serial), the three data-parallel steps (resolve_parallel) and the one scan (resolve_fused): prints the
//                         number of lists on which they differ
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <random>

#include "index_query.hpp"

static std::vector<uint8_t> slurp(const char* path)
{
    std::vector<uint8_t> b;
    FILE* f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
    uint8_t buf[65536];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) b.insert(b.end(), buf, buf + n);
    fclose(f);
    return b;
}

template <class T> static void table(FILE* out, const char* name, const std::vector<T>& v)
{
    fprintf(out, "T %s", name);
    for (const T& x : v) fprintf(out, " %llu", (unsigned long long)(uint64_t)x);
    fprintf(out, "\n");
}

static int cases(const char* in, const char* outPath)
{
    const std::vector<uint8_t> b = slurp(in);
    FILE* out = fopen(outPath, "w");
    if (!out) return 2;
    size_t at = 0;
    auto i32 = [&]() { int32_t v; memcpy(&v, b.data() + at, 4); at += 4; return v; };
    auto i64 = [&]() { int64_t v; memcpy(&v, b.data() + at, 8); at += 8; return v; };
    const int32_t n = i32();
    for (int32_t k = 0; k < n; ++k) {
        const int32_t kind = i32(), prefixes = i32();
        const int64_t len = i64();
        uint8_t* raw = (uint8_t*)malloc((size_t)len ? (size_t)len : 1);         // (its own block: the sanitizer watches its end)
        memcpy(raw, b.data() + at, (size_t)len);
        at += (size_t)len;
        idxq::Flat F;
        const int rc = idxq::flatten(raw, (size_t)len, kind, F);
        fprintf(out, "I %d %d %lld\n", rc, F.nRef, (long long)F.noCoor);
        table(out, "ref_bin_first", F.refBinFirst); table(out, "bin_id", F.binId); table(out, "bin_chunk_first", F.binChunkFirst);
        table(out, "chunk_u", F.chunkU); table(out, "chunk_v", F.chunkV); table(out, "ref_lin_first", F.refLinFirst); table(out, "lin_fill", F.linFill);
        for (const std::string& s : F.names) { fprintf(out, "N "); for (unsigned char c : s) fprintf(out, "%02x", c); fprintf(out, "\n"); }
        const int32_t nq = i32();
        for (int32_t q = 0; q < nq; ++q) {
            const int32_t tid = i32(), beg = i32(), end = i32();
            std::vector<int64_t> u, v;
            int32_t count = 0, gathered = 0;
            const int qrc = rc == 0 ? idxq::query(F, tid, beg, end, u, v, &count, &gathered) : rc;
            fprintf(out, "Q %d %d %d\n", qrc, count, gathered);
            for (size_t j = 0; j < u.size(); ++j) fprintf(out, "%llu %llu\n", (unsigned long long)u[j], (unsigned long long)v[j]);
        }
        if (prefixes) {
            fprintf(out, "P");
            for (int64_t L = 0; L < len; ++L) {
                uint8_t* p = (uint8_t*)malloc((size_t)L ? (size_t)L : 1);
                memcpy(p, raw, (size_t)L);
                idxq::Flat G;
                if (idxq::flatten(p, (size_t)L, kind, G) == 0) fprintf(out, " %lld", (long long)L);
                free(p);
            }
            fprintf(out, "\n");
        }
        free(raw);
    }
    fclose(out);
    return at == b.size() ? 0 : 3;
}

static int loops(uint64_t seed, long n)
{
    std::mt19937_64 rng(seed);
    long differ = 0, chunks = 0, ties = 0, empty = 0;
    for (long k = 0; k < n; ++k) {
        const int sizes[] = {0, 1, 2, 3, 5, 8, 13, 40, 130};
        const int m = sizes[rng() % 9];
        const uint64_t span = 1ull << (17 + rng() % 4);
        std::vector<idxq::Chunk> c;
        for (int i = 0; i < m; ++i) {
            const uint64_t u = !c.empty() && rng() % 8 == 0 ? c.back().first : rng() % span;       // (ties in u)
            const uint64_t kind = rng() % 5, len = kind < 2 ? 0 : kind == 2 ? 1 : kind == 3 ? rng() % 65536 : rng() % span;
            c.emplace_back(u, u + len);
            empty += len == 0;
        }
        std::sort(c.begin(), c.end());
        for (size_t i = 1; i < c.size(); ++i) ties += c[i].first == c[i - 1].first;
        chunks += m;
        const std::vector<idxq::Chunk> a = idxq::resolve_serial(c), p = idxq::resolve_parallel(c), f = idxq::resolve_fused(c);
        if (a != p || a != f) ++differ;
    }
    printf("%ld %ld %ld %ld %ld\n", differ, n, chunks, ties, empty);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 4 && !strcmp(argv[1], "cases")) return cases(argv[2], argv[3]);
    if (argc == 4 && !strcmp(argv[1], "loops")) return loops(strtoull(argv[2], nullptr, 10), atol(argv[3]));
    fprintf(stderr, "usage: driver cases IN OUT | driver loops SEED N\n");
    return 9;
}
