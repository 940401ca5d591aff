// The host twin of the tabix indexer and its finishing stage (platypus_amd/csrc/tabix_index.hpp -- the record's rule is the text the device
// compiles) over blocks walked and inflated by the caller library's own block list (csrc/host/bgzf_blocks.hpp over csrc/bgzf_inflate.hpp,
// the file as one chunk), as a stand-alone program for tests/test_tabix_index_cpu.py: built with -fsanitize=address,undefined where that links.
//   driver IN OUT
// IN:  u32 n_cases; per case i64 len, the bgzipped file's bytes
// OUT: per case i64 status[13]; i64 n_runs, i32 run_tid[], i32 run_bin[], i64 run_u[]; i64 n_ref, i64 name_off[], i32 name_len[],
//      i64 lin_first[n_ref + 1]; i64 n_windows, i64 lin[]; i64 raw_len, the index's bytes before BGZF (raw_len -1 for a refused file)
// The inflated bytes are allocated to the byte: a read past them is the sanitizer's to find.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#define PLAT_BGZF_BLOCKS_HOST_ONLY
#include "host/bgzf_blocks.hpp"
#include "tabix_index.hpp"

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
template <class T> static void put(FILE* out, const std::vector<T>& v) { if (!v.empty()) fwrite(v.data(), sizeof(T), v.size(), out); }
static void put(FILE* out, int64_t x) { fwrite(&x, sizeof x, 1, out); }

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: driver IN OUT\n"); return 2; }
    const std::vector<uint8_t> raw = readAll(argv[1]);
    FILE* out = fopen(argv[2], "wb");
    if (!out) { perror(argv[2]); return 2; }
    size_t at = 0;
    auto need = [&](size_t n) { if (at + n > raw.size()) { fprintf(stderr, "short input\n"); exit(2); } };
    need(4);
    uint32_t nCases;
    memcpy(&nCases, raw.data(), 4); at = 4;
    for (uint32_t k = 0; k < nCases; ++k) {
        int64_t len;
        need(8); memcpy(&len, raw.data() + at, 8); at += 8;
        need((size_t)len);
        const std::vector<uint8_t> file(raw.begin() + (long)at, raw.begin() + (long)at + (long)len);
        at += (size_t)len;
        // as host/tbi_out.hpp: the file as one chunk, the blocks up to the last that holds data, the address behind it
        std::string error;
        plathost::BgzfBlockList L("driver", [](const plathost::BgzfChunkAt&) { return std::string(); }, false, error);
        plat_bgzf_chunk ch{file.data(), len, 0, -1, 0};
        if (L.add(0, 0, 0, ch) != 0) { fprintf(stderr, "case %u: %s\n", k, error.c_str()); return 2; }
        size_t nData = L.blkOff.size();
        while (nData > 0 && L.inflatedEnd((int)nData - 1) == L.blkInflated[nData - 1]) --nData;
        std::vector<int64_t> outOff(L.blkInflated.begin(), L.blkInflated.begin() + (long)nData), addr(L.blkOff.begin(), L.blkOff.begin() + (long)nData);
        outOff.push_back(L.inflated);
        addr.push_back(nData < L.blkOff.size() ? L.blkOff[nData] : len);
        const int64_t inflated = L.inflated;
        std::unique_ptr<uint8_t[]> data(new uint8_t[(size_t)inflated ? (size_t)inflated : 1]);
        const int64_t bad = L.inflateOnHost(data.get());
        if (bad >= 0) { L.blockRefused(bad, -9); fprintf(stderr, "case %u: %s\n", k, error.c_str()); return 2; }
        tbxindex::Intermediate I;
        tbxindex::build_serial(data.get(), inflated, outOff.data(), addr.data(), (int)nData, I);
        fwrite(I.status, sizeof(int64_t), tbxindex::ST_WORDS, out);
        put(out, (int64_t)I.runU.size()); put(out, I.runTid); put(out, I.runBin); put(out, I.runU);
        put(out, (int64_t)I.nameOff.size()); put(out, I.nameOff); put(out, I.nameLen); put(out, I.linFirst);
        put(out, (int64_t)I.lin.size()); put(out, I.lin);
        if (I.status[tbxindex::ST_VERDICT] != 0) { put(out, (int64_t)-1); continue; }
        const std::vector<uint8_t> tbi = tbxindex::finish(I, tbxindex::names_of(I));
        put(out, (int64_t)tbi.size()); put(out, tbi);
    }
    fclose(out);
    return 0;
}
