// The host build of platypus_amd/csrc/bam_aux.hpp for tests/test_bam_read_groups_cpu.py: the rule of plat_bam_route_batch run over a file
// of records, every record copied into a heap block of exactly its size (the sanitizers see the first byte outside) and read through an
// accessor that aborts on an index outside it (so a build without sanitizers sees it too).
//   bam_aux_host_driver CASES OUT    cases: u32 n_groups, then per group u32 len + the ID's bytes + i32 sample;
//                                           u32 n_records, then per record u32 lead + u32 len + the record's bytes
//                                    out:   per record i32 verdict (bamaux::ROUTED ...), i32 sample (-1 when refused)
// `lead`: the offset the record is given (its bytes are indexed lead .. lead + len, as a record inside a blob is).  Exit status 0; 2 for
// a malformed case file.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "bam_aux.hpp"

struct Checked {                                          // a byte accessor that refuses to leave the record
    const uint8_t* p; int64_t lo, hi;
    uint8_t operator[](int64_t at) const {
        if (at < lo || at >= hi) { fprintf(stderr, "read outside the record: %lld of [%lld, %lld)\n", (long long)at, (long long)lo, (long long)hi); abort(); }
        return p[at - lo];
    }
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

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    std::vector<uint8_t> cases;
    if (!read_all(argv[1], cases)) return 2;
    FILE* fo = fopen(argv[2], "wb");
    if (!fo) return 2;
    size_t at = 0;
    auto u32 = [&]() -> uint32_t { if (at + 4 > cases.size()) exit(2); uint32_t v; memcpy(&v, &cases[at], 4); at += 4; return v; };
    // the table: the IDs in a block of exactly their size
    const uint32_t nGroups = u32();
    std::vector<uint8_t> idBytes;
    std::vector<int32_t> idOff(1, 0), sample;
    for (uint32_t g = 0; g < nGroups; ++g) {
        const uint32_t len = u32();
        if (at + len > cases.size()) return 2;
        idBytes.insert(idBytes.end(), cases.begin() + (long)at, cases.begin() + (long)(at + len));
        at += len;
        idOff.push_back((int32_t)idBytes.size());
        sample.push_back((int32_t)u32());
    }
    uint8_t* ids = (uint8_t*)malloc(idBytes.empty() ? 1 : idBytes.size());
    if (!idBytes.empty()) memcpy(ids, idBytes.data(), idBytes.size());
    const uint32_t slots = bamaux::table_slots((int32_t)nGroups);
    std::vector<uint32_t> slotHash(slots, 0);
    std::vector<int32_t> slotGroup(slots, -1);
    for (uint32_t g = 0; g < nGroups; ++g)
        bamaux::table_insert(slotHash.data(), slotGroup.data(), slots - 1, bamaux::hash_id(ids + idOff[g], idOff[g + 1] - idOff[g]), (int32_t)g);
    const bamaux::GroupTable table{slotHash.data(), slotGroup.data(), slots - 1, ids, idOff.data()};

    const uint32_t n = u32();
    for (uint32_t c = 0; c < n; ++c) {
        const uint32_t lead = u32(), len = u32();
        if (at + len > cases.size()) return 2;
        uint8_t* rec = (uint8_t*)malloc(len ? len : 1);      // (an exact-size copy: a read past the record is a read past the allocation)
        if (len) memcpy(rec, cases.data() + at, len);
        at += len;
        const Checked m{rec, (int64_t)lead, (int64_t)lead + len};
        int32_t group = -1;
        const int32_t v = bamaux::route(m, (int64_t)lead, (int64_t)lead + len, table, &group);
        const int32_t s = v == bamaux::ROUTED ? sample[(size_t)group] : -1;
        if ((v == bamaux::ROUTED) != (group >= 0)) abort();
        fwrite(&v, 4, 1, fo); fwrite(&s, 4, 1, fo);
        free(rec);
    }
    free(ids);
    fclose(fo);
    return 0;
}
