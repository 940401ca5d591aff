// mate_rule_host_driver.cpp -- csrc/mate_rule.hpp as a stand-alone program (tests/test_bam_mates_cpu.py compiles and runs it, also under
// -fsanitize=address,undefined).  It reads cases from the file named on its command line and prints what the rule makes of them:
//
//   case <n_contigs> <chrom_id> <start> <end> <n_reads> <n_second>
//   <name> ... (n_contigs)
//   <flag> <mtid> <mpos> ... (n_reads)          the fetched reads
//   <mtid> <mpos> ... (n_second)                records of a second-round fetch
//
// per case: "P <mtid> <mpos>" for every read that gives a coordinate, in input order; "S <mtid> <mpos>" the same sorted; "Q <name> <start>
// <end>" per query; "W <itr_beg> <itr_end>" the query's fetch window; "M <0|1>" per second-round record; "end".
// The reads go through real record bytes: 32 fixed bytes written at every alignment mod 16 inside a larger buffer, read back by fields_of.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "mate_rule.hpp"

static void put32(std::vector<uint8_t>& b, size_t at, int32_t v) { for (int k = 0; k < 4; ++k) b[at + k] = (uint8_t)((uint32_t)v >> (8 * k)); }

struct Bytes { const uint8_t* p; uint8_t operator[](int at) const { return p[at]; } };

int main(int argc, char** argv)
{
    if (argc < 2) { fprintf(stderr, "usage: mate_rule_host_driver CASES\n"); return 2; }
    FILE* in = fopen(argv[1], "r");
    if (!in) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    char word[256];
    int nContigs, chromId, nReads, nSecond;
    long long start, end;
    long long nCase = 0;
    while (fscanf(in, "%255s", word) == 1) {
        if (strcmp(word, "case") != 0 || fscanf(in, "%d %d %lld %lld %d %d", &nContigs, &chromId, &start, &end, &nReads, &nSecond) != 6) return 3;
        std::vector<std::string> names;
        for (int t = 0; t < nContigs; ++t) { if (fscanf(in, "%255s", word) != 1) return 3; names.push_back(word); }
        auto field = [&](const std::vector<uint8_t>& buf, size_t at) { return mate::fields_of(Bytes{buf.data() + at}); };
        std::vector<mate::Coord> coords;
        for (int i = 0; i < nReads; ++i) {
            long long flag, mtid, mpos;
            if (fscanf(in, "%lld %lld %lld", &flag, &mtid, &mpos) != 3) return 3;
            const size_t at = (size_t)((i + nCase) % 16);                   // the record's refID at every alignment
            std::vector<uint8_t> buf(at + mate::FIXED_BYTES, 0xA5);         // (exactly as long as the fixed part: a read past it is the sanitizer's to find)
            put32(buf, at + 0, chromId); buf[at + mate::OFF_FLAG] = (uint8_t)(flag & 0xff); buf[at + mate::OFF_FLAG + 1] = (uint8_t)((flag >> 8) & 0xff);
            put32(buf, at + mate::OFF_MTID, (int32_t)mtid); put32(buf, at + mate::OFF_MPOS, (int32_t)mpos);
            const mate::Fields f = field(buf, at);
            if (f.flag != (uint16_t)flag || f.mtid != (int32_t)mtid || f.mpos != (int32_t)mpos) { fprintf(stderr, "fields_of reads other bytes\n"); return 4; }
            if (mate::gives_coord(f)) { coords.push_back(mate::Coord{f.mtid, f.mpos}); printf("P %d %d\n", f.mtid, f.mpos); }
        }
        auto nameCmp = [&](int32_t a, int32_t b) { return names[(size_t)a].compare(names[(size_t)b]); };
        std::stable_sort(coords.begin(), coords.end(), [&](const mate::Coord& a, const mate::Coord& b) { return mate::coord_less(a, b, nameCmp); });
        for (const mate::Coord& c : coords) printf("S %d %d\n", c.mtid, c.mpos);
        mate::merge_queries(coords.data(), (long long)coords.size(), [&](int32_t a, int32_t b) { return names[(size_t)a] == names[(size_t)b]; }, [&](const mate::Query& q) {
            int32_t b = 0, e = 0;
            mate::query_window(q, &b, &e);
            printf("Q %s %lld %lld\nW %d %d\n", names[(size_t)q.mtid].c_str(), (long long)q.start, (long long)q.end, b, e);
        });
        for (int i = 0; i < nSecond; ++i) {
            long long mtid, mpos;
            if (fscanf(in, "%lld %lld", &mtid, &mpos) != 2) return 3;
            const size_t at = (size_t)((i + 7 * nCase) % 16);
            std::vector<uint8_t> buf(at + mate::FIXED_BYTES, 0x5A);
            put32(buf, at + mate::OFF_MTID, (int32_t)mtid); put32(buf, at + mate::OFF_MPOS, (int32_t)mpos);
            printf("M %d\n", mate::is_mate(field(buf, at), chromId, (int32_t)start, (int32_t)end) ? 1 : 0);
        }
        printf("end\n");
        ++nCase;
    }
    fclose(in);
    return 0;
}
