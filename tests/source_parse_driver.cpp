// The host parser of source VCF lines (platypus_amd/csrc/host/source_variants.hpp over csrc/source_rule.hpp -- the rule the device compiles
// too) as a stand-alone program for the sanitizers: tests/test_source_variants_cpu.py builds it with -fsanitize=address,undefined and runs
// it.  Input file: records of {int64 length, int32 maxSize, int32 longHaps, bytes}.  Every text is copied into an exact-size heap block
// per region (no slack: a read past the region's end is a heap overflow the sanitizer sees), parsed whole, then as seeded random bytes
// made of the rule's alphabet, then truncated at every length.  Prints counts; "ok" at the end.
#define PLAT_SOURCE_PARSER_ONLY
#include <cstdio>
#include <cstdlib>
#include <string>

#include "../platypus_amd/csrc/host/source_variants.hpp"

using namespace plathost;

static long long parseExact(const std::string& t, int maxSize, int longHaps, long long* lines) {
    uint8_t* block = (uint8_t*)malloc(t.size() ? t.size() : 1);         // exact size: the parser may not read one byte more
    memcpy(block, t.data(), t.size());
    const int64_t off[2] = {0, (int64_t)t.size()}, name[1] = {12345};
    SourceAlleles a;
    parseSourceLinesHost(block, (int64_t)t.size(), off, name, 1, maxSize, longHaps, -1, a);
    long long n = (long long)a.size();
    for (size_t i = 0; i < a.size(); ++i) {                              // every allele lies inside the text
        if (a.remOff[i] < 0 || a.remOff[i] + a.nRem[i] > (int64_t)t.size() || a.addOff[i] < 0 || a.addOff[i] + a.nAdd[i] > (int64_t)t.size() || a.nRem[i] < 0 || a.nAdd[i] < 0) {
            fprintf(stderr, "allele %zu outside the text\n", i);
            exit(2);
        }
    }
    const std::vector<int> order = sourceSetSorted(block, a, 0, (int)a.size());
    if (order.size() > a.size()) exit(3);
    if (lines) *lines = a.status[3];
    free(block);
    return n;
}

int main(int argc, char** argv) {
    if (argc < 2) return 1;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 1;
    std::vector<std::string> texts;
    std::vector<int> maxSizes, longs;
    for (;;) {
        int64_t len; int32_t ms, lh;
        if (fread(&len, 8, 1, f) != 1) break;
        if (fread(&ms, 4, 1, f) != 1 || fread(&lh, 4, 1, f) != 1) return 1;
        std::string t((size_t)len, '\0');
        if (len && fread(&t[0], 1, (size_t)len, f) != (size_t)len) return 1;
        texts.push_back(t); maxSizes.push_back(ms); longs.push_back(lh);
    }
    fclose(f);
    long long alleles = 0;
    for (size_t k = 0; k < texts.size(); ++k) alleles += parseExact(texts[k], maxSizes[k], longs[k], nullptr);
    printf("golden %zu %lld\n", texts.size(), alleles);
    // seeded random bytes of the rule's alphabet (tabs, newlines, commas, digits, bases, a few others)
    static const char alphabet[] = "\t\t\t\n\n,,0123456789ACGTNacgt.*<>#-+ \r";
    unsigned long long x = 88172645463325252ull;
    auto rnd = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
    long long fuzzAlleles = 0, fuzzLines = 0;
    for (int k = 0; k < 4000; ++k) {
        std::string t((size_t)(rnd() % 200), ' ');
        for (char& c : t) c = alphabet[rnd() % (sizeof alphabet - 1)];
        long long lines = 0;
        fuzzAlleles += parseExact(t, (int)(rnd() % 3 ? 1500 : 2), (int)(rnd() & 1), &lines);
        fuzzLines += lines;
    }
    printf("fuzz 4000 texts, %lld lines, %lld alleles\n", fuzzLines, fuzzAlleles);
    // the golden texts truncated at every length (a fetch cut anywhere: inside a column, behind a tab, inside ALT)
    long long cut = 0;
    for (size_t k = 0; k < texts.size() && k < 12; ++k)
        for (size_t n = 0; n <= texts[k].size(); ++n) { parseExact(texts[k].substr(0, n), maxSizes[k], longs[k], nullptr); ++cut; }
    printf("truncated %lld texts\nok\n", cut);
    return 0;
}
