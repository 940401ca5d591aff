// ref_context_driver.cpp -- a stand-alone program over platypus_amd/csrc/host/records.hpp (tests/test_ref_context_cpu.py), built with
// -fsanitize=address,undefined: the readers of a Variant's reference context next to the same readers on the reference itself.
//   ref_context_driver CASES     CASES: one case per line, "<reference> <pos> <remPos> <nRemoved> <added or ->"
// The reference of every case is copied into a heap block of exactly its length, so a read past either end is one the sanitizer sees.
// Per case two lines, probeRefContext() without and with the context; then "PP <posterior>: <PP> <PPnum> <PPint> | <the same parsed from
// the text>" for the posteriors of the setPP case, and the NO_REFCTX switch under its spellings.  Exit status 1 when the two lines of a
// case differ in anything but their CTX field.
#include "host/records.hpp"
#include "host/switches.hpp"

#include <cstdio>
#include <fstream>
#include <sstream>

using namespace plathost;

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: ref_context_driver CASES\n"); return 2; }
    std::ifstream in(argv[1]);
    std::string line;
    int bad = 0;
    while (std::getline(in, line)) {
        std::istringstream ls(line);
        std::string ref, added;
        long long pos, remPos;
        int nrem;
        if (!(ls >> ref >> pos >> remPos >> nrem >> added)) continue;
        if (added == "-") added.clear();
        char* block = new char[ref.size()];
        memcpy(block, ref.data(), ref.size());
        Fasta fa;
        fa.seq = (const uint8_t*)block; fa.len = (int64_t)ref.size();
        const std::string a = probeRefContext(fa, (int)pos, remPos, (size_t)nrem, added.data(), added.size(), false);
        const std::string b = probeRefContext(fa, (int)pos, remPos, (size_t)nrem, added.data(), added.size(), true);
        delete[] block;
        printf("%s\n%s\n", a.c_str(), b.c_str());
        if (a.substr(a.find('\t')) != b.substr(b.find('\t'))) { fprintf(stderr, "paths differ: %s\n  %s\n  %s\n", line.c_str(), a.c_str(), b.c_str()); ++bad; }
    }
    for (double p : {0.0, 0.49, 0.5, 1.5, 2.5, 99.5, 2500.0, 2500.5, 1e9}) {
        VarInfo d;
        d.setPP(p);
        printf("PP %.17g: %s %.17g %d | %.17g %d\n", p, d.PP.c_str(), d.PPnum, d.PPint, strtod(d.PP.c_str(), nullptr), atoi(d.PP.c_str()));
        if (d.PPnum != strtod(d.PP.c_str(), nullptr) || d.PPint != atoi(d.PP.c_str())) { fprintf(stderr, "setPP differs from its text at %.17g\n", p); ++bad; }
    }
    for (const char* s : {(const char*)nullptr, "", "0", "1", "yes"}) {
        if (s) setenv("PLAT_CALLER_NO_REFCTX", s, 1); else unsetenv("PLAT_CALLER_NO_REFCTX");
        printf("NO_REFCTX %s: noRefCtx=%d\n", s ? (s[0] ? s : "empty") : "unset", Switches::read().noRefCtx);
    }
    return bad ? 1 : 0;
}
