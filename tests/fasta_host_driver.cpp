// fasta_host_driver.cpp -- the host side of csrc/fasta_rule.hpp alone, for tests/fasta_cases.py (built as a shared library: the host twin
// the CPU tests pin to the fixture and the GPU tests take their expectations from) and, with -DFASTA_DRIVER_MAIN, as a stand-alone
// program that runs the rule over seeded indexes and queries under the sanitizers (tests/test_fasta_cpu.py builds and runs it).
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>

#include "fasta_rule.hpp"

// queries: n x {StartPos, LineLength, FullLineLength, SeqLength, beg, end, mode}; off [n + 1], status [n], out [cap].  Returns the bytes of
// all answers; no byte past cap is written.
extern "C" int64_t fasta_twin_fetch(const uint8_t* cut, int64_t cut_len, int64_t file_base, int64_t file_size, int64_t n, const int64_t* q,
                                    int64_t* off, int32_t* status, uint8_t* out, int64_t cap)
{
    int64_t total = 0;
    for (int64_t k = 0; k < n; ++k) {
        const int64_t* v = q + 7 * k;
        const fasta::Entry e{v[0], v[1], v[2], v[3]};
        const fasta::Span s = fasta::span_of(e, v[4], v[5], v[6] ? fasta::MODE_CONTIG : fasta::MODE_SEQUENCE, file_size);
        status[k] = fasta::cut_of(s, file_base, cut_len);
        off[k] = total;
        if (status[k] != fasta::ST_OK) continue;
        for (int64_t i = s.lo; i < s.hi; ++i) {
            const uint8_t c = cut[i - file_base];
            if (!fasta::keeps(c)) continue;
            if (total < cap) out[total] = fasta::upper(c);
            ++total;
        }
    }
    off[n] = total;
    return total;
}

// rows: per line {rc, the name's offset in fai, its length, SeqLength, StartPos, LineLength, FullLineLength}; returns the lines
extern "C" int64_t fasta_twin_parse(const uint8_t* fai, int64_t len, int parseNCBI, int64_t cap, int64_t* rows)
{
    int64_t lines = 0;
    for (int64_t at = 0; at < len && lines < cap; ++lines) {
        int64_t nl = at;
        while (nl < len && fai[nl] != '\n') ++nl;
        const int64_t next = nl < len ? nl + 1 : len;
        fasta::FaiLine L;
        memset(&L, 0, sizeof L);
        int64_t* r = rows + 7 * lines;
        r[0] = fasta::parse_fai_line(fai + at, next - at, parseNCBI, &L);
        r[1] = at + L.name_at; r[2] = L.name_len; r[3] = L.e.seq_len; r[4] = L.e.start_pos; r[5] = L.e.line_len; r[6] = L.e.full_len;
        at = next;
    }
    return lines;
}

// the byte in the low eight bits (0x100: nothing, the file ends in front of it), the status from bit 12 on
extern "C" int fasta_twin_char(const uint8_t* file, int64_t file_size, int64_t start_pos, int64_t line_len, int64_t full_len, int64_t seq_len, int64_t pos)
{
    int32_t st = 0;
    const int c = fasta::character_at(fasta::Entry{start_pos, line_len, full_len, seq_len}, pos, file, file_size, &st);
    return (c < 0 ? 0x100 : c) | (st << 12);
}

#ifdef FASTA_DRIVER_MAIN
// seeded files, indexes that lie in every field and queries far outside them: the twin must stay inside the cut (the sanitizers watch) and
// upper4 must agree with upper on every byte pair
int main()
{
    uint64_t x = 88172645463325252ull;
    auto rnd = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
    for (unsigned w = 0; w < 65536; ++w) {
        const uint32_t word = w | ((uint32_t)(rnd() & 0xffff) << 16);
        const uint32_t u = fasta::upper4(word);
        for (int j = 0; j < 4; ++j)
            if ((uint8_t)(u >> (8 * j)) != fasta::upper((uint8_t)(word >> (8 * j)))) { printf("upper4 differs at %08x\n", word); return 1; }
    }
    long long bytes = 0, refused = 0;
    for (int round = 0; round < 2000; ++round) {
        const int64_t size = (int64_t)(rnd() % 4000), base = (int64_t)(rnd() % (size + 1)), len = (int64_t)(rnd() % (size - base + 1));
        std::vector<uint8_t> cut((size_t)len);
        for (auto& c : cut) c = (uint8_t)(rnd() % 5 == 0 ? '\n' : rnd());
        const int64_t n = 40;
        std::vector<int64_t> q((size_t)(7 * n)), off((size_t)n + 1);
        std::vector<int32_t> st((size_t)n);
        for (int64_t k = 0; k < n; ++k) {
            int64_t* v = q.data() + 7 * k;
            const bool wild = rnd() % 4 == 0;
            v[0] = wild ? (int64_t)rnd() : (int64_t)(rnd() % (size + 10)) - 3;
            v[1] = wild ? (int64_t)rnd() >> (rnd() % 64) : (int64_t)(rnd() % 80) - 2;
            v[2] = wild ? (int64_t)rnd() >> (rnd() % 64) : v[1] + (int64_t)(rnd() % 4) - 1;
            v[3] = wild ? (int64_t)rnd() >> (rnd() % 64) : (int64_t)(rnd() % 5000) - 5;
            v[4] = wild ? (int64_t)rnd() : (int64_t)(rnd() % 5000) - 20;
            v[5] = wild ? (int64_t)rnd() : v[4] + (int64_t)(rnd() % 300) - 5;
            v[6] = (int64_t)(rnd() % 2);
        }
        const int64_t cap = (int64_t)(rnd() % 3000);
        std::vector<uint8_t> out((size_t)cap);
        bytes += fasta_twin_fetch(cut.data(), len, base, size, n, q.data(), off.data(), st.data(), out.data(), cap);
        for (int32_t s : st) refused += s != 0;
        std::vector<uint8_t> fai((size_t)(rnd() % 200));
        for (auto& c : fai) { const uint64_t r = rnd() % 12; c = r == 0 ? '\t' : r == 1 ? '\n' : r == 2 ? '|' : r == 3 ? ' ' : r < 8 ? (uint8_t)('0' + rnd() % 10) : (uint8_t)("gi|ref-+x"[rnd() % 9]); }
        std::vector<int64_t> rows(7 * 64);
        fasta_twin_parse(fai.data(), (int64_t)fai.size(), (int)(rnd() % 2), 64, rows.data());
    }
    printf("fasta rule driver OK: %lld bytes fetched, %lld queries without bytes\n", bytes, refused);
    return 0;
}
#endif
