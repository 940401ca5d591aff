// caller_lifetime_driver.cpp -- a stand-alone program (tests/test_native_caller_cpu.py) over the whole native region loop on the CPU stand-in
// device: platypus_amd/csrc/host/region_caller.cpp + tools/synth/region_source.cpp + tests/fakedev/fake_device.c, all built with
// -fsanitize=address,undefined.  It makes a caller, calls six synthetic regions through plat_call_regions_stream, frees the text, destroys the caller,
// and looks at what the heap still holds: four cases, twice over, then the text blocks.
//   * a buffer of a worker that nothing frees is a leak LeakSanitizer reports at exit, and in the second pass (the process's one-time statics are
//     made by then) the allocated bytes after a case must be what they were before it;
//   * a buffer freed after its context is a use after free: the stand-in's plat_free / plat_host_free / plat_stream_destroy read their context;
//   * a text block of more than 8 MB is kept for the next call only while a caller exists.
// Prints one line per case and pass; exit status 1 when a check fails (each failure on stderr).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../include/platypus_caller.h"

extern "C" size_t __sanitizer_get_current_allocated_bytes(void);             // (sanitizer/allocator_interface.h)
// libplat_synth's entry points (tools/synth/region_source.cpp has no header: tools/synth/source.py binds them the same way)
struct plat_synth;
extern "C" size_t plat_synth_slot_bytes(int region_len, int flank, int n_samples, int depth, int read_len, int encoding);
extern "C" int plat_synth_create(uint64_t seed, int region_len, int flank, int n_samples, int depth, int read_len, double snp_rate, double indel_rate, double err,
                                 int encoding, const int32_t* region_index, int n_regions, void* slot_memory, size_t slot_bytes, int n_slots, plat_synth** out);
extern "C" int plat_synth_load(void* user, int index, int slot, plat_region* out);
extern "C" void plat_synth_destroy(plat_synth* g);

static int g_bad = 0;
#define CHECK(cond, ...) do { if (!(cond)) { fprintf(stderr, "FAILED %s: ", #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); ++g_bad; } } while (0)

static long long heapBytes() { return (long long)__sanitizer_get_current_allocated_bytes(); }
static const long long SLACK = 1024, MB = 1 << 20;

struct Case { int samples, encoding, assemble, workers, perChunk; };

// one caller's whole life; *held: bytes allocated while the call's text is held
static std::string runCase(const Case& k, long long* held) {
    const int32_t ids[6] = {11, 5, 8, 2, 9, 3};
    const int nSlots = 7, regionLen = 3000, flank = 600, depth = 25, readLen = 100;
    const size_t slotBytes = plat_synth_slot_bytes(regionLen, flank, k.samples, depth, readLen, k.encoding);
    std::vector<uint8_t> mem(slotBytes * (size_t)nSlots);
    plat_synth* g = nullptr;
    CHECK(plat_synth_create(7, regionLen, flank, k.samples, depth, readLen, 3e-3, 1.5e-3, 0.002, k.encoding, ids, 6, mem.data(), slotBytes, nSlots, &g) == 0, "plat_synth_create");
    plat_caller* c = nullptr;
    CHECK(plat_caller_create(0, k.workers, k.perChunk, &c) == 0, "plat_caller_create");
    if (!g || !c) exit(1);
    plat_caller_options o;
    plat_caller_default_options(&o);
    o.assemble = k.assemble;
    const char* names[2] = {"S1", "S2"};
    char* text = nullptr;
    size_t len = 0;
    const int rc = plat_call_regions_stream(c, 6, k.samples, names, &o, plat_synth_load, g, nSlots, 2, &text, &len, nullptr);
    CHECK(rc == 0, "plat_call_regions_stream: %d (%s)", rc, plat_caller_last_error(c));
    *held = heapBytes();
    std::string out(text ? text : "", len);
    plat_caller_free(text);
    CHECK(plat_caller_destroy(c) == 0, "plat_caller_destroy");
    plat_synth_destroy(g);
    return out;
}

// sorted record lines of `bytes` bytes: chromosome 1, every `step`-th position from `first`
static std::string recordText(size_t bytes, long long first, long long step) {
    std::string t;
    t.reserve(bytes + 128);
    char line[128];
    for (long long pos = first; t.size() < bytes; pos += step) {
        const int n = snprintf(line, sizeof line, "1\t%lld\t.\tA\tC\t50\tPASS\tFR=0.5000;TC=30;TR=15\tGT:GL:GOF:GQ:NR:NV\t0/1:-30.0,0.0,-30.0:5:99:30:15\n", pos);
        t.append(line, (size_t)n);
    }
    return t;
}

// A text block of more than 8 MB, made while a caller exists and given back with plat_caller_free, is gone when the last caller is
static void textBlocks(bool blocks) {
    const std::string a = recordText((size_t)5 * MB, 2, 2), b = recordText((size_t)5 * MB, 1, 2);
    const long long before = heapBytes();
    plat_caller* c = nullptr;
    CHECK(plat_caller_create(0, 1, 1, &c) == 0, "plat_caller_create");
    char* out = nullptr;
    size_t len = 0;
    if (blocks) {                                                          // plat_merge_region_blocks: the allocation plat_call_regions makes for a text this large
        const char* src[2] = {a.data(), b.data()};
        const size_t l[2] = {a.size(), b.size()}, at[2] = {0, a.size()};
        len = a.size() + b.size();
        CHECK(plat_merge_region_blocks(2, src, l, at, len, &out) == 0, "plat_merge_region_blocks");
        CHECK(out && memcmp(out, a.data(), a.size()) == 0 && memcmp(out + a.size(), b.data(), b.size()) == 0 && out[len] == 0, "the blocks' bytes");
    } else {
        const char* texts[2] = {a.data(), b.data()};
        const size_t lens[2] = {a.size(), b.size()};
        CHECK(plat_merge_record_texts(texts, lens, 2, &out, &len) == 0, "plat_merge_record_texts");
        CHECK(len == a.size() + b.size() && out && strncmp(out, "1\t1\t", 4) == 0 && out[len] == 0, "the merged text: %zu bytes", len);
    }
    const long long held = heapBytes() - before;
    CHECK(len > (size_t)8 * MB && held > 8 * MB, "a block of more than 8 MB: %zu bytes of text, %lld held", len, held);
    plat_caller_free(out);
    CHECK(plat_caller_destroy(c) == 0, "plat_caller_destroy");
    const long long left = heapBytes() - before;
    printf("text %s: bytes %zu held %lld left %lld\n", blocks ? "blocks" : "records", len, held, left);
    CHECK(left <= SLACK && left >= -SLACK, "%lld bytes left after the last caller", left);
}

int main() {
    const Case cases[4] = {{1, PLAT_READS_PACKED, 0, 2, 2}, {2, PLAT_READS_ASCII, 0, 3, 1}, {2, PLAT_READS_PACKED, 1, 1, 4}, {1, PLAT_READS_ASCII, 1, 2, 3}};
    std::string first[4];
    for (int pass = 1; pass <= 2; ++pass)
        for (int k = 0; k < 4; ++k) {
            const long long before = heapBytes();
            long long held = 0;
            size_t lines = 0;
            {
                const std::string text = runCase(cases[k], &held);
                for (char ch : text) lines += ch == '\n';
                if (pass == 2) CHECK(text == first[k], "case %d: the second pass writes another text", k + 1);
                else first[k] = text;                                      // (kept: the first pass's balance is not looked at)
            }
            const long long left = heapBytes() - before;
            printf("case %d pass %d: lines %zu held %lld left %lld\n", k + 1, pass, lines, held - before, left);
            CHECK(lines > 60, "case %d: %zu record lines", k + 1, lines);
            CHECK(held - before >= 8 * MB, "case %d: %lld bytes live while the text is held", k + 1, held - before);
            if (pass == 2) CHECK(left <= SLACK && left >= -SLACK, "case %d: %lld bytes left after the caller", k + 1, left);
        }
    textBlocks(false);
    textBlocks(true);
    fflush(stdout);
    return g_bad ? 1 : 0;
}
