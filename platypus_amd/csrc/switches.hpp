// switches.hpp -- the PLAT_* environment switches of the device library (libplat_mi355x.so).  Host code only: no HIP header, nothing of
// plat_internal.hpp, so tests/device_switches_driver.cpp compiles it alone.  No .hip file calls getenv; every variable is parsed here.
//
// Two lifetimes:
//   per call     the entry point reads its own struct ONCE at the top and hands it down (align_impl -> align_seed_launch, asm_launch -> AsmParams,
//                plat_em_window_batch).  A variable set or cleared between two calls takes effect at the next call; inside one call -- the seeding's
//                retry included -- nothing changes.  One struct per entry point, so that no call reads a variable it does not use.
//   per process  plat_stream_sync is on every worker's wait path: SyncSwitches is read at the first wait of the process and kept.
//
//   variable               on when / value                  what it does                                                      who sets it                  read
//   AlignSwitches (plat_align_window_batch, plat_align_window_batch_async)
//   PLAT_NO_UNGAPPED       begins with '1'                  no ungapped-alignment shortcut: such pairs go through the DP      tests, bench.py              per call
//   PLAT_NO_EXACT          begins with '1'                  no exact-match shortcut: every reference DP is run                tests, bench.py              per call
//   PLAT_NO_NLOW           begins with '1'                  the ungapped proof counts every base as a low-quality one         tests, measurements          per call
//   PLAT_UNGAPPED_BIGQ     begins with '1'                  the ungapped proof takes reads of the wrap regime too             tools/ungapped_crosscheck.py per call
//   PLAT_SEED_XCD          not beginning '0'                the waves of a window / haplotype on one XCD ("0": w on wg w)     measurements                 per call
//   PLAT_SEED_ONE_DIAG     begins with '1'                  k_pairs proves on one diagonal by X < C, no neighbour pass (A/B)  tests, measurements          per call
//   PLAT_SLOW_GROUP        1..SLOW_GROUP, else 8            k_seed_slow: queue entries per workgroup round                    measurements                 per call
//   PLAT_SLOW_WAVES        1..SLOW_WAVES, else SLOW_WAVES   k_seed_slow: waves per workgroup (before the LDS rule halves it)  measurements                 per call
//   PLAT_SLOW_TIMING       set at all                       k_seed_slow's ticks per phase on stderr (waits for the stream)    measurements                 per call
//   PLAT_SEED_DEBUG        integer, bit 512 only            k_pairs counts why a pair reached the DP; printed with stats      measurements                 per call
//   PLAT_DP_GRID_PER_CU    integer > 0, else 8              k_dp_jobs: workgroups of the fixed grid per CU                    measurements                 per call (it was
//                                                                                                                                          once per process before this table)
//   PLAT_TB_SLAB           integer >= 256, else not given   traceback mode: jobs per slab of back-pointers, rounded up to a    tests                        per call
//                                                           multiple of 256, where that is less than what 6 GiB hold
//   AsmSwitches (plat_assemble_batch, plat_assemble_batch_async)
//   PLAT_ASM_TIMING        set at all                       k_assemble's ticks per phase on stderr (waits for the stream)     measurements                 per call
//   PLAT_ASM_DEBUG         integer, bits 4, 8 only          4: walks in the slice, 8: one-thread extraction (rare paths)      tests                        per call
//   PLAT_ASM_WG_PER_CU     integer > 0, else not given      workgroups per CU instead of the computed 1                       measurements                 per call
//   PLAT_ASM_NO_KEEP       set at all                       no workgroup keeps its scratch slice's signature                  tests                        per call
//   EmSwitches (plat_em_window_batch)
//   PLAT_EM_NARROW         set at all                       the one-wave kernel although the window fits k_em_wide            tests, measurements          per call
//   SyncSwitches (plat_stream_sync)
//   PLAT_SYNC_SPIN         begins with '1'                  hipStreamSynchronize, the runtime's own wait                      measurements                 per process
//   PLAT_SYNC_POLL_US      integer >= 0, else not given     poll interval in microseconds, wins over plat_sync_poll_us        measurements                 per process
//
// Retired, read by nothing (profiles/HISTORY.md, rounds 11 and 15, has what each measured): PLAT_DP_IMPL, PLAT_DP_TILES, PLAT_ASM_STATIC,
// PLAT_ASM_FUSED, bit 256 of PLAT_SEED_DEBUG, and bits 1, 2 of PLAT_ASM_DEBUG.  -DPLAT_ASM_SECTIONS is a build flag, not a variable.
#pragma once
#include <cstdlib>
#include <ctime>

namespace plat {

constexpr int SLOW_WAVES = 4, SLOW_GROUP = 32;             // k_seed_slow: waves per workgroup, and the most queue entries a workgroup takes per round

namespace env {
inline bool isSet(const char* name) { return getenv(name) != nullptr; }
inline bool isOne(const char* name) { const char* e = getenv(name); return e && e[0] == '1'; }
inline bool notZero(const char* name) { const char* e = getenv(name); return !(e && e[0] == '0'); }
inline int number(const char* name, int unset) { const char* e = getenv(name); return e ? atoi(e) : unset; }
}  // namespace env

struct AlignSwitches {
    bool noUngapped = false, noExact = false, noNlow = false, ungappedBigq = false, seedXcd = true, slowTiming = false, seedOneDiag = false;
    int slowGroup = 8, slowWaves = SLOW_WAVES, seedDebug = 0, dpGridPerCu = 8;
    long long tbSlab = 0;                                  // 0: not given (the 6 GiB rule holds)

    static AlignSwitches read() {
        AlignSwitches w;
        w.noUngapped = env::isOne("PLAT_NO_UNGAPPED");
        w.noExact = env::isOne("PLAT_NO_EXACT");
        w.noNlow = env::isOne("PLAT_NO_NLOW");
        w.ungappedBigq = env::isOne("PLAT_UNGAPPED_BIGQ");
        w.seedXcd = env::notZero("PLAT_SEED_XCD");
        w.slowTiming = env::isSet("PLAT_SLOW_TIMING");
        w.seedOneDiag = env::isOne("PLAT_SEED_ONE_DIAG");
        { const int v = env::number("PLAT_SLOW_GROUP", 0); if (v > 0 && v <= SLOW_GROUP) w.slowGroup = v; }
        { const int v = env::number("PLAT_SLOW_WAVES", 0); if (v > 0 && v <= SLOW_WAVES) w.slowWaves = v; }
        w.seedDebug = env::number("PLAT_SEED_DEBUG", 0) & 0x200;
        { const int v = env::number("PLAT_DP_GRID_PER_CU", 0); if (v > 0) w.dpGridPerCu = v; }
        { const int v = env::number("PLAT_TB_SLAB", 0); if (v >= 256) w.tbSlab = ((long long)v + 255) & ~255ll; }
        return w;
    }
};

struct AsmSwitches {
    bool timing = false, noKeep = false;
    int debug = 0, wgPerCu = 0;                            // wgPerCu 0: not given

    static AsmSwitches read() {
        AsmSwitches w;
        w.timing = env::isSet("PLAT_ASM_TIMING");
        w.debug = env::number("PLAT_ASM_DEBUG", 0) & 12;
        { const int v = env::number("PLAT_ASM_WG_PER_CU", 0); if (v > 0) w.wgPerCu = v; }
        w.noKeep = env::isSet("PLAT_ASM_NO_KEEP");
        return w;
    }
};

struct EmSwitches {
    bool narrow = false;

    static EmSwitches read() { EmSwitches w; w.narrow = env::isSet("PLAT_EM_NARROW"); return w; }
};

struct SyncSwitches {
    bool spin = false;
    long pollNs = -1;                                      // -1: not given (the context's own interval holds)

    static SyncSwitches read() {
        SyncSwitches w;
        w.spin = env::isOne("PLAT_SYNC_SPIN");
        { const char* e = getenv("PLAT_SYNC_POLL_US"); const long v = e ? atol(e) : -1; w.pollNs = v < 0 ? -1L : v * 1000L; }
        return w;
    }
};

// A poll interval as nanosleep takes it: tv_nsec stays below a second (an interval of a second or more in tv_nsec alone is EINVAL, and the
// wait that was to sleep spins).
inline timespec poll_timespec(long poll_ns) {
    timespec ts;
    ts.tv_sec = (time_t)(poll_ns / 1000000000L);
    ts.tv_nsec = poll_ns % 1000000000L;
    return ts;
}

}  // namespace plat
