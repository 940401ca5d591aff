// device_switches_driver.cpp -- a stand-alone program over platypus_amd/csrc/switches.hpp alone (tests/test_native_caller_cpu.py): for every PLAT_*
// switch of the device library, what the four read()s make of the variable unset and set to each spelling below, every other variable unset.
// One line per (variable, spelling): "<NAME> <spelling>: field=value ...", every field of the four structs.  Then one line with the retired
// variables set ("RETIRED set: ..."), and one per poll interval: "poll <microseconds>: sec=... nsec=...".
#include "switches.hpp"

#include <cstdio>

static void show(const char* name, const char* spelling) {
    const plat::AlignSwitches a = plat::AlignSwitches::read();
    const plat::AsmSwitches s = plat::AsmSwitches::read();
    const plat::EmSwitches e = plat::EmSwitches::read();
    const plat::SyncSwitches y = plat::SyncSwitches::read();
    printf("%s %s: noUngapped=%d noExact=%d noNlow=%d ungappedBigq=%d seedXcd=%d slowGroup=%d slowWaves=%d slowTiming=%d seedDebug=%d dpGridPerCu=%d tbSlab=%lld "
           "asmTiming=%d asmDebug=%d asmWgPerCu=%d asmNoKeep=%d emNarrow=%d syncSpin=%d syncPollNs=%ld\n", name, spelling,
           a.noUngapped, a.noExact, a.noNlow, a.ungappedBigq, a.seedXcd, a.slowGroup, a.slowWaves, a.slowTiming, a.seedDebug, a.dpGridPerCu, a.tbSlab,
           s.timing, s.debug, s.wgPerCu, s.noKeep, e.narrow, y.spin, y.pollNs);
}

int main() {
    const char* names[] = {"PLAT_NO_UNGAPPED", "PLAT_NO_EXACT", "PLAT_NO_NLOW", "PLAT_UNGAPPED_BIGQ", "PLAT_SEED_XCD", "PLAT_SLOW_GROUP", "PLAT_SLOW_WAVES",
                           "PLAT_SLOW_TIMING", "PLAT_SEED_DEBUG", "PLAT_DP_GRID_PER_CU", "PLAT_TB_SLAB", "PLAT_ASM_TIMING", "PLAT_ASM_DEBUG",
                           "PLAT_ASM_WG_PER_CU", "PLAT_ASM_NO_KEEP", "PLAT_EM_NARROW", "PLAT_SYNC_SPIN", "PLAT_SYNC_POLL_US"};
    const char* retired[][2] = {{"PLAT_DP_IMPL", "unpacked"}, {"PLAT_DP_TILES", "1"}, {"PLAT_ASM_STATIC", "1"}, {"PLAT_ASM_FUSED", "0"}};
    const char* spellings[] = {"", "0", "1", "yes", "7", "-3", "33", "2000000", "512", "256", "768", "255", "257"};
    for (const char* n : names) unsetenv(n);
    for (const auto& r : retired) unsetenv(r[0]);
    for (const char* n : names) {
        show(n, "unset");
        for (const char* s : spellings) {
            setenv(n, s, 1);
            show(n, s[0] ? s : "empty");
        }
        unsetenv(n);
    }
    for (const auto& r : retired) setenv(r[0], r[1], 1);
    show("RETIRED", "set");
    const long intervals[] = {0L, 40L, 999999L, 1000000L, 2000000L};
    for (const long us : intervals) {
        const timespec ts = plat::poll_timespec(us * 1000L);
        printf("poll %ld: sec=%lld nsec=%ld\n", us, (long long)ts.tv_sec, (long)ts.tv_nsec);
    }
    return 0;
}
