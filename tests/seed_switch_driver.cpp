// seed_switch_driver.cpp -- a stand-alone program over platypus_amd/csrc/switches.hpp alone (tests/test_seed_bound_cpu.py): what AlignSwitches::read()
// makes of PLAT_SEED_ONE_DIAG unset and set to each spelling below, every other variable unset ("PLAT_SEED_ONE_DIAG <spelling>: field=value ..."),
// then with every OTHER variable of AlignSwitches set to "1" and this one unset ("OTHERS 1: ...").
#include "switches.hpp"

#include <cstdio>

static void show(const char* name, const char* spelling) {
    const plat::AlignSwitches a = plat::AlignSwitches::read();
    printf("%s %s: noUngapped=%d noExact=%d noNlow=%d ungappedBigq=%d seedXcd=%d slowGroup=%d slowWaves=%d slowTiming=%d seedDebug=%d dpGridPerCu=%d "
           "seedOneDiag=%d\n", name, spelling, a.noUngapped, a.noExact, a.noNlow, a.ungappedBigq, a.seedXcd, a.slowGroup, a.slowWaves, a.slowTiming,
           a.seedDebug, a.dpGridPerCu, a.seedOneDiag);
}

int main() {
    const char* others[] = {"PLAT_NO_UNGAPPED", "PLAT_NO_EXACT", "PLAT_NO_NLOW", "PLAT_UNGAPPED_BIGQ", "PLAT_SEED_XCD", "PLAT_SLOW_GROUP", "PLAT_SLOW_WAVES",
                            "PLAT_SLOW_TIMING", "PLAT_SEED_DEBUG", "PLAT_DP_GRID_PER_CU"};
    const char* spellings[] = {"", "0", "1", "yes", "7", "-3", "10", "1x", "01", "true"};
    const char* name = "PLAT_SEED_ONE_DIAG";
    for (const char* n : others) unsetenv(n);
    unsetenv(name);
    show(name, "unset");
    for (const char* s : spellings) {
        setenv(name, s, 1);
        show(name, s[0] ? s : "empty");
    }
    unsetenv(name);
    for (const char* n : others) setenv(n, "1", 1);
    show("OTHERS", "1");
    return 0;
}
