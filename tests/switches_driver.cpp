// switches_driver.cpp -- a stand-alone program over platypus_amd/csrc/host/switches.hpp (tests/test_native_caller_cpu.py): for every
// PLAT_CALLER_* switch, what Switches::read() makes of the variable unset and set to "", "0", "1" and "yes", every other variable unset.
// One line per (variable, spelling): "<NAME> <spelling>: field=0|1 ...", every field of the struct.
#include "host/switches.hpp"

#include <cstdio>

static void show(const char* name, const char* spelling) {
    const plathost::Switches w = plathost::Switches::read();
    printf("%s %s: noCodes=%d expand=%d hostTally=%d hostB=%d noDeviceReplay=%d hostInfo=%d firstOccurrenceOrder=%d evenTail=%d keepSpare=%d checkHints=%d "
           "noRefCtx=%d noRefPrefetch=%d trace=%d traceStages=%d\n", name, spelling, w.noCodes, w.expand, w.hostTally, w.hostB, w.noDeviceReplay, w.hostInfo, w.firstOccurrenceOrder,
           w.evenTail, w.keepSpare, w.checkHints, w.noRefCtx, w.noRefPrefetch, w.trace, w.traceStages);
}

int main() {
    const char* names[] = {"NO_CODES", "EXPAND", "HOST_TALLY", "HOST_B", "NO_DEVICE_REPLAY", "HOST_INFO", "FIRST_OCCURRENCE_ORDER", "EVEN_TAIL", "KEEP_SPARE",
                           "CHECK_HINTS", "NO_REFCTX", "NO_REFPREFETCH", "TRACE"};
    const char* spellings[] = {"", "0", "1", "yes"};
    char var[64];
    for (const char* n : names) { snprintf(var, sizeof var, "PLAT_CALLER_%s", n); unsetenv(var); }
    for (const char* n : names) {
        snprintf(var, sizeof var, "PLAT_CALLER_%s", n);
        unsetenv(var);
        show(n, "unset");
        for (const char* s : spellings) {
            setenv(var, s, 1);
            show(n, s[0] ? s : "empty");
        }
        unsetenv(var);
    }
    return 0;
}
