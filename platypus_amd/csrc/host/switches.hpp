// switches.hpp -- the PLAT_CALLER_* environment switches of the native region loop (libplat_caller.so), read ONCE PER CALL:
// the region loop behind plat_call_regions (callRegions) and plat_call_regions_stream call Switches::read() at entry (the fetched / BAM / BGZF /
// read-group front ends end in callRegions and read nothing themselves: front_end.hpp) and the result travels in Options.  A variable set or cleared between two calls takes effect at the next call;
// inside one call nothing changes.  None of them changes the record text (FIRST_OCCURRENCE_ORDER excepted: that is what it is there to show).
//
//   variable (PLAT_CALLER_...)   on when            what it does                                                          who sets it
//   NO_CODES                     set at all         the candidate scan on bytes: no 2-bit codes, the chunk is expanded    tests, measurements
//   EXPAND                       set at all         packed chunks are expanded (bytes + codes), not read where they lie   tests, measurements (the A/B baseline)
//   HOST_TALLY                   set at all         the scan's records are merged on the host, stage B runs there         tests, measurements
//   HOST_B                       begins with '1'    stage B on the host although the chunk is eligible for the device     tests, measurements
//   NO_DEVICE_REPLAY             set at all         device stage B gets no records to replay the dictionaries from        tests (the replay matters)
//   HOST_INFO                    set at all         the ABPV / SbPval / MMLQ loops on the host                            measurements
//   FIRST_OCCURRENCE_ORDER       set at all         host stage B never replays the dictionaries                           tests (the replay matters)
//   NO_REFCTX                    begins with '1'    device stage B's variants carry no reference context: HP, SC and     tests, measurements (the A/B baseline)
//                                                   the SNP REF read the reference itself, nothing is prefetched
//   NO_REFPREFETCH               begins with '1'    the context is copied but no reference line is asked for ahead       measurements (what the prefetch alone is worth)
//   EVEN_TAIL                    not beginning '0'  the last round of chunks is cut into equal parts, one per worker      measurements ("0": whole chunks to the end)
//   KEEP_SPARE                   begins with '1'    a worker keeps its spare window storage for the next call             measurements (slower: region_caller.cpp)
//   CHECK_HINTS                  begins with '1'    plat_read_table.longest_read / most_bases are checked against a walk  tests, a loader under suspicion
//   HOST_SOURCE                  begins with '1'    source VCF lines are parsed by the host parser, not on the device      tests, measurements (the kernel's A/B)
//   HOST_REFCOV                  begins with '1'    REFCALL read counts by the host's per-position loop, not on the device   tests, measurements (the kernel's A/B)
//   HOST_TABIX                   begins with '1'    plat_caller_set_source_blocks inflates and walks on the host           tests, measurements (the kernels' A/B);
//                                                                                                                         read when that entry point is called
//   HOST_DEFLATE                 begins with '1'    plat_caller_compress_text deflates on the host (csrc/bgzf_deflate.hpp)   tests, measurements (the kernels' A/B);
//                                                                                                                         read when that entry point is called
//   HOST_TBI                     begins with '1'    plat_caller_index_bgzf inflates and indexes on the host (csrc/tabix_index.hpp)   tests, measurements (the kernels' A/B);
//                                                                                                                         read when that entry point is called
//   HOST_INDEX                   begins with '1'    plat_index_query and plat_caller_set_source_files answer every index query with the host twin (csrc/index_query.hpp)   tests, measurements (the kernels' A/B);
//                                                                                                                         read when those entry points are called
//   HOST_FASTA                   begins with '1'    plat_fasta_load, plat_fasta_contig and plat_fasta_get_sequences answer with the host twin (csrc/fasta_rule.hpp)   tests, measurements (the kernels' A/B);
//                                                                                                                         read when those entry points are called
//   TRACE                        set at all         per-chunk / per-call lines on stderr;                                 measurements
//                                begins with '1'    ... and the per-stage seconds of every call (traceStages)
// PLAT_CALLER_POLL_US is not here: it is a property of the caller object and is read where that is made (plat_caller_create).
#pragma once
#include <cstdlib>
#include <cstring>

namespace plathost {

struct Switches {
    bool noCodes = false, expand = false, hostTally = false, hostB = false, noDeviceReplay = false, hostInfo = false, firstOccurrenceOrder = false;
    bool evenTail = true, keepSpare = false, checkHints = false, noRefCtx = false, noRefPrefetch = false, hostSource = false, hostRefcov = false, hostTabix = false, hostDeflate = false, hostTbi = false, hostIndex = false, hostFasta = false;
    bool trace = false, traceStages = false;                              // PLAT_CALLER_TRACE: set at all / begins with '1'

    static Switches read() {
        auto isSet = [](const char* name) { return getenv(name) != nullptr; };
        auto isOne = [](const char* name) { const char* e = getenv(name); return e && e[0] == '1'; };
        Switches w;
        w.noCodes = isSet("PLAT_CALLER_NO_CODES");
        w.expand = isSet("PLAT_CALLER_EXPAND");
        w.hostTally = isSet("PLAT_CALLER_HOST_TALLY");
        w.hostB = isOne("PLAT_CALLER_HOST_B");
        w.noDeviceReplay = isSet("PLAT_CALLER_NO_DEVICE_REPLAY");
        w.hostInfo = isSet("PLAT_CALLER_HOST_INFO");
        w.firstOccurrenceOrder = isSet("PLAT_CALLER_FIRST_OCCURRENCE_ORDER");
        { const char* e = getenv("PLAT_CALLER_EVEN_TAIL"); w.evenTail = !(e && e[0] == '0'); }
        w.noRefCtx = isOne("PLAT_CALLER_NO_REFCTX");
        w.noRefPrefetch = isOne("PLAT_CALLER_NO_REFPREFETCH");
        w.keepSpare = isOne("PLAT_CALLER_KEEP_SPARE");
        w.checkHints = isOne("PLAT_CALLER_CHECK_HINTS");
        w.hostSource = isOne("PLAT_CALLER_HOST_SOURCE");
        w.hostRefcov = isOne("PLAT_CALLER_HOST_REFCOV");
        w.hostTabix = isOne("PLAT_CALLER_HOST_TABIX");
        w.hostDeflate = isOne("PLAT_CALLER_HOST_DEFLATE");
        w.hostTbi = isOne("PLAT_CALLER_HOST_TBI");
        w.hostIndex = isOne("PLAT_CALLER_HOST_INDEX");
        w.hostFasta = isOne("PLAT_CALLER_HOST_FASTA");
        w.trace = isSet("PLAT_CALLER_TRACE");
        w.traceStages = isOne("PLAT_CALLER_TRACE");
        return w;
    }
};

}  // namespace plathost
