"""The `callVariants` command-line surface of the reference (option names, dests and defaults of
src/python/runner.py:519-597), kept so that scripts driving Platypus keep working.

Only the options that reach the hot path are interpreted by this package (rlen/maxReadLength,
calculateFlankScore, HLATyping, the assembly and QC thresholds, nCPU -> number of GPU ranks); the others are
accepted, stored on the options object and ignored here (their consumers are outside the hot-path scope,
SURVEY.md 2.1).

With --bamFiles AND --refFile and no --synthetic the files themselves are read (platypus_amd.__main__.call_variants_bam_files,
include/platypus_caller_bamfile.h): --bamFiles, --regions (None, or a list of chr / chr:start-end; region files are refused),
--bufferSize, --refFile, --source, --output and --outputIndex are then interpreted as well."""
import argparse

# (flag, dest, type, default)  -- facts of the reference's CLI, no help texts
CALL_VARIANTS_OPTIONS = [
    ("--output", "output", str, "AllVariants.vcf"), ("--refFile", "refFile", str, None),
    ("--regions", "regions", "list", None), ("--skipRegionsFile", "skipRegionsFile", str, None),
    ("--bamFiles", "bamFiles", "list", None), ("--bufferSize", "bufferSize", int, 100000),
    ("--minReads", "minReads", int, 2), ("--maxReads", "maxReads", float, 5000000),
    ("--verbosity", "verbosity", int, 2), ("--maxReadLength", "rlen", int, 150),
    ("--logFileName", "logFileName", str, "log.txt"), ("--source", "sourceFile", "list", None),
    ("--nCPU", "nCPU", int, 1), ("--parseNCBI", "parseNCBI", int, 0), ("--longHaps", "longHaps", int, 0),
    ("--alignScoreFile", "alignScoreFile", str, ""), ("--HLATyping", "HLATyping", int, 0),
    ("--compressReads", "compressReads", int, 0), ("--qualBinSize", "qualBinSize", int, 1),
    ("--fileCaching", "fileCaching", int, 0),
    ("--maxSize", "maxSize", int, 1500), ("--largeWindows", "largeWindows", int, 0),
    ("--maxVariants", "maxVariants", int, 8), ("--coverageSamplingLevel", "coverageSamplingLevel", int, 30),
    ("--maxHaplotypes", "maxHaplotypes", int, 50), ("--skipDifficultWindows", "skipDifficultWindows", int, 0),
    ("--getVariantsFromBAMs", "getVariantsFromBAMs", int, 1), ("--genSNPs", "genSNPs", int, 1),
    ("--genIndels", "genIndels", int, 1), ("--mergeClusteredVariants", "mergeClusteredVariants", int, 1),
    ("--minFlank", "minFlank", int, 10), ("--trimReadFlank", "trimReadFlank", int, 0),
    ("--filterVarsByCoverage", "filterVarsByCoverage", int, 1), ("--filteredReadsFrac", "filteredReadsFrac", float, 0.7),
    ("--maxVarDist", "maxVarDist", int, 15), ("--minVarDist", "minVarDist", int, 9),
    ("--useEMLikelihoods", "useEMLikelihoods", int, 0),
    ("--countOnlyExactIndelMatches", "countOnlyExactIndelMatches", int, 0),
    ("--calculateFlankScore", "calculateFlankScore", int, 0),
    ("--assemble", "assemble", int, 0), ("--assembleAll", "assembleAll", int, 1),
    ("--assemblyRegionSize", "assemblyRegionSize", int, 1500), ("--assembleBadReads", "assembleBadReads", int, 1),
    ("--assemblerKmerSize", "assemblerKmerSize", int, 15), ("--assembleBrokenPairs", "assembleBrokenPairs", int, 0),
    ("--noCycles", "noCycles", int, 0),
    ("--minMapQual", "minMapQual", int, 20), ("--minBaseQual", "minBaseQual", int, 20),
    ("--minGoodQualBases", "minGoodQualBases", int, 20), ("--filterDuplicates", "filterDuplicates", int, 1),
    ("--filterReadsWithUnmappedMates", "filterReadsWithUnmappedMates", int, 1),
    ("--filterReadsWithDistantMates", "filterReadsWithDistantMates", int, 1),
    ("--filterReadPairsWithSmallInserts", "filterReadPairsWithSmallInserts", int, 1),
    ("--trimOverlapping", "trimOverlapping", int, 1), ("--trimAdapter", "trimAdapter", int, 1),
    ("--trimSoftClipped", "trimSoftClipped", int, 1),
    ("--maxGOF", "maxGOF", int, 30), ("--minPosterior", "minPosterior", int, 5),
    ("--sbThreshold", "sbThreshold", float, 1e-3), ("--scThreshold", "scThreshold", float, 0.95),
    ("--abThreshold", "abThreshold", float, 1e-3), ("--minVarFreq", "minVarFreq", float, 0.05),
    ("--badReadsWindow", "badReadsWindow", int, 11), ("--badReadsThreshold", "badReadsThreshold", int, 15),
    ("--rmsmqThreshold", "rmsmqThreshold", int, 40), ("--qdThreshold", "qdThreshold", int, 10),
    ("--hapScoreThreshold", "hapScoreThreshold", int, 4),
    ("--outputRefCalls", "outputRefCalls", int, 0), ("--refCallBlockSize", "refCallBlockSize", int, 1000),
]


SOURCE_HELP = ("FILE[,FILE]: VCF file(s) of known alleles to genotype next to (or, with --getVariantsFromBAMs=0, instead of) the candidates from the "
               "reads.  With --synthetic=config4:N: when EVERY file is bgzipped and has a tabix index FILE.tbi next to it, the index is read, the "
               "chunks of each region's fetch are cut out of the file and handed to the library as BGZF blocks, which inflates and iterates them on "
               "the device as tabix does (include/platypus_caller_tabix.h).  Otherwise the files are read as plain or gzip/bgzip text and every "
               "region is handed the data lines whose "
               "[POS-1, POS-1+len(REF)) overlaps it: this is the CLI's OWN STAND-IN for a tabix fetch (no .tbi index is read); an integrator hands "
               "the library the lines its tabix fetch returned (include/platypus_caller_source.h).  The stand-in cannot place a line without five columns "
               "or with a POS that is no number and LEAVES IT OUT; the library, handed such a line, ends the call with an error that names it.  "
               "--longHaps is honoured.")


REF_HELP = ("FILE: the reference FASTA; its index is read from FILE.fai.  With --synthetic=config4:N the regions' contigs are taken from FILE instead of from "
            "the generator: the file is mapped, the index parsed on the host and the sequence fetched on the device by the reference's own line "
            "arithmetic (include/platypus_caller_fasta.h) -- whole contigs for the native region loop (contig_seq and dev_contig_seq), "
            "getSequence / getCharacter through hostapi.IndexedFastaFile for the Python loop.  A region whose contig the index lacks ends the run "
            "with the reference's message.  bgzipped FASTA is not read.  Without --synthetic=config4 the option is parsed and not used; without "
            "--refFile nothing changes.")


BAM_HELP = ("FILE[,FILE]: BAM files, each with its index FILE.bai (or FILE without .bam plus .bai) next to it.  Read only together with --refFile and "
            "without --synthetic: the files are mapped, samples come from the @RG header lines as the reference reads them (one sample per file, or "
            "files split by read group on the device), regions from --regions (a list of chr or chr:start-end; by default the header's @SQ lines), "
            "cut at --bufferSize; every region's reads are fetched through the .bai, inflated and decoded on the device "
            "(include/platypus_caller_bamfile.h).  Region files (.txt / .bed), CRAM, CSI indexes and --assembleBrokenPairs=1 with --assemble=1 are "
            "refused.  Without --refFile the option is parsed and not used.")


def _list(s):
    return s.split(",")


def build_parser():
    p = argparse.ArgumentParser(prog="Platypus.py callVariants", allow_abbrev=False)
    for flag, dest, typ, default in CALL_VARIANTS_OPTIONS:
        p.add_argument(flag, *(["-o"] if flag == "--output" else []), dest=dest,
                       type=_list if typ == "list" else typ, default=default, **({"help": {"--source": SOURCE_HELP, "--refFile": REF_HELP, "--bamFiles": BAM_HELP}[flag]} if flag in ("--source", "--refFile", "--bamFiles") else {}))
    p.add_argument("--synthetic", dest="synthetic", type=str, default=None,
                   help="(this build) run the hot path on a synthetic BASELINE config instead of BAM input: config1|config2[:N]|config5[:N]")
    p.add_argument("--outputIndex", dest="outputIndex", type=int, default=0,
                   help="(this build) 1: with an --output name that ends in .gz, also write OUTPUT.tbi, the tabix index of the file, built on the "
                        "device from the bytes just written (include/platypus_caller_tbi.h), so that --source can take the file as it is")
    return p


def default_options(**overrides):
    """An options object carrying the reference's defaults (what `options` is inside the reference)."""
    ns = build_parser().parse_args([])
    for k, v in overrides.items():
        if not hasattr(ns, k):
            raise AttributeError("unknown Platypus option %r" % k)
        setattr(ns, k, v)
    ns.originalMaxHaplotypes = ns.maxHaplotypes          # set once per process by the reference, variantcaller.pyx:920
    return ns
