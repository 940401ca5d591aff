"""`python -m platypus_amd callVariants ...` -- the reference's entry point name (Platypus.py:23-46).

With `--bamFiles F[,F]` AND `--refFile R` (and no `--synthetic`) the files themselves are read (call_variants_bam_files,
include/platypus_caller_bamfile.h): header, samples, regions, the .bai fetch and the records on the device, the contigs from R.  CRAM, the
rest of htslib's I/O and `--bamFiles` without `--refFile` stay outside this build; there the command explains that
instead of silently doing something else.  With `--synthetic=config4:N`, `--refFile FILE` takes the regions' contigs from FILE and
FILE.fai, fetched on the device (include/platypus_caller_fasta.h)."""
import json
import sys

from .options import build_parser


def call_variants(argv):
    opts = build_parser().parse_args(argv)
    if opts.HLATyping:
        sys.exit("platypus_amd: --HLATyping=1 (useMapQualCap) is not implemented on the device path")
    if opts.outputIndex and not opts.output.endswith(".gz"):
        sys.exit("platypus_amd: --outputIndex=1 indexes a compressed output: give --output a name that ends in .gz")
    if opts.synthetic is None and opts.bamFiles and opts.refFile:
        return call_variants_bam_files(opts)
    if opts.synthetic is None:
        sys.exit("platypus_amd: BAM/FASTA input needs the reference's htslib I/O layer, which is outside this build's "
                 "scope (see DESIGN.md, 'out of scope').  Use --synthetic=config2[:N] or the in-memory API "
                 "(platypus_amd.hostapi / include/platypus_mi355x.h).")
    from . import synth
    from .engine import Engine
    name, _, n = opts.synthetic.partition(":")
    if name == "config4":
        return call_variants_config4(opts, int(n or 8))
    hb = {"config1": lambda: synth.config1(), "config2": lambda: synth.config2(int(n or 10000)),
          "config5": lambda: synth.config5(int(n or 200), 100)}[name]()
    from . import sharding
    eng = Engine(0)
    db = eng.upload(hb)
    st = eng.align(db, calc_flank_score=int(opts.calculateFlankScore))      # Haplotype.alignReads for every haplotype
    eng.genotype(db)                                                         # Population.setup
    eng.em(db, 100, int(opts.useEMLikelihoods))                              # Population.call: EM + callGenotypes
    eng.synchronize()
    # per-window records (the VCF writer is outside this build's scope): chrom, window start, #haplotypes, genotype
    # log-likelihoods, then EM haplotype frequencies and the called genotype index per sample
    recs = sharding.format_window_records(hb, db.logl.cpu().numpy())
    freq, calls = db.freq.cpu().numpy(), db.calls.cpu().numpy().reshape(hb.n_windows, hb.n_ind)
    with open(opts.output, "w") as f:
        for w, (chrom, pos, line) in enumerate(recs):
            fr = ",".join("%.4f" % v for v in freq[hb.win_hap_begin[w]:hb.win_hap_begin[w + 1]])
            f.write("%s\t%s\t%s\n" % (line, fr, ",".join(str(int(c)) for c in calls[w])))
    print(json.dumps(dict(windows=hb.n_windows, pairs=int(st.n_pairs), dp_reference=int(st.n_dp_reference),
                          dp_launched=int(st.n_dp_launched), output=opts.output)))


def read_source_lines(path):
    """The data lines of a plain or gzip / bgzip-compressed VCF (Python's gzip reads both), as a list of bytes."""
    import gzip
    with open(path, "rb") as f:
        magic = f.read(2)
    with (gzip.open(path, "rb") if magic == b"\x1f\x8b" else open(path, "rb")) as f:
        return [ln.rstrip(b"\r\n") for ln in f if ln.strip() and not ln.startswith(b"#")]


def write_output(opts, sample_names, merged, local_rank=0):
    """The VCF header for `sample_names` and the merged record lines to --output: plain text, or -- for a name that ends in .gz -- BGZF
    deflated on the device, with its tabix index under --outputIndex=1."""
    import datetime
    import io
    from .vcfrecords import VCF
    vcf = VCF(list(sample_names))
    vcf.setheader([("fileDate", datetime.date.today()), ("source", "platypus_amd (records as Platypus_Version_0.8.1.1 writes them)"),
                   ("platypusOptions", str(dict(sorted((k, v) for k, v in vars(opts).items() if k != "outputIndex" or v))))])         # variantcaller.pyx:51,942
    if opts.output.endswith(".gz"):
        # as the reference's filez.Open does for .gz names (variantcaller.pyx:951-956), as BGZF: the header's block(s), the merged
        # records', the EOF block -- deflated on the device (include/platypus_caller_bgzfout.h)
        from . import fastcaller as F
        import torch
        head = io.StringIO()
        vcf.writeheader(head)
        parts = [head.getvalue().encode(), "".join(line + "\n" for line in merged).encode()]
        zc = F.NativeCaller(local_rank % max(1, torch.cuda.device_count()), 1, 1)
        try:
            packed, _ = zc.compress_text(b"".join(parts), [len(p) for p in parts], level=1, eof=True)
            with open(opts.output, "wb") as f:
                f.write(packed)
            if opts.outputIndex:
                # the index tabix would build of the file, from the bytes just written (include/platypus_caller_tbi.h)
                with open(opts.output + ".tbi", "wb") as f:
                    f.write(zc.index_bgzf(packed))
        finally:
            zc.close()
    else:
        with open(opts.output, "w") as f:
            vcf.writeheader(f)
            f.write("".join(line + "\n" for line in merged))


def bam_regions(header_sq, fai_refs, asked, buffer_size):
    """The region list of getRegions (platypusutils.pyx:999-1085) for --regions=None or a list of chr / chr:start-end.  header_sq: the
    (SN, LN) pairs of the first BAM file's @SQ lines, None where reading them raises (NativeBamFile.header_sq); fai_refs: (name, length)
    of the FASTA index in file order -- where the reference falls back to ALL of them it walks a dict, whose order is Python 2's; file
    order is this build's choice there.  Returns [(chrom, start, end)]."""
    lengths = dict(fai_refs)
    regions = []
    if asked is None:
        regions = [(n, 0, l) for n, l in (header_sq if header_sq is not None else fai_refs)]
    else:
        for region in asked:
            split = region.rsplit(":", 1)
            chrom = split[0]
            if len(split) == 2:
                start, end = split[1].split("-")
                regions.append((chrom, int(start) - 1, int(end)))
                if regions[-1][2] - regions[-1][1] > 1e9:
                    raise ValueError("Invalid input region: %s" % region)
            elif header_sq is not None and chrom in dict(header_sq):
                regions.append((chrom, 0, dict(header_sq)[chrom]))
            else:
                regions = [(n, 0, l) for n, l in fai_refs if n == chrom]          # (the reference's list starts over here, :1033)
    final = []
    for chrom, start, end in regions:
        if chrom not in lengths or start > lengths[chrom]:
            continue
        if end - start > buffer_size:
            final.extend((chrom, i, min(i + buffer_size, end)) for i in range(start, end, buffer_size))
        else:
            final.append((chrom, start, end))
    return final


def call_variants_bam_files(opts):
    """--bamFiles with --refFile: whole BAM files through the native region loop (include/platypus_caller_bamfile.h).  Every file and its
    .bai (FILE.bai, else FILE without .bam plus .bai) and the FASTA are mapped; samples and mode are the library's plan, the regions
    getRegions' (bam_regions), the contigs the FASTA's, fetched on the device; header and merged records go through write_output."""
    import mmap
    import os
    import time
    import numpy as np
    import torch
    from . import fastcaller as F, sharding
    if opts.regions is not None and os.path.exists(opts.regions[0]):
        sys.exit("platypus_amd: --regions=%s names a file; region files (.txt / .bed) are not read: give a list of chr or chr:start-end" % opts.regions[0])
    if opts.skipRegionsFile:
        sys.exit("platypus_amd: --skipRegionsFile is not read")
    opts.originalMaxHaplotypes = opts.maxHaplotypes
    nc = F.NativeCaller(int(os.environ.get("LOCAL_RANK", 0)) % max(1, torch.cuda.device_count()), int(os.environ.get("PLAT_CALLER_WORKERS", "8")),
                        int(os.environ.get("PLAT_CALLER_CHUNK", "4")))
    maps, files, ref_file = [], [], None

    def mapped(path):
        with open(path, "rb") as f:
            if os.fstat(f.fileno()).st_size == 0:
                return np.zeros(0, dtype=np.uint8)
            maps.append(mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ))
        return np.frombuffer(maps[-1], dtype=np.uint8)
    try:
        for name in opts.bamFiles:
            if not name.lower().endswith(".bam"):
                sys.exit("platypus_amd: input file %s is not a BAM file (CRAM and text files of file names are not read)" % name)
            bai = name + ".bai" if os.path.exists(name + ".bai") else name[:-4] + ".bai"
            with open(bai, "rb") as f:
                files.append(nc.open_bam(mapped(name), f.read(), name))
        with open(opts.refFile + ".fai", "rb") as f:
            ref_file = nc.open_fasta(mapped(opts.refFile), f.read(), int(opts.parseNCBI))
        plan = nc.bam_plan(files)
        sq = files[0].header_sq
        regions = bam_regions(None if sq is None else [(n.decode(), l) for n, l in sq], [(r[0].decode(), r[1]) for r in ref_file.refs], opts.regions,
                              int(opts.bufferSize))
        tids = [ref_file.tid(c) for c, _, _ in regions]
        if tids:
            ref_file.load(sorted(set(tids)))
        rr = [F.FastaContigRegion(F.BamFilesRegion(c, s, e, b""), ref_file, t) for (c, s, e), t in zip(regions, tids)]
        t0 = time.time()
        source = None
        if opts.sourceFile:
            source = []
            for f in opts.sourceFile:
                with open(f, "rb") as data, open(f + ".tbi", "rb") as tbi:
                    source.append((data.read(), nc.open_index(tbi.read(), "tbi")))
        # (--assemble 1 with --assembleBrokenPairs 1: the mates of improper pairs are fetched too; every other combination is call_bam_files)
        mates = int(getattr(opts, "assemble", 0)) and int(getattr(opts, "assembleBrokenPairs", 0))
        text = (nc.call_bam_files_mates if mates else nc.call_bam_files)(files, rr, opts, source_files=source) if rr else ""
        for _, index in source or []:
            index.close()
        dt = time.time() - t0
        n_windows = nc.stats["n_windows"] if rr else 0
    finally:
        for f in files:
            f.close()
        if ref_file is not None:
            ref_file.close()
        nc.close()
    recs = sorted(sharding.records_from_vcf_text(text), key=lambda r: (sharding.chrom_key(r[0]), r[1]))
    merged = sharding.merge_record_streams([recs])
    write_output(opts, [s.decode(errors="surrogateescape") for s in plan["samples"]], merged)
    print(json.dumps(dict(files=len(opts.bamFiles), mode=plan["mode"], samples=len(plan["samples"]), regions=len(regions), windows=n_windows,
                          records=len(merged), seconds=round(dt, 3), output=opts.output)))


def call_variants_config4(opts, n_regions):
    """BASELINE config 4 in miniature: procedurally generated regions with reads -> candidates -> windows -> records, every
    device stage batched over all windows (platypus_amd.caller.callVariantsInRegions).  Under torch.distributed.run the regions
    are dealt round-robin to the ranks (runner.py:473-474), each rank drives its own GPU, and the record lines are gathered to
    rank 0 and merged in (chromosome, position) order (runner.py:301-352).  VCF records (no header) go to --output."""
    import io
    import os
    import time
    from . import caller, hostapi as H, sharding, synth
    from .vcfrecords import VCF
    rank, world = int(os.environ.get("RANK", 0)), int(os.environ.get("WORLD_SIZE", 1))
    dist = None
    if world > 1:
        import torch
        import torch.distributed as dist
        gpu = torch.cuda.is_available()
        # (PLAT_DIST_BACKEND=gloo: ranks sharing one GPU, as the single-GPU test box needs; RCCL wants one device per rank)
        dist.init_process_group(os.environ.get("PLAT_DIST_BACKEND", "nccl" if gpu else "gloo"), rank=rank, world_size=world)
        if gpu:
            torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", rank)) % torch.cuda.device_count())
    opts.originalMaxHaplotypes = opts.maxHaplotypes
    size = min(int(opts.bufferSize), 100000)
    mine = sharding.regions_for_rank(n_regions, rank, world)
    t0 = time.time()
    text = io.StringIO()
    source_files = [read_source_lines(f) for f in (opts.sourceFile or [])]
    reader = None
    if source_files:
        # the CLI's own stand-in for a tabix fetch: the data lines whose [POS - 1, POS - 1 + len(REF)) overlaps the region, in file order
        reader = H.VariantCandidateReader(source_files, opts)
    no_contig = "Invalid contig name %s. Make sure your FASTA reference file and query regions have the same naming convention"     # fastafile.pyx:145
    if os.environ.get("PLAT_PYTHON_CALLER") == "1" or opts.assemble or (not opts.getVariantsFromBAMs and not source_files):
        # the Python region loop (platypus_amd.caller): window lists, haplotypes and records as Python objects
        regs = [synth.config4_region(i, region_len=size, n_samples=1, read_len=int(opts.rlen)) for i in mine]
        if opts.refFile:
            # the contigs come from the file: sequence windows fetched on the device, cached per region as the reference's callers do
            fasta = H.IndexedFastaFile(opts.refFile, opts.refFile + ".fai", autoCache=1 << 20)
            for r in regs:
                if r["chrom"] not in fasta.refs:
                    sys.exit(no_contig % r["chrom"])
        else:
            fasta = H.FastaFile({r["chrom"]: r["ref"] for r in regs})
        work = [(r["chrom"], r["start"], r["end"],
                 [H.bamReadBuffer([H.AlignedRead(x["seq"], x["qual"], x["pos"], x["mapq"], x["flag"], end=x["end"], cigarOps=x["cigar"])
                                   for x in r["samples"][0]], sample="S1")]) for r in regs]
        t0 = time.time()
        names, opts.sourceFile = opts.sourceFile, (source_files or None)      # (the Python loop's reader takes the lines themselves)
        n_windows = caller.callVariantsInRegions(work, fasta, opts, VCF(["S1"]), text) if work else 0
        opts.sourceFile = names
        if opts.refFile:
            fasta.close()
    else:
        # the native region loop (libplat_caller.so): reads as arrays, host threads, every device stage batched per chunk
        from . import fastcaller as F
        regs = [synth.config4_region_arrays(i, region_len=size, n_samples=1, read_len=int(opts.rlen)) for i in mine]
        rr = [F.region_from_arrays(r) for r in regs]
        local = int(os.environ.get("LOCAL_RANK", rank))
        import torch
        nc = F.NativeCaller(local % max(1, torch.cuda.device_count()), int(os.environ.get("PLAT_CALLER_WORKERS", "8")),
                            int(os.environ.get("PLAT_CALLER_CHUNK", "4")))
        ref_file = ref_map = None
        if opts.refFile:
            # contig_seq and dev_contig_seq of every region come from the file: mapped, its contigs fetched whole in one device batch
            import mmap
            import numpy as np
            with open(opts.refFile, "rb") as f, open(opts.refFile + ".fai", "rb") as fai:
                ref_map = mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ)
                ref_file = nc.open_fasta(np.frombuffer(ref_map, dtype=np.uint8), fai.read(), 1)
            tids = [ref_file.tid(r["chrom"]) for r in regs]
            if -1 in tids:
                sys.exit(no_contig % regs[tids.index(-1)]["chrom"])
            if tids:
                ref_file.load(sorted(set(tids)))
            rr = [F.FastaContigRegion(x, ref_file, t) for x, t in zip(rr, tids)]
        t0 = time.time()
        if source_files and all(os.path.exists(f + ".tbi") for f in opts.sourceFile):
            # every source file has a tabix index next to it: the library takes each file and its index once, answers every region's
            # lookup in one device batch per file, and inflates and iterates the chunks on the device (include/platypus_caller_index.h);
            # a file whose fetch raises (a name its index lacks) is left out of that region
            files = []
            for f in opts.sourceFile:
                with open(f, "rb") as data, open(f + ".tbi", "rb") as tbi:
                    files.append((data.read(), nc.open_index(tbi.read(), "tbi")))
            text.write(nc.call_regions(rr, ["S1"], opts, source_files=files) if rr else "")
            for _, index in files:
                index.close()
        else:
            lines = [b"".join(reader.texts(r["chrom"], r["start"], r["end"])) for r in regs] if reader else None
            text.write(nc.call_regions(rr, ["S1"], opts, source_lines=lines) if rr else "")
        n_windows = nc.stats["n_windows"] if rr else 0
        if ref_file is not None:
            ref_file.close()
        nc.close()
    recs = sorted(sharding.records_from_vcf_text(text.getvalue()), key=lambda r: (sharding.chrom_key(r[0]), r[1]))
    device = None
    if dist is not None and dist.get_backend() == "nccl":
        import torch
        device = torch.device("cuda", torch.cuda.current_device())
    got = sharding.gather_records(sharding.encode_records(recs), dist, device)
    dt = time.time() - t0
    if rank == 0:
        merged = sharding.merge_record_streams([sharding.decode_records(p) for p in got])
        write_output(opts, ["S1"], merged, int(os.environ.get("LOCAL_RANK", rank)))
        print(json.dumps(dict(regions=n_regions, region_len=size, ranks=world, windows_rank0=n_windows, records=len(merged),
                              seconds=round(dt, 3), output=opts.output)))
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


def main():
    if len(sys.argv) < 2 or sys.argv[1] != "callVariants":
        sys.exit("usage: python -m platypus_amd callVariants [options]   (options as in Platypus.py callVariants)")
    call_variants(sys.argv[2:])


if __name__ == "__main__":
    main()
