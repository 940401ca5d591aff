"""Python host for libplat_mi355x.so: device buffers (via torch, plumbing only) + the batched entry points.

`Engine` owns one `plat_ctx` (one per process / GPU, like one PlatypusSingleProcess per worker in the
reference, variantcaller.pyx:935-980).  All heavy lifting happens in the HIP library; nothing here
computes alignment scores or likelihoods on the CPU.
"""
import ctypes as C

import numpy as np

from . import _lib
from .batch import HostBatch, pad_blob


def _torch():
    import torch
    return torch


class DeviceBatch:
    """HBM image of a HostBatch (fields of plat_window_batch) + the ctypes struct pointing at it."""

    def __init__(self, hb: HostBatch, device):
        torch = _torch()
        self.host = hb
        self.device = device

        def up(a, dtype):
            return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(device)
        self.t = dict(
            win_hap_begin=up(hb.win_hap_begin, np.int32), win_read_begin=up(hb.win_read_begin, np.int32),
            win_start=up(hb.win_start, np.int32), win_end=up(hb.win_end, np.int32),
            win_flank=up(hb.win_flank, np.int32), pair_off=up(hb.pair_off, np.int64),
            hap_seq=up(pad_blob(hb.hap_seq), np.uint8), hap_off=up(hb.hap_off, np.int64),
            read_seq=up(pad_blob(hb.read_seq), np.uint8), read_qual=up(pad_blob(hb.read_qual), np.uint8),
            read_off=up(hb.read_off, np.int64), read_pos=up(hb.read_pos, np.int32),
            read_end=up(hb.read_end, np.int32), read_mapq=up(hb.read_mapq, np.uint8),
            read_flags=up(hb.read_flags, np.int32), read_kind=up(hb.read_kind, np.uint8),
            seg_read_begin=up(hb.seg_read_begin, np.int32), seg_n_good=up(hb.seg_n_good, np.int32),
            gl_off=up(hb.gl_off, np.int64))
        s = _lib.WindowBatch()
        s.n_windows, s.n_haps, s.n_reads = hb.n_windows, hb.n_haps, hb.n_reads
        for name, _ in _lib.WindowBatch._fields_[4:]:
            setattr(s, name, self.t[name].data_ptr())
        self.struct = s
        # what the host knows about its own batch: lets the asynchronous entry point skip the internal read-backs
        hl = np.diff(hb.hap_off)
        rl = np.diff(hb.read_off)
        h = _lib.BatchHints()
        h.max_hap_len = int(hl.max()) if len(hl) else 0
        h.max_read_len = int(rl.max()) if len(rl) else 0
        h.max_reads_per_window = int(np.diff(hb.win_read_begin).max()) if hb.n_windows else 0
        h.n_pairs, h.hap_blob_len, h.read_blob_len, h.extra_jobs_cap = int(hb.n_pairs), int(hb.hap_off[-1]), int(hb.read_off[-1]), 0
        self.hints = h
        self.loglik = torch.empty(max(hb.n_pairs, 1), dtype=torch.float64, device=device)
        self.score = torch.empty(max(hb.n_pairs, 1), dtype=torch.int32, device=device)
        ng = max(int(hb.gl_off[-1]), 1)
        self.gl = torch.empty(ng, dtype=torch.float64, device=device)
        self.logl = torch.empty(ng, dtype=torch.float64, device=device)
        self.gof = torch.empty(ng, dtype=torch.float64, device=device)


class LikelihoodBatch:
    """HBM image of genotype likelihoods that were computed elsewhere (e.g. handed over by a caller that kept
    Population.setup on its side): what em() / variant_posteriors() / genotype_calls() need of a DeviceBatch.

    hap_counts[w] = H_w; n_reads [nW][n_ind]; gl[w] = [n_ind][G_w]; gof[w] = [G_w][n_ind] (optional)."""

    class _Host:
        pass

    def __init__(self, n_ind, hap_counts, n_reads, gl, gof, device):
        torch = _torch()
        hb = self.host = LikelihoodBatch._Host()
        hb.n_ind, hb.n_windows = int(n_ind), len(hap_counts)
        hb.win_hap_begin = np.concatenate([[0], np.cumsum(hap_counts)]).astype(np.int32)
        hb.n_haps = int(hb.win_hap_begin[-1])
        G = np.asarray(hap_counts, dtype=np.int64) * (np.asarray(hap_counts, dtype=np.int64) + 1) // 2
        hb.gl_off = np.concatenate([[0], np.cumsum(G * n_ind)]).astype(np.int64)

        def up(a, dt):
            return torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(device)
        self.t = dict(win_hap_begin=up(hb.win_hap_begin, np.int32), gl_off=up(hb.gl_off, np.int64),
                      seg_n_good=up(np.asarray(n_reads).reshape(-1), np.int32))
        self.gl = up(np.concatenate([np.asarray(x, dtype=np.float64).reshape(-1) for x in gl] + [np.zeros(1)]), np.float64)
        if gof is None:
            gof = [np.zeros(int(g) * n_ind) for g in G]
        self.gof = up(np.concatenate([np.asarray(x, dtype=np.float64).reshape(-1) for x in gof] + [np.zeros(1)]), np.float64)


class AssemblyDeviceBatch:
    """HBM image of a plat_assembly_batch + the output buffers of plat_assemble_batch."""

    def __init__(self, ab, device, max_vars=512, blob_per_region=1 << 16):
        torch = _torch()

        def dev(a, dt):
            return torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(device)
        self.device, self.max_vars, self.blob_per_region = device, max_vars, blob_per_region
        nG = self.n_regions = int(ab["n_regions"])
        self.t = dict(ref_seq=dev(pad_blob(ab["ref_seq"]), np.uint8), ref_off=dev(ab["ref_off"], np.int64),
                      ref_start=dev(ab["ref_start"], np.int32), assem_start=dev(ab["assem_start"], np.int32),
                      assem_end=dev(ab["assem_end"], np.int32), reg_read_begin=dev(ab["reg_read_begin"], np.int32),
                      read_seq=dev(pad_blob(ab["read_seq"]), np.uint8), read_qual=dev(pad_blob(ab["read_qual"]), np.uint8),
                      read_off=dev(ab["read_off"], np.int64))
        s = _lib.AssemblyBatch()
        s.n_regions, s.n_reads = nG, int(ab["n_reads"])
        for name, _ in _lib.AssemblyBatch._fields_[2:]:
            setattr(s, name, self.t[name].data_ptr())
        self.struct = s
        i32 = dict(dtype=torch.int32, device=device)
        self.cnt = torch.zeros(nG, **i32); self.status = torch.zeros(nG, **i32)
        self.pos = torch.zeros(nG * max_vars, **i32); self.nrem = torch.zeros(nG * max_vars, **i32)
        self.nadd = torch.zeros(nG * max_vars, **i32); self.off = torch.zeros(nG * max_vars, **i32)
        self.blob = torch.zeros(nG * blob_per_region, dtype=torch.uint8, device=device)

    def results(self):
        """[syncs] per region the list of (pos, removed, added) in the reference's sorted() order."""
        if self.device.type == "cuda":
            _torch().cuda.synchronize(self.device)
        cnt, status, pos, nrem, nadd, off = (x.cpu().numpy() for x in (self.cnt, self.status, self.pos, self.nrem, self.nadd, self.off))
        blob = self.blob.cpu().numpy()
        out = []
        for g in range(self.n_regions):
            if status[g] != 0:
                _lib.check(int(status[g]), "plat_assemble_batch(region %d)" % g)
            vs = []
            if cnt[g]:
                raw = blob[g * self.blob_per_region:(g + 1) * self.blob_per_region].tobytes()
                for i in range(cnt[g]):
                    k = g * self.max_vars + i
                    o = off[k]
                    vs.append((int(pos[k]), raw[o:o + nrem[k]], raw[o + nrem[k]:o + nrem[k] + nadd[k]]))
            out.append(vs)
        return out


class Engine:
    def __init__(self, device_index=0):
        torch = _torch()
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise _lib.PlatypusDeviceError(-7, "torch reports no GPU; the HIP path has no CPU fallback", "Engine")
        self.device = torch.device("cuda", device_index)
        torch.cuda.set_device(self.device)
        ctx = C.c_void_p()
        _lib.check(self.lib.plat_ctx_create(device_index, C.byref(ctx)), "plat_ctx_create")
        self.ctx = ctx

    def close(self):
        if getattr(self, "ctx", None):
            self.lib.plat_ctx_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _stream(self):
        return C.c_void_p(_torch().cuda.current_stream(self.device).cuda_stream)

    def _sync(self):
        _torch().cuda.synchronize(self.device)

    # ---- a1 --------------------------------------------------------------------------------------
    def dp_batch(self, haps, reads, quals, gos, lens, gapextend=3, nucprior=2):
        """Score-only fastAlignmentRoutine for padded rows (numpy in, numpy out)."""
        torch = _torch()
        n, lmax = reads.shape
        assert haps.shape == (n, lmax + 15) and gos.shape == (n, lmax + 15) and quals.shape == (n, lmax)
        d = [torch.from_numpy(pad_blob(a.reshape(-1))).to(self.device) for a in (haps, reads, quals, gos)]
        dl = torch.from_numpy(np.ascontiguousarray(lens, dtype=np.int32)).to(self.device)
        out = torch.empty(n, dtype=torch.int32, device=self.device)
        _lib.check(self.lib.plat_dp_batch(self.ctx, n, lmax, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(),
                                          d[3].data_ptr(), dl.data_ptr(), gapextend, nucprior, out.data_ptr(),
                                          self._stream()), "plat_dp_batch")
        self._sync()
        return out.cpu().numpy()

    # ---- a3..a10 ---------------------------------------------------------------------------------
    def upload(self, hb: HostBatch) -> DeviceBatch:
        return DeviceBatch(hb, self.device)

    def align_async(self, db: DeviceBatch, want_score=True, calc_flank_score=0, use_mapq_cap=0, hints=None):
        """Same as align(), enqueued without any internal read-back (sizes from db.hints).  Device-side errors are
        raised by the next synchronize()."""
        rc = self.lib.plat_align_window_batch_async(self.ctx, C.byref(db.struct), C.byref(hints if hints is not None else db.hints),
                                                    calc_flank_score, use_mapq_cap, db.loglik.data_ptr(),
                                                    db.score.data_ptr() if want_score else None, self._stream())
        _lib.check(rc, "plat_align_window_batch_async")

    def align(self, db: DeviceBatch, want_stats=True, want_score=True, calc_flank_score=0, use_mapq_cap=0):
        """Haplotype.alignReads for every haplotype of every window.  Results stay in HBM (db.loglik)."""
        st = _lib.AlignStats()
        rc = self.lib.plat_align_window_batch(self.ctx, C.byref(db.struct), calc_flank_score, use_mapq_cap,
                                              db.loglik.data_ptr(), db.score.data_ptr() if want_score else None,
                                              C.byref(st) if want_stats else None, self._stream())
        _lib.check(rc, "plat_align_window_batch")
        return st

    # ---- a11/a12 ---------------------------------------------------------------------------------
    def genotype(self, db: DeviceBatch):
        rc = self.lib.plat_genotype_window_batch(self.ctx, C.byref(db.struct), db.host.n_ind,
                                                 db.t["seg_read_begin"].data_ptr(), db.t["seg_n_good"].data_ptr(),
                                                 db.loglik.data_ptr(), db.t["gl_off"].data_ptr(), db.gl.data_ptr(),
                                                 db.logl.data_ptr(), db.gof.data_ptr(), self._stream())
        _lib.check(rc, "plat_genotype_window_batch")

    def call_windows(self, db: DeviceBatch, want_stats=True, asynchronous=False, calc_flank_score=0):
        """One pass of the hot path: likelihood arrays, then genotype likelihoods (Population.setup).
        asynchronous=True: nothing is read back and nothing waits (no statistics; errors surface in synchronize()).
        calc_flank_score = options.calculateFlankScore (chaplotype.pyx:606-612)."""
        if asynchronous and not want_stats:
            self.align_async(db, calc_flank_score=calc_flank_score)
            st = None
        else:
            st = self.align(db, want_stats=want_stats, calc_flank_score=calc_flank_score)
        self.genotype(db)
        return st

    # ---- EM, genotype calls, posteriors, per-site marginalisation -------------------
    def upload_likelihoods(self, n_ind, hap_counts, n_reads, gl, gof=None) -> LikelihoodBatch:
        return LikelihoodBatch(n_ind, hap_counts, n_reads, gl, gof, self.device)

    def haplotype_scores(self, db: DeviceBatch):
        """computeHaplotypeScore (INFO['HapScore']) for every window of `db` from the likelihoods left in HBM by align().
        Returns (hap_like [n_haps] = what DiploidGenotype.hap1Like holds after Population.setup, hap_score [n_windows])."""
        torch = _torch()
        hb = db.host
        like = torch.empty(max(hb.n_haps, 1), dtype=torch.float64, device=self.device)
        score = torch.empty(max(hb.n_windows, 1), dtype=torch.int32, device=self.device)
        maxh = int(np.max(np.diff(hb.win_hap_begin))) if hb.n_windows else 0
        rc = self.lib.plat_haplotype_score_batch(self.ctx, C.byref(db.struct), hb.n_ind, maxh, db.t["seg_read_begin"].data_ptr(),
                                                 db.t["seg_n_good"].data_ptr(), db.loglik.data_ptr(), like.data_ptr(),
                                                 score.data_ptr(), self._stream())
        _lib.check(rc, "plat_haplotype_score_batch")
        self._sync()
        return like.cpu().numpy()[:hb.n_haps], score.cpu().numpy()[:hb.n_windows]

    def em(self, db, max_iters=100, use_em_likelihoods=0):
        """Population.call (EM + callGenotypes) for every window of `db`, on the genotype likelihoods left in HBM by
        genotype().  Results stay in HBM: db.freq [n_haps], db.em [like db.gl], db.calls [n_windows*n_ind], db.em_iters."""
        torch = _torch()
        hb = db.host
        db.freq = torch.empty(max(hb.n_haps, 1), dtype=torch.float64, device=self.device)
        db.em = torch.empty_like(db.gl)
        db.calls = torch.empty(max(hb.n_windows * hb.n_ind, 1), dtype=torch.int32, device=self.device)
        db.em_iters = torch.empty(max(hb.n_windows, 1), dtype=torch.int32, device=self.device)
        maxh = int(np.max(np.diff(hb.win_hap_begin))) if hb.n_windows else 0
        db.max_haps = maxh
        rc = self.lib.plat_em_window_batch(self.ctx, hb.n_windows, hb.n_ind, maxh, db.t["win_hap_begin"].data_ptr(),
                                           db.t["gl_off"].data_ptr(), db.t["seg_n_good"].data_ptr(), db.gl.data_ptr(),
                                           max_iters, use_em_likelihoods, db.freq.data_ptr(), db.em.data_ptr(),
                                           db.calls.data_ptr(), db.em_iters.data_ptr(), self._stream())
        _lib.check(rc, "plat_em_window_batch")

    def variant_posteriors(self, db, var_window, hap_masks, priors):
        """Population.calculatePosterior for a list of variants: var_window[v] = window, hap_masks[v] = 0/1 per haplotype
        of that window (`var in hap.variants`), priors[v].  Needs em().  Returns a numpy array of phred posteriors."""
        torch = _torch()
        n = len(var_window)
        if n == 0:
            return np.zeros(0)
        hb = db.host
        off = np.concatenate([[0], np.cumsum([len(m) for m in hap_masks])]).astype(np.int64)
        blob = np.concatenate([np.asarray(m, dtype=np.uint8) for m in hap_masks])

        def up(a, dt):
            return torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(self.device)
        d_w, d_off, d_blob, d_pr = up(var_window, np.int32), up(off, np.int64), up(blob, np.uint8), up(priors, np.float64)
        out = torch.empty(n, dtype=torch.float64, device=self.device)
        rc = self.lib.plat_variant_posterior_batch(self.ctx, n, hb.n_ind, db.max_haps, db.t["win_hap_begin"].data_ptr(),
                                                   db.t["gl_off"].data_ptr(), db.t["seg_n_good"].data_ptr(),
                                                   db.gl.data_ptr(), db.freq.data_ptr(), d_w.data_ptr(), d_off.data_ptr(),
                                                   d_blob.data_ptr(), d_pr.data_ptr(), out.data_ptr(), self._stream())
        _lib.check(rc, "plat_variant_posterior_batch")
        self._sync()
        return out.cpu().numpy()

    def genotype_calls(self, db, sites):
        """computeGenotypeCallAndLikelihoods for every (site, sample).  `sites`: list of dicts {window, var_in_hap
        [H][nVar], is_ref [H]}.  Needs em().  Returns per site (phased [n_ind][2], likelihoods [n_ind][NL], out4 [n_ind][4])."""
        torch = _torch()
        nS = len(sites)
        if nS == 0:
            return []
        hb = db.host
        nvar = np.array([np.asarray(s["var_in_hap"]).shape[1] for s in sites], dtype=np.int32)
        vih = [np.asarray(s["var_in_hap"], dtype=np.int32).reshape(-1) for s in sites]
        ref = [np.asarray(s["is_ref"], dtype=np.int32) for s in sites]
        vih_off = np.concatenate([[0], np.cumsum([len(v) for v in vih])]).astype(np.int64)
        ref_off = np.concatenate([[0], np.cumsum([len(r) for r in ref])]).astype(np.int64)
        NL = (nvar.astype(np.int64) + 1) * (nvar + 2) // 2
        lik_off = np.concatenate([[0], np.cumsum(NL * hb.n_ind)]).astype(np.int64)

        def up(a, dt):
            return torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(self.device)
        d_win = up([s["window"] for s in sites], np.int32)
        d_nvar, d_vo, d_ro, d_lo = up(nvar, np.int32), up(vih_off, np.int64), up(ref_off, np.int64), up(lik_off, np.int64)
        d_vih = up(np.concatenate(vih + [np.zeros(1, dtype=np.int32)]), np.int32)
        d_ref = up(np.concatenate(ref), np.int32)
        ph = torch.empty(nS * hb.n_ind * 2, dtype=torch.int32, device=self.device)
        lik = torch.empty(int(lik_off[-1]), dtype=torch.float64, device=self.device)
        out4 = torch.empty(nS * hb.n_ind * 4, dtype=torch.float64, device=self.device)
        rc = self.lib.plat_genotype_call_batch(self.ctx, nS, hb.n_ind, db.t["win_hap_begin"].data_ptr(),
                                               db.t["gl_off"].data_ptr(), db.gl.data_ptr(), db.gof.data_ptr(),
                                               db.freq.data_ptr(), d_win.data_ptr(), d_nvar.data_ptr(), d_vo.data_ptr(),
                                               d_ro.data_ptr(), d_vih.data_ptr(), d_ref.data_ptr(), d_lo.data_ptr(),
                                               ph.data_ptr(), lik.data_ptr(), out4.data_ptr(), self._stream())
        _lib.check(rc, "plat_genotype_call_batch")
        self._sync()
        ph, lik, out4 = ph.cpu().numpy().reshape(nS, hb.n_ind, 2), lik.cpu().numpy(), out4.cpu().numpy().reshape(nS, hb.n_ind, 4)
        return [(ph[s], lik[lik_off[s]:lik_off[s + 1]].reshape(hb.n_ind, int(NL[s])), out4[s]) for s in range(nS)]

    # ---- VariantCandidateGenerator ------------------------------------------------------
    @staticmethod
    def base_codes(blob):
        """The 2-bit codes of a byte blob as the device lays them out ((ASCII >> 1) & 3, base i at bits 2 (i & 15) of dword i >> 4), + 8 zero words."""
        a = np.frombuffer(bytes(blob), dtype=np.uint8)
        n = (len(a) + 15) // 16
        c = np.zeros(n * 16, dtype=np.uint32)
        c[:len(a)] = (a >> 1) & 3
        words = (c.reshape(n, 16) << (2 * np.arange(16, dtype=np.uint32))).sum(axis=1, dtype=np.uint64).astype(np.uint32)
        return np.concatenate([words, np.zeros(8, dtype=np.uint32)])

    def pack_reads(self, seqs, quals, gaps=None):
        """Reads as a PLAT_READS_PACKED table on the device, for the entry points that read packed bases where they lie: one byte per base
        ((ASCII >> 1) & 3 | min(quality, 63) << 2), exceptions (a base other than A/C/G/T, a quality above 63) indexed by the read blob's byte
        index.  gaps[i]: bytes left free in front of read i's packed bytes (its source pointer then has that alignment shift; default none).
        Returns dict(reads=_lib.PackedReads, src, blob, off, exc_index, exc_base, exc_qual); keep it alive while `reads` is used."""
        torch = _torch()
        n = len(seqs)
        gaps = [0] * n if gaps is None else list(gaps)
        lens = np.array([len(x) for x in seqs], dtype=np.int64)
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        seq = np.frombuffer(b"".join(bytes(x) for x in seqs), dtype=np.uint8)
        qual = np.frombuffer(b"".join(bytes(x) for x in quals), dtype=np.uint8)
        plain = (seq == 65) | (seq == 67) | (seq == 71) | (seq == 84)
        ex = np.nonzero(~plain | (qual > 63))[0].astype(np.int64)
        byte = (((seq >> 1) & 3) | (np.minimum(qual, 63) << 2)).astype(np.uint8)
        at = np.cumsum(np.asarray(gaps, dtype=np.int64) + np.concatenate([[0], lens[:-1]])) if n else np.zeros(0, dtype=np.int64)
        blob = np.full(int(at[-1] + lens[-1]) + _lib.PLAT_BLOB_PAD if n else _lib.PLAT_BLOB_PAD, 0xA7, dtype=np.uint8)
        for i in range(n):
            blob[at[i]:at[i] + lens[i]] = byte[off[i]:off[i + 1]]

        def dev(a, dt):
            return torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(self.device)
        t = dict(blob=dev(blob, np.uint8), off=dev(off, np.int64), exc_index=dev(np.concatenate([ex, [0]]), np.int64),
                 exc_base=dev(np.concatenate([seq[ex], [0]]), np.uint8), exc_qual=dev(np.concatenate([qual[ex], [0]]), np.uint8))
        t["src"] = dev(t["blob"].data_ptr() + at if n else np.zeros(1), np.int64)
        pk = _lib.PackedReads()
        pk.read_src, pk.n_exc = t["src"].data_ptr(), len(ex)
        pk.exc_index, pk.exc_base, pk.exc_qual = t["exc_index"].data_ptr(), t["exc_base"].data_ptr(), t["exc_qual"].data_ptr()
        t["reads"] = pk
        return t

    def pack_codes_pieces(self, pieces, n_pieces, max_piece_bytes, codes, total_bytes, exc_index=None, exc_base=None):
        """plat_pack_codes_pieces on device tensors (pieces: plat_unpack_piece records as bytes; codes: the output words)."""
        n_exc = 0 if exc_index is None else int(exc_index.numel())
        _lib.check(self.lib.plat_pack_codes_pieces(self.ctx, n_pieces, max_piece_bytes, pieces.data_ptr(), codes.data_ptr(), total_bytes, n_exc,
                                                   exc_index.data_ptr() if n_exc else 0, exc_base.data_ptr() if n_exc else 0, self._stream()), "plat_pack_codes_pieces")
        self._sync()

    def gather_reads_packed(self, n_dst, src_index, dst_off, packed, src_off, src_pos, src_end, src_mapq, src_flags, dst_seq, dst_qual, dst_pos, dst_end,
                            dst_mapq, dst_flags):
        """plat_gather_reads_packed on device tensors (packed: a _lib.PackedReads, e.g. pack_reads()["reads"])."""
        _lib.check(self.lib.plat_gather_reads_packed(self.ctx, n_dst, src_index.data_ptr(), dst_off.data_ptr(), C.byref(packed), src_off.data_ptr(), src_pos.data_ptr(),
                                                     src_end.data_ptr(), src_mapq.data_ptr(), src_flags.data_ptr(), dst_seq.data_ptr(), dst_qual.data_ptr(),
                                                     dst_pos.data_ptr(), dst_end.data_ptr(), dst_mapq.data_ptr(), dst_flags.data_ptr(), self._stream()),
                   "plat_gather_reads_packed")
        self._sync()

    def candidates(self, regions, min_flank=10, min_base_qual=20, gen_snps=1, gen_indels=1, max_per_read=64, codes=False, packed=False, gaps=None,
                   retry=True, keep_device=False):
        """VariantCandidateGenerator.addCandidatesFromReads for a list of regions.

        `regions`: list of dicts {ref: bytes (contig[ref_seq_start:...]), ref_seq_start, contig_len, reads: [dict(seq, qual,
        pos, flag, cigar [(op, len), ...])]}.  Returns per region the per-occurrence records [(refPos, removed, added,
        read index)] in the reference's emission order (merging equal variants is the caller's dictionary step).
        keep_device: the records and the tables behind them stay on the device for candidates_merge() / stage_b() until the next scan."""
        torch = _torch()
        self._cand_dev = self._merge_dev = None
        nG = len(regions)
        reads = [r for g in regions for r in g["reads"]]
        nR = len(reads)
        if nR == 0:
            return [[] for _ in regions]

        def dev(a, dt):
            return torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(self.device)
        ref_blob = b"".join(bytes(g["ref"]) for g in regions)
        ref_off = np.concatenate([[0], np.cumsum([len(g["ref"]) for g in regions])]).astype(np.int64)
        seq_blob = b"".join(r["seq"] for r in reads)
        qual_blob = b"".join(r["qual"] for r in reads)
        read_off = np.concatenate([[0], np.cumsum([len(r["seq"]) for r in reads])]).astype(np.int64)
        cig = np.array([x for r in reads for c in r["cigar"] for x in c] + [0, 0], dtype=np.int16)
        cig_off = np.concatenate([[0], np.cumsum([len(r["cigar"]) for r in reads])]).astype(np.int32)
        region_of = np.repeat(np.arange(nG, dtype=np.int32), [len(g["reads"]) for g in regions])
        t = dict(ref=dev(pad_blob(np.frombuffer(ref_blob, dtype=np.uint8)), np.uint8), ref_off=dev(ref_off, np.int64),
                 rss=dev([g["ref_seq_start"] for g in regions], np.int32), clen=dev([g["contig_len"] for g in regions], np.int32),
                 seq=dev(pad_blob(np.frombuffer(seq_blob, dtype=np.uint8)), np.uint8),
                 qual=dev(pad_blob(np.frombuffer(qual_blob, dtype=np.uint8)), np.uint8), read_off=dev(read_off, np.int64),
                 pos=dev([r["pos"] for r in reads], np.int32), flags=dev([r["flag"] for r in reads], np.int32),
                 cig=dev(cig, np.int16), cig_off=dev(cig_off, np.int32), region_of=dev(region_of, np.int32))
        b = _lib.CandidateBatch()
        b.n_regions, b.n_reads = nG, nR
        b.ref_seq, b.ref_off, b.ref_seq_start, b.contig_len = t["ref"].data_ptr(), t["ref_off"].data_ptr(), t["rss"].data_ptr(), t["clen"].data_ptr()
        b.read_seq, b.read_qual, b.read_off = t["seq"].data_ptr(), t["qual"].data_ptr(), t["read_off"].data_ptr()
        b.read_pos, b.read_flags, b.cigar, b.cig_off = t["pos"].data_ptr(), t["flags"].data_ptr(), t["cig"].data_ptr(), t["cig_off"].data_ptr()
        if packed:
            # plat_candidates_batch_packed: letters and qualities from the packed bytes (pack_reads); read_seq is its OUTPUT for the records' read-side
            # alleles (filled with a pattern here) and there are no expanded qualities
            pk = self.pack_reads([r["seq"] for r in reads], [r["qual"] for r in reads], gaps)
            t["seq"] = torch.full((len(seq_blob) + _lib.PLAT_BLOB_PAD,), 0xEE, dtype=torch.uint8, device=self.device)
            b.read_seq, b.read_qual = t["seq"].data_ptr(), 0
        while True:
            rec = torch.full((nR * max_per_read * 5,), -77, dtype=torch.int32, device=self.device)
            cnt = torch.empty(nR, dtype=torch.int32, device=self.device)
            stt = torch.empty(nR, dtype=torch.int32, device=self.device)
            if packed:
                rc_t = dev(self.base_codes(seq_blob), np.uint32)
                fc_t = torch.zeros((len(ref_blob) + 15) // 16 + 16, dtype=torch.int32, device=self.device)
                irr = torch.zeros(nG + 1, dtype=torch.int32, device=self.device)
                _lib.check(self.lib.plat_ref_codes(self.ctx, nG, t["ref"].data_ptr(), t["ref_off"].data_ptr(), len(ref_blob), fc_t.data_ptr(), irr.data_ptr(),
                                                   self._stream()), "plat_ref_codes")
                rc = self.lib.plat_candidates_batch_packed(self.ctx, C.byref(b), C.byref(pk["reads"]), rc_t.data_ptr(), fc_t.data_ptr(), irr.data_ptr(), min_flank,
                                                           min_base_qual, gen_snps, gen_indels, max_per_read, t["region_of"].data_ptr(), rec.data_ptr(),
                                                           cnt.data_ptr(), stt.data_ptr(), self._stream())
                self.last_ref_irregular = irr
            elif codes:
                # the scan on 2-bit codes (plat_candidates_batch_codes): the reads' codes from the host here (the region loop gets them from the unpack
                # kernel), the reference's from plat_ref_codes; the caller promises reads of A, C, G, T, N only
                rc_t = dev(self.base_codes(seq_blob), np.uint32)
                fc_t = torch.zeros((len(ref_blob) + 15) // 16 + 16, dtype=torch.int32, device=self.device)
                irr = torch.zeros(nG + 1, dtype=torch.int32, device=self.device)
                _lib.check(self.lib.plat_ref_codes(self.ctx, nG, t["ref"].data_ptr(), t["ref_off"].data_ptr(), len(ref_blob), fc_t.data_ptr(), irr.data_ptr(),
                                                   self._stream()), "plat_ref_codes")
                rc = self.lib.plat_candidates_batch_codes(self.ctx, C.byref(b), rc_t.data_ptr(), fc_t.data_ptr(), irr.data_ptr(), min_flank, min_base_qual, gen_snps,
                                                          gen_indels, max_per_read, t["region_of"].data_ptr(), rec.data_ptr(), cnt.data_ptr(), stt.data_ptr(),
                                                          self._stream())
                self.last_ref_irregular = irr
            else:
                rc = self.lib.plat_candidates_batch(self.ctx, C.byref(b), min_flank, min_base_qual, gen_snps, gen_indels, max_per_read,
                                                    t["region_of"].data_ptr(), rec.data_ptr(), cnt.data_ptr(), stt.data_ptr(), self._stream())
            _lib.check(rc, "plat_candidates_batch")
            self._sync()
            cnt_h, st_h = cnt.cpu().numpy(), stt.cpu().numpy()
            # (tests: what this pass wrote, as it is -- records, counts, statuses, the read blob the kernel was given)
            self.last_candidates = dict(rec=rec.cpu().numpy().reshape(nR, max_per_read, 5), count=cnt_h, status=st_h, read_seq=t["seq"].cpu().numpy()[:len(seq_blob)],
                                        max_per_read=max_per_read)
            if keep_device:
                # (candidates_merge / stage_b: the records and the tables those two read, as they lie on the device)
                self._cand_dev = dict(tensors={k: t[k] for k in ("ref", "ref_off", "rss", "clen", "seq", "pos")}, rec=rec, count=cnt, status=stt,
                                      max_per_read=max_per_read, n_regions=nG, n_reads=nR)
            if not retry:
                return None
            if (st_h == -9).any():
                raise _lib.PlatypusDeviceError(-9, "a read reaches outside the reference window handed over", "plat_candidates_batch")
            if (st_h == -8).any():
                max_per_read = int(cnt_h.max())            # a read with more candidates than the slice: rerun with room for it
                continue
            break
        rec_h = rec.cpu().numpy().reshape(nR, max_per_read, 5)
        out = [[] for _ in regions]
        first = np.concatenate([[0], np.cumsum([len(g["reads"]) for g in regions])])
        for r in np.nonzero(cnt_h)[0].tolist():
            g = int(region_of[r])
            for p_, nrem, nadd, ro, ao in rec_h[r, :cnt_h[r]].tolist():
                out[g].append((p_, ref_blob[ro:ro + nrem] if nrem else b"", seq_blob[ao:ao + nadd] if nadd else b"", r - int(first[g])))
        return out

    # ---- the dictionary step behind the scan, and stage B ----------------------------------------------------
    SENTINEL = 0xA5                                                              # every byte of an output array before the call
    _cand_dev = _merge_dev = None

    def _sentinel(self, n, dt):
        torch = _torch()
        return torch.full((int(n) * np.dtype(dt).itemsize,), self.SENTINEL, dtype=torch.uint8, device=self.device)

    @classmethod
    def sentinel_of(cls, dt):
        """The value an untouched element of an output array of candidates_merge / stage_b holds."""
        return np.frombuffer(bytes([cls.SENTINEL]) * np.dtype(dt).itemsize, dtype=dt)[0]

    def candidates_merge(self, scan_read_begin, read_end, scan_longest, min_var_freq, cap_per_scan):
        """plat_candidates_merge_batch on the records the last candidates(keep_device=True) call left on the device.  Scan g = reads
        [scan_read_begin[g], scan_read_begin[g + 1]) of that call's read table; read_end[r] = cAlignedRead.end.  Returns (out_cand
        [n_scans, cap_per_scan, 8], out_n [n_scans, 2]) on the host; rows the kernels did not write hold the sentinel.  The device
        arrays stay for stage_b()."""
        torch = _torch()
        cd = self._cand_dev
        if cd is None:
            raise RuntimeError("candidates_merge() needs the records of a candidates(..., keep_device=True) call")
        nS = len(scan_read_begin) - 1
        t = cd["tensors"]
        b = _lib.CandidateBatch()                                                # the merge reads the alleles' bytes and the reads' positions, nothing else
        b.n_regions, b.n_reads = cd["n_regions"], cd["n_reads"]
        b.ref_seq, b.read_seq, b.read_pos = t["ref"].data_ptr(), t["seq"].data_ptr(), t["pos"].data_ptr()
        dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(self.device)
        t_end, t_begin, t_long = dev(read_end, np.int32), dev(scan_read_begin, np.int32), dev(scan_longest, np.int32)
        assert len(read_end) == cd["n_reads"] and len(scan_longest) == nS
        out_cand, out_n = self._sentinel(max(nS, 1) * cap_per_scan * 8, np.int32), self._sentinel(2 * max(nS, 1), np.int32)
        _lib.check(self.lib.plat_candidates_merge_batch(self.ctx, C.byref(b), t_end.data_ptr(), nS, t_begin.data_ptr(), t_long.data_ptr(),
                                                        cd["max_per_read"], cd["rec"].data_ptr(), cd["count"].data_ptr(), cd["status"].data_ptr(),
                                                        float(min_var_freq), cap_per_scan, out_cand.data_ptr(), out_n.data_ptr(), self._stream()),
                   "plat_candidates_merge_batch")
        self._sync()
        self._merge_dev = dict(cand=out_cand, cand_n=out_n, cap_per_scan=cap_per_scan, n_scans=nS, read_end=t_end, keep=(t_begin, t_long))
        return (out_cand.cpu().numpy().view(np.int32).reshape(max(nS, 1), cap_per_scan, 8)[:nS],
                out_n.cpu().numpy().view(np.int32).reshape(max(nS, 1), 2)[:nS])

    def _empty_merge(self, n_scans):
        """The context's table of distinct records, sized for n_scans scans and empty: what plat_stage_b_batch reads when the candidates
        do not come from a merge on this context."""
        torch = _torch()
        z = torch.zeros(64 + n_scans + 1, dtype=torch.int32, device=self.device)
        o = torch.zeros(8 + 2 * n_scans, dtype=torch.int32, device=self.device)
        b = _lib.CandidateBatch()
        b.n_regions, b.n_reads = n_scans, 0
        for k, _ in _lib.CandidateBatch._fields_[2:]:
            setattr(b, k, z.data_ptr())
        _lib.check(self.lib.plat_candidates_merge_batch(self.ctx, C.byref(b), z.data_ptr(), n_scans, z.data_ptr(), z.data_ptr(), 1, z.data_ptr(), z.data_ptr(),
                                                        z.data_ptr(), 0.0, 1, o.data_ptr(), o.data_ptr(), self._stream()), "plat_candidates_merge_batch")
        self._sync()

    def stage_b(self, regions, tables, options, cand=None, cand_n=None, read_seq=None, cap_per_scan=None, with_records=False, cap_vars=64, cap_windows=32,
                cap_added=256, cap_batch_windows=64, cap_batch_haps=512, cap_batch_reads=1024, cap_hap_bytes=1 << 20):
        """plat_stage_b_batch.  `regions`: dicts {ref, ref_seq_start, contig_len, start, end, rlen[, name_hash]}; `tables`: the read table the
        window pointers and the batch index into -- dict(read_off [n + 1], read_pos [n], read_end [n], tab_begin / tab_n / tab_longest
        [3 * regions], broken_mate_pos, broken_base).  Candidates: `cand` [regions, cap_per_scan, 8] rows of plat_candidates_merge_batch's
        out_cand made by hand (offsets into the concatenated `ref`s and into `read_seq`) with `cand_n` [regions, 2]; cand_rec is NULL then.
        Or cand=None: the arrays candidates_merge() left on the device, with the reference windows and the read blob of that scan (`ref`,
        `ref_seq_start`, `contig_len` of the dicts and `read_seq` are not used then); with_records hands the scan's records over for the
        dictionary replay (cand_rec, region_name_hash), otherwise both are NULL.  `options`: the fields of plat_stage_b_options.
        Every output array starts filled with the sentinel byte.  Returns a dict of every array of plat_stage_b_out on the host (hdr
        [regions, 8], per-region arrays [regions, cap], win_ptrs [regions, cap_windows, 6], totals [16]); the scratch stays on the device."""
        torch = _torch()
        nG = len(regions)
        dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(self.device)
        keep = []

        def ptr(a, dt):
            keep.append(dev(a, dt))
            return keep[-1].data_ptr()
        bi = _lib.StageBIn()
        bi.n_regions = nG
        if cand is None:
            cd, md = self._cand_dev, self._merge_dev
            assert md["n_scans"] == nG == cd["n_regions"]
            t = cd["tensors"]
            bi.cap_per_scan, bi.cand, bi.cand_n = md["cap_per_scan"], md["cand"].data_ptr(), md["cand_n"].data_ptr()
            bi.ref_seq, bi.ref_off, bi.ref_seq_start, bi.contig_len = t["ref"].data_ptr(), t["ref_off"].data_ptr(), t["rss"].data_ptr(), t["clen"].data_ptr()
            bi.read_seq = t["seq"].data_ptr()
            if with_records:
                bi.cand_rec = cd["rec"].data_ptr()
                bi.region_name_hash = ptr([g["name_hash"] for g in regions], np.int64)
        else:
            cand = np.ascontiguousarray(cand, dtype=np.int32)
            assert cand.shape == (nG, cap_per_scan, 8) and read_seq is not None
            self._empty_merge(nG)
            bi.cap_per_scan, bi.cand, bi.cand_n = cap_per_scan, ptr(cand, np.int32), ptr(cand_n, np.int32)
            ref_blob = b"".join(bytes(g["ref"]) for g in regions)
            bi.ref_seq = ptr(pad_blob(np.frombuffer(ref_blob, dtype=np.uint8)), np.uint8)
            bi.ref_off = ptr(np.concatenate([[0], np.cumsum([len(g["ref"]) for g in regions])]), np.int64)
            bi.ref_seq_start, bi.contig_len = ptr([g["ref_seq_start"] for g in regions], np.int32), ptr([g["contig_len"] for g in regions], np.int32)
            bi.read_seq = ptr(pad_blob(np.frombuffer(bytes(read_seq), dtype=np.uint8)), np.uint8)
        bi.region_start, bi.region_end = ptr([g["start"] for g in regions], np.int32), ptr([g["end"] for g in regions], np.int32)
        bi.region_rlen = ptr([g["rlen"] for g in regions], np.int32)
        n_reads = len(tables["read_pos"])
        assert len(tables["read_off"]) == n_reads + 1 and len(tables["read_end"]) == n_reads
        for k in ("tab_begin", "tab_n", "tab_longest"):
            assert len(tables[k]) == 3 * nG
        assert all(0 <= b0 and b0 + n <= n_reads for b0, n in zip(tables["tab_begin"], tables["tab_n"]))
        bi.read_off, bi.read_pos, bi.read_end = ptr(tables["read_off"], np.int64), ptr(list(tables["read_pos"]) + [0], np.int32), ptr(list(tables["read_end"]) + [0], np.int32)
        bi.tab_begin, bi.tab_n, bi.tab_longest = ptr(tables["tab_begin"], np.int32), ptr(tables["tab_n"], np.int32), ptr(tables["tab_longest"], np.int32)
        bi.broken_mate_pos, bi.broken_base = ptr(list(tables["broken_mate_pos"]) + [0], np.int32), int(tables["broken_base"])
        bi.cap_vars, bi.cap_windows, bi.cap_added = cap_vars, cap_windows, cap_added
        bi.cap_batch_windows, bi.cap_batch_haps, bi.cap_batch_reads, bi.cap_hap_bytes = cap_batch_windows, cap_batch_haps, cap_batch_reads, cap_hap_bytes
        so = _lib.StageBOptions()
        for k, _ in _lib.StageBOptions._fields_:
            setattr(so, k, options[k] if isinstance(options, dict) else getattr(options, k))
        per = dict(hdr=8 * nG, added=nG * cap_added, win_ptrs=6 * nG * cap_windows, totals=16, b_hap_off=cap_batch_haps + 1, b_hap_mask=cap_batch_haps,
                   b_hap_seq=cap_hap_bytes, b_read_off=cap_batch_reads + 1, b_read_src=cap_batch_reads, b_read_kind=cap_batch_reads,
                   scratch=56 * nG * cap_windows + 48 * nG + 64)
        for k in ("b_hap_begin", "b_read_begin", "b_pair_off", "b_gl_off", "b_seg_begin"):
            per[k] = cap_batch_windows + 1
        for k in ("b_start", "b_end", "b_flank", "b_n_good"):
            per[k] = cap_batch_windows
        bo = _lib.StageBOut()
        outs = {}
        for k, dt in _lib.STAGE_B_OUT_FIELDS:
            n = per.get(k, nG * (cap_vars if k.startswith("var_") else cap_windows))
            outs[k] = self._sentinel(n, dt)
            setattr(bo, k, outs[k].data_ptr())
        _lib.check(self.lib.plat_stage_b_batch(self.ctx, C.byref(bi), C.byref(so), C.byref(bo), self._stream()), "plat_stage_b_batch")
        self._sync()
        res = {k: outs[k].cpu().numpy().view(dt) for k, dt in _lib.STAGE_B_OUT_FIELDS if k != "scratch"}
        res["hdr"] = res["hdr"].reshape(nG, 8)
        res["added"] = res["added"].reshape(nG, cap_added)
        for k in res:
            if k.startswith("var_"):
                res[k] = res[k].reshape(nG, cap_vars)
            elif k == "win_ptrs":
                res[k] = res[k].reshape(nG, cap_windows, 6)
            elif k.startswith("win_"):
                res[k] = res[k].reshape(nG, cap_windows)
        return res

    # ---- read QC / trimming (checkAndTrimRead) ---------------------------------------------------------------
    def read_qc(self, streams, min_good_qual_bases=20, min_map_qual=20, min_base_qual=20, trim_overlapping=1, trim_adapter=1,
                trim_read_flank=0, trim_soft_clipped=1, enabled=(1, 1, 1, 1)):
        """checkAndTrimRead over whole streams of reads (one stream = the reads one bamReadBuffer sees, in order).
        `streams`: list of lists of dicts {qual, pos, mapq, flag, chromID, mateChromID, insertSize, matePos, cigar}.
        Returns per stream (ok [n], flags_out [n], quals_out [list of uint8 arrays], reason [n])."""
        torch = _torch()
        reads = [r for st in streams for r in st]
        n = len(reads)
        if n == 0:
            return [(np.zeros(0, np.int32), np.zeros(0, np.int32), [], np.zeros(0, np.int32)) for _ in streams]

        def dev(a, dt):
            return torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(self.device)
        off = np.concatenate([[0], np.cumsum([len(r["qual"]) for r in reads])]).astype(np.int64)
        qual = dev(pad_blob(np.concatenate([np.asarray(r["qual"], dtype=np.uint8) for r in reads])), np.uint8)
        t = dict(off=dev(off, np.int64), pos=dev([r["pos"] for r in reads], np.int32), mapq=dev([r["mapq"] for r in reads], np.uint8),
                 flags=dev([r["flag"] for r in reads], np.int32), cid=dev([r["chromID"] for r in reads], np.int16),
                 mcid=dev([r["mateChromID"] for r in reads], np.int16), ins=dev([r["insertSize"] for r in reads], np.int32),
                 mpos=dev([r["matePos"] for r in reads], np.int32),
                 cig=dev([x for r in reads for c in r["cigar"] for x in c] + [0, 0], np.int16),
                 coff=dev(np.concatenate([[0], np.cumsum([len(r["cigar"]) for r in reads])]), np.int32),
                 sof=dev(np.repeat(np.arange(len(streams)), [len(st) for st in streams]), np.int32))
        b = _lib.ReadQCBatch()
        b.n_reads = n
        b.read_qual, b.read_off, b.read_pos, b.read_mapq, b.read_flags = qual.data_ptr(), t["off"].data_ptr(), t["pos"].data_ptr(), t["mapq"].data_ptr(), t["flags"].data_ptr()
        b.chrom_id, b.mate_chrom_id, b.insert_size, b.mate_pos = t["cid"].data_ptr(), t["mcid"].data_ptr(), t["ins"].data_ptr(), t["mpos"].data_ptr()
        b.cigar, b.cig_off, b.stream_of = t["cig"].data_ptr(), t["coff"].data_ptr(), t["sof"].data_ptr()
        o = _lib.ReadQCOptions(min_good_qual_bases, min_map_qual, min_base_qual, trim_overlapping, trim_adapter, trim_read_flank,
                               trim_soft_clipped, *[int(x) for x in enabled])
        ok = torch.empty(n, dtype=torch.int32, device=self.device)
        why = torch.empty(n, dtype=torch.int32, device=self.device)
        _lib.check(self.lib.plat_read_qc_batch(self.ctx, C.byref(b), C.byref(o), ok.data_ptr(), why.data_ptr(), self._stream()),
                   "plat_read_qc_batch")
        self._sync()
        ok_h, why_h, fl_h, q_h = ok.cpu().numpy(), why.cpu().numpy(), t["flags"].cpu().numpy(), qual.cpu().numpy()
        out, a = [], 0
        for st in streams:
            e = a + len(st)
            out.append((ok_h[a:e], fl_h[a:e], [q_h[off[i]:off[i + 1]] for i in range(a, e)], why_h[a:e]))
            a = e
        return out

    def read_buffers(self, streams, min_good_qual_bases=20, min_map_qual=20, min_base_qual=20, trim_overlapping=1, trim_adapter=1,
                     trim_read_flank=0, trim_soft_clipped=1, enabled=(1, 1, 1, 1), packed=False):
        """plat_read_buffers_batch: checkAndTrimRead over whole streams (as read_qc), then every stream's split into `reads` / `badReads`
        and the two buffers gathered.  `streams`: list of lists of dicts {seq, qual, pos, end, mapq, flag, chromID, mateChromID, insertSize,
        matePos, cigar} in fetch order.  Returns per stream a dict: ok, reason, flags (after QC, fetch order), perm (indices into the stream:
        accepted then rejected), n_good, unsorted, hist [8], and reads / bad: the gathered buffers (seq, qual, off, pos, end, mapq, flags,
        mate_pos, cigar [n, 2], cig_off).
        packed=True: the reads go over as PLAT_READS_PACKED (one byte per base, exceptions for bases other than A/C/G/T and qualities above
        63) through plat_read_buffers_packed_batch; no quality array is built.  The buffers' seq / qual are then DECODED from the gathered
        packed bytes and the trimmed exceptions, and each buffer also holds `packed` (its gathered bytes) and `exc_index` (its exceptions,
        indexed into those bytes); every stream holds exc_qual (its exceptions' trimmed qualities, in input order)."""
        torch = _torch()
        reads = [r for st in streams for r in st]
        n, ns = len(reads), len(streams)

        def dev(a, dt):
            return torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(self.device)
        lens = [len(r["qual"]) for r in reads]
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        ncig = [len(r["cigar"]) for r in reads]
        coff = np.concatenate([[0], np.cumsum(ncig)]).astype(np.int32)
        raw = lambda x: x.encode() if isinstance(x, str) else bytes(x)
        cat = lambda key: np.concatenate([np.frombuffer(raw(r[key]), dtype=np.uint8) for r in reads]) if n else np.zeros(0, np.uint8)
        nb, npairs = int(off[-1]), int(coff[-1])
        if packed:
            seq_h, qual_h = cat("seq"), cat("qual")
            exc = np.nonzero(~np.isin(seq_h, np.frombuffer(b"ACGT", np.uint8)) | (qual_h > 63))[0].astype(np.int64)
            exc_base, exc_qual_in = seq_h[exc].copy(), qual_h[exc].copy()
            qual = None
            seq = dev(pad_blob((((seq_h >> 1) & 3) | (np.minimum(qual_h, 63) << 2)).astype(np.uint8)), np.uint8)
            d_exc = dict(idx=dev(np.append(exc, 0), np.int64), base=dev(np.append(exc_base, 0), np.uint8), qual=dev(np.append(exc_qual_in, 0), np.uint8))
        else:
            qual = dev(pad_blob(cat("qual")), np.uint8)
            seq = dev(pad_blob(cat("seq")), np.uint8)
        sbeg = np.concatenate([[0], np.cumsum([len(st) for st in streams])]).astype(np.int32)
        t = dict(off=dev(off, np.int64), pos=dev([r["pos"] for r in reads] + [0], np.int32), end=dev([r["end"] for r in reads] + [0], np.int32),
                 mapq=dev([r["mapq"] for r in reads] + [0], np.uint8), flags=dev([r["flag"] for r in reads] + [0], np.int32),
                 cid=dev([r["chromID"] for r in reads] + [0], np.int16), mcid=dev([r["mateChromID"] for r in reads] + [0], np.int16),
                 ins=dev([r["insertSize"] for r in reads] + [0], np.int32), mpos=dev([r["matePos"] for r in reads] + [0], np.int32),
                 cig=dev([x for r in reads for c in r["cigar"] for x in c] + [0, 0], np.int16), coff=dev(coff, np.int32),
                 sof=dev(np.repeat(np.arange(ns), [len(st) for st in streams]).tolist() + [0], np.int32), sbeg=dev(sbeg, np.int32))
        b = _lib.ReadBuffersPackedIn() if packed else _lib.ReadBuffersIn()
        q = b.qc
        q.n_reads = n
        q.read_qual, q.read_off, q.read_pos, q.read_mapq, q.read_flags = (0 if packed else qual.data_ptr()), t["off"].data_ptr(), t["pos"].data_ptr(), t["mapq"].data_ptr(), t["flags"].data_ptr()
        q.chrom_id, q.mate_chrom_id, q.insert_size, q.mate_pos = t["cid"].data_ptr(), t["mcid"].data_ptr(), t["ins"].data_ptr(), t["mpos"].data_ptr()
        q.cigar, q.cig_off, q.stream_of = t["cig"].data_ptr(), t["coff"].data_ptr(), t["sof"].data_ptr()
        if packed:
            b.n_streams, b.stream_begin, b.read_packed, b.read_end = ns, t["sbeg"].data_ptr(), seq.data_ptr(), t["end"].data_ptr()
            b.n_exc, b.exc_index, b.exc_base, b.exc_qual = len(exc), d_exc["idx"].data_ptr(), d_exc["base"].data_ptr(), d_exc["qual"].data_ptr()
        else:
            b.n_streams, b.stream_begin, b.read_seq, b.read_end = ns, t["sbeg"].data_ptr(), seq.data_ptr(), t["end"].data_ptr()
        o = _lib.ReadQCOptions(min_good_qual_bases, min_map_qual, min_base_qual, trim_overlapping, trim_adapter, trim_read_flank,
                               trim_soft_clipped, *[int(x) for x in enabled])
        e = lambda k, dt: torch.zeros(max(k, 1), dtype=dt, device=self.device)
        ok, why, perm, counts = e(n, torch.int32), e(n, torch.int32), e(n, torch.int32), e(10 * ns, torch.int32)
        g = dict(off=e(n + 2 * ns, torch.int64), cig_off=e(n + 2 * ns, torch.int32), seq=e(nb + _lib.PLAT_BLOB_PAD, torch.uint8),
                 qual=e(nb + _lib.PLAT_BLOB_PAD, torch.uint8), cigar=e(2 * npairs, torch.int16), pos=e(n, torch.int32), end=e(n, torch.int32),
                 mapq=e(n, torch.uint8), flags=e(n, torch.int32), mate_pos=e(n, torch.int32))
        if packed:
            g["qual"] = None
        tab = _lib.ReadBuffersTables(*[(g[k].data_ptr() if g[k] is not None else 0) for k, _ in _lib.ReadBuffersTables._fields_])
        fn = "plat_read_buffers_packed_batch" if packed else "plat_read_buffers_batch"
        _lib.check(getattr(self.lib, fn)(self.ctx, C.byref(b), C.byref(o), ok.data_ptr(), why.data_ptr(), perm.data_ptr(), counts.data_ptr(),
                                         C.byref(tab), self._stream()), fn)
        self._sync()
        h = {k: v.cpu().numpy() for k, v in g.items() if v is not None}
        ok_h, why_h, perm_h, cnt_h, fl_h = ok.cpu().numpy(), why.cpu().numpy(), perm.cpu().numpy(), counts.cpu().numpy(), t["flags"].cpu().numpy()
        if packed:
            # decode the gathered bytes: every input byte's place in the gathered blob (through the split), then the trimmed exceptions there
            exc_trim = d_exc["qual"].cpu().numpy()[:len(exc)]
            h["packed"] = h["seq"]
            h["seq"] = np.frombuffer(b"ACTG", np.uint8)[h["packed"] & 3]
            h["qual"] = (h["packed"] >> 2).astype(np.uint8)
            dst = np.zeros(n, dtype=np.int64)
            for s in range(ns):
                a, z = int(sbeg[s]), int(sbeg[s + 1])
                ng = int(cnt_h[10 * s])
                byte = int(off[a])
                for p0, p1, ob in ((0, ng, a + 2 * s), (ng, z - a, a + 2 * s + ng + 1)):
                    to = h["off"][ob:ob + p1 - p0 + 1]
                    dst[perm_h[a + p0:a + p1]] = byte + to[:-1]
                    byte += int(to[-1])
            src = np.searchsorted(off, exc, side="right") - 1
            at = dst[src] + (exc - off[src]) if len(exc) else np.zeros(0, np.int64)
            h["seq"][at], h["qual"][at] = exc_base, exc_trim
        out = []
        for s in range(ns):
            a, z = int(sbeg[s]), int(sbeg[s + 1])
            ng = int(cnt_h[10 * s])
            res = dict(ok=ok_h[a:z], reason=why_h[a:z], flags=fl_h[a:z], perm=perm_h[a:z] - a, n_good=ng, unsorted=int(cnt_h[10 * s + 1]),
                       hist=cnt_h[10 * s + 2:10 * s + 10])
            byte, pair = int(off[a]), int(coff[a])
            for name, p0, p1, ob in (("reads", 0, ng, a + 2 * s), ("bad", ng, z - a, a + 2 * s + ng + 1)):
                m = p1 - p0
                to, tc = h["off"][ob:ob + m + 1], h["cig_off"][ob:ob + m + 1]
                res[name] = dict(off=to, cig_off=tc, seq=h["seq"][byte:byte + to[-1]], qual=h["qual"][byte:byte + to[-1]],
                                 cigar=h["cigar"][2 * pair:2 * (pair + tc[-1])].reshape(-1, 2), pos=h["pos"][a + p0:a + p1], end=h["end"][a + p0:a + p1],
                                 mapq=h["mapq"][a + p0:a + p1], flags=h["flags"][a + p0:a + p1], mate_pos=h["mate_pos"][a + p0:a + p1])
                if packed:
                    res[name]["packed"] = h["packed"][byte:byte + to[-1]]
                    res[name]["exc_index"] = np.sort(at[(at >= byte) & (at < byte + to[-1])]) - byte
                byte += int(to[-1]); pair += int(tc[-1])
            if packed:
                res["exc_qual"] = exc_trim[(exc >= off[a]) & (exc < off[z])]
            out.append(res)
        return out

    def bam_decode(self, blob, rec_off, cap_bases=None, cap_pairs=None, rec_limit=None, check=True):
        """plat_bam_decode_batch: ReadIterator.get (htslibWrapper.pyx:328-406) on the device.  blob: the bytes (uint8 array or bytes) holding
        uncompressed BAM alignment records, record i starting (at its refID) at blob[rec_off[i]].  Returns a dict of numpy arrays: off
        [n+1], cig_off [n+1], seq / qual [bases], cigar [pairs, 2], pos, end, mapq, flags, chrom_id, mate_chrom_id, insert_size, mate_pos
        [n], status [4] = {error, first offending record, bases, pairs}, and guard_intact: nothing was written behind the capacities (the
        PLAT_BLOB_PAD zeros behind the last base aside).  cap_bases / cap_pairs default to the bound the blob's length gives.  A refused
        record or a short capacity raises PlatypusDeviceError (check=False: returns, with status saying so)."""
        torch = _torch()
        blob = np.frombuffer(blob, dtype=np.uint8) if isinstance(blob, (bytes, bytearray)) else np.ascontiguousarray(blob, dtype=np.uint8)
        rec_off = np.ascontiguousarray(rec_off, dtype=np.int64)
        n, nbytes = len(rec_off), len(blob)
        body = max(0, nbytes - 32 * n)
        cap_b = body * 2 // 3 + n if cap_bases is None else int(cap_bases)
        cap_p = body // 4 if cap_pairs is None else int(cap_pairs)
        guard, fill = 64, 0xEE
        d_blob = torch.from_numpy(np.append(blob, np.zeros(1, np.uint8))).to(self.device)
        d_off = torch.from_numpy(np.append(rec_off, 0)).to(self.device)
        d_lim = torch.from_numpy(np.append(np.ascontiguousarray(rec_limit, dtype=np.int64), 0)).to(self.device) if rec_limit is not None else None
        e = lambda k, dt: torch.full((k,), fill if dt in (torch.uint8,) else 0, dtype=dt, device=self.device)
        g = dict(read_off=e(n + 1, torch.int64), cig_off=e(n + 1, torch.int32), seq=e(cap_b + _lib.PLAT_BLOB_PAD + guard, torch.uint8),
                 qual=e(cap_b + _lib.PLAT_BLOB_PAD + guard, torch.uint8), cigar=torch.full((2 * cap_p + guard,), 0x7EEE, dtype=torch.int16, device=self.device),
                 pos=e(max(n, 1), torch.int32), end=e(max(n, 1), torch.int32), mapq=e(max(n, 1), torch.uint8), flags=e(max(n, 1), torch.int32),
                 chrom_id=e(max(n, 1), torch.int16), mate_chrom_id=e(max(n, 1), torch.int16), insert_size=e(max(n, 1), torch.int32),
                 mate_pos=e(max(n, 1), torch.int32), status=e(4, torch.int64))
        o = _lib.BamDecodeOut(cap_b, cap_p, *[g[k].data_ptr() for k, _ in _lib.BamDecodeOut._fields_[2:]])
        _lib.check(self.lib.plat_bam_decode_batch(self.ctx, n, d_blob.data_ptr(), nbytes, d_off.data_ptr(), d_lim.data_ptr() if d_lim is not None else None,
                                                  C.byref(o), self._stream()), "plat_bam_decode_batch")
        self._sync()
        h = {k: v.cpu().numpy() for k, v in g.items()}
        st = h["status"]
        fits = int(st[0]) != -8
        nb, npairs = (int(st[2]), int(st[3])) if fits else (0, 0)
        tail = h["seq"][nb:], h["qual"][nb:]
        pad = _lib.PLAT_BLOB_PAD if fits else 0
        intact = all(not t[:pad].any() and (t[pad:] == fill).all() for t in tail) and bool((h["cigar"][2 * npairs:] == 0x7EEE).all())
        out = dict(off=h["read_off"], cig_off=h["cig_off"], seq=h["seq"][:nb], qual=h["qual"][:nb], cigar=h["cigar"][:2 * npairs].reshape(-1, 2),
                   status=st, guard_intact=intact)
        for k in ("pos", "end", "mapq", "flags", "chrom_id", "mate_chrom_id", "insert_size", "mate_pos"):
            out[k] = h[k][:n]
        if check and int(st[0]) != 0:
            raise _lib.PlatypusDeviceError(int(st[0]), "record %d" % int(st[1]), "plat_bam_decode_batch")
        return out

    def bgzf_inflate(self, blob, blk_off, cap_bytes=None, blk_limit=None, check=True, keep_device=False):
        """plat_bgzf_inflate_batch: the BGZF blocks starting at blob[blk_off[i]] inflated and CRC-checked on the device.  Returns a dict: data
        (the inflated bytes, back to back), out_off [n+1], status [4] = {error, lowest offending block, total bytes, 0} and guard_intact:
        nothing was written in front of data or behind cap_bytes (the PLAT_BLOB_PAD zeros behind the last byte aside).  cap_bytes defaults to
        the sum of the blocks' ISIZE words as a reader of the trailers finds them.  A refused block or a short capacity raises
        PlatypusDeviceError (check=False: returns, with status saying so).  keep_device=True adds the device tensors (for bam_find_records)."""
        torch = _torch()
        blob = np.frombuffer(blob, dtype=np.uint8) if isinstance(blob, (bytes, bytearray)) else np.ascontiguousarray(blob, dtype=np.uint8)
        blk_off = np.ascontiguousarray(blk_off, dtype=np.int64)
        n, nbytes = len(blk_off), len(blob)
        if cap_bytes is None:                                             # BSIZE at its usual place, ISIZE in the last four bytes
            cap_bytes = 0
            for o in blk_off.tolist():
                if 0 <= o and o + 18 <= nbytes:
                    end = o + int(blob[o + 16]) + (int(blob[o + 17]) << 8) + 1
                    if end <= nbytes and end - 4 >= 0:
                        cap_bytes += min(int.from_bytes(blob[end - 4:end].tobytes(), "little"), 65536)
        cap = int(cap_bytes)
        guard, fill = 64, 0xEE
        d_blob = torch.from_numpy(np.append(blob, np.zeros(1, np.uint8))).to(self.device)
        d_off = torch.from_numpy(np.append(blk_off, 0)).to(self.device)
        d_lim = torch.from_numpy(np.append(np.ascontiguousarray(blk_limit, dtype=np.int64), 0)).to(self.device) if blk_limit is not None else None
        d_all = torch.full((guard + cap + _lib.PLAT_BLOB_PAD + guard,), fill, dtype=torch.uint8, device=self.device)
        assert d_all.data_ptr() % 16 == 0 and guard % 16 == 0
        d_out_off = torch.zeros(n + 1, dtype=torch.int64, device=self.device)
        d_status = torch.zeros(4, dtype=torch.int64, device=self.device)
        o = _lib.BgzfInflateOut(cap, d_all.data_ptr() + guard, d_out_off.data_ptr(), d_status.data_ptr())
        _lib.check(self.lib.plat_bgzf_inflate_batch(self.ctx, n, d_blob.data_ptr(), nbytes, d_off.data_ptr(), d_lim.data_ptr() if d_lim is not None else None,
                                                    C.byref(o), self._stream()), "plat_bgzf_inflate_batch")
        self._sync()
        h, st = d_all.cpu().numpy(), d_status.cpu().numpy()
        fits = int(st[0]) != -8
        total = int(st[2]) if fits else 0
        pad = _lib.PLAT_BLOB_PAD if fits else 0
        tail = h[guard + total:]
        intact = bool((h[:guard] == fill).all()) and not tail[:pad].any() and bool((tail[pad:] == fill).all())
        out = dict(data=h[guard:guard + total], out_off=d_out_off.cpu().numpy(), status=st, guard_intact=intact)
        if keep_device:
            out["device"] = dict(all=d_all, data_ptr=d_all.data_ptr() + guard, out_off=d_out_off, n_blocks=n)
        if check and int(st[0]) != 0:
            raise _lib.PlatypusDeviceError(int(st[0]), "block %d" % int(st[1]), "plat_bgzf_inflate_batch")
        return out

    def bgzf_deflate(self, text, piece_off, level=1, cap_bytes=None, check=True):
        """plat_bgzf_deflate_batch: the pieces text[piece_off[i]:piece_off[i + 1]] deflated to BGZF blocks on the device (no EOF block).
        Returns a dict: data (the blocks, back to back), piece_out_off [n+1], status [4] = {error, first piece that does not fit or -1, total
        compressed bytes, blocks} and guard_intact: nothing was written in front of data or behind cap_bytes (the PLAT_BLOB_PAD zeros
        behind the last byte aside; on overflow nothing at all).  cap_bytes defaults to the bound the header gives, text_len + 31 per
        possible block.  A short capacity or refused offsets raise PlatypusDeviceError (check=False: returns, with status saying so)."""
        torch = _torch()
        text = np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray)) else np.ascontiguousarray(text, dtype=np.uint8)
        piece_off = np.ascontiguousarray(piece_off, dtype=np.int64)
        n, nbytes = len(piece_off) - 1, len(text)
        if n < 0:
            raise ValueError("piece_off holds n_pieces + 1 offsets")
        cap = int(nbytes + 31 * (nbytes // 0xff00 + n) if cap_bytes is None else cap_bytes)
        guard, fill = 64, 0xEE
        d_text = torch.from_numpy(np.append(text, np.zeros(1, np.uint8))).to(self.device)
        d_off = torch.from_numpy(piece_off.copy()).to(self.device)
        d_all = torch.full((guard + cap + _lib.PLAT_BLOB_PAD + guard,), fill, dtype=torch.uint8, device=self.device)
        assert d_all.data_ptr() % 16 == 0 and guard % 16 == 0
        d_out_off = torch.zeros(n + 1, dtype=torch.int64, device=self.device)
        d_status = torch.zeros(4, dtype=torch.int64, device=self.device)
        i = _lib.BgzfDeflateIn(d_text.data_ptr(), nbytes, n, int(level), d_off.data_ptr())
        o = _lib.BgzfDeflateOut(cap, d_all.data_ptr() + guard, d_out_off.data_ptr(), d_status.data_ptr())
        _lib.check(self.lib.plat_bgzf_deflate_batch(self.ctx, C.byref(i), C.byref(o), self._stream()), "plat_bgzf_deflate_batch")
        self._sync()
        h, st = d_all.cpu().numpy(), d_status.cpu().numpy()
        fits = int(st[0]) == 0
        total = int(st[2]) if fits else 0
        pad = _lib.PLAT_BLOB_PAD if int(st[0]) != -8 else 0
        tail = h[guard + total:]
        intact = bool((h[:guard] == fill).all()) and not tail[:pad].any() and bool((tail[pad:] == fill).all())
        out = dict(data=h[guard:guard + total], piece_out_off=d_out_off.cpu().numpy(), status=st, guard_intact=intact)
        if check and int(st[0]) != 0:
            raise _lib.PlatypusDeviceError(int(st[0]), "piece %d, %d bytes needed" % (int(st[1]), int(st[2])), "plat_bgzf_deflate_batch")
        return out

    def bam_find_records(self, inflated, streams, cap_records=None, check=True):
        """plat_bam_find_records: sam_itr_next over the output of bgzf_inflate(..., keep_device=True).  streams: per stream (tid, beg, end,
        chunks), chunks a list of (blk_first, blk_end, first_uoffset, stop_blk or -1, stop_uoffset).  Returns a dict: rec_off / rec_limit
        (the kept records of all streams back to back), stream_begin [n+1], status [4] = {error, lowest offending stream, kept, walked} and
        guard_intact: nothing was written behind cap_records (default: one record per 36 inflated bytes, the bound the format gives)."""
        torch = _torch()
        dv = inflated["device"]
        total = int(inflated["status"][2])
        cap = total // 36 + 1 if cap_records is None else int(cap_records)
        i32 = lambda a: torch.from_numpy(np.append(np.asarray(a, dtype=np.int32), np.int32(0))).to(self.device)
        chunks = [c for s in streams for c in s[3]]
        begin = np.concatenate([[0], np.cumsum([len(s[3]) for s in streams])]) if streams else np.zeros(1)
        cols = [i32([c[k] for c in chunks]) for k in range(5)]
        d_begin, d_tid, d_beg, d_end = i32(begin)[:len(streams) + 1], i32([s[0] for s in streams]), i32([s[1] for s in streams]), i32([s[2] for s in streams])
        guard, fill = 16, 0x7EEE7EEE7EEE7EEE
        d_off = torch.full((cap + guard,), fill, dtype=torch.int64, device=self.device)
        d_lim = torch.full((cap + guard,), fill, dtype=torch.int64, device=self.device)
        d_sb = torch.zeros(len(streams) + 1, dtype=torch.int32, device=self.device)
        d_status = torch.zeros(4, dtype=torch.int64, device=self.device)
        fi = _lib.BamFindIn(len(streams), len(chunks), dv["n_blocks"], 0, dv["data_ptr"], dv["out_off"].data_ptr(), d_begin.data_ptr(),
                            *[c.data_ptr() for c in cols], d_tid.data_ptr(), d_beg.data_ptr(), d_end.data_ptr())
        fo = _lib.BamFindOut(cap, d_off.data_ptr(), d_lim.data_ptr(), d_sb.data_ptr(), d_status.data_ptr())
        _lib.check(self.lib.plat_bam_find_records(self.ctx, C.byref(fi), C.byref(fo), self._stream()), "plat_bam_find_records")
        self._sync()
        st, off, lim = d_status.cpu().numpy(), d_off.cpu().numpy(), d_lim.cpu().numpy()
        kept = min(int(st[2]), cap)
        out = dict(rec_off=off[:kept], rec_limit=lim[:kept], stream_begin=d_sb.cpu().numpy(), status=st,
                   guard_intact=bool((off[kept:] == fill).all() and (lim[kept:] == fill).all()))
        if check and int(st[0]) != 0:
            raise _lib.PlatypusDeviceError(int(st[0]), "stream %d" % int(st[1]), "plat_bam_find_records")
        return out

    def bam_route(self, blob, rec_off, rec_end, stream_begin, group_ids, group_sample, n_samples, n_records=None, check=True):
        """plat_bam_route_batch: the records of a merged BAM file routed to samples by their RG field, on the device.  blob / rec_off as
        bam_decode takes them, rec_end [n] the records' ends; stream_begin [n_streams + 1]: the fetches; group_ids: the read groups' IDs
        (bytes), group_sample [n_groups] their samples.  n_records: the record capacity handed to the call (default: len(rec_off); the
        records behind stream_begin[-1] are not looked at).  Returns a dict: rec_off / rec_limit (the routed records, per stream sample
        after sample), out_begin [n_streams * n_samples + 1], rec_sample [n] (-1: refused), status [4] = {error, lowest offending record,
        routed, refused}, why (the rule that refused that record, an index of _lib.ROUTE_WHY) and guard_intact: nothing was written behind
        any output (or, when the call is refused as invalid, at all).  A refused record raises PlatypusDeviceError (check=False:
        returns, with status saying so); limits exceeded raise it with PLAT_ERR_UNSUPPORTED either way."""
        torch = _torch()
        blob = np.frombuffer(blob, dtype=np.uint8) if isinstance(blob, (bytes, bytearray)) else np.ascontiguousarray(blob, dtype=np.uint8)
        rec_off, rec_end = np.ascontiguousarray(rec_off, dtype=np.int64), np.ascontiguousarray(rec_end, dtype=np.int64)
        stream_begin = np.ascontiguousarray(stream_begin, dtype=np.int32)
        n = len(rec_off) if n_records is None else int(n_records)
        n_streams, n_groups = len(stream_begin) - 1, len(group_ids)
        ids = [bytes(g) for g in group_ids]
        g_off = np.concatenate([[0], np.cumsum([len(g) for g in ids])]).astype(np.int32)
        dev = lambda a, dt: torch.from_numpy(np.append(np.asarray(a, dtype=dt), np.zeros(1, dtype=dt))).to(self.device)
        d_blob, d_off, d_end, d_sb = dev(blob, np.uint8), dev(rec_off, np.int64), dev(rec_end, np.int64), dev(stream_begin, np.int32)
        d_ids, d_goff, d_gs = dev(np.frombuffer(b"".join(ids), dtype=np.uint8), np.uint8), dev(g_off, np.int32), dev(group_sample, np.int32)
        guard, f64, f32 = 16, 0x7EEE7EEE7EEE7EEE, 0x7EEE7EEE
        keys = n_streams * int(n_samples)
        o_off = torch.full((n + guard,), f64, dtype=torch.int64, device=self.device)
        o_lim = torch.full((n + guard,), f64, dtype=torch.int64, device=self.device)
        o_begin = torch.full((keys + 1 + guard,), f32, dtype=torch.int32, device=self.device)
        o_sample = torch.full((n + guard,), f32, dtype=torch.int32, device=self.device)
        o_status = torch.full((4 + guard,), f64, dtype=torch.int64, device=self.device)
        o_why = torch.full((1 + guard,), f32, dtype=torch.int32, device=self.device)
        qi = _lib.BamRouteIn(n, n_streams, n_groups, int(n_samples), d_blob.data_ptr(), len(blob), d_off.data_ptr(), d_end.data_ptr(), d_sb.data_ptr(),
                             d_ids.data_ptr(), d_goff.data_ptr(), d_gs.data_ptr())
        qo = _lib.BamRouteOut(o_off.data_ptr(), o_lim.data_ptr(), o_begin.data_ptr(), o_sample.data_ptr(), o_status.data_ptr(), o_why.data_ptr())
        _lib.check(self.lib.plat_bam_route_batch(self.ctx, C.byref(qi), C.byref(qo), self._stream()), "plat_bam_route_batch")
        self._sync()
        off, lim, begin, smp, st, why = (t.cpu().numpy() for t in (o_off, o_lim, o_begin, o_sample, o_status, o_why))
        invalid = int(st[0]) == -1
        routed = 0 if invalid else int(st[2])
        used = 0 if invalid else int(stream_begin[-1])
        kb = 0 if invalid else keys + 1
        intact = bool((off[routed:] == f64).all() and (lim[routed:] == f64).all() and (begin[kb:] == f32).all() and (smp[used:] == f32).all() and
                      (st[4:] == f64).all() and (why[1:] == f32).all())
        out = dict(rec_off=off[:routed], rec_limit=lim[:routed], out_begin=begin[:kb], rec_sample=smp[:used], status=st[:4], why=int(why[0]),
                   guard_intact=intact)
        if check and int(st[0]) != 0:
            raise _lib.PlatypusDeviceError(int(st[0]), "record %d: %s" % (int(st[1]), _lib.ROUTE_WHY[out["why"]] if 0 <= out["why"] < 8 else "?"),
                                           "plat_bam_route_batch")
        return out

    def bam_mates(self, blob, rec_off, rec_limit, stream_begin, mode, want_tid=None, lo=None, hi=None, cap_records=None, cap_bytes=None,
                  n_records=None, check=True):
        """plat_bam_mates_batch: the device pass of the broken-mate fetch over records as plat_bam_find_records leaves them (blob, rec_off /
        rec_limit, stream_begin [n_streams + 1]).  mode "coords": the (mtid, mpos) pairs of the records that give one; "fetch": the records
        of stream s with mtid == want_tid[s] and lo[s] <= mpos <= hi[s], copied back to back.  cap_records / cap_bytes: the capacities
        handed over (default: every record, every byte).  Returns a dict: status [4] = {error, lowest offending stream, kept, looked at},
        need_bytes, begin [n_streams + 1], coords [kept, 2] or data / rec_off / rec_len / mpos, pad (the PLAT_BLOB_PAD bytes behind the last
        record) and guard_intact: nothing was written behind a capacity.  A refusal raises PlatypusDeviceError (check=False: returns)."""
        torch = _torch()
        blob = np.frombuffer(blob, dtype=np.uint8) if isinstance(blob, (bytes, bytearray)) else np.ascontiguousarray(blob, dtype=np.uint8)
        rec_off, rec_limit = np.ascontiguousarray(rec_off, dtype=np.int64), np.ascontiguousarray(rec_limit, dtype=np.int64)
        stream_begin = np.ascontiguousarray(stream_begin, dtype=np.int32)
        fetch = mode == "fetch"
        n = len(rec_off) if n_records is None else int(n_records)
        n_streams = len(stream_begin) - 1
        pad = _lib.PLAT_BLOB_PAD
        cap_r = n if cap_records is None else int(cap_records)
        cap_b = len(blob) if cap_bytes is None else int(cap_bytes)
        dev = lambda a, dt: torch.from_numpy(np.append(np.asarray(a, dtype=dt), np.zeros(1, dtype=dt))).to(self.device)
        d_blob = torch.from_numpy(np.concatenate([blob, np.zeros(pad, dtype=np.uint8)])).to(self.device)
        d_off, d_lim, d_sb = dev(rec_off, np.int64), dev(rec_limit, np.int64), dev(stream_begin, np.int32)
        zeros = np.zeros(n_streams, dtype=np.int32)
        d_want, d_lo, d_hi = (dev(zeros if a is None else a, np.int32) for a in (want_tid, lo, hi))
        guard, f64, f32, f8 = 16, 0x7EEE7EEE7EEE7EEE, 0x7EEE7EEE, 0xEE
        o_coords = torch.full((2 * cap_r + guard,), f32, dtype=torch.int32, device=self.device)
        o_begin = torch.full((n_streams + 1 + guard,), f32, dtype=torch.int32, device=self.device)
        o_data = torch.full((cap_b + pad + 4 * guard,), f8, dtype=torch.uint8, device=self.device)
        o_off = torch.full((cap_r + guard,), f64, dtype=torch.int64, device=self.device)
        o_len = torch.full((cap_r + guard,), f32, dtype=torch.int32, device=self.device)
        o_mpos = torch.full((cap_r + guard,), f32, dtype=torch.int32, device=self.device)
        o_status = torch.full((4 + guard,), f64, dtype=torch.int64, device=self.device)
        o_need = torch.full((1 + guard,), f64, dtype=torch.int64, device=self.device)
        mi = _lib.BamMatesIn(n_streams, n, _lib.MATES_FETCH if fetch else _lib.MATES_COORDS, 0, d_blob.data_ptr(), len(blob), d_off.data_ptr(), d_lim.data_ptr(),
                             d_sb.data_ptr(), d_want.data_ptr(), d_lo.data_ptr(), d_hi.data_ptr())
        mo = _lib.BamMatesOut(cap_r, cap_b, o_coords.data_ptr(), o_begin.data_ptr(), o_data.data_ptr(), o_off.data_ptr(), o_len.data_ptr(), o_mpos.data_ptr(),
                              o_begin.data_ptr(), o_status.data_ptr(), o_need.data_ptr())
        _lib.check(self.lib.plat_bam_mates_batch(self.ctx, C.byref(mi), C.byref(mo), self._stream()), "plat_bam_mates_batch")
        self._sync()
        coords, begin, data, off, ln, mpos, st, need = (t.cpu().numpy() for t in (o_coords, o_begin, o_data, o_off, o_len, o_mpos, o_status, o_need))
        over = int(st[0]) == -8
        kept = min(int(st[2]), cap_r) if int(st[0]) != -1 else 0
        nb = int(need[0])
        out = dict(status=st[:4], need_bytes=nb, begin=begin[:n_streams + 1])
        intact = bool((begin[n_streams + 1:] == f32).all() and (st[4:] == f64).all() and (need[1:] == f64).all())
        if fetch:
            end = min(nb, cap_b) + (0 if over else pad)
            if over:                                                           # (what was written is a prefix that fits both capacities)
                fits = (off[:kept] != f64) & (off[:kept] + ln[:kept] <= cap_b)
                kept = int(fits.sum()) if fits.all() or not fits.any() else int(np.argmin(fits))
                end = int(off[kept - 1] + ln[kept - 1]) if kept else 0
            intact = intact and bool((data[end:] == f8).all() and (off[kept:] == f64).all() and (ln[kept:] == f32).all() and (mpos[kept:] == f32).all() and
                                     (coords == f32).all())
            out.update(data=data[:min(nb, cap_b)], rec_off=off[:kept], rec_len=ln[:kept], mpos=mpos[:kept], pad=data[min(nb, cap_b):min(nb, cap_b) + pad])
        else:
            intact = intact and bool((coords[2 * kept:] == f32).all() and (data == f8).all() and (off == f64).all() and (ln == f32).all() and (mpos == f32).all())
            out.update(coords=coords[:2 * kept].reshape(-1, 2))
        out["guard_intact"] = intact
        if check and int(st[0]) != 0:
            raise _lib.PlatypusDeviceError(int(st[0]), "stream %d" % int(st[1]), "plat_bam_mates_batch")
        return out

    def source_variants(self, regions, names, max_size=1500, long_haps=0, cap_variants=None, lead=0, text_off=None, check=True):
        """plat_source_variants_batch: VariantCandidateReader.Variants' line loop (variantutils.py:72-159,168-197) on the device.  regions:
        per region the bytes a fetch returned (the source files' fetches back to back); names: the regions' chromosomes (bytes / str) or
        their Python-2 string hashes.  lead: bytes of other text in front of the first region (the regions then start at text_off[0] = lead);
        text_off: offsets to hand over instead of the ones the regions' lengths give (tests of the checks).  Returns a dict: region_begin
        [n + 1], pos / rem_off / n_rem / add_off / n_add / hash / line [alleles written], stats [n, 4] = {lines, skipped, invalid, over
        maxSize}, status [4] = {error, lowest refused (region << 32 | line), alleles, lines}, text (the uploaded bytes: what the offsets
        index) and guard_intact: nothing was written behind the capacity (or, when the call is refused as invalid, at all).  A refused line
        or a short capacity raises PlatypusDeviceError (check=False: returns, with status saying so)."""
        from .vcfrecords import _py2_string_hash
        torch = _torch()
        blobs = [bytes(r) for r in regions]
        n = len(blobs)
        text = b"\n" * int(lead) + b"".join(blobs)
        off = np.concatenate([[int(lead)], int(lead) + np.cumsum([len(b) for b in blobs])]).astype(np.int64) if text_off is None else np.asarray(text_off, dtype=np.int64)
        hashes = np.array([(h if isinstance(h, int) else _py2_string_hash(h.decode("latin-1") if isinstance(h, bytes) else h)) for h in names], dtype=np.uint64).view(np.int64)
        cap = len(text) + 1 if cap_variants is None else int(cap_variants)
        guard, f64, f32 = 16, 0x7EEE7EEE7EEE7EEE, 0x7EEE7EEE
        d_text = torch.from_numpy(np.frombuffer(text + b"\xff" * (_lib.PLAT_BLOB_PAD + 16), dtype=np.uint8).copy()).to(self.device)
        d_off = torch.from_numpy(np.append(off, 0)).to(self.device)
        d_hash = torch.from_numpy(np.append(hashes, 0)).to(self.device)
        i32 = lambda k: torch.full((k + guard,), f32, dtype=torch.int32, device=self.device)
        i64 = lambda k: torch.full((k + guard,), f64, dtype=torch.int64, device=self.device)
        g = dict(region_begin=i32(n + 1), pos=i32(cap), rem_off=i64(cap), n_rem=i32(cap), add_off=i64(cap), n_add=i32(cap), hash=i32(cap), line=i32(cap),
                 region_stats=i32(4 * n), status=i64(4))
        qi = _lib.SourceVariantsIn(n, int(max_size), int(long_haps), 0, d_text.data_ptr(), len(text), d_off.data_ptr(), d_hash.data_ptr())
        qo = _lib.SourceVariantsOut(cap, *[g[k].data_ptr() for k, _ in _lib.SourceVariantsOut._fields_[1:]])
        _lib.check(self.lib.plat_source_variants_batch(self.ctx, C.byref(qi), C.byref(qo), self._stream()), "plat_source_variants_batch")
        self._sync()
        h = {k: v.cpu().numpy() for k, v in g.items()}
        st = h["status"]
        invalid = int(st[0]) == -1
        written = 0 if invalid else min(int(st[2]), cap)
        sizes = dict(region_begin=0 if invalid else n + 1, region_stats=0 if invalid else 4 * n, status=4)
        intact = all(bool((h[k][sizes.get(k, written):] == (f64 if h[k].dtype == np.int64 else f32)).all()) for k in h)
        out = {k: h[k][:sizes.get(k, written)] for k in h if k not in ("region_stats", "status")}
        out.update(stats=h["region_stats"][:sizes["region_stats"]].reshape(-1, 4), status=st[:4], text=text, guard_intact=intact)
        if check and int(st[0]) != 0:
            raise _lib.PlatypusDeviceError(int(st[0]), "region %d line %d" % (int(st[1]) >> 32, int(st[1]) & 0xffffffff) if int(st[0]) == -9 else "%d alleles" % int(st[2]),
                                           "plat_source_variants_batch")
        return out

    def tabix_fetch(self, inflated, geometry, cap_text=None):
        """plat_tabix_fetch_batch: tabix's iterator (ti_iter_read, index.c.pysam.c:872-911) over the output of bgzf_inflate(...,
        keep_device=True).  geometry: the arrays plat_tabix_fetch_in names (stream_chunk_begin, chunk_blk_first, chunk_blk_end,
        chunk_first_uoffset, chunk_stop_blk, chunk_stop_uoffset, names, name_off, beg, end).  Returns a dict: text (the kept lines, at most
        cap_text bytes -- default: inflated bytes + chunks, which always suffices), off [n + 1], counts [2 n] (walked, kept per stream),
        status [4] = {error, lowest refused stream, kept lines, kept bytes} and guard_intact: nothing was written behind the text but the
        PLAT_BLOB_PAD zeros, or behind any other output (nothing at all but the status when the call is refused as invalid)."""
        torch = _torch()
        dv = inflated["device"]
        total = int(inflated["status"][2])
        n, n_chunks = len(geometry["beg"]), len(geometry["chunk_blk_first"])
        cap = total + n_chunks if cap_text is None else int(cap_text)
        dev = lambda a, dt: torch.from_numpy(np.append(np.asarray(a, dtype=dt), np.zeros(1, dtype=dt))).to(self.device)
        keys = ("stream_chunk_begin", "chunk_blk_first", "chunk_blk_end", "chunk_first_uoffset", "chunk_stop_blk", "chunk_stop_uoffset")
        d = {k: dev(geometry[k], np.int32) for k in keys + ("name_off", "beg", "end")}
        d_names = dev(geometry["names"], np.uint8)
        guard, fill, f64 = 64, 0xEE, 0x7EEE7EEE7EEE7EEE
        d_text = torch.full((guard + cap + _lib.PLAT_BLOB_PAD + guard,), fill, dtype=torch.uint8, device=self.device)
        assert d_text.data_ptr() % 16 == 0
        d_off = torch.full((n + 1 + 16,), f64, dtype=torch.int64, device=self.device)
        d_counts = torch.full((2 * n + 16,), f64, dtype=torch.int64, device=self.device)
        d_status = torch.full((4 + 16,), f64, dtype=torch.int64, device=self.device)
        fi = _lib.TabixFetchIn(n, n_chunks, dv["n_blocks"], 0, dv["data_ptr"], total, dv["out_off"].data_ptr(), *[d[k].data_ptr() for k in keys],
                               d_names.data_ptr(), d["name_off"].data_ptr(), d["beg"].data_ptr(), d["end"].data_ptr())
        fo = _lib.TabixFetchOut(cap, d_text.data_ptr() + guard, d_off.data_ptr(), d_counts.data_ptr(), d_status.data_ptr())
        _lib.check(self.lib.plat_tabix_fetch_batch(self.ctx, C.byref(fi), C.byref(fo), self._stream()), "plat_tabix_fetch_batch")
        self._sync()
        h, off, counts, st = (t.cpu().numpy() for t in (d_text, d_off, d_counts, d_status))
        invalid = int(st[0]) == -1
        used = 0 if invalid else min(int(st[3]), cap)
        pad = 0 if invalid else _lib.PLAT_BLOB_PAD
        tail = h[guard + used:]
        n_off, n_counts = (0, 0) if invalid else (n + 1, 2 * n)
        intact = (bool((h[:guard] == fill).all()) and not tail[:pad].any() and bool((tail[pad:] == fill).all()) and bool((off[n_off:] == f64).all()) and
                  bool((counts[n_counts:] == f64).all()) and bool((st[4:] == f64).all()))
        return dict(text=h[guard:guard + used].tobytes(), off=off[:n_off].tolist(), counts=counts[:n_counts].tolist(), status=st[:4].tolist(), guard_intact=intact)

    def tabix_index(self, inflated, blk_addr, cap_runs=None, cap_names=None, cap_windows=None, cap_name_bytes=None):
        """plat_tabix_index_batch: ti_index_core (index.c.pysam.c:320-393) over the output of bgzf_inflate(..., keep_device=True) for a whole
        bgzipped VCF.  blk_addr [n_blocks + 1]: the blocks' file addresses and the address behind the last.  Returns a dict: runs [(tid, bin,
        u)], names [(offset, length)] into the data, name_bytes (the names back to back), lin_first, lin (what fits the capacities -- default: a run per 16 bytes, 4096 contigs,
        64 KiB of names, 2^18 windows), status [13] and guard_intact: nothing was written behind a capacity or the status block."""
        torch = _torch()
        dv = inflated["device"]
        total, n_blocks = int(inflated["status"][2]), dv["n_blocks"]
        cap_r = total // 16 + 64 if cap_runs is None else int(cap_runs)
        cap_n = 4096 if cap_names is None else int(cap_names)
        cap_w = 1 << 18 if cap_windows is None else int(cap_windows)
        cap_b = 1 << 16 if cap_name_bytes is None else int(cap_name_bytes)
        d_nbytes = torch.full((cap_b + 64,), 0xEE, dtype=torch.uint8, device=self.device)
        f64, f32 = 0x7EEE7EEE7EEE7EEE, 0x7EEE7EEE
        d_addr = torch.from_numpy(np.ascontiguousarray(blk_addr, dtype=np.int64).copy()).to(self.device)
        full = lambda n, big: torch.full((n + 16,), f64 if big else f32, dtype=torch.int64 if big else torch.int32, device=self.device)
        d_tid, d_bin, d_u, d_noff, d_nlen = full(cap_r, False), full(cap_r, False), full(cap_r, True), full(cap_n, True), full(cap_n, False)
        d_first, d_lin, d_status = full(cap_n + 1, True), full(cap_w, True), full(_lib.TBI_STATUS_WORDS, True)
        i = _lib.TabixIndexIn(n_blocks, 0, dv["data_ptr"], total, dv["out_off"].data_ptr(), d_addr.data_ptr())
        o = _lib.TabixIndexOut(cap_r, cap_n, cap_w, cap_b, d_tid.data_ptr(), d_bin.data_ptr(), d_u.data_ptr(), d_noff.data_ptr(), d_nlen.data_ptr(), d_nbytes.data_ptr(), d_first.data_ptr(),
                               d_lin.data_ptr(), d_status.data_ptr())
        _lib.check(self.lib.plat_tabix_index_batch(self.ctx, C.byref(i), C.byref(o), self._stream()), "plat_tabix_index_batch")
        self._sync()
        tid, b, u, noff, nlen, first, lin, st = (t.cpu().numpy() for t in (d_tid, d_bin, d_u, d_noff, d_nlen, d_first, d_lin, d_status))
        ok = int(st[0]) in (0, -8)
        n_r = min(int(st[4]), cap_r) if ok else 0
        n_n = min(int(st[5]), cap_n) if ok else 0
        n_w = int(st[6]) if ok and int(st[6]) <= cap_w else 0
        n_b = int(st[12]) if ok and int(st[12]) <= cap_b else 0
        nbytes = d_nbytes.cpu().numpy()
        intact = (bool((st[_lib.TBI_STATUS_WORDS:] == f64).all()) and bool((tid[cap_r:] == f32).all()) and bool((b[cap_r:] == f32).all()) and
                  bool((u[cap_r:] == f64).all()) and bool((noff[cap_n:] == f64).all()) and bool((nlen[cap_n:] == f32).all()) and
                  bool((first[cap_n + 1:] == f64).all()) and bool((lin[cap_w:] == f64).all()) and bool((nbytes[cap_b:] == 0xEE).all()))
        if ok:                                                           # (short of a capacity nothing but what the counts name is written either)
            intact = (intact and bool((tid[n_r:] == f32).all()) and bool((u[n_r:] == f64).all()) and bool((noff[n_n:] == f64).all()) and
                      bool((lin[n_w:] == f64).all()) and bool((nbytes[n_b:] == 0xEE).all()))
        return dict(runs=list(zip(tid[:n_r].tolist(), b[:n_r].tolist(), u[:n_r].tolist())), names=list(zip(noff[:n_n].tolist(), nlen[:n_n].tolist())),
                    name_bytes=nbytes[:n_b].tobytes(), lin_first=first[:n_n + 1].tolist() if ok else [], lin=lin[:n_w].tolist(), status=st[:_lib.TBI_STATUS_WORDS].tolist(), guard_intact=intact)

    def index_tables(self, flat):
        """The flat tables of one index (a dict of ref_bin_first, bin_id, bin_chunk_first, chunk_u, chunk_v, ref_lin_first, lin_fill, as
        tests/index_query_cases.py and csrc/index_query.hpp make them) uploaded once: what index_query takes."""
        torch = _torch()
        dt = dict(bin_id=np.int32)
        up = lambda k: torch.from_numpy(np.append(np.asarray(flat[k], dtype=dt.get(k, np.int64)), np.zeros(1, dtype=dt.get(k, np.int64)))).to(self.device)
        d = {k: up(k) for k in ("ref_bin_first", "bin_id", "bin_chunk_first", "chunk_u", "chunk_v", "ref_lin_first", "lin_fill")}
        d["sizes"] = (len(flat["ref_bin_first"]) - 1, len(flat["bin_id"]), len(flat["chunk_u"]), len(flat["lin_fill"]))
        return d

    def index_query(self, tables, queries, cap_chunks=None, sizes=None):
        """plat_index_query_batch: ti_iter_query (index.c.pysam.c:776-870) for queries [(tid, beg, end)] over index_tables(...).  sizes: (n_ref,
        n_bins, n_chunks, n_lin) to hand over instead of the tables' own (tests of the checks).  Returns a dict: chunks [per query a list of
        (u, v), None for count -1 and -2, all None when they do not fit cap_chunks -- default 4 per query + 4096], count, gathered, first
        [n + 1], status [6] and guard_intact: nothing was written behind a capacity (nothing at all but the status when the call is
        refused as invalid, no chunk on an overflow)."""
        torch = _torch()
        n = len(queries)
        cap = 4 * n + 4096 if cap_chunks is None else int(cap_chunks)
        q = np.asarray(queries, dtype=np.int32).reshape(n, 3)
        d_q = [torch.from_numpy(np.append(q[:, k], np.zeros(1, dtype=np.int32)).astype(np.int32)).to(self.device) for k in range(3)]
        f64, f32, guard = 0x7EEE7EEE7EEE7EEE, 0x7EEE7EEE, 16
        full = lambda k, big: torch.full((k + guard,), f64 if big else f32, dtype=torch.int64 if big else torch.int32, device=self.device)
        d_count, d_gath, d_first, d_u, d_v, d_status = full(n, False), full(n, False), full(n + 1, True), full(cap, True), full(cap, True), full(_lib.IDXQ_STATUS_WORDS, True)
        n_ref, n_bins, n_chunks, n_lin = tables["sizes"] if sizes is None else sizes
        i = _lib.IndexQueryIn(n_ref, n, n_bins, n_chunks, n_lin, *[tables[k].data_ptr() for k in ("ref_bin_first", "bin_id", "bin_chunk_first", "chunk_u", "chunk_v",
                                                                                              "ref_lin_first", "lin_fill")], *[t.data_ptr() for t in d_q])
        o = _lib.IndexQueryOut(cap, d_count.data_ptr(), d_gath.data_ptr(), d_first.data_ptr(), d_u.data_ptr(), d_v.data_ptr(), d_status.data_ptr())
        _lib.check(self.lib.plat_index_query_batch(self.ctx, C.byref(i), C.byref(o), self._stream()), "plat_index_query_batch")
        self._sync()
        count, gath, first, u, v, st = (t.cpu().numpy() for t in (d_count, d_gath, d_first, d_u, d_v, d_status))
        verdict = int(st[0])
        n_q = n if verdict in (0, -8) else 0
        used = int(st[2]) if verdict == 0 else 0
        intact = (bool((st[_lib.IDXQ_STATUS_WORDS:] == f64).all()) and bool((count[n_q:] == f32).all()) and bool((gath[n_q:] == f32).all()) and
                  bool((first[(n + 1 if verdict in (0, -8) else 0):] == f64).all()) and bool((u[used:] == f64).all()) and bool((v[used:] == f64).all()))
        chunks = None
        if verdict == 0:
            u64, v64 = u.view(np.uint64), v.view(np.uint64)
            chunks = [None if count[k] < 0 else list(zip(u64[first[k]:first[k + 1]].tolist(), v64[first[k]:first[k + 1]].tolist())) for k in range(n)]
        return dict(chunks=chunks, count=count[:n_q].tolist(), gathered=gath[:n_q].tolist(), first=first[:n_q + 1].tolist() if verdict in (0, -8) else [],
                    status=st[:_lib.IDXQ_STATUS_WORDS].tolist(), guard_intact=intact)

    def fasta_fetch(self, cut, queries, file_base=0, file_size=None, cap_bytes=None, guard=64):
        """plat_fasta_fetch_batch: FastaFile.getSequence (fastafile.pyx:173-207) and the whole-contig fetch for queries [(StartPos, LineLength,
        FullLineLength, SeqLength, beg, end, mode)] over `cut`, the bytes file_base .. file_base + len(cut) of a file of file_size bytes
        (default: the cut is the file's end).  Returns a dict: seqs [per query bytes, None when they do not fit cap_bytes -- default: the
        cut's length], status [n], off [n + 1], totals [4] and guard_intact: no byte in front of the blob, behind the bytes the totals name
        or behind an array's end was written."""
        torch = _torch()
        n = len(queries)
        cut = np.frombuffer(bytes(cut), dtype=np.uint8)
        size = file_base + len(cut) if file_size is None else int(file_size)
        cap = len(cut) if cap_bytes is None else int(cap_bytes)
        q = np.asarray([[int(x) for x in t] for t in queries], dtype=np.int64).reshape(n, 7)
        d_file = torch.from_numpy(np.append(cut, np.zeros(16, dtype=np.uint8))).to(self.device)[:len(cut)]        # (torch allocates aligned)
        d_q = [torch.from_numpy(np.append(q[:, k], np.zeros(1, dtype=np.int64))).to(self.device) for k in range(6)]
        d_mode = torch.from_numpy(np.append(q[:, 6], np.zeros(1, dtype=np.int64)).astype(np.uint8)).to(self.device)
        f64, f32 = 0x7EEE7EEE7EEE7EEE, 0x7EEE7EEE
        d_off = torch.full((n + 1 + 16,), f64, dtype=torch.int64, device=self.device)
        d_status = torch.full((n + 16,), f32, dtype=torch.int32, device=self.device)
        d_totals = torch.full((_lib.FASTA_STATUS_WORDS + 16,), f64, dtype=torch.int64, device=self.device)
        d_out = torch.full((guard + cap + guard,), 0xEE, dtype=torch.uint8, device=self.device)
        i = _lib.FastaFetchIn(d_file.data_ptr(), len(cut), int(file_base), size, n, *[t.data_ptr() for t in d_q], d_mode.data_ptr())
        o = _lib.FastaFetchOut(cap, d_off.data_ptr(), d_status.data_ptr(), d_out.data_ptr() + guard, d_totals.data_ptr())
        _lib.check(self.lib.plat_fasta_fetch_batch(self.ctx, C.byref(i), C.byref(o), self._stream()), "plat_fasta_fetch_batch")
        self._sync()
        off, status, totals, out = (t.cpu().numpy() for t in (d_off, d_status, d_totals, d_out))
        fits = int(totals[0]) == 0
        used = int(totals[1]) if fits else 0
        intact = (bool((off[n + 1:] == f64).all()) and bool((status[n:] == f32).all()) and bool((totals[_lib.FASTA_STATUS_WORDS:] == f64).all()) and
                  bool((out[:guard] == 0xEE).all()) and bool((out[guard + used:] == 0xEE).all()))
        blob = out[guard:guard + used].tobytes()
        return dict(seqs=[blob[off[k]:off[k + 1]] if fits else None for k in range(n)], status=status[:n].tolist(), off=off[:n + 1].tolist(),
                    totals=totals[:_lib.FASTA_STATUS_WORDS].tolist(), guard_intact=intact)

    def refcall_coverage(self, read_pos, read_end, slices, intervals, tile_first=None):
        """plat_refcall_coverage_batch: the loop of outputRefCall (variantcaller.pyx:774-784) over ReadArray.countReadsCoveringRegion
        (cwindow.pyx:176-206) on the device.  read_pos / read_end: the read table; slices: [(begin, n, longest)], one sample's good reads each;
        intervals: [(start, end, slice_first, n_samples, per_position)].  tile_first: the tile list to hand over instead of the one the
        intervals' lengths give (tests).  Returns (iv_min [n_intervals], counts): counts[k] is None or the interval's per-position
        minima over its samples (no entries for an interval without samples: nothing is written for it); PLAT_REFCOV_RAISES where the reference raises, PLAT_REFCOV_EMPTY for a minimum over nothing."""
        torch = _torch()
        nI, nS = len(intervals), len(slices)
        if nI == 0:
            return np.zeros(0, dtype=np.int32), []
        pos, end = np.ascontiguousarray(read_pos, dtype=np.int32), np.ascontiguousarray(read_end, dtype=np.int32)
        iv = np.asarray([[int(x) for x in t] for t in intervals], dtype=np.int64).reshape(nI, 5)
        length = np.maximum(iv[:, 1] - iv[:, 0], 0)
        off = np.full(nI, -1, dtype=np.int64)
        total = 0
        for k in range(nI):
            if iv[k, 4]:
                off[k] = total
                total += int(length[k])
        tiles = np.maximum(1, (length + _lib.PLAT_REFCOV_TILE - 1) // _lib.PLAT_REFCOV_TILE)
        first = np.concatenate([[0], np.cumsum(tiles)]).astype(np.int32) if tile_first is None else np.asarray(tile_first, dtype=np.int32)
        n_tiles = int(first[-1])

        def dev(a, dt):
            return torch.from_numpy(np.append(np.ascontiguousarray(a, dtype=dt), np.zeros(1, dtype=dt))).to(self.device)
        sl = np.asarray(slices, dtype=np.int64).reshape(nS, 3)
        d = dict(pos=dev(pos, np.int32), end=dev(end, np.int32), sb=dev(sl[:, 0], np.int32), sn=dev(sl[:, 1], np.int32), slong=dev(sl[:, 2], np.int32),
                 s=dev(iv[:, 0], np.int32), e=dev(iv[:, 1], np.int32), sf=dev(iv[:, 2], np.int32), ns=dev(iv[:, 3], np.int32), off=dev(off, np.int64),
                 first=dev(first, np.int32))
        guard, fill = 16, 0x7EEE7EEE
        o_min = torch.full((nI + guard,), fill, dtype=torch.int32, device=self.device)
        o_cnt = torch.full((total + guard,), fill, dtype=torch.int32, device=self.device)
        qi = _lib.RefCovIn(nI, nS, n_tiles, len(pos), d["pos"].data_ptr(), d["end"].data_ptr(), d["sb"].data_ptr(), d["sn"].data_ptr(), d["slong"].data_ptr(),
                           d["s"].data_ptr(), d["e"].data_ptr(), d["sf"].data_ptr(), d["ns"].data_ptr(), d["off"].data_ptr(), d["first"].data_ptr())
        qo = _lib.RefCovOut(total, o_min.data_ptr(), o_cnt.data_ptr())
        _lib.check(self.lib.plat_refcall_coverage_batch(self.ctx, C.byref(qi), C.byref(qo), self._stream()), "plat_refcall_coverage_batch")
        self._sync()
        mins, cnt = o_min.cpu().numpy(), o_cnt.cpu().numpy()
        if not ((mins[nI:] == fill).all() and (cnt[total:] == fill).all()):
            raise RuntimeError("plat_refcall_coverage_batch wrote behind its outputs")
        return mins[:nI].copy(), [cnt[off[k]:off[k] + (length[k] if iv[k, 3] > 0 else 0)].copy() if off[k] >= 0 else None for k in range(nI)]

    # ---- read statistics of the VCF INFO field --------------------------------------------
    def variant_read_stats(self, windows, bad_reads_window=11, exact=0, packed=False, gaps=None):
        """vcfINFO's per-read loop for a list of windows.  A window: dict {variants: [dict(pos, removed, added, bam_min,
        bam_max)], samples: [dict(good=[reads], bad=[reads])], var_in_genotype: [nVars][nInd]}; a read = dict(seq, qual, pos, end,
        mapq, flag, cigar).  All windows must have the same number of samples.  Returns per window a list over its variants of
        (counts[16], n_reads[nInd], n_var_reads[nInd], min_quals)."""
        torch = _torch()
        nI = len(windows[0]["samples"]) if windows else 0
        reads, gb, ge, bb, be, vw, vars_, vig, moff = [], [], [], [], [], [], [], [], []
        mtot = 0
        for w, win in enumerate(windows):
            assert len(win["samples"]) == nI
            ngood = 0
            for s_ in win["samples"]:
                gb.append(len(reads)); reads += s_["good"]; ge.append(len(reads)); ngood += len(s_["good"])
                bb.append(len(reads)); reads += s_["bad"]; be.append(len(reads))
            for k, v in enumerate(win["variants"]):
                vw.append(w); vars_.append(v); vig.append(win["var_in_genotype"][k]); moff.append(mtot); mtot += max(ngood, 1)
        nV = len(vars_)
        if nV == 0:
            return [[] for _ in windows]

        def dev(a, dt):
            return torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(self.device)
        blob = lambda parts: dev(pad_blob(np.frombuffer(b"".join(parts), dtype=np.uint8)), np.uint8)
        nadd = [len(v["added"]) for v in vars_]
        t = dict(vw=dev(vw, np.int32), vpos=dev([v["pos"] for v in vars_], np.int32), vmin=dev([v["bam_min"] for v in vars_], np.int32),
                 vmax=dev([v["bam_max"] for v in vars_], np.int32), nadd=dev(nadd, np.int32),
                 nrem=dev([len(v["removed"]) for v in vars_], np.int32), added=blob([v["added"] for v in vars_]),
                 aoff=dev(np.concatenate([[0], np.cumsum(nadd)[:-1]]), np.int64), vig=dev(np.asarray(vig, dtype=np.uint8).reshape(-1), np.uint8),
                 moff=dev(moff, np.int64), gb=dev(gb, np.int32), ge=dev(ge, np.int32), bb=dev(bb, np.int32), be=dev(be, np.int32),
                 seq=blob([r["seq"] for r in reads]), qual=blob([r["qual"] for r in reads]),
                 off=dev(np.concatenate([[0], np.cumsum([len(r["seq"]) for r in reads])]), np.int64),
                 pos=dev([r["pos"] for r in reads], np.int32), end=dev([r["end"] for r in reads], np.int32),
                 mapq=dev([r["mapq"] for r in reads], np.uint8), flags=dev([r["flag"] for r in reads], np.int32),
                 cig=dev([x for r in reads for c in r["cigar"] for x in c] + [0, 0], np.int16),
                 coff=dev(np.concatenate([[0], np.cumsum([len(r["cigar"]) for r in reads])]), np.int32))
        b = _lib.InfoStatsBatch()
        b.n_vars, b.n_ind = nV, nI
        for name, key in (("var_window", "vw"), ("var_pos", "vpos"), ("var_bam_min", "vmin"), ("var_bam_max", "vmax"), ("var_n_added", "nadd"),
                          ("var_n_removed", "nrem"), ("var_added", "added"), ("var_added_off", "aoff"), ("var_in_genotype", "vig"),
                          ("minq_off", "moff"), ("good_begin", "gb"), ("good_end", "ge"), ("bad_begin", "bb"), ("bad_end", "be"),
                          ("read_seq", "seq"), ("read_qual", "qual"), ("read_off", "off"), ("read_pos", "pos"), ("read_end", "end"),
                          ("read_mapq", "mapq"), ("read_flags", "flags"), ("cigar", "cig"), ("cig_off", "coff")):
            setattr(b, name, t[key].data_ptr())
        out = torch.empty(nV * 16, dtype=torch.int64, device=self.device)
        ps = torch.empty(nV * nI * 2, dtype=torch.int32, device=self.device)
        mq = torch.empty(max(mtot, 1), dtype=torch.int32, device=self.device)
        nmq = torch.empty(nV, dtype=torch.int32, device=self.device)
        if packed:                                  # plat_variant_read_stats_packed_batch: no expanded bases or qualities at all
            pk = self.pack_reads([r["seq"] for r in reads], [r["qual"] for r in reads], gaps)
            b.read_seq, b.read_qual = 0, 0
            _lib.check(self.lib.plat_variant_read_stats_packed_batch(self.ctx, C.byref(b), C.byref(pk["reads"]), bad_reads_window, exact, out.data_ptr(),
                                                                     ps.data_ptr(), mq.data_ptr(), nmq.data_ptr(), self._stream()),
                       "plat_variant_read_stats_packed_batch")
        else:
            _lib.check(self.lib.plat_variant_read_stats_batch(self.ctx, C.byref(b), bad_reads_window, exact, out.data_ptr(), ps.data_ptr(),
                                                              mq.data_ptr(), nmq.data_ptr(), self._stream()), "plat_variant_read_stats_batch")
        self._sync()
        out_h, ps_h, mq_h, nmq_h = out.cpu().numpy().reshape(nV, 16), ps.cpu().numpy().reshape(nV, nI, 2), mq.cpu().numpy(), nmq.cpu().numpy()
        res = [[] for _ in windows]
        for v in range(nV):
            res[vw[v]].append((out_h[v].tolist(), ps_h[v, :, 0].tolist(), ps_h[v, :, 1].tolist(), mq_h[moff[v]:moff[v] + nmq_h[v]].tolist()))
        return res

    # ---- a14..a18 ------------------------------------------------------------------------------------
    def upload_assembly(self, ab, max_vars=512, blob_per_region=1 << 16):
        """HBM image of the host arrays of plat_assembly_batch (dict as synth.config3 returns) + output buffers."""
        return AssemblyDeviceBatch(ab, self.device, max_vars, blob_per_region)

    def assemble_device(self, adb, kmer_size=15, min_qual=20, min_weight=40, no_cycles=0, hints=None):
        """plat_assemble_batch on a resident batch; enqueues only, results stay in HBM (adb.results() reads them).  hints = (longest
        reference window, most reads of a tile, most k-mer positions of a tile): plat_assemble_batch_async, which reads nothing back."""
        tail = (adb.max_vars, adb.blob_per_region, adb.cnt.data_ptr(), adb.pos.data_ptr(), adb.nrem.data_ptr(), adb.nadd.data_ptr(), adb.off.data_ptr(),
                adb.blob.data_ptr(), adb.status.data_ptr(), self._stream())
        if hints is None:
            rc = self.lib.plat_assemble_batch(self.ctx, C.byref(adb.struct), kmer_size, min_qual, min_weight, no_cycles, *tail)
        else:
            h = _lib.AssemblyHints(int(hints[0]), int(hints[1]), int(hints[2]))
            rc = self.lib.plat_assemble_batch_async(self.ctx, C.byref(adb.struct), C.byref(h), kmer_size, min_qual, min_weight, no_cycles, *tail)
        _lib.check(rc, "plat_assemble_batch")

    def assemble(self, regions, kmer_size=15, min_qual=20, min_weight=40, no_cycles=0, max_vars=512,
                 blob_per_region=1 << 16, hints=None):
        """assembleReadsAndDetectVariants for a list of regions.

        `regions`: list of dicts {ref: bytes, ref_start, assem_start, assem_end, seqs: [bytes], quals: [bytes]}
        (reads already in loadBAMDataIntoGraph order, QCFail reads removed).  Returns per region the list of
        (pos, removed, added) in the reference's sorted() order."""
        nG = len(regions)
        if nG == 0:
            return []
        ref_len = np.array([len(r["ref"]) for r in regions], dtype=np.int64)
        nreads = np.array([len(r["seqs"]) for r in regions], dtype=np.int64)
        rl = np.array([len(s) for r in regions for s in r["seqs"]], dtype=np.int64)
        ab = dict(n_regions=nG, n_reads=int(nreads.sum()),
                  ref_seq=np.frombuffer(b"".join(r["ref"] for r in regions), dtype=np.uint8),
                  ref_off=np.concatenate([[0], np.cumsum(ref_len)]),
                  ref_start=[r["ref_start"] for r in regions], assem_start=[r["assem_start"] for r in regions],
                  assem_end=[r["assem_end"] for r in regions], reg_read_begin=np.concatenate([[0], np.cumsum(nreads)]),
                  read_seq=np.frombuffer(b"".join(s for r in regions for s in r["seqs"]), dtype=np.uint8),
                  read_qual=np.frombuffer(b"".join(q for r in regions for q in r["quals"]), dtype=np.uint8),
                  read_off=np.concatenate([[0], np.cumsum(rl)]))
        adb = self.upload_assembly(ab, max_vars, blob_per_region)
        if hints == "exact":                                               # what a caller that built the batch knows
            per = [int(ref_len[g]) + 2 + sum(len(q) for q in regions[g]["seqs"]) + 2 * int(nreads[g]) for g in range(nG)]
            hints = (int(ref_len.max()), int(nreads.max()), max(per))
        self.assemble_device(adb, kmer_size, min_qual, min_weight, no_cycles, hints)
        return adb.results()

    def profile_enable(self, on=True):
        _lib.check(self.lib.plat_profile_enable(self.ctx, int(on)), "plat_profile_enable")

    def profile_last(self):
        p = _lib.Profile()
        _lib.check(self.lib.plat_profile_last(self.ctx, C.byref(p)), "plat_profile_last")
        return p

    def kernel_times(self):
        """{kernel name: (summed ms, launches)} of the launches bracketed since the profile was switched on / the last call (plat_kernel_times)."""
        ms = (C.c_double * 32)()
        n = (C.c_int64 * 32)()
        _lib.check(self.lib.plat_kernel_times(self.ctx, ms, n), "plat_kernel_times")
        return {(self.lib.plat_kernel_timer_name(i) or b"?").decode(): (float(ms[i]), int(n[i])) for i in range(32) if n[i]}

    def synchronize(self):
        """Waits for the stream and raises the first error an asynchronous call recorded since the last synchronize()."""
        _lib.check(self.lib.plat_stream_sync(self.ctx, self._stream()), "plat_stream_sync")
        self._sync()
