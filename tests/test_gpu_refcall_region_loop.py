"""--outputRefCalls=1 in the native region loop with the blocks' read counts from the device (plat_refcall_coverage_batch: one launch per
chunk over the gap blocks and the windows' spans) and stage B on the device for one-sample regions: the text of the Python region loop,
and the text of the same loop with the host's per-position loop (PLAT_CALLER_HOST_REFCOV=1)."""
import io

import pytest

from platypus_amd import caller, fastcaller as F
from platypus_amd.options import default_options
from platypus_amd.vcfrecords import VCF
from tests.test_gpu_caller import _array_regions

pytestmark = pytest.mark.gpu

KW = dict(region_len=6000, snp_rate=6e-3, indel_rate=1.5e-3, read_len=150, depth=30)
OPTIONS = [dict(), dict(refCallBlockSize=37), dict(refCallBlockSize=150), dict(refCallBlockSize=100000), dict(minPosterior=60),
           dict(maxVariants=2, skipDifficultWindows=1), dict(maxSize=40)]
_cache = {}


def _regions(ns):
    if ns not in _cache:
        _cache[ns] = _array_regions(4, ns, **KW)
    return _cache[ns]


def _native(regs, names, opt, monkeypatch, host_refcov):
    if host_refcov:
        monkeypatch.setenv("PLAT_CALLER_HOST_REFCOV", "1")
    else:
        monkeypatch.delenv("PLAT_CALLER_HOST_REFCOV", raising=False)
    nc = F.NativeCaller(0, 2, 2)
    try:
        txt = nc.call_regions([F.region_from_arrays(r, packed=True) for r in regs], names, default_options(**opt))
        return txt, nc.stats
    finally:
        nc.close()
        monkeypatch.delenv("PLAT_CALLER_HOST_REFCOV", raising=False)


@pytest.mark.parametrize("ns", [1, 2])
@pytest.mark.parametrize("extra", OPTIONS, ids=lambda o: "-".join("%s%s" % kv for kv in o.items()) or "default")
def test_reference_calls_with_device_read_counts_equal_the_python_loop(extra, ns, monkeypatch):
    regs, names, fasta, _ = _regions(ns)
    opt = dict(outputRefCalls=1, **extra)
    py = io.StringIO()
    caller.callVariantsInRegions(_array_regions(4, ns, **KW)[3], fasta, default_options(**opt), VCF(names), py)      # (fresh buffers: the loop moves their pointers)
    txt, st = _native(regs, names, opt, monkeypatch, False)
    host_txt, host_st = _native(regs, names, opt, monkeypatch, True)
    print("[refcall region loop] %s, %d sample(s): %d lines, %d REFCALL; device intervals %d (%d positions), host decisions %d / %d under HOST_REFCOV; "
          "windows %d, stage B regions device %d host %d" % (opt, ns, txt.count("\n"), txt.count("\tREFCALL\t"), st["n_refcall_intervals_device"],
                                                            st["n_refcall_positions_device"], st["n_refcall_intervals_host"], host_st["n_refcall_intervals_host"],
                                                            st["n_windows"], st["n_regions_stage_b_device"], st["n_regions_stage_b_host"]))
    assert txt == py.getvalue()
    assert txt == host_txt
    assert st["n_refcall_intervals_device"] > 0 and st["n_refcall_positions_device"] >= st["n_refcall_intervals_device"]
    assert host_st["n_refcall_intervals_device"] == 0 and host_st["n_refcall_intervals_host"] > 0
    assert st["n_refcall_intervals_host"] == 0                              # (every decision's range lies inside an interval of the launch)
    assert st["n_refcall_records"] == txt.count("\tREFCALL\t") > 30
    if ns == 1:
        assert st["n_regions_stage_b_device"] == 4 and host_st["n_regions_stage_b_device"] == 4
    else:
        assert st["n_regions_stage_b_device"] == 0


@pytest.mark.parametrize("ns", [1, 2])
def test_nothing_changes_without_reference_calls(ns, monkeypatch):
    regs, names, fasta, _ = _regions(ns)
    txt, st = _native(regs, names, dict(), monkeypatch, False)
    host_txt, host_st = _native(regs, names, dict(), monkeypatch, True)
    assert txt == host_txt and txt.count("\n") > 30 and "REFCALL" not in txt
    new = ("n_refcall_intervals_device", "n_refcall_positions_device", "n_refcall_intervals_host")
    for k, v in st.items():
        if k in new:
            assert v == 0 and host_st[k] == 0, k
        elif isinstance(v, int):
            assert v == host_st[k], (k, v, host_st[k])
