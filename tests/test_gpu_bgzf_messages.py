"""GPU test of the messages of the host's shared BGZF block list (tests/bgzf_message_cases.py) on the device paths: with the host twins
switched off, plat_caller_set_source_blocks and plat_caller_index_bgzf refuse each case with exactly the string written out there -- the
walk's refusals on the host before anything is uploaded, the block that does not inflate by plat_bgzf_inflate_batch's status.  Every
refusal is an error return of the library; none provokes a fault.  (tests/test_gpu_front_ends.py pins the same for the two BAM callers.)"""
import pytest

from platypus_amd import fastcaller as F
from tests import bgzf_message_cases as M

pytestmark = pytest.mark.gpu


def test_device_paths_refuse_with_the_whole_message(monkeypatch):
    monkeypatch.delenv("PLAT_CALLER_HOST_TABIX", raising=False)
    monkeypatch.delenv("PLAT_CALLER_HOST_TBI", raising=False)
    nc = F.NativeCaller(0, 1, 1)
    try:
        M.check(nc)
    finally:
        nc.close()
