"""CPU test of the messages of the host's shared BGZF block list (tests/bgzf_message_cases.py) on the stand-in device library with the host
twins switched on: plat_caller_set_source_blocks under PLAT_CALLER_HOST_TABIX=1 and plat_caller_index_bgzf under PLAT_CALLER_HOST_TBI=1
refuse each case with exactly the string written out there."""
from platypus_amd import fastcaller as F
from tests import bgzf_message_cases as M


def test_host_twins_refuse_with_the_whole_message(monkeypatch):
    from tests.fakedev import fake_caller_lib
    monkeypatch.setenv("PLAT_CALLER_HOST_TABIX", "1")
    monkeypatch.setenv("PLAT_CALLER_HOST_TBI", "1")
    nc = F.NativeCaller(0, 1, 1, lib=fake_caller_lib())
    try:
        M.check(nc)
    finally:
        nc.close()
