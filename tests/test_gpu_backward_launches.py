"""The launches of a backward, per profile scope, are the parent commit's.

Every weight-gradient path is one list of layers walked by one driver; which scopes a
step opens and how often is what bench.py and tools/pmc_summary.py read, and no rewrite of the host
code may change it.  One step of each case of step2_sched_cases.LAUNCH_CASES with the library's profile
hooks on must open the scopes, each as many times, that the parent commit's library opened
(tests/golden/backward_launches.json, written by tools/make_backward_launches.py from a build of the
commit named in the file).  Counts only: they are exact.
"""
import json
import os

import pytest

import step2_sched_cases as sc

pytestmark = pytest.mark.gpu

LAUNCHES_JSON = os.path.join(sc.HERE, "golden", "backward_launches.json")


@pytest.mark.parametrize("case", sc.LAUNCH_CASES)
def test_launches_equal_parent(case, monkeypatch):
    import marf_hip
    ref = json.load(open(LAUNCHES_JSON))["cases"][case]
    try:
        got = sc.case_launches(case, monkeypatch.setenv)
    finally:  # (case_launches does so itself; a failure inside it must not leave the hooks on either)
        marf_hip.profile_enable(False)
        marf_hip.profile_reset()
    assert got == ref, (case, got, ref)
    assert not marf_hip.profile_read(), case
