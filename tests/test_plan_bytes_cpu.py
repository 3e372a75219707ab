"""The host buffer plans give the byte counts of tests/golden/plan_bytes.json (written by
tools/make_plan_bytes.py from the library of the commit named in the file), entry by entry: a change
of the planning code in csrc/marf_abi.hip that moves a byte of any buffer shows here, without a GPU."""
import json
import os

import pytest

import plan_bytes_cases as cases
from conftest import GOLDEN


@pytest.fixture(scope="module")
def want():
    with open(os.path.join(GOLDEN, "plan_bytes.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def lib():
    import build_lib
    build_lib.build(verbose=False)


def test_fixture_covers_the_table(want):
    assert set(want["nets"]) == set(cases.NETS)
    assert set(want["mask_nets"]) == set(cases.MASK_NETS)
    for e in list(want["nets"].values()) + list(want["mask_nets"].values()):
        assert set(e["geometries"]) == set(cases.GEOMETRIES)


def test_entries_that_take_different_paths_differ(want):
    """A condition on the table: an entry whose switch moved no byte would repeat another's total."""
    totals = {k: want["nets"][k]["geometries"]["3x16x20"]["step_saved_bytes"] for k in cases.DISTINCT}
    assert len(set(totals.values())) == len(totals), totals
    assert totals["s2-dzl-on"] == 23043840 and totals["s2-dzl-off"] == 23621376
    assert totals["s2-pipe"] == 23160576 and totals["s2-fp16x2"] == 23842560


@pytest.mark.parametrize("name", list(cases.NETS))
def test_net_plan_bytes(name, want, lib):
    got = cases.record_net(name)
    exp = want["nets"][name]
    for gname in cases.GEOMETRIES:
        assert got["geometries"][gname] == exp["geometries"][gname], (name, gname)
    assert got == exp, name
    # every full-step and unfused plan exists; a warp-only plan unless the recipe has none
    for g in got["geometries"].values():
        assert g["saved_bytes"] > 0 and g["workspace_bytes"] > 0 and g["step_saved_bytes"] > 0


@pytest.mark.parametrize("name", list(cases.MASK_NETS))
def test_mask_net_plan_bytes(name, want, lib):
    got = cases.record_mask_net(name)
    assert got == want["mask_nets"][name], name
    for g in got["geometries"].values():
        assert g["saved_bytes"] > 0 and g["workspace_bytes"] > 0
