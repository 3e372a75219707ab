"""The step kernel's register placement and instruction order change no result bit.

Where k_step2's operand fragments and accumulators live, how many register copies surround its
MFMAs and in which order independent instructions issue (the pipelined last-layer weight gradient)
are free; every arithmetic operation, its operands and its order are not.  So one
fused step of each case of step2_sched_cases.py -- every compile-time instantiation, the generic
kernel, k_step2dz and k_step2h, on grids small enough that a block takes many tiles -- must give the
sha1 digests that the parent commit's library gave (tests/golden/step2_sched_bits.json, written by
tools/make_step2_sched_bits.py from a build of the commit named in the file).
"""
import json

import pytest
import torch

import step2_sched_cases as sc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", sc.ALL_CASES)
def test_step_bits_equal_parent(case, monkeypatch):
    """rgb, loss, every MLP gradient and bias gradient and d warp of one fused step (the render's rgb;
    the mask network's m and parameter gradients): the digests of the parent commit's library."""
    ref = json.load(open(sc.BITS_JSON))["cases"][case]
    got = sc.case_bits(case, monkeypatch.setenv)
    assert got["kernel"] == ref["kernel"], (case, got["kernel"], ref["kernel"])
    assert sorted(got["bits"]) == sorted(ref["bits"]), case
    bad = sorted(k for k in ref["bits"] if got["bits"][k] != ref["bits"][k])
    assert not bad, (case, got["kernel"], bad)


def test_rerun_is_bit_identical(monkeypatch):
    """The `acc` shape twice in one process (11, 11 and 10 tiles per block): a pipelined last-layer
    weight gradient that read an LDS buffer before it was written would pick up the previous
    launch's or tile's leftovers and differ between the runs."""
    m, var = sc.build("acc", monkeypatch.setenv)
    a = sc.step(m, var)
    b = sc.step(m, var)
    bad = sorted(k for k in a if not torch.equal(a[k], b[k]))
    assert not bad, bad
    ref = json.load(open(sc.BITS_JSON))["cases"]["acc"]["bits"]
    assert {k: sc.digest(v) for k, v in b.items()} == ref
