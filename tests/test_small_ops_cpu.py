"""The CPU oracle's Lie exponential and point warp (oracle/marf_oracle.c, the HIP kernels' twin)
pinned to the installed torch, bit for bit, on inputs that reach every branch of
torch.linalg.matrix_exp: the six batch-of-one degrees, every squaring count up to 4, both sides of
every threshold (tests/small_ops_cases.py builds and classifies them, and asserts the coverage).
The GPU twins of these checks are tests/test_gpu_lie_branches.py and tests/test_gpu_small_ops.py.
"""
import numpy as np
import pytest
import torch

import oracle
import small_ops_cases as soc


@pytest.fixture(scope="module")
def fwd():
    return soc.lie_forward_cases()


@pytest.fixture(scope="module")
def bwd():
    return soc.lie_backward_cases()


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def test_case_builders_cover_every_branch(fwd, bwd):
    """The builders assert their own coverage; here: the classification agrees with its definition at
    the thresholds (a norm on theta[i] takes the lower degree, except theta[4], which takes T18)."""
    assert [soc.classify(v)[0] for v in soc.THETA] == ["T1", "T2", "T4", "T8", "T18", "T18"]
    assert [soc.classify(soc.ulp_step(v, 1))[0] for v in soc.THETA] == ["T2", "T4", "T8", "T12", "T18", "T18s"]
    assert soc.classify(soc.ulp_step(soc.THETA[4], -1))[0] == "T12"
    for k in range(5):
        assert soc.classify(np.ldexp(soc.THETA[5], k))[1] == k
    assert len(fwd.h) == len(fwd.path) and len(bwd.h) == len(bwd.dH) == len(bwd.path)


def test_oracle_sl3_rows_equal_torch(fwd):
    want = soc.torch_sl3_rows(fwd.h)
    assert np.isnan(want[fwd.path.index("nan")]).all()  # torch fills a batch of one with NaN
    for i, h in enumerate(fwd.h):
        assert _same(oracle.sl3_to_SL3(h[None])[0], want[i]), (fwd.tag[i], fwd.path[i])


def test_oracle_sl3_batches_equal_torch(fwd):
    h = fwd.h[[p != "nan" for p in fwd.path]]  # (torch turns a NaN norm of a batch into an integer)
    assert _same(oracle.sl3_to_SL3(h), soc.torch_sl3(h))
    for i in range(0, len(h) - 1, 2):
        assert _same(oracle.sl3_to_SL3(h[i:i + 2]), soc.torch_sl3(h[i:i + 2])), i


@pytest.mark.parametrize("n", [3, 6])
def test_oracle_expm_equals_torch(fwd, bwd, n):
    """oracle.expm itself on the 3x3 generators and the 6x6 block matrices, as batches of one and whole."""
    if n == 3:
        A = np.stack([soc.generator_np(h) for h, p in zip(fwd.h, fwd.path) if p != "nan"])
    else:
        A = np.stack([soc.block_matrix_np(h, g) for h, g in zip(bwd.h, bwd.dH)])
    At = torch.from_numpy(A)
    for i in range(len(A)):
        assert _same(oracle.expm(A[i:i + 1]), torch.linalg.matrix_exp(At[i:i + 1]).numpy()), i
    assert _same(oracle.expm(A), torch.linalg.matrix_exp(At).numpy())


def test_oracle_sl3_backward_equals_torch_autograd(bwd):
    want = soc.torch_sl3_backward_rows(bwd.h, bwd.dH)
    for i in range(len(bwd.h)):
        got = oracle.sl3_to_SL3_backward(bwd.h[i:i + 1], bwd.dH[i:i + 1])[0]
        assert _same(got, want[i]), (bwd.tag[i], bwd.path[i])
    assert _same(oracle.sl3_to_SL3_backward(bwd.h, bwd.dH), soc.torch_sl3_backward(bwd.h, bwd.dH))
    for i in range(0, len(bwd.h) - 1, 2):
        assert _same(oracle.sl3_to_SL3_backward(bwd.h[i:i + 2], bwd.dH[i:i + 2]),
                     soc.torch_sl3_backward(bwd.h[i:i + 2], bwd.dH[i:i + 2])), i


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("n", soc.WARP_N)
def test_oracle_warp_points_equal_torch(B, n):
    """oracle.warp_points == the reference's expression in torch float32, its matmul rounded as
    tests/golden pins it (small_ops_cases.warp_reference: torch's BLAS kernel differs between hosts)."""
    xy, Hm, _ = soc.warp_case(B, n)
    assert np.array_equal(oracle.warp_points(xy, Hm), soc.warp_reference(xy, Hm))
