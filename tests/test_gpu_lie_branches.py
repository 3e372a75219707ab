"""The HIP Lie exponential (csrc/marf_lie.hip: expm, k_sl3_to_SL3, k_sl3_backward,
k_reduce_dH_lie_bwd) on every branch of torch.linalg.matrix_exp: the six batch-of-one Taylor degrees,
T18 with 0..5 squarings, both float32 neighbours of every threshold and of theta[5] * 2^k, h = 0 and a
NaN -- forward on the 3x3 generator, backward on the 6x6 block matrix [[A^T, G], [0, A^T]] with the
small upstream gradients of training (tests/small_ops_cases.py builds and classifies the inputs).

Checks, none of them derived from the kernels' output:
  * bit equality with torch CPU float32 (matrix_exp and its autograd), as batches of one and as batches;
  * accuracy against float64 matrix_exp / autograd: max-abs error within twice the error torch's own
    float32 CPU result makes on the same input, plus one float32 ulp of the tensor's largest entry.
    Bits differ + accuracy holds: a rounding order or the device libm; both fail: a wrong branch or
    wrong coefficients;
  * one fp32 fused step whose k_reduce_dH_lie_bwd feeds a batch-of-one backward a dH in the T4/T8
    range: d warp against the float64 reference ops, the project's fp32 bound (_compare_step).
"""
import numpy as np
import pytest
import torch

import small_ops_cases as soc
from test_gpu_parity import DEV, _err, t

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import marf_hip
    marf_hip.lib()
    yield


@pytest.fixture(scope="module")
def fwd():
    c = soc.lie_forward_cases()
    c.rows32 = soc.torch_sl3_rows(c.h)                       # each row as a batch of one
    c.rows64 = soc.torch_sl3_rows(c.h, torch.float64)
    return c


@pytest.fixture(scope="module")
def bwd():
    c = soc.lie_backward_cases()
    c.rows32 = soc.torch_sl3_backward_rows(c.h, c.dH)
    c.rows64 = soc.torch_sl3_backward_rows(c.h, c.dH, torch.float64)
    return c


def _gpu_fwd(h, lie_batch=0):
    import marf_hip
    with torch.no_grad():
        return marf_hip.sl3_to_SL3(t(h), lie_batch=lie_batch).cpu().numpy()


def _gpu_bwd(h, dH, lie_batch=0):
    import marf_hip
    x = t(h).requires_grad_()
    marf_hip.sl3_to_SL3(x, lie_batch=lie_batch).backward(t(dH))
    return x.grad.cpu().numpy()


def _mismatches(got, want, c):
    bad = [i for i in range(len(want)) if not np.array_equal(got[i], want[i], equal_nan=True)]
    return [(i, c.tag[i], c.path[i], int(c.s[i]), float(c.norm[i])) for i in bad]


def _accuracy(got, c, what):
    """Per row: |got - f64| <= 2 |torch f32 - f64| + ulp32(max |f64|).  Prints the worst ratio of each path."""
    worst, bad = {}, []
    for i in range(len(got)):
        if c.path[i] == "nan":
            continue
        e_got, e_ref = soc.abs_err(got[i], c.rows64[i]), soc.abs_err(c.rows32[i], c.rows64[i])
        scale = max(float(np.abs(c.rows64[i]).max()), 1e-300)
        allow = 2 * e_ref + soc.ulp_of_max(c.rows64[i])
        w = worst.setdefault(c.path[i], [0.0, 0.0])
        w[0], w[1] = max(w[0], e_got / scale), max(w[1], e_ref / scale)
        if e_got > allow:
            bad.append((i, c.tag[i], c.path[i], e_got / scale, e_ref / scale))
    for p in soc.PATHS:
        print(f"{what} {p}: worst err {worst[p][0]:.3e} of max (torch fp32: {worst[p][1]:.3e})")
    return bad


# ------------------------------------------------------------------------ forward

def test_forward_batch_of_one_bits(fwd):
    """lie_batch=1: every row is exponentiated as torch exponentiates a batch of one."""
    got = _gpu_fwd(fwd.h, lie_batch=1)
    assert np.isnan(got[fwd.path.index("nan")]).all() and np.isnan(fwd.rows32[fwd.path.index("nan")]).all()
    assert _mismatches(got, fwd.rows32, fwd) == []
    for i in soc.one_row_per_path(fwd):  # a real batch of one, no hint
        assert np.array_equal(_gpu_fwd(fwd.h[i:i + 1])[0], fwd.rows32[i], equal_nan=True), (fwd.tag[i], fwd.path[i])


def test_forward_batched_bits(fwd):
    """The rows as one batch and as batches of two: T18 with each row's own squaring count.  (Without the
    NaN row: torch converts a batch's NaN norm to an integer, which is undefined.)"""
    keep = [i for i, p in enumerate(fwd.path) if p != "nan"]
    h = fwd.h[keep]
    sub = soc.SimpleNamespace(tag=[fwd.tag[i] for i in keep], path=[fwd.path[i] for i in keep], s=fwd.s[keep],
                              norm=fwd.norm[keep])
    want = soc.torch_sl3(h)
    assert _mismatches(_gpu_fwd(h), want, sub) == []
    assert _mismatches(_gpu_fwd(h, lie_batch=2), want, sub) == []  # every row as a batch of two treats it
    for i in range(0, len(h) - 1, 8):
        assert np.array_equal(_gpu_fwd(h[i:i + 2]), soc.torch_sl3(h[i:i + 2])), (i, sub.tag[i], sub.tag[i + 1])


def test_forward_accuracy_vs_float64(fwd):
    assert _accuracy(_gpu_fwd(fwd.h, lie_batch=1), fwd, "exp") == []


# ------------------------------------------------------------------------ backward

def test_backward_batch_of_one_bits(bwd):
    got = _gpu_bwd(bwd.h, bwd.dH, lie_batch=1)
    assert _mismatches(got, bwd.rows32, bwd) == []
    for i in soc.one_row_per_path(bwd):
        assert np.array_equal(_gpu_bwd(bwd.h[i:i + 1], bwd.dH[i:i + 1])[0], bwd.rows32[i]), (bwd.tag[i], bwd.path[i])


def test_backward_batched_bits(bwd):
    assert _mismatches(_gpu_bwd(bwd.h, bwd.dH), soc.torch_sl3_backward(bwd.h, bwd.dH), bwd) == []
    for i in range(0, len(bwd.h) - 1, 8):
        assert np.array_equal(_gpu_bwd(bwd.h[i:i + 2], bwd.dH[i:i + 2]),
                              soc.torch_sl3_backward(bwd.h[i:i + 2], bwd.dH[i:i + 2])), (i, bwd.tag[i], bwd.tag[i + 1])


def test_backward_accuracy_vs_float64(bwd):
    assert _accuracy(_gpu_bwd(bwd.h, bwd.dH, lie_batch=1), bwd, "exp backward") == []


# ------------------------------------------------------------------------ through the fused step

def _ref_step(dims, L, H, W, ph, pw, params, warp, gt, mask, progress, c2f, dtype):
    """The reference's forward + masked loss_rgb with torch CPU autograd in dtype: (d warp, dH)."""
    import cpu_ref
    B = warp.shape[0]
    ps = [p.to(dtype) for p in params]
    w = warp.detach().clone().to(dtype).requires_grad_()
    Hm = cpu_ref.sl3_to_SL3(w)
    Hm.retain_grad()
    xy = cpu_ref.pixel_grid(H, W, ph, pw, crop=True, dtype=dtype).repeat(B, 1, 1)
    uv = soc.warp_expr(xy, Hm)
    x = torch.cat([uv, cpu_ref.positional_encoding(uv, L, torch.tensor(progress, dtype=dtype), c2f)], -1)
    for i in range(0, len(ps), 2):
        x = x @ ps[i].T + ps[i + 1]
        if i + 2 < len(ps):
            x = torch.relu(x)
    pred = torch.sigmoid(x).view(B, ph, pw, 3).permute(0, 3, 1, 2)
    mk = mask.to(dtype)
    ((((pred.contiguous() - gt.to(dtype)) * mk) ** 2).sum() / (mk.sum() * 3)).backward()
    return w.grad.numpy(), Hm.grad.numpy()


@pytest.mark.parametrize("B", [1, 2])
def test_fused_step_reduction_feeds_low_degree_backward(B):
    """One fp32 fused step (B patches of 20 x 30, net 34-64-64-3, L = 8): k_reduce_dH_lie_bwd sums the
    tile partials into dH and runs the same backward.  The target is scaled so that the float64
    reference's dH puts the 6x6 block matrix of every patch in the T4/T8 range (checked here from
    the reference, not from the kernel); B = 1 then takes that degree, B = 2 takes T18.  d warp: within
    1e-5 of its max or within twice the reference's own fp32 error (the project's fp32 bound)."""
    import marf_hip
    H, W, ph, pw, L = 40, 60, 20, 30, 8
    dims = [2 + 4 * L, 64, 64, 3]
    g = torch.Generator().manual_seed(17 + B)
    params = []
    for i in range(3):
        bound = 1 / np.sqrt(dims[i])
        params += [(torch.rand(dims[i + 1], dims[i], generator=g) * 2 - 1) * bound,
                   (torch.rand(dims[i + 1], generator=g) * 2 - 1) * bound]
    warp = torch.randn(B, 8, generator=g) * 0.02
    gt = torch.rand(B, 3, ph, pw, generator=g) * 1.0  # (scale of the target: |dH| ~ 5e-3 here, T4; 8.0 gives ~0.1, T8)
    mask = (torch.rand(B, 1, ph, pw, generator=g) < 0.85).float()
    c2f, progress = [0, 0.4], 0.3
    dh64, dH64 = _ref_step(dims, L, H, W, ph, pw, params, warp, gt, mask, progress, c2f, torch.float64)
    dh32, _ = _ref_step(dims, L, H, W, ph, pw, params, warp, gt, mask, progress, c2f, torch.float32)
    for b in range(B):  # dH on its own and the whole block matrix both sit in the T4/T8 range
        G = dH64[b].astype(np.float32)
        for norm in (soc.one_norm_f32(G), soc.one_norm_f32(soc.block_matrix_np(warp[b].numpy(), G))):
            assert soc.classify(norm)[0] in ("T4", "T8"), (b, norm)

    eng = marf_hip.Engine(dims, L, marf_hip.MARF_FP32, c2f, H, W, ph, pw, lie_batch=B)
    ps = [p.to(DEV).requires_grad_() for p in params]
    w = warp.to(DEV).requires_grad_()
    rgb, loss = marf_hip.render_step(w, torch.tensor(progress, device=DEV), eng, ps, gt.to(DEV), mask.to(DEV))
    loss.backward()
    got = w.grad.cpu().numpy()
    e, e32 = _err(got, dh64), _err(dh32, dh64)
    print(f"B={B}: d warp err {e:.3e} of max (reference fp32: {e32:.3e})")
    assert e <= max(1e-5, 2 * e32), (e, e32)
