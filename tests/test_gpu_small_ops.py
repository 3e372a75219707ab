"""The small kernels of csrc/marf_misc.hip (and k_mse_mask_bwd of csrc/marf_mask.hip) on their own, at
the sizes where their launch geometry and input-dependent branches change:

  * k_warp_points / k_warp_points_bwd: both sides of the 9 n < 400 rounding switch (n = 44 / 45), n
    below and beside a wave (63, 65) and a 1024-point pass (1023, 1024, 1025, 4100), B = 1 and 3;
  * k_adam / k_adam_sched: one element to one more than the 8192-block grid cap covers in one pass,
    steps 1 .. 200000, grad_scale, untouched (g = m = v = 0) elements, scheduled == host-scalar;
  * k_mse_partial / k_mse_final / k_mse_backward / k_mse_mask_bwd: one pixel to past every grid cap
    (1024, 8192, 4096 blocks), no mask / binary / soft / one patch masked out, denom_override.

Every expected value is computed here from plain torch on the CPU (tests/small_ops_cases.py): bit
equality with float32 torch, the project's stated fp32 bounds, or twice the error float32 torch makes
against float64 on the same input (measured in the test).
"""
import ctypes

import numpy as np
import pytest
import torch

import small_ops_cases as soc
from test_gpu_parity import DEV, t

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import marf_hip
    marf_hip.lib()
    yield


# ------------------------------------------------------------------------ point warp

@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("n", soc.WARP_N)
def test_warp_points_forward_bits(B, n):
    """Bit equality with the reference's expression in torch CPU float32, its matmul rounded as
    tests/golden pins it (small_ops_cases.warp_reference checks that against the installed torch)."""
    import marf_hip
    xy, Hm, _ = soc.warp_case(B, n)
    with torch.no_grad():
        got = marf_hip.warp_points(t(xy), t(Hm)).cpu().numpy()
        assert np.array_equal(got, soc.warp_reference(xy, Hm))
        # one shared point set [1, n, 2] == the per-patch run on the repeated points
        shared = marf_hip.warp_points(t(xy[:1]), t(Hm)).cpu().numpy()
        rep = marf_hip.warp_points(t(np.repeat(xy[:1], B, 0)), t(Hm)).cpu().numpy()
    assert np.array_equal(shared, rep)
    assert np.array_equal(rep, soc.warp_reference(np.repeat(xy[:1], B, 0), Hm))


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("n", soc.WARP_N)
def test_warp_points_backward_vs_float64(B, n):
    """d xy and d H against float64 autograd: within max(1e-5, 2 x float32 torch's own error) of each
    tensor's max."""
    import marf_hip
    xy, Hm, G = soc.warp_case(B, n)
    x, Hh = t(xy).requires_grad_(), t(Hm).requires_grad_()
    marf_hip.warp_points(x, Hh).backward(t(G))
    ref64 = soc.warp_backward_ref(xy, Hm, G, torch.float64)
    ref32 = soc.warp_backward_ref(xy, Hm, G, torch.float32)
    for name, got, r64, r32 in zip(("d xy", "d H"), (x.grad, Hh.grad), ref64, ref32):
        scale = np.abs(r64).max()
        e, e32 = soc.abs_err(got.cpu().numpy(), r64) / scale, soc.abs_err(r32, r64) / scale
        print(f"warp bwd B={B} n={n} {name}: err {e:.3e} of max (torch fp32: {e32:.3e})")
        assert e <= max(1e-5, 2 * e32), (name, e, e32)


# ------------------------------------------------------------------------ Adam

LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-8
GRID_CAP_N = 8192 * 256 + 77  # one pass of the capped grid covers 8192 * 256 elements


def _adam_case(n, seed):
    """p, g, m, v float32: |g| log-uniform in 1e-12 .. 1e3 with random sign, m != 0, v >= 0 of g's
    size, and a block with g = m = v = 0 (up to 64 elements from n // 2; none at n = 1)."""
    rng = np.random.default_rng(seed)
    mag = 10.0 ** rng.uniform(-12, 3, n)
    g = (mag * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    p = rng.standard_normal(n).astype(np.float32)
    m = (mag * rng.standard_normal(n) * 0.5).astype(np.float32)
    v = (mag * mag * rng.uniform(0, 2, n)).astype(np.float32)
    z = slice(n // 2, n // 2 + min(64, n // 4))
    g[z] = m[z] = v[z] = 0
    return p, g, m, v, z


@pytest.mark.parametrize("scaled", [False, True], ids=["noscale", "scale0.37"])
@pytest.mark.parametrize("step", [1, 2, 1000, 200000])
@pytest.mark.parametrize("n", [1, 255, 256, 257, GRID_CAP_N])
def test_adam_step_vs_float64(n, step, scaled):
    """One update against torch.optim.Adam's single-tensor formulas in float64: for each of p, m, v the
    max abs error is at most twice that of the same formulas in float32 torch on the CPU, plus one
    float32 ulp of the tensor's max.  The g = m = v = 0 block keeps p's bits, m = v = 0."""
    import marf_hip
    p, g, m, v, z = _adam_case(n, 7 * n + step)
    sc = np.float32(0.37)
    g64 = g.astype(np.float64) * (np.float64(sc) if scaled else 1.0)
    g32 = (g * sc).astype(np.float32) if scaled else g
    ref64 = soc.adam_ref(p, g64, m, v, LR, B1, B2, EPS, step, torch.float64)
    ref32 = soc.adam_ref(p, g32, m, v, LR, B1, B2, EPS, step, torch.float32)
    dp, dg, dm, dv = t(p), t(g), t(m), t(v)
    marf_hip.adam_step(dp, dg, dm, dv, LR, B1, B2, EPS, step, grad_scale=t(np.array([sc])) if scaled else None)
    got = [x.cpu().numpy() for x in (dp, dm, dv)]
    assert np.array_equal(dg.cpu().numpy(), g)  # the gradient is read only
    for name, a, r64, r32 in zip("pmv", got, ref64, ref32):
        assert np.isfinite(a).all(), name
        e, e32 = soc.abs_err(a, r64), soc.abs_err(r32, r64)
        print(f"adam n={n} step={step} scaled={scaled} {name}: err {e:.3e} (torch fp32: {e32:.3e}, "
              f"ulp of max {soc.ulp_of_max(r64):.3e})")
        assert e <= 2 * e32 + soc.ulp_of_max(r64), (name, e, e32)
    assert np.array_equal(got[0][z].view(np.uint32), p[z].view(np.uint32))
    assert not got[1][z].any() and not got[2][z].any()


@pytest.mark.parametrize("scaled", [False, True], ids=["noscale", "scale0.37"])
@pytest.mark.parametrize("k", [1, 7, 1000])
def test_adam_scheduled_equals_host_scalars(k, scaled):
    """marf_adam_step_sched with row k - 1 of marf_adam_schedule's table == marf_adam_step at step k."""
    import marf_hip
    lib = marf_hip.lib()
    n = 257
    p, g, m, v, _ = _adam_case(n, 31 * k)
    gs = t(np.array([0.37], np.float32)) if scaled else None
    a = [t(x) for x in (p, g, m, v)]
    marf_hip.adam_step(*a, LR, B1, B2, EPS, k, grad_scale=gs)
    buf = (ctypes.c_float * 2000)()
    marf_hip._check(lib.marf_adam_schedule(LR, B1, B2, 1, 1000, buf))
    table = t(np.ctypeslib.as_array(buf).copy())
    index = torch.tensor([k - 1], dtype=torch.int32, device=DEV)
    b = [t(x) for x in (p, g, m, v)]
    marf_hip._check(lib.marf_adam_step_sched(*(marf_hip._ptr(x) for x in b), n, B1, B2, EPS, marf_hip._ptr(table),
                                             marf_hip._ptr(index), marf_hip._ptr(gs), marf_hip._stream(b[0])))
    for name, x, y in zip("pgmv", a, b):
        assert torch.equal(x, y), name
    assert not torch.equal(a[0], t(p))  # (the update did happen)


# ------------------------------------------------------------------------ masked MSE

MSE_SIZES = [(1, 1), (3, 257), (5, 420001)]  # the last is past the 1024-, 8192- and 4096-block caps


def _mse_case(B, Np, kind):
    rng = np.random.default_rng(B * 1000003 + Np)
    pred = rng.random((B, Np, 3)).astype(np.float32)
    gt = rng.random((B, 3, Np)).astype(np.float32)
    if kind == "none":
        return pred, gt, None
    if kind == "soft":
        return pred, gt, rng.uniform(0.05, 0.95, (B, 1, Np)).astype(np.float32)
    mask = (rng.random((B, 1, Np)) < 0.8).astype(np.float32)
    mask[0, 0, 0] = 1  # (never an empty mask: the denominator is not zero)
    if kind == "patch1_out":
        mask[1] = 0
    return pred, gt, mask


def _mse_params():
    out = []
    for B, Np in MSE_SIZES:
        for kind in ("none", "binary", "soft", "patch1_out"):
            if kind == "patch1_out" and B < 3:
                continue
            for gout in (1.0, 1.7):
                out.append(pytest.param(B, Np, kind, gout, id=f"{B}x{Np}-{kind}-g{gout}"))
    return out


def _local_denom(mask, B, Np):
    """3 * sum(mask) as the reference computes it in float32 (an exact count for a binary mask)."""
    s = np.float64(B * Np) if mask is None else mask.sum(dtype=np.float64)
    return np.float32(s) * np.float32(3)


@pytest.mark.parametrize("B,Np,kind,gout", _mse_params())
def test_masked_mse_vs_float64(B, Np, kind, gout):
    """Loss 1e-6 relative, d pred rtol 1e-6 / atol 1e-12 (the bounds of test_masked_mse_vs_oracle), and
    for a soft mask that requires grad d mask within 1e-5 of its max (the bound of
    test_step_gradient_into_a_soft_mask), all against the reference's mse_loss in float64."""
    import marf_hip
    pred, gt, mask = _mse_case(B, Np, kind)
    loss64, dpred64, dmask64 = soc.mse_ref(pred, gt, mask, gout)
    p = t(pred).requires_grad_()
    mk = None if mask is None else t(mask)
    if kind == "soft":
        mk.requires_grad_()
    loss = marf_hip.masked_mse(p, t(gt), mk)
    loss.backward(torch.tensor(gout, device=DEV))
    print(f"mse {B}x{Np} {kind} gout={gout}: loss rel err {abs(float(loss) / loss64 - 1):.3e}, d pred rel err "
          f"{np.abs(p.grad.cpu().numpy() / np.where(dpred64 == 0, 1, dpred64) - 1)[dpred64 != 0].max():.3e}")
    np.testing.assert_allclose(float(loss), loss64, rtol=1e-6)
    np.testing.assert_allclose(p.grad.cpu().numpy(), dpred64, rtol=1e-6, atol=1e-12)
    if kind == "soft":
        e = soc.abs_err(mk.grad.cpu().numpy(), dmask64) / np.abs(dmask64).max()
        print(f"    d mask err {e:.3e} of max")
        assert e <= 1e-5, e
    stats = marf_hip.mse_stats(t(pred), t(gt), None if mask is None else t(mask)).cpu().numpy()
    want = _local_denom(mask, B, Np)
    np.testing.assert_allclose(stats[0], loss64, rtol=1e-6)
    # float32(sum) * 3: exact for counts; a soft mask's float64 sum may round to the neighbouring float32
    tol = 2.0 ** -23 if kind == "soft" else 0
    assert stats[1] == stats[2] and abs(float(stats[2]) / float(want) - 1) <= tol, (stats, want)


def test_masked_mse_denominator_override():
    """denom_override = 3 * sum(mask) * 2 (the global denominator of two equal shards): the loss and
    d pred use it, out[1] reports it and out[2] stays the local 3 * sum(mask)."""
    import marf_hip
    lib = marf_hip.lib()
    B, Np, gout = 3, 257, 1.7
    pred, gt, mask = _mse_case(B, Np, "binary")
    local = _local_denom(mask, B, Np)
    over = np.float32(local * np.float32(2))
    loss64, dpred64, _ = soc.mse_ref(pred, gt, mask, gout, denom=np.float64(over))
    p, d_over = t(pred).requires_grad_(), t(np.array([over]))
    loss = marf_hip.masked_mse(p, t(gt), t(mask), denom_override=d_over)
    loss.backward(torch.tensor(gout, device=DEV))
    np.testing.assert_allclose(float(loss), loss64, rtol=1e-6)
    np.testing.assert_allclose(p.grad.cpu().numpy(), dpred64, rtol=1e-6, atol=1e-12)
    out = torch.empty(3, device=DEV)
    ws = torch.empty(lib.marf_mse_workspace_bytes(), dtype=torch.uint8, device=DEV)
    dp, dg, dm = t(pred), t(gt), t(mask)
    ptr = marf_hip._ptr
    marf_hip._check(lib.marf_masked_mse(ptr(dp), ptr(dg), ptr(dm), B, Np, ptr(d_over), ptr(out), ptr(ws),
                                        marf_hip._stream(dp)))
    out = out.cpu().numpy()
    np.testing.assert_allclose(out[0], loss64, rtol=1e-6)
    assert out[1] == over and out[2] == local, (out, over, local)
