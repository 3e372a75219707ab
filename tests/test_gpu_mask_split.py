"""The learned mask beside the 16-bit image recipes on the GPU: the mask network's all-operands-split
bf16 recipe (MARF_BF16X3A, option mask_precision: bf16x3a) and the mixed mode (image net bf16x3, mask
net fp32).

Bounds.  The split recipe, emulated in torch (tests/mask_split_ref.py), is <= 2.0e-7 on m, <= 1.3e-5 on a
hidden pre-activation and <= 6.2e-5 of max on a gradient tensor against float64; a kernel that forgets
one lo operand is >= 1.3e-3 of max on every gradient tensor.  Hence m <= 1e-5 abs and every gradient tensor
<= 5e-4 of its max, with the pixels whose float64 hidden pre-activation lies within 3e-5 of 0 (2.3 x the
pre-activation error: ReLU has no derivative there) given a zero upstream gradient.  Against the reference
fixtures the gradient bound is max(5e-4, 3 x torch's own recorded float32 error of that tensor).  No bound
comes from the kernels' output.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mask_ref
import mask_split_ref as sr
from conftest import PKG
from mask_common import LOSS_KEYS, MASK_PARAM_NAMES, fixture_model
from test_gpu_implicit_mask import _bound, _check_grad, _iteration, _linear_params, _need_gpu, _zero_edges

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.mark.parametrize("shape", list(sr.SHAPES))
def test_split_mask_net_forward_backward(shape):
    _need_gpu()
    import marf_hip
    B, ph, pw = sr.SHAPES[shape]
    c = sr.case(shape)
    print(f"{shape}: excluded share {c['excluded']:.3f}")
    assert c["excluded"] <= 0.25
    eng = marf_hip.MaskEngine(sr.N_VOCAB, marf_hip.MARF_BF16X3A, 2 * ph, 2 * pw, ph, pw)
    index = c["index"].to(torch.int32).to(DEV)
    embed = c["embed"].to(DEV)
    runs = []
    for _ in range(2):
        ps = [p.to(DEV).requires_grad_() for p in c["params"]]
        m = marf_hip.mask_forward(eng, index, embed, ps)
        assert m.shape == (B, ph * pw, 1)
        m.backward(c["dm"].to(DEV))
        torch.cuda.synchronize()
        runs.append((m.detach().clone(), [p.grad.clone() for p in ps]))
    with torch.no_grad():
        m_inf = marf_hip.mask_forward(eng, index, embed, [p.detach() for p in ps])
    torch.cuda.synchronize()
    (m, grads), (m2, grads2) = runs
    em = float((m.cpu().double() - c["m64"]).abs().max())
    print(f"{shape}: m max-abs err {em:.3e} (bound 1e-5)")
    rows = []
    for name, g, r in zip(MASK_PARAM_NAMES, grads, c["g64"]):
        e = float((g.cpu().double() - r).abs().max() / r.abs().max())
        rows.append((name, e))
        print(f"    {name}: grad err {e:.3e} of max (bound 5e-4)")
    assert em <= 1e-5
    for name, e in rows:
        assert e <= 5e-4, (name, e)
    assert torch.equal(m_inf, m)  # the inference launch (nothing saved) gives the same bits
    assert torch.equal(m, m2)     # two runs are bit-identical
    for name, a, b in zip(MASK_PARAM_NAMES, grads, grads2):
        assert torch.equal(a, b), name


@pytest.mark.parametrize("use_edges", [0, 1], ids=["edges_off", "edges_on"])
def test_split_mask_one_iteration_vs_reference(use_edges, golden, tmp_path, monkeypatch):
    _need_gpu()
    from util import EasyDict as edict
    z = golden(f"mask_edges{use_edges}")
    _zero_edges(monkeypatch)
    m = fixture_model(z, use_edges, DEV, tmp_path, mask_precision="bf16x3a")
    m.setup_optimizer()
    var, loss = _iteration(m, edict(idx=torch.arange(3), images=m.images))
    torch.cuda.synchronize()
    errs32 = {str(n): float(v) for n, v in zip(z["err32_names"], z["err32_grads"])}
    em = float(np.abs(var.mask_prediction.detach().cpu().numpy() - z["m0"]).max())
    print(f"m max-abs err {em:.3e}")
    assert em <= 1e-5
    for k in LOSS_KEYS:
        ref = float(z["loss0_" + k])
        got = float(loss[k].detach())
        print(f"    loss {k}: {got!r} vs {ref!r}")
        if ref == 0:
            assert got == 0, k
        else:
            assert got == pytest.approx(ref, rel=1e-5), k
    dh = m.graph.warp_param.weight.grad.cpu().numpy()
    e = float(np.abs(dh - z["grad0_warp"]).max() / np.abs(z["grad0_warp"]).max())
    print(f"    warp_param.grad: {e:.3e} of max")
    assert e <= 1e-4
    for name, p in m.graph.implicit_mask.named_parameters():
        _check_grad(p.grad.cpu().numpy(), z, name, max(5e-4, 3 * errs32[name]))
    assert m.graph.embedding_view.weight.grad is None


@pytest.mark.parametrize("dims", [[34, 256, 256, 256, 256, 3], [34, 64, 64, 3]], ids=["k_step2_256x4", "generic"])
def test_step2_gradient_into_a_soft_mask(dims):
    """The bf16x3 fused step with a soft mask m: d (1.7 loss) / d m against float64 autograd of the masked
    MSE on the step's own prediction (<= 1e-5 of max), the loss (1e-6 rel), and parameter / warp gradients
    that do not depend on whether m asks for a gradient (same bits)."""
    _need_gpu()
    import marf_hip
    B, H, W, ph, pw = 3, 100, 108, 50, 54
    Np = ph * pw
    g = torch.Generator().manual_seed(5)
    params = _linear_params(dims, g)
    warp = (torch.randn(B, 8, generator=g) * 0.02)
    gt = torch.rand(B, 3, ph, pw, generator=g)
    m0 = torch.rand(B, Np, 1, generator=g) * 0.9 + 0.05
    progress = torch.tensor(0.3, device=DEV)
    eng = marf_hip.Engine(dims, 8, marf_hip.MARF_BF16X3, [0, 0.4], H, W, ph, pw, lie_batch=B)
    out = []
    for need in (True, False):
        ps = [p.to(DEV).requires_grad_() for p in params]
        w = warp.to(DEV).requires_grad_()
        m = m0.to(DEV).requires_grad_(need)
        rgb, loss = marf_hip.render_step(w, progress, eng, ps, gt.to(DEV), m)
        (1.7 * loss).backward()
        torch.cuda.synchronize()
        out.append((rgb.detach(), loss.detach(), m.grad, w.grad, [p.grad for p in ps]))
    rgb, loss, dm, dw, dps = out[0]
    p64 = rgb.cpu().double()
    m64 = m0.double().view(B, 1, Np).requires_grad_()
    L = mask_ref.masked_mse(p64.permute(0, 2, 1), gt.double().view(B, 3, Np), m64)
    (1.7 * L).backward()
    assert float(loss) == pytest.approx(float(L.detach()), rel=1e-6)
    e_dm = float((dm.cpu().double().view(B, 1, Np) - m64.grad).abs().max() / m64.grad.abs().max())
    print(f"d loss / d m: err {e_dm:.3e} of max")
    assert e_dm <= 1e-5
    assert out[1][2] is None
    assert torch.equal(dw, out[1][3])
    for a, b in zip(dps, out[1][4]):
        assert torch.equal(a, b)


def test_mixed_iteration_bf16x3_image_fp32_mask(golden, tmp_path, monkeypatch):
    """Image net bf16x3, mask net fp32: m is the fp32 mask net's (it does not depend on the image net),
    loss.mask with it; loss.rgb and the mask-net gradients carry the image recipe's error, within the
    project's bound for a 16-bit image recipe (2e-2 on the loss, 1e-2 of max on a gradient tensor)."""
    _need_gpu()
    from util import EasyDict as edict
    z = golden("mask_edges0")
    _zero_edges(monkeypatch)
    m = fixture_model(z, 0, DEV, tmp_path, precision="bf16x3", mask_precision="fp32")
    m.setup_optimizer()
    var, loss = _iteration(m, edict(idx=torch.arange(3), images=m.images))
    torch.cuda.synchronize()
    em = float(np.abs(var.mask_prediction.detach().cpu().numpy() - z["m0"]).max())
    print(f"m max-abs err {em:.3e}")
    assert em <= _bound(1e-5, float(z["err32_m"]))
    print(f"    loss mask {float(loss.mask.detach())!r} vs {float(z['loss0_mask'])!r}, "
          f"rgb {float(loss.rgb.detach())!r} vs {float(z['loss0_rgb'])!r}")
    assert float(loss.mask.detach()) == pytest.approx(float(z["loss0_mask"]), rel=1e-6)
    assert float(loss.rgb.detach()) == pytest.approx(float(z["loss0_rgb"]), rel=2e-2)
    for k in LOSS_KEYS:
        assert np.isfinite(float(loss[k].detach() if torch.is_tensor(loss[k]) else loss[k])), k
    assert torch.isfinite(m.graph.warp_param.weight.grad).all()
    for name, p in m.graph.implicit_mask.named_parameters():
        assert torch.isfinite(p.grad).all(), name
        _check_grad(p.grad.cpu().numpy(), z, name, 1e-2)
    for layer in m.graph.neural_image.mlp:
        assert torch.isfinite(layer.weight.grad).all() and torch.isfinite(layer.bias.grad).all()


def test_train_py_bf16x3_with_split_mask(tmp_path):
    """train.py --precision=bf16x3 --mask_precision=bf16x3a --use_implicit_mask, 40 iterations at 50 x 54."""
    _need_gpu()
    B, ph, pw = 3, 50, 54
    yy, xx = np.mgrid[0:ph, 0:pw].astype(np.float32)
    img = np.stack([0.5 + 0.35 * np.sin(xx / 9 + c) * np.cos(yy / 11 - c) for c in range(3)])
    img[:, 10:20, 12:24] = 1.0  # a saturated block: vocabulary row 1 occurs
    rgb = np.stack([np.roll(img, s, axis=2) for s in range(B)])
    mask = np.ones((B, 1, ph, pw), np.uint8)
    mask[:, :, :5] = 0
    np.savez(tmp_path / "data.npz", rgb=(rgb * 255).round().astype(np.uint8), mask=mask)
    cmd = [sys.executable, "train.py", "--group=mask", "--model=planar", "--yaml=planar", "--name=run", "--seed=3",
           "--barf_c2f=[0,0.4]", f"--dataset_npz={tmp_path / 'data.npz'}", "--precision=bf16x3",
           "--mask_precision=bf16x3a", f"--output_root={tmp_path}", "--use_implicit_mask", "--use_edges=false",
           "--use_homographies=false", "--H=100", "--W=108", "--patch_H=50", "--patch_W=54", "--batch_size=3",
           "--max_iter=40", "--freq.scalar=10", "--freq.vis=20", "--arch.layers=[null,64,64,3]"]
    r = subprocess.run(cmd, cwd=PKG, capture_output=True, text=True, timeout=200, env=dict(os.environ))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = tmp_path / "mask" / "run_seed3"
    rows = [json.loads(x) for x in (out / "metrics.jsonl").read_text().splitlines()]
    assert [row["step"] for row in rows] == [10, 20, 30, 40]
    for row in rows:
        assert "train/Mask_Error" in row and "train/loss_mask" in row, row
        assert all(v is not None and np.isfinite(v) for v in row.values()), row
    print([(row["step"], row["train/loss_rgb"], row["train/loss_mask"], row["train/Mask_Error"]) for row in rows])
    assert rows[-1]["train/loss_rgb"] < rows[0]["train/loss_rgb"]
