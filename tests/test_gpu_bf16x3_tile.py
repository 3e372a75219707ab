"""precision: bf16x3 on nets the pixel-per-wave kernel cannot hold (more than 5 layers, or wider than
256): the split tile kernel k_mlp_step_split and its forward-only render, on the GPU.

Inputs: test_gpu_parity._synthetic_setup("bf16x3", tmp_path, 2, 64, L, hidden) -- 2 patches of 64x64 on
the 512 canvas, seed 3, non-zero warps -- and one ragged patch size (50x54 = 2700 pixels, no multiple
of the 64- or 128-slot tile).  The recipe's statement is tests/bf16x3_tile_ref.py; that it meets the
contract on these inputs is checked without the kernel in tests/test_bf16x3_tile_cpu.py."""
import numpy as np
import pytest
import torch

import bf16x3_tile_ref as R
import oracle
from test_gpu_parity import (DEV, _Loader, _compare_step, _synthetic_setup, g, gpu, make_opt,  # noqa: F401 (gpu: fixture)
                             one_step_grads, t)

pytestmark = pytest.mark.gpu

CASES = ["c5", "deep", "wide", "odd", "ragged"]


def _setup(case, tmp_path, **over):
    """Model, var and the checkers' inputs of a case; the ragged one (a non-square patch, which
    _synthetic_setup does not make) from the same seeded recipe in bf16x3_tile_ref.synthetic_inputs."""
    hidden, L, ph, pw = R.SHAPES[case]
    if case != "ragged" and not over:
        m, var, inputs = _synthetic_setup("bf16x3", tmp_path, 2, ph, L, hidden)
        ref_inputs = R.synthetic_inputs(case)  # the CPU tests' inputs are these
        assert all(np.array_equal(a, b) for pa, pb in zip(inputs[1], ref_inputs[1]) for a, b in zip(pa, pb))
        assert all(np.array_equal(inputs[i], ref_inputs[i]) for i in (2, 3, 4))
        return m, var, inputs
    from model import planar
    from util import EasyDict as edict
    inputs = R.synthetic_inputs(case)
    cfg, params, warp, rgb, mask, progress = inputs
    opt = make_opt(tmp_path, H=512, W=512, patch_H=ph, patch_W=pw, batch_size=2, precision="bf16x3", use_edges=False,
                   arch={"layers": [None] + list(hidden) + [3], "skip": [], "posenc": {"L_2D": L}}, barf_c2f=[0, 0.4], **over)
    torch.manual_seed(3)
    m = planar.Model(opt)
    m.images = edict(rgb=t(rgb), masks=t(mask), masks_eroded=t(mask), edges=None, gt_hom=None, gt=None)
    m.build_networks()
    for i, (W, b) in enumerate(params):
        assert np.array_equal(m.graph.neural_image.mlp[i].weight.detach().cpu().numpy(), W)
    m.graph.warp_param.weight.data.copy_(t(warp))
    m.graph.neural_image.progress.data.fill_(progress)
    m.setup_optimizer()
    return m, edict(idx=torch.arange(2), images=m.images), inputs


def _grads(m, nl):
    out = []
    for i in range(nl):
        out += [m.graph.neural_image.mlp[i].weight.grad.cpu().numpy().copy(), m.graph.neural_image.mlp[i].bias.grad.cpu().numpy().copy()]
    return out, m.graph.warp_param.weight.grad.cpu().numpy().copy()


def _cos(got, ref):
    return float(got.ravel().astype(np.float64) @ ref.ravel() / (np.linalg.norm(got) * np.linalg.norm(ref) + 1e-30))


@pytest.mark.parametrize("case", CASES)
def test_step_vs_oracle_and_emulation(case, tmp_path):
    """One step per case.

    Kernel and losses: step_kernel is k_mlp_step_split; rgb <= 1e-5 abs and loss <= 1e-5 rel against
    oracle.PlanarStep (the bounds of every bf16x3 test).

    Gradients: every MLP gradient tensor and d warp against float64 (cpu_ref.CpuRefStep) within
    max(1e-2, 2 E_emu) of the tensor's max, cosine >= 0.9999 for the MLP tensors.  1e-2 is the north-star
    bound; E_emu is the emulated recipe's own error on the same inputs (bf16x3_tile_ref, float64
    accumulation: never the kernel's); the factor 2 because fp32 accumulation order alone moves these
    cancelling sums by as much as the recipe does (the reference's own fp32 error at c5 is 3-4e-3).

    Kernel against emulation (catches a dropped dgrad term, which 1e-2 cannot see), on the MLP gradient
    tensors.  A pixel with a hidden pre-activation at a ReLU kink flips with the accumulation order and
    then moves a whole row of a weight gradient by its own contribution -- as much as a dropped term,
    because the sums cancel (measured: deep, one pixel, row 24 of dW_3 off by 1.3e-3, every other row
    <= 2.1e-5).  So this comparison runs a second step with those pixels' mask zeroed
    (bf16x3_tile_ref.kink_pixels: the emulation's own pre-activations within 4 x its float32-against-
    float64 accumulation difference of 0; the precedent is mask_split_ref.case), kernel and emulation
    alike.  With E_sum = the emulation accumulating in float32 against float64 and E_drop = the emulation
    with a dgrad lo term dropped (the smaller of W_l^T dz_h and W_h^T dz_l) against the full one, both the
    worst over the tensors, the kernel is held to sqrt(E_sum E_drop) of the emulation where
    E_drop >= 10 E_sum and not held elsewhere.  Not applied to d warp: its float32 sum over the tile's
    pixels and the dH partials has no counterpart in E_sum (the emulation's adjoint is one autograd pass
    in both accumulation modes).  Measured on one MI355X (kink pixels / E_sum / E_drop / kernel against
    emulation): c5 61 % / 1.8e-4 / 4.9e-3 / 2.6e-4, deep 5.2 % / 3.6e-5 / 9.5e-4 / 3.2e-5, wide 1.6 % /
    3.0e-5 / 6.1e-4 / 3.6e-5, odd 3.1 % / 3.1e-5 / 9.4e-4 / 3.6e-5, ragged 5.8 % / 3.8e-5 / 1.2e-3 / 4.3e-5:
    held on every shape.  The contract figures there (E_emu / the reference's fp32 / kernel; MLP, then d
    warp): c5 6.2e-3 / 4.3e-3 / 6.2e-3 and 9.1e-3 / 3.1e-3 / 1.13e-2; deep 1.1e-3 / 1.5e-3 / 1.1e-3 and
    5.4e-4 / 7.1e-4 / 5.4e-4; wide 3.7e-3 / 1.3e-3 / 1.5e-3 and 5.1e-3 / 2.1e-3 / 3.7e-3; odd 3.5e-3 /
    1.4e-6 / 3.5e-3 and 1.9e-3 / 1.9e-6 / 2.1e-3; ragged 2.7e-3 / 2.1e-6 / 2.7e-3 and 1.3e-3 / 5.1e-7 / 8.3e-4.

    Reproducibility: a second step gives the same bits in rgb, loss and every gradient.
    Render: no_grad Graph.forward gives the training forward's rgb bit for bit."""
    hidden, L, ph, pw = R.SHAPES[case]
    nl = len(hidden) + 1
    m, var, inputs = _setup(case, tmp_path)
    cfg, params, warp, rgb, mask, progress = inputs
    eng = m.graph.neural_image.engine(torch.device(DEV))
    assert eng.net.step_kernel == "k_mlp_step_split"
    o = _compare_step(m, var, inputs, "bf16x3", nl)
    assert o["rgb"] <= 1e-5 and o["loss"] <= 1e-5, o
    ours, dh = _grads(m, nl)
    rgb1 = var.rgb_prediction.detach().clone()

    t64 = R.truth(inputs, torch.float64, DEV)
    emu = R.step(cfg, params, warp, rgb, mask, progress, device=DEV)
    e_emu = R.errors(emu, t64)
    g64 = [x for pair in t64["grads"] for x in pair]
    gem = [x for pair in emu["grads"] for x in pair]
    kerr = [R.err(a, b) for a, b in zip(ours, g64)]
    print(case, "E_emu grads %.2e dh %.2e | ref32 grads %.2e dh %.2e | kernel grads %.2e dh %.2e" %
          (max(e_emu["grads"]), e_emu["dh"], o["grad_err_ref32"], o["dh_err_ref32"], max(kerr), R.err(dh, t64["dh"])))
    for i, (k, e) in enumerate(zip(kerr, e_emu["grads"])):
        assert k <= max(1e-2, 2 * e), (case, i, k, e)
        assert _cos(ours[i], g64[i]) >= 0.9999, (case, i)
    assert R.err(dh, t64["dh"]) <= max(1e-2, 2 * e_emu["dh"]), (case, R.err(dh, t64["dh"]), e_emu["dh"])

    # ---- reproducibility, and the render's bits
    var2, loss2 = one_step_grads(m, var)
    ours2, dh2 = _grads(m, nl)
    assert torch.equal(var2.rgb_prediction.detach().view(torch.int32), rgb1.view(torch.int32))
    assert all(np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in zip(ours + [dh], ours2 + [dh2]))
    var3, loss3 = one_step_grads(m, var)
    assert float(loss3.rgb) == float(loss2.rgb)
    with torch.no_grad():
        got = m.graph.forward(var, mode="eval").rgb_prediction
    assert torch.equal(got.reshape(-1).view(torch.int32), rgb1.reshape(-1).view(torch.int32))

    # ---- kernel against emulation, the pixels at a ReLU kink masked out
    near, thr = R.kink_pixels(inputs, DEV)
    assert (1 - near).sum() >= 2048, (case, near.mean(), thr)  # (c5: 4096 pre-activations a pixel, 61 % at a kink)
    mask2 = mask * (1 - near)
    inputs2 = (cfg, params, warp, rgb, mask2, progress)
    m.images.masks = m.images.masks_eroded = t(mask2)
    one_step_grads(m, var)
    ours_k, _ = _grads(m, nl)
    emu2 = R.step(*inputs2, device=DEV)
    flat = lambda s_: [x for pair in s_["grads"] for x in pair]  # noqa: E731
    e_sum = max(R.errors(R.step(*inputs2, acc=torch.float32, device=DEV), emu2)["grads"])
    e_drop = min(max(R.errors(R.step(*inputs2, drop=(d,), device=DEV), emu2)["grads"]) for d in ("dgrad_wl", "dgrad_dzl"))
    kve = max(R.err(a, b) for a, b in zip(ours_k, flat(emu2)))
    print(case, "kink pixels %.3f (|z| < %.1e) E_sum %.2e E_drop %.2e kernel vs emulation %.2e" %
          (near.mean(), thr, e_sum, e_drop, kve))
    if e_drop >= 10 * e_sum:
        assert kve <= np.sqrt(e_sum * e_drop), (case, kve, e_sum, e_drop)

def test_predict_entire_image_deep_vs_oracle(tmp_path):
    """Model.predict_entire_image (explicit coordinates, forward-only instantiation) on a 45 x 61 canvas
    with the deep net: 2745 pixels, a ragged last tile; 1e-5 abs against the oracle's forward."""
    hidden, L, _, _ = R.SHAPES["deep"]
    from model import planar
    opt = make_opt(tmp_path, H=45, W=61, patch_H=32, patch_W=32, batch_size=2, precision="bf16x3", use_edges=False,
                   arch={"layers": [None] + list(hidden) + [3], "skip": [], "posenc": {"L_2D": L}})
    torch.manual_seed(3)
    m = planar.Model(opt)
    m.build_networks()
    m.graph.neural_image.progress.data.fill_(0.2)
    assert m.graph.neural_image.engine(torch.device(DEV)).net.step_kernel == "k_mlp_step_split"
    img = m.predict_entire_image()
    assert tuple(img.shape) == (3, 45, 61)
    params = [(l.weight.detach().cpu().numpy(), l.bias.detach().cpu().numpy()) for l in m.graph.neural_image.mlp]
    import cpu_ref
    xy = cpu_ref.pixel_grid(45, 61, 0, 0, crop=False).numpy()
    w = oracle.c2f_weights(np.float32(0.2), [0, 0.4], L)
    _, ref = oracle.mlp_forward(oracle.posenc_features(xy, L, w), params)
    got = img.permute(1, 2, 0).reshape(-1, 3).cpu().numpy()
    assert np.abs(got - ref).max() <= 1e-5, np.abs(got - ref).max()


def _train(case, tmp_path, iters, **over):
    import time
    from util import EasyDict as edict
    m, var, _ = _setup(case, tmp_path, **over)
    m.timer = edict(start=time.time(), it_mean=None)
    losses = []
    for _ in range(iters):
        losses.append(float(m.train_iteration(var, _Loader()).rgb))
        m.graph.warp_param.weight.data[0] = 0
    st = [m.optim.state[p] for p in m.graph.neural_image.mlp.parameters()]
    return m, losses, ([p.detach().cpu() for p in m.graph.neural_image.mlp.parameters()] + [m.graph.warp_param.weight.detach().cpu()] +
                       [s_["exp_avg"].detach().cpu() for s_ in st] + [s_["exp_avg_sq"].detach().cpu() for s_ in st])


def test_captured_step_matches_eager_deep(tmp_path):
    """cuda_graph: true on the deep net: the captured iteration (forward, loss, backward, Adam) replays
    the split tile step bit for bit over 3 iterations -- losses, parameters, warps and Adam moments."""
    me, le, se = _train("deep", tmp_path / "eager", 3, cuda_graph=False)
    mg, lg, sg = _train("deep", tmp_path / "graph", 3, cuda_graph=True)
    assert me._step_graph is None and mg._step_graph is not None
    assert le == lg and all(np.isfinite(le)), (le, lg)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(se, sg))


def test_two_training_iterations_stay_finite(tmp_path):
    m, losses, state = _train("deep", tmp_path, 2, cuda_graph=False)
    assert all(np.isfinite(losses)) and all(bool(torch.isfinite(s).all()) for s in state), losses


def test_train_py_reduces_the_loss(tmp_path):
    """train.py with --precision=bf16x3 and a 6 x 128 net on the C1 batch: 20 iterations reduce loss.rgb."""
    import json
    import os
    import subprocess
    import sys
    from conftest import GOLDEN, PKG
    cmd = [sys.executable, "train.py", "--group=tile", "--model=planar", "--yaml=planar", "--name=deep", "--seed=3",
           "--barf_c2f=[0,0.4]", f"--dataset_npz={os.path.join(GOLDEN, 'cat_batch3_c1.npz')}", "--precision=bf16x3",
           "--arch.layers=[null,128,128,128,128,128,128,3]", "--max_iter=20", "--freq.scalar=1", "--freq.vis=20",
           f"--output_root={tmp_path}"]
    r = subprocess.run(cmd, cwd=PKG, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = tmp_path / "tile" / "deep_seed3"
    rows = [json.loads(x) for x in (out / "metrics.jsonl").read_text().splitlines()]
    losses = [row["train/loss_rgb"] for row in sorted(rows, key=lambda row: row["step"])]
    print(losses)
    assert len(losses) == 20 and all(np.isfinite(losses)) and losses[-1] < losses[0], losses
