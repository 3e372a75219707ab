"""warp_solver: lm on the GPU -- Levenberg-Marquardt on the Gauss-Newton normal equations of every patch
(Graph.lm_step over marf_gn_normal), fp32 and bf16x3.

The problem is realisable (gn_ref.realisable): a frozen random image ([64, 64], L = 2, c2f off, 3 patches of
48 x 48 on a 64 x 64 canvas) whose targets are marf_render's own render at known warps h*, so the
residual at the solution is zero; the start is h* + 0.01 noise (seed 3), fix_first on.  The float64
reference's LM on the same start (float64 targets) reaches |h - h*|_inf = 1.6e-8 after 10 iterations
(tests/test_gn_cpu.py asserts < 1e-4), below both floors used here; on the float32 targets rendered
here it reaches 1.8e-7 (fp32) and 4.1e-7 (bf16x3), the kernel 1.9e-7 and 1.6e-7 (one MI355X)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import gn_ref
from test_gpu_gn import setup
from test_gpu_parity import DEV, gpu, t  # noqa: F401 (gpu: fixture)

pytestmark = pytest.mark.gpu


def _problem(prec, tmp_path, **over):
    """The model on the realisable problem: the targets rendered by marf_render (Graph.forward without
    autograd) at h*, the warps then set to h0.  Returns (model, var, inputs with those targets, h*, h0)."""
    inputs, hstar, h0 = gn_ref.realisable(seed=3, dtype=prec)
    m, var, eng = setup(inputs, prec, tmp_path, warp_solver="lm", **over)
    B = hstar.shape[0]
    if m.graph.warp_param.weight.shape[1] == 8:
        m.graph.warp_param.weight.data.copy_(t(hstar))
        with torch.no_grad():
            target = m.graph.forward(var).rgb_prediction.detach().clone()
        m.images.rgb = target.view(B, 48, 48, 3).permute(0, 3, 1, 2).contiguous()
        m.graph.warp_param.weight.data.copy_(t(h0))
        inputs = gn_ref.with_targets(inputs, target.cpu().numpy())
    return m, var, inputs, hstar, h0


@pytest.mark.parametrize("prec,floor", [("fp32", 1e-4), ("bf16x3", 1e-3)])
def test_lm_converges_monotonically(prec, floor, tmp_path):
    """10 iterations from h* + 0.01 noise: the accepted point's per-patch sse is non-increasing at every
    iteration (exact: the trial's sse is the loss-only launch's, whose bits the next full launch repeats);
    patch 0 never moves; |h - h*|_inf ends within 10 x the float64 gn_ref LM's value on the same start, or
    within the floor (fp32 1e-4, bf16x3 1e-3: the warp-parameter scale at which the recipes' rgb error of
    1e-5 stops moving sse), whichever is larger."""
    m, var, inputs, hstar, h0 = _problem(prec, tmp_path)
    g = m.graph
    hist = []
    for it in range(10):
        g.lm_step(var)
        if m.opt.warp.fix_first:
            g.warp_param.weight.data[0] = 0  # (Model.train's loop)
        hist.append(g.lm_last.sse.cpu().numpy().copy())
        assert np.array_equal(g.warp_param.weight.detach()[0].cpu().numpy(), h0[0]), it
        # an accepted trial's sse comes back, bit for bit, as the next iteration's sse
        if it:
            want = np.where(acc_prev, trial_prev, hist[-2])
            assert np.array_equal(hist[-1], want), (it, hist[-1], want)
        acc_prev = g.lm_last.accepted.cpu().numpy().copy()
        trial_prev = g.lm_last.sse_trial.cpu().numpy().copy()
    hist = np.array(hist)
    assert (np.diff(hist, axis=0) <= 0).all(), hist
    h = g.warp_param.weight.detach().cpu().numpy().astype(np.float64)
    href, _ = gn_ref.lm(inputs, h0, 10)
    e, eref = np.abs(h - hstar).max(), np.abs(href - hstar).max()
    print(prec, "sse", hist.sum(1), "| |h - h*|_inf kernel %.2e float64 reference %.2e" % (e, eref),
          "| lambda", g.lm_lambda.cpu().numpy())
    assert np.isfinite(h).all()
    assert hist[-1].sum() < 1e-2 * hist[0].sum()
    assert e <= max(10 * eref, floor), (e, eref)


def test_se2_step_is_the_projected_sl3_step(tmp_path):
    """warp.type: se2 -- A is 3 x 3 and the step equals the embedded sl(3) problem's projected one: with P
    = d h / d p (the embedding is linear), A_3 = P^T A_8 P, rhs_3 = P^T rhs_8 and delta_3 solves them; 1e-6
    of the step's max."""
    import marf_hip
    m, var, inputs, hstar, h0 = _problem("fp32", tmp_path, warp={"type": "se2", "dof": 3, "noise_h": 0.1, "noise_t": 0.2,
                                                                 "fix_first": True})
    g = m.graph
    B = 3
    p0 = torch.tensor([[0, 0, 0], [0.02, -0.01, 0.03], [-0.015, 0.02, -0.02]], device=DEV, dtype=torch.float32)
    g.warp_param.weight.data.copy_(p0)
    # targets: the image at slightly different se(2) warps
    g.warp_param.weight.data.add_(torch.tensor([[0, 0, 0], [0.01, 0.005, -0.01], [-0.005, 0.01, 0.008]], device=DEV))
    with torch.no_grad():
        target = g.forward(var).rgb_prediction.detach().clone()
    m.images.rgb = target.view(B, 48, 48, 3).permute(0, 3, 1, 2).contiguous()
    g.warp_param.weight.data.copy_(p0)
    h = marf_hip.se2_to_sl3(p0)
    out, _ = g.neural_image.render_gn(h, m.images.rgb, m.images.masks)
    eng = g.neural_image.engine(torch.device(DEV))
    A8, rhs8 = marf_hip.gn_system(out, marf_hip.gn_tangent(h, eng.lie_batch(B)))
    P = marf_hip.se2_to_sl3(torch.eye(3, device=DEV)).t().to(torch.float64)  # [8, 3]
    A3, rhs3 = P.t() @ A8 @ P, rhs8 @ P
    lam = torch.full((B,), g.lm.lambda0, dtype=torch.float64, device=DEV)
    want = marf_hip.gn_solve(A3, rhs3, lam, g.LM_EPS)
    want[0] = 0
    g.lm_step(var)
    got = g.lm_last.delta
    assert got.shape == (B, 3) and bool(want[1:].abs().sum() > 0)
    e = float((got - want).abs().max() / want.abs().max())
    print("se2 step", got.cpu().numpy(), "rel err %.2e" % e)
    assert e <= 1e-6
    assert bool(g.lm_last.accepted[1:].all()) and bool((g.warp_param.weight.detach()[0] == 0).all())


def test_train_py_registers_with_lm(tmp_path):
    """train.py --load=... --freeze_image=true --warp_solver=lm, 5 iterations on the C1 fixture's patches at
    a reduced crop (the centre 48 x 64 of each): return code 0, five finite logged losses, the warps moved,
    the image parameters and the full-canvas render bit-identical to the loaded checkpoint's."""
    import step_bits
    from conftest import GOLDEN, PKG
    from model import planar
    z = np.load(os.path.join(GOLDEN, "cat_batch3_c1.npz"))
    y0, x0 = (180 - 48) // 2, (240 - 64) // 2
    npz = tmp_path / "crop.npz"
    np.savez(npz, rgb=z["rgb"][:, :, y0:y0 + 48, x0:x0 + 64], mask=z["mask"][:, :, y0:y0 + 48, x0:x0 + 64])
    arch = {"layers": [None, 64, 64, 3], "skip": [], "posenc": {"L_2D": 8}}
    opt = step_bits._opt(str(tmp_path / "src"), arch=arch, max_iter=5, patch_H=48, patch_W=64, precision="bf16x3")
    torch.manual_seed(3)
    src = planar.Model(opt)
    src.build_networks()
    ck1 = tmp_path / "image.ckpt"
    src.save_checkpoint(str(ck1))
    cmd = [sys.executable, "train.py", "--group=gn", "--model=planar", "--yaml=planar", "--seed=3", "--barf_c2f=[0,0.4]",
           f"--dataset_npz={npz}", "--precision=bf16x3", "--arch.layers=[null,64,64,3]", "--patch_H=48", "--patch_W=64",
           "--max_iter=5", "--freq.scalar=1", "--freq.vis=1000", "--save_ckpt=true", f"--output_root={tmp_path}",
           "--name=register", f"--load={ck1}", "--freeze_image=true", "--warp_solver=lm"]
    r = subprocess.run(cmd, cwd=PKG, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = tmp_path / "gn" / "register_seed3"
    rows = [json.loads(x) for x in (out / "metrics.jsonl").read_text().splitlines()]
    losses = [row["train/loss_rgb"] for row in rows]
    assert len(losses) == 5 and all(np.isfinite(losses)), losses
    a = torch.load(ck1, map_location="cpu")["graph"]
    b = torch.load(out / "model.ckpt", map_location="cpu")["graph"]
    # (neural_image.progress is the run's place in the c2f schedule, it / max_iter, not the image)
    image_keys = [k for k in a if k.startswith("neural_image.mlp.")]
    assert image_keys and all(torch.equal(a[k], b[k]) for k in image_keys)
    assert float(a["neural_image.progress"]) == 0.0 and float(b["neural_image.progress"]) == 1.0
    assert list(a) == list(b)  # the checkpoint's keys are what they were (no solver state in it)
    assert not torch.equal(a["warp_param.weight"], b["warp_param.weight"]) and not b["warp_param.weight"][0].any()
    frames = []
    for ck in (ck1, out / "model.ckpt"):
        src.load_checkpoint(str(ck), image_only=True)
        src.graph.neural_image.progress.data.fill_(1.0)  # both at the same band weights
        frames.append(src.predict_entire_image())
    assert torch.isfinite(frames[0]).all() and torch.equal(frames[0].view(torch.int32), frames[1].view(torch.int32))
