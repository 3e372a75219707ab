"""lm.robust on the GPU -- Graph.lm_step over marf_gn_normal_robust on the occluded problem, fp32 and bf16x3.

The problem is gn_robust_ref's: gn_ref.realisable() (a frozen random image, 3 patches of 48 x 48, start h* +
0.01 noise, patch 0 fixed, mask all ones) with the targets rendered by marf_render at h* in the run's own
precision and one 16 x 20 rectangle of a constant colour painted into each (13.9 % of the patch).  The
float64 reference (tests/test_gn_robust_cpu.py): Cauchy at delta = 0.01 ends 2.8e-4 / 2.5e-4 from h*, a
hundredth of the start's 0.028 / 0.014, with weights <= 4.6e-4 inside the rectangles and >= 0.99998 outside;
plain LM ends 0.92 / 0.91 away."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import gn_ref
import gn_robust_ref as G
from test_gpu_gn import setup
from test_gpu_parity import DEV, gpu, t  # noqa: F401 (gpu: fixture)

pytestmark = pytest.mark.gpu


def _problem(prec, tmp_path, **over):
    """The model on the occluded problem: (model, var, h*, h0, inside [B, Np] bool on the device)."""
    inputs, hstar, h0 = gn_ref.realisable(seed=3, dtype=prec)
    m, var, eng = setup(inputs, prec, tmp_path, warp_solver="lm", **over)
    B = hstar.shape[0]
    m.graph.warp_param.weight.data.copy_(t(hstar))
    with torch.no_grad():
        target = m.graph.forward(var).rgb_prediction.detach().clone()
    painted, inside = G.occlude(target.cpu().numpy())
    m.images.rgb = t(painted).view(B, 48, 48, 3).permute(0, 3, 1, 2).contiguous()
    m.graph.warp_param.weight.data.copy_(t(h0))
    return m, var, hstar, h0, t(inside)


def _iterate(m, var, n):
    g = m.graph
    for _ in range(n):
        g.lm_step(var)
        if m.opt.warp.fix_first:
            g.warp_param.weight.data[0] = 0  # (Model.train's loop)
        yield g.lm_last


@pytest.mark.parametrize("prec", ["fp32", "bf16x3"])
def test_cauchy_recovers_the_warps_and_the_occluder(prec, tmp_path):
    """Cauchy, delta = 0.01, 25 iterations: every moving patch ends at most a tenth of its starting distance
    from h* (the float64 reference reaches a hundredth; the factor of ten absorbs fp32 and different accept
    decisions); the per-patch accepted cost never increases, exactly (an accepted trial's cost comes back,
    bit for bit, as the next iteration's); the mean weight is at most 0.01 inside each rectangle and at
    least 0.99 outside."""
    m, var, hstar, h0, inside = _problem(prec, tmp_path, lm={"robust": "cauchy", "robust_delta": 0.01})
    hist = []
    for it, last in enumerate(_iterate(m, var, 25)):
        hist.append(last.sse.cpu().numpy().copy())
        if it:
            want = np.where(acc_prev, trial_prev, hist[-2])
            assert np.array_equal(hist[-1], want), (it, hist[-1], want)
        acc_prev, trial_prev = last.accepted.cpu().numpy().copy(), last.sse_trial.cpu().numpy().copy()
    assert (np.diff(np.array(hist), axis=0) <= 0).all(), hist
    h = m.graph.warp_param.weight.detach().cpu().numpy().astype(np.float64)
    d0, d = np.abs(h0 - hstar).max(1), np.abs(h - hstar).max(1)
    w = m.graph.lm_last.weight
    assert w.shape == inside.shape and w.dtype == torch.float32
    assert var.robust_weight_map.shape == (3, 1, 48, 48) and torch.equal(var.robust_weight_map.reshape(3, -1), w)
    w_in = [float(w[b][inside[b]].mean()) for b in range(3)]
    w_out = [float(w[b][~inside[b]].mean()) for b in range(3)]
    print(prec, "|h - h*|_inf", d, "start", d0, "| mean weight inside", w_in, "outside", w_out)
    assert np.array_equal(h[0], h0[0]) and np.isfinite(h).all()
    assert (d[1:] <= 0.1 * d0[1:]).all(), (d, d0)
    assert max(w_in) <= 0.01 and min(w_out) >= 0.99


@pytest.mark.parametrize("prec", ["fp32", "bf16x3"])
def test_plain_lm_is_dragged_away(prec, tmp_path):
    """The same input under the plain lm_step (lm.robust: none), 12 iterations: both moving patches end
    farther from h* than they started -- the behaviour the feature answers -- and lm_last has no weight."""
    m, var, hstar, h0, _ = _problem(prec, tmp_path)
    for last in _iterate(m, var, 12):
        pass
    h = m.graph.warp_param.weight.detach().cpu().numpy().astype(np.float64)
    d0, d = np.abs(h0 - hstar).max(1), np.abs(h - hstar).max(1)
    print(prec, "plain LM |h - h*|_inf", d, "start", d0)
    assert (d[1:] > d0[1:]).all()
    assert "weight" not in last and "robust_weight_map" not in var


def test_robust_iteration_launches(tmp_path):
    """One train_iteration under lm.robust: one full robust launch, one loss-only robust launch and their two
    reductions; no plain gn launch, no step or weight-gradient kernel."""
    import marf_hip
    import step_bits
    import time
    from util import EasyDict as edict
    m, var, _, _, _ = _problem("bf16x3", tmp_path, lm={"robust": "huber", "robust_delta": 0.01})
    m.timer = edict(start=time.time(), it_mean=None)
    m.train_iteration(var, step_bits._Loader())  # (packs, sizes the buffers)
    marf_hip.profile_enable(True)
    try:
        marf_hip.profile_reset()
        loss = m.train_iteration(var, step_bits._Loader())
        torch.cuda.synchronize()
        ran = marf_hip.profile_read()
    finally:
        marf_hip.profile_enable(False)
    print(sorted((k, c) for k, (_, c) in ran.items()))
    count = lambda k: ran.get(k, (0, 0))[1]  # noqa: E731
    assert count("gn_robust") == 1 and count("gn_robust_loss") == 1 and count("gn_reduce") == 2, ran
    assert count("gn") == 0 and count("gn_loss") == 0, ran
    assert not [k for k in ran if k.startswith("mlp_step") or k.startswith("wgrad")], ran
    # loss.rgb is the robust cost: sum cost / (3 sum msum)
    last = m.graph.lm_last
    assert float(loss.rgb) == pytest.approx(float(last.sse.sum() / (3 * last.msum.sum())), rel=1e-6)


def test_train_py_writes_the_weight_map(tmp_path):
    """train.py --freeze_image=true --warp_solver=lm --lm.robust=cauchy --lm.robust_delta=0.01, 3 iterations
    on the C1 fixture's patches at a reduced crop: return code 0, finite logged losses, and
    robust_weight.npy is float32 [B, h, w] with every weight in (0, 1]."""
    import step_bits
    from conftest import GOLDEN, PKG
    from model import planar
    z = np.load(os.path.join(GOLDEN, "cat_batch3_c1.npz"))
    y0, x0 = (180 - 48) // 2, (240 - 64) // 2
    npz = tmp_path / "crop.npz"
    np.savez(npz, rgb=z["rgb"][:, :, y0:y0 + 48, x0:x0 + 64], mask=z["mask"][:, :, y0:y0 + 48, x0:x0 + 64])
    B = z["rgb"].shape[0]
    arch = {"layers": [None, 64, 64, 3], "skip": [], "posenc": {"L_2D": 8}}
    opt = step_bits._opt(str(tmp_path / "src"), arch=arch, max_iter=3, patch_H=48, patch_W=64, precision="bf16x3")
    torch.manual_seed(3)
    src = planar.Model(opt)
    src.build_networks()
    ck1 = tmp_path / "image.ckpt"
    src.save_checkpoint(str(ck1))
    cmd = [sys.executable, "train.py", "--group=gn", "--model=planar", "--yaml=planar", "--seed=3", "--barf_c2f=[0,0.4]",
           f"--dataset_npz={npz}", "--precision=bf16x3", "--arch.layers=[null,64,64,3]", "--patch_H=48", "--patch_W=64",
           "--max_iter=3", "--freq.scalar=1", "--freq.vis=1000", f"--output_root={tmp_path}", "--name=robust",
           f"--load={ck1}", "--freeze_image=true", "--warp_solver=lm", "--lm.robust=cauchy", "--lm.robust_delta=0.01"]
    r = subprocess.run(cmd, cwd=PKG, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = tmp_path / "gn" / "robust_seed3"
    rows = [json.loads(x) for x in (out / "metrics.jsonl").read_text().splitlines()]
    losses = [row["train/loss_rgb"] for row in rows]
    assert len(losses) == 3 and all(np.isfinite(losses)), losses
    w = np.load(out / "robust_weight.npy")
    assert w.dtype == np.float32 and w.shape == (B, 48, 64)
    assert (w > 0).all() and (w <= 1).all() and (w < 1).any()
