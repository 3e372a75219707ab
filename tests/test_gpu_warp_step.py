"""The warp-only fused step on the GPU: a frozen image registers further patches.

k_step2w and the tile kernels' warp-only instantiations run the full step's forward, loss, dgrad chain
and adjoint with nothing kept for weight gradients, so rgb, the loss and d warp are the full step's
BITS: the digests of tests/golden/step2_sched_bits.json (the parent commit's full step) must come out
of the frozen model too.  Beside that: the buffer plan is honest (guard bytes), a frozen trajectory is
the lr = 0 trajectory of the full step, the soft-mask gradient is render_step's, and train.py registers
on a loaded checkpoint without moving the image."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import step2_sched_cases as sc
import step_bits

pytestmark = pytest.mark.gpu
DEV = sc.DEV

BIT_CASES = ["acc", "pad-L8", "L10", "L13", "narrow", "generic-full",
             "tile-bf16", "tile-fp32", "tile-fp16", "tile-skip",
             "split-tp128", "split-tp64-ring", "split-odd", "split-pad"]


def _variant(case, **over):
    """Register a copy of `case` with extra model options in the helper module's table (at run time:
    the file is a yardstick and stays as it is); returns its name."""
    name = case + "+" + ",".join(f"{k}={over[k]}" for k in sorted(over))
    B, ph, pw, L, hidden, env, opts = sc.CASES[case]
    sc.CASES[name] = (B, ph, pw, L, hidden, env, dict(opts, **over))
    return name


def _step(m, var):
    """One step as step2_sched_cases.step runs it; the image gradients are returned as they are (None
    on a frozen model)."""
    m.optim.zero_grad()
    v = m.graph.forward(var, mode="train")
    assert v.fused_loss is not None
    loss = m.summarize_loss(m.graph.compute_loss(v, mode="train"))
    # the upstream gradient the step's backward receives (loss.all may be loss.rgb itself: weight 10^0)
    if loss.all is loss.rgb:
        gout = torch.ones(1, device=DEV)
    else:
        gout = torch.autograd.grad(loss.all, loss.rgb, retain_graph=True)[0].detach().reshape(1).clone()
    loss.all.backward()
    out = {"rgb": v.rgb_prediction.detach().clone(), "loss": loss.rgb.detach().reshape(1).clone(),
           "dh": m.graph.warp_param.weight.grad.detach().clone()}
    grads = [g for lay in m.graph.neural_image.mlp for g in (lay.weight.grad, lay.bias.grad)]
    return out, grads, gout


@pytest.mark.parametrize("case", BIT_CASES)
def test_bits_equal_the_full_steps_fixture(case, monkeypatch):
    ref = json.load(open(sc.BITS_JSON))["cases"][case]
    m, var = sc.build(_variant(case, freeze_image=True), monkeypatch.setenv)
    assert m.graph.neural_image.engine(torch.device(DEV)).net.step_kernel == ref["kernel"]
    import marf_hip
    marf_hip.profile_enable(True)
    try:
        marf_hip.profile_reset()
        out, grads, _ = _step(m, var)
        torch.cuda.synchronize()
        ran = marf_hip.profile_read()
    finally:
        marf_hip.profile_enable(False)
    # the warp-only instantiation ran, once; the full step kernel and every weight-gradient launch did not
    print(case, sorted((k, c) for k, (_, c) in ran.items()))
    assert ran.get("mlp_step_warp", (0, 0))[1] == 1, ran
    assert ran.get("warp_bwd", (0, 0))[1] == 1, ran
    assert "mlp_step" not in ran and not [k for k in ran if k.startswith("wgrad")], ran
    assert all(torch.isfinite(v).all() for v in out.values())
    bad = sorted(k for k in out if sc.digest(out[k]) != ref["bits"][k])
    assert not bad, (case, ref["kernel"], bad)
    assert all(g is None for g in grads), case


@pytest.mark.parametrize("case", ["acc", "split-pad"])
def test_saved_bytes_are_all_the_step_touches(case, monkeypatch):
    """marf_warp_step_forward / _backward through ctypes on a buffer of marf_warp_step_saved_bytes + 1 MiB
    of 0xA5: the last MiB stays, d_dh has the model path's bits."""
    import marf_hip
    m, var = sc.build(_variant(case, freeze_image=True), monkeypatch.setenv)
    want, _, gout = _step(m, var)
    L = marf_hip.lib()
    dev = torch.device(DEV)
    eng = m.graph.neural_image.engine(dev)
    w = m.graph.warp_param.weight.detach().contiguous()
    B = w.shape[0]
    st = marf_hip._stream(w)
    Hm = torch.empty(B, 3, 3, device=dev)
    marf_hip._check(L.marf_sl3_to_SL3(w.data_ptr(), Hm.data_ptr(), B, eng.lie_batch(B), st))
    geo = eng.grid_geo(B, Hm)
    Np = marf_hip.geo_np(eng)
    n = eng.net.warp_step_saved_bytes(geo)
    guard = 1 << 20
    buf = torch.full((n + guard,), 0xA5, dtype=torch.uint8, device=dev)
    gt = m.images.rgb.reshape(B, 3, Np).contiguous()
    mask = m.images.masks.reshape(B, 1, Np).contiguous()
    rgb = torch.empty(B, Np, 3, device=dev)
    stats = torch.empty(3, device=dev)
    dh = torch.empty(B, 8, device=dev)
    packed = eng.packed_for(m.graph.neural_image._params())
    cf = marf_hip.make_c2f(m.graph.neural_image.progress.detach(), eng.c2f)
    marf_hip._check(L.marf_warp_step_forward(eng.net.handle, ctypes.byref(geo), ctypes.byref(cf), packed.data_ptr(),
                                             gt.data_ptr(), mask.data_ptr(), None, rgb.data_ptr(), stats.data_ptr(),
                                             buf.data_ptr(), st))
    marf_hip._check(L.marf_warp_step_backward(eng.net.handle, ctypes.byref(geo), buf.data_ptr(), w.data_ptr(),
                                              eng.lie_batch(B), gout.data_ptr(), stats.data_ptr(), dh.data_ptr(), st))
    torch.cuda.synchronize()
    assert bool((buf[n:] == 0xA5).all()), case
    assert torch.equal(rgb.view(torch.int32), want["rgb"].view(torch.int32))
    assert torch.equal(stats[:1].view(torch.int32), want["loss"].view(torch.int32))
    assert torch.equal(dh.view(torch.int32), want["dh"].view(torch.int32)), case


def _adam_state(m):
    st = m.optim.state[m.graph.warp_param.weight]
    return [m.graph.warp_param.weight.detach().clone(), st["exp_avg"].detach().clone(), st["exp_avg_sq"].detach().clone()]


@pytest.mark.parametrize("case", ["pad-L8", "tile-fp32"])
def test_frozen_trajectory_is_the_lr0_trajectory(case, monkeypatch):
    """5 iterations of train_iteration with freeze_image against the same model at optim.lr = 0 (the
    library's Adam at lr 0 leaves p as it was): warps and their Adam moments bit-identical after every
    iteration, the image parameters the initial ones in both runs, no optimizer state for them in the
    frozen one."""
    lr0 = {"lr": 0.0}
    a, va = sc.build(_variant(case, freeze_image=True), monkeypatch.setenv)
    b, vb = sc.build(_variant(case, optim=lr0), monkeypatch.setenv)
    init = [p.detach().clone() for p in a.graph.neural_image.mlp.parameters()]
    assert all(torch.equal(x, y) for x, y in zip(init, b.graph.neural_image.mlp.parameters()))
    for it in range(5):
        a.train_iteration(va, step_bits._Loader())
        b.train_iteration(vb, step_bits._Loader())
        for x, y in zip(_adam_state(a), _adam_state(b)):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), (case, it)
    assert bool(a.graph.warp_param.weight.detach().abs().sum() > 0)
    for mm in (a, b):
        assert all(torch.equal(x, y) for x, y in zip(init, mm.graph.neural_image.mlp.parameters())), case
    image = {id(p) for p in a.graph.neural_image.parameters()}
    assert not any(id(p) in image for p in a.optim.state)
    assert all(p.grad is None for p in a.graph.neural_image.parameters())


def test_soft_mask_gradient_is_render_steps(tmp_path):
    """d2-L8 of step2_shapes.py with a random soft mask that requires grad: the mask gradient and d warp
    of render_warp_step are render_step's bits; a gradient into rgb itself is refused with the reason."""
    import time
    import marf_hip
    import step2_shapes as S
    from model import planar
    from util import EasyDict as edict
    c = S.CASES["d2-L8"]
    cfg, params, warp, rgb, mask, progress = S.inputs("d2-L8")
    opt = step_bits._opt(str(tmp_path), H=S.CANVAS, W=S.CANVAS, patch_H=c["ph"], patch_W=c["pw"], batch_size=c["B"],
                         use_edges=False, arch=S.arch("d2-L8"), barf_c2f=list(c["c2f"]))
    torch.manual_seed(c["seed"])
    m = planar.Model(opt)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)  # noqa: E731
    m.images = edict(rgb=t(rgb), masks=t(mask), masks_eroded=t(mask), edges=None, gt_hom=None, gt=None)
    m.build_networks()
    m.graph.neural_image.progress.data.fill_(progress)
    m.timer = edict(start=time.time(), it_mean=None)
    ni = m.graph.neural_image
    eng = ni.engine(torch.device(DEV))
    assert eng.net.step_kernel == "k_step2"
    soft = torch.rand(c["B"], c["ph"] * c["pw"], 1, device=DEV, generator=torch.Generator(DEV).manual_seed(5))
    got = {}
    for name, fn in (("full", marf_hip.render_step), ("warp", marf_hip.render_warp_step)):
        w = t(warp).requires_grad_()
        mk = soft.clone().requires_grad_()
        out_rgb, loss = fn(w, ni.progress.detach(), eng, ni._params(), m.images.rgb, mk)
        (loss * 3.0).backward()
        got[name] = (out_rgb.detach().clone(), loss.detach().reshape(1).clone(), w.grad.clone(), mk.grad.clone())
    assert bool(got["full"][3].abs().sum() > 0) and bool(got["full"][2].abs().sum() > 0)
    for x, y in zip(got["full"], got["warp"]):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    w = t(warp).requires_grad_()
    out_rgb, loss = marf_hip.render_warp_step(w, ni.progress.detach(), eng, ni._params(), m.images.rgb, soft)
    with pytest.raises(RuntimeError, match="rgb directly"):
        out_rgb.sum().backward()


def test_warp_step_stale_buffer_raises(tmp_path):
    """The warp-only step's dH partials live in one buffer per device: a backward after a later forward has
    reused it raises, as the full step's does (test_gpu_parity.test_fused_step_stale_buffer_raises)."""
    from test_gpu_parity import small_setup
    z, m, var, nl = small_setup("a", "fp32", tmp_path, freeze_image=True)
    v1 = m.graph.forward(var, mode="train")
    assert v1.fused_loss is not None
    l1 = m.graph.compute_loss(v1, mode="train").rgb
    m.graph.forward(var, mode="train")  # reuses the saved buffer
    with pytest.raises(RuntimeError, match="warp-only step's saved buffer was reused"):
        l1.backward()


def test_train_py_registers_on_a_loaded_image(tmp_path):
    """train.py --save_ckpt=true, then --load=... --freeze_image=true on the same patches: return code 0,
    finite losses, and the entire image renders bit-identically from both checkpoints."""
    from conftest import GOLDEN, PKG
    from model import planar
    common = [sys.executable, "train.py", "--group=warp", "--model=planar", "--yaml=planar", "--seed=3", "--barf_c2f=[0,0.4]",
              f"--dataset_npz={os.path.join(GOLDEN, 'cat_batch3_c1.npz')}", "--precision=bf16x3",
              "--arch.layers=[null,64,64,3]", "--max_iter=10", "--freq.scalar=1", "--freq.vis=1000", "--save_ckpt=true",
              f"--output_root={tmp_path}"]
    r = subprocess.run(common + ["--name=train"], cwd=PKG, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    first = tmp_path / "warp" / "train_seed3"
    ck1 = first / "model.ckpt"
    assert ck1.exists()
    r = subprocess.run(common + ["--name=register", f"--load={ck1}", "--freeze_image=true"], cwd=PKG, capture_output=True,
                       text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    second = tmp_path / "warp" / "register_seed3"
    for out in (first, second):
        rows = [json.loads(x) for x in (out / "metrics.jsonl").read_text().splitlines()]
        losses = [row["train/loss_rgb"] for row in rows]
        assert len(losses) == 10 and all(np.isfinite(losses)), losses
    a = torch.load(ck1, map_location="cpu")["graph"]
    b = torch.load(second / "model.ckpt", map_location="cpu")["graph"]
    image_keys = [k for k in a if k.startswith("neural_image.")]
    assert image_keys and all(torch.equal(a[k], b[k]) for k in image_keys)
    assert not torch.equal(a["warp_param.weight"], b["warp_param.weight"])  # the warps did move
    # the entire image before and after the second run, rendered here from either checkpoint
    opt = step_bits._opt(str(tmp_path / "render"), arch={"layers": [None, 64, 64, 3], "skip": [], "posenc": {"L_2D": 8}},
                         max_iter=10)
    torch.manual_seed(0)
    m = planar.Model(opt)
    m.build_networks()
    frames = []
    for ck in (ck1, second / "model.ckpt"):
        m.load_checkpoint(str(ck), image_only=True)
        frames.append(m.predict_entire_image())
    assert torch.isfinite(frames[0]).all() and torch.equal(frames[0].view(torch.int32), frames[1].view(torch.int32))
