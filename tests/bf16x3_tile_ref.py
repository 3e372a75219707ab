"""Torch statement of the split-bf16 tile recipe (MARF_BF16X3 on k_mlp_step_split: nets of more than
5 layers or wider than 256), for the tests.  Nothing here is used by the product.

    split(x)   hi = bf16_rne(x), lo = bf16_rne(x - float(hi))
    forward    per layer z = W_h a_h + W_h a_l + W_l a_h + b, one accumulator; a' = relu(z) split; the
               layer-0 input is the fp32 prologue's features (grid, warp, posenc + c2f in float32) split;
               the last layer in the same three terms; sigmoid, masked MSE and d rgb in float32
    dgrad      da = W_h^T dz_h + W_h^T dz_l + W_l^T dz_h; dz = da * relu'(z), split; the layer-0 adjoint
               (posenc, warp) by autograd through the float32 prologue
    wgrad      dW_l = dz_h^T a_h, db_l = sum dz_h (the saved hi planes); last layer: dW = (g_h + g_l)^T a_h,
               db = sum g in float32

step(...) returns what cpu_ref.CpuRefStep.step() returns (loss_rgb, rgb, grads, dh), the gradient of
loss.all = 2 loss.rgb (use_edges off).  Switches:
    drop   names of terms left out: "fwd_hl" (W_h a_l), "fwd_lh" (W_l a_h), "dgrad_wl" (W_l^T dz_h),
           "dgrad_dzl" (W_h^T dz_l)
    acc    torch.float64 (default: the recipe's operand rounding alone) or torch.float32 (torch's own
           float32 summation order on top of it)
    recipe "tile" (default), or "k_step2" / "k_step2dz": the pixel-per-wave kernel's dgrad (tests/step2_ref.py)
    features, mutate: tests/step2_ref.py
kink_pixels(inputs) names the pixels whose ReLU decisions depend on the accumulation order.
The accumulators are float32 in the kernel, so every GEMM result is rounded to float32 here too.
"""
import numpy as np
import torch

import cpu_ref

SHAPES = {  # case -> (hidden widths, L, patch h, patch w); 2 patches on the 512 x 512 canvas, seed 3
    "c5": ([512] * 8, 16, 64, 64),
    "deep": ([128] * 6, 8, 64, 64),
    "wide": ([512] * 2, 16, 64, 64),
    "odd": ([288, 512, 288], 8, 64, 64),
    "ragged": ([128] * 6, 8, 50, 54),
}


def split(x):
    hi = x.to(torch.bfloat16).to(torch.float32)
    lo = (x - hi).to(torch.bfloat16).to(torch.float32)
    return hi, lo


def _mm(a, b, acc):
    return (a.to(acc) @ b.to(acc))


def mm3(a, b, acc, skip_a_lo=False, skip_b_lo=False):
    """a_h b_h + a_h b_l + a_l b_h in `acc`, rounded to float32; a, b: (hi, lo) float32 pairs."""
    r = _mm(a[0], b[0], acc)
    if not skip_b_lo:
        r = r + _mm(a[0], b[1], acc)
    if not skip_a_lo:
        r = r + _mm(a[1], b[0], acc)
    return r


def _dgrad_step2(dz, W, acc, drop, last, dz_lo):
    """k_step2's dgrad GEMM (marf_step2.hip gemm MODE 2: A = W_h then W_l against one B): the last layer's
    B holds g_h and g_l along k, so four terms; below it B is dz's one bf16 word, so two; k_step2dz's
    hidden GEMMs (dz_lo) add W_h^T dz_l."""
    r = _mm(dz[0], W[0], acc)
    if "dgrad_wl" not in drop:
        r = r + _mm(dz[0], W[1], acc)
    if last or (dz_lo and "dgrad_dzl" not in drop):
        r = r + _mm(dz[1], W[0], acc)
    if last and "dgrad_wl" not in drop:
        r = r + _mm(dz[1], W[1], acc)
    return r


def step(cfg, params, warp, rgb, mask, progress, drop=(), acc=torch.float64, device="cpu", recipe="tile", mutate=None,
         features=None):
    f32 = torch.float32
    assert recipe in ("tile", "k_step2", "k_step2dz"), recipe
    dev = torch.device(device)

    def T(a):
        return torch.as_tensor(np.asarray(a, np.float32)).to(dev)
    L, n = cfg["L"], len(params)
    B, _, h, w = rgb.shape
    # ---- the float32 prologue (autograd keeps its adjoint)
    wp = T(warp).clone().requires_grad_()
    xy = cpu_ref.pixel_grid(cfg["H"], cfg["W"], cfg["patch_H"], cfg["patch_W"], crop=True, dtype=f32).to(dev)
    uv = cpu_ref.warp_grid(xy.repeat(B, 1, 1), wp)
    x = uv
    if L > 0:
        x = torch.cat([uv, cpu_ref.positional_encoding(uv, L, torch.tensor(progress, dtype=f32, device=dev), cfg["c2f"])], -1)
    x = x.reshape(B * h * w, -1)
    Ws = [split(T(W)) for W, _ in params]
    bs = [T(b) for _, b in params]
    # ---- forward (features: the prologue's values from elsewhere, [pixels, 2 + 4L]; its adjoint stays torch's)
    a = split(x.detach() if features is None else T(features).reshape(x.shape))
    acts, zs = [], []
    for l in range(n):
        # activations x weights^T: the "a" operand of mm3 is the activation pair, "b" the weight pair
        z = mm3(a, (Ws[l][0].t(), Ws[l][1].t()), acc, skip_a_lo="fwd_hl" in drop, skip_b_lo="fwd_lh" in drop)
        if mutate is not None:  # (a defect put into the emulation: the mutation check of tests/step2_ref.py)
            z = z + mutate(l, a, Ws[l]).to(z.dtype)
        z = (z + bs[l].to(acc)).to(f32)
        acts.append(a)
        zs.append(z)
        if l < n - 1:
            a = split(torch.relu(z))
    y = torch.sigmoid(zs[-1])
    tgt = T(rgb).permute(0, 2, 3, 1).reshape(-1, 3)
    m = T(mask).reshape(-1, 1)
    xm = (y - tgt) * m
    denom = m.sum() * 3
    loss = (xm * xm).sum() / denom
    g = ((2.0 * xm) * m * (1.0 - y)) * y  # unit upstream gradient; 2 / denom is applied to the sums below
    scale = (2.0 / denom).to(f32)
    # ---- backward
    grads = [None] * n
    dz = split(g)
    grads[n - 1] = ((_mm(dz[0].t(), acts[n - 1][0], acc) + _mm(dz[1].t(), acts[n - 1][0], acc)).to(f32), g.sum(0))
    for l in range(n - 1, -1, -1):
        if l < n - 1:
            grads[l] = (_mm(dz[0].t(), acts[l][0], acc).to(f32), dz[0].to(acc).sum(0).to(f32))
        if recipe == "tile":
            da = mm3(dz, Ws[l], acc, skip_a_lo="dgrad_dzl" in drop, skip_b_lo="dgrad_wl" in drop).to(f32)
        else:  # (the layer-0 adjoint reads dz_1's hi word in both k_step2 and k_step2dz)
            da = _dgrad_step2(dz, Ws[l], acc, drop, l == n - 1, recipe == "k_step2dz" and l > 0).to(f32)
        if l > 0:
            dz = split(da * (zs[l - 1] > 0))
    x.backward(da)
    return dict(loss_rgb=float(loss), rgb=y.cpu().numpy(), zs=zs[:-1],
                grads=[((gw * scale).cpu().numpy(), (gb * scale).cpu().numpy()) for gw, gb in grads],
                dh=(wp.grad * scale).cpu().numpy())


def kink_pixels(inputs, device="cpu", factor=4.0):
    """Pixels whose ReLU decision the accumulation order can flip: any hidden pre-activation of the
    emulation (float64 accumulation) within `factor` x the largest pre-activation difference between the
    emulation's float32 and float64 accumulation.  One such pixel moves a whole row of a weight gradient by
    its own contribution, which is no smaller than a dropped dgrad term (the gradient sums cancel), so a
    comparison of two implementations of the recipe zeroes these pixels' mask first (the precedent:
    mask_split_ref.case).  Returns the pixels as a [B, 1, h, w] float array of 0 / 1 and the threshold."""
    z64 = step(*inputs, device=device)["zs"]
    z32 = step(*inputs, acc=torch.float32, device=device)["zs"]
    thr = factor * max(float((a - b).abs().max()) for a, b in zip(z32, z64))
    near = torch.zeros(z64[0].shape[0], dtype=torch.bool, device=z64[0].device)
    for z in z64:
        near |= (z.abs() < thr).any(-1)
    return near.cpu().numpy().astype(np.float32).reshape(inputs[4].shape), thr


def truth(inputs, dtype=torch.float64, device="cpu"):
    """The reference's ops in `dtype` (cpu_ref.CpuRefStep) on the same inputs."""
    cfg, params, warp, rgb, mask, progress = inputs
    s = cpu_ref.CpuRefStep(cfg, params, warp, rgb, mask, dtype=dtype, device=device)
    s.progress.data.fill_(progress)
    return s.step()


def err(got, ref):
    return float(np.abs(got - ref).max() / (np.abs(ref).max() + 1e-30))


def errors(got, ref):
    """rgb abs error; every MLP gradient tensor's and d warp's max error relative to the tensor's max."""
    n = len(ref["grads"])
    return dict(rgb=float(np.abs(got["rgb"] - ref["rgb"]).max()),
                grads=[err(got["grads"][i][j], ref["grads"][i][j]) for i in range(n) for j in range(2)],
                dh=err(got["dh"], ref["dh"]))


def synthetic_inputs(case, seed=3, c2f=(0, 0.4), progress=0.2):
    """The inputs test_gpu_parity._synthetic_setup("bf16x3", ..., 2, crop, L, hidden) hands out, built
    without a GPU: the seeded init of NeuralImageFunction (the first module Model builds under the seed),
    the procedural targets, Bernoulli(0.85) masks and non-zero warps."""
    from model import planar
    from test_gpu_parity import make_opt
    hidden, L, ph, pw = SHAPES[case]
    B = 2
    opt = make_opt(None, H=512, W=512, patch_H=ph, patch_W=pw, batch_size=B, precision="bf16x3", use_edges=False,
                   arch={"layers": [None] + list(hidden) + [3], "skip": [], "posenc": {"L_2D": L}}, barf_c2f=list(c2f))
    torch.manual_seed(seed)
    nif = planar.NeuralImageFunction(opt)
    params = [(l.weight.detach().numpy().copy(), l.bias.detach().numpy().copy()) for l in nif.mlp]
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.linspace(0, 1, ph), np.linspace(0, 1, pw), indexing="ij")
    rgb = np.stack([[0.5 + 0.4 * np.sin(2 * np.pi * (rng.uniform(1, 4) * xx + rng.uniform(1, 4) * yy) + rng.uniform(0, 6))
                     for _ in range(3)] for _ in range(B)]).astype(np.float32)
    mask = (rng.random((B, 1, ph, pw)) < 0.85).astype(np.float32)
    warp = (rng.standard_normal((B, 8)) * 0.01).astype(np.float32)
    cfg = dict(H=512, W=512, patch_H=ph, patch_W=pw, L=L, c2f=list(c2f), max_iter=3000, lr=1e-3, lr_warp=1e-3,
               fix_first=True, use_edges=False, alpha_initial=0.0, alpha_final=1.0, skip=())
    return cfg, params, warp, rgb, mask, progress
