"""Torch statement of k_step2's recipe (MARF_BF16X3 on the pixel-per-wave kernel, marf_step2.hip; the
arithmetic include/marf.h states), for the tests.  Nothing here is used by the product.

It is bf16x3_tile_ref.step with the tile kernel's dgrad replaced (recipe="k_step2"); what differs:

    forward    as the tile recipe: z = W_h a_h + W_h a_l + W_l a_h + b into float32, a' = relu(z) split; the
               fp32 prologue's features split; sigmoid, masked MSE and d rgb in float32
    dgrad      the last layer: da = (W_h + W_l)^T (g_h + g_l), g = d z_last split (the GEMM's k axis holds
               [g_h, g_l], its A operand W_h then W_l: four terms); below it dz = bf16(da * relu'(z)), ONE
               word, and da = W_h^T dz + W_l^T dz (two terms); the layer-0 adjoint da_0 = (W_h + W_l)^T dz_1
               in float32, then posenc and warp by autograd through the float32 prologue
               k_step2dz (MARF_STEP2_DZ=1): dz split, da = W_h^T dz_h + W_l^T dz_h + W_h^T dz_l in the hidden
               GEMMs; dz_1 as the layer-0 adjoint reads it, and every saved dz, stay the hi word
    wgrad      dW_l = dz_h^T a_h, db_l = sum dz_h from the saved bf16 words; the last layer in the kernel:
               dW = (g_h + g_l)^T a_h, db = sum g in float32

Read against the kernel: gemm MODE 1 / MODE 2 (forward / dgrad terms), the "g operand of the last-layer
dgrad" block and dw_last (g_h rows 0-2, g_l rows 4-6 against feat's hi words), k_pack2 kind 2 (k = [g hi, 0,
g lo, 0]) and the adjoint stage (MODE 2 on Dh, the hi words).

The prologue's values come from the oracle's C restatement (oracle.warp_points / posenc_features), which the
kernel's prologue matches (rgb to 4.5e-7 with every band of L = 20 open); torch's float32 prologue does so on
some hosts only, and a last-place difference of a warped coordinate is multiplied by 2^k pi in band k: the
difference doubled per band, and with bands up to 19 open it was 8e-5 on rgb and 2e-2 on the gradients
between the kernel and an emulation on torch's prologue, on a host where the oracle agreed with the kernel to
4.5e-7.  The adjoint of the prologue is torch's autograd (d warp is not compared with the kernel's here).

step / kink_pixels take bf16x3_tile_ref's switches (drop=, acc=, device=); drop="dgrad_wl" leaves W_l^T dz
out of every dgrad GEMM, "dgrad_dzl" the W_h^T dz_l term k_step2dz adds.  The mutation check
(profiles/step2_shapes/README.md) uses mutate_pad_lo and drop."""
import numpy as np
import torch

import bf16x3_tile_ref as R
import oracle

errors, err, truth, split = R.errors, R.err, R.truth, R.split


def features(cfg, warp, progress):
    """The MLP's input [pixels, 2 + 4L] by the oracle's float32 prologue (as oracle.PlanarStep.forward)."""
    xy = oracle.pixel_grid(cfg["H"], cfg["W"], cfg["patch_H"], cfg["patch_W"], crop=True)
    warp = np.asarray(warp, np.float32)
    uv = oracle.warp_points(np.broadcast_to(xy, (warp.shape[0],) + xy.shape).copy(), oracle.sl3_to_SL3(warp))
    w = oracle.c2f_weights(np.float32(progress), cfg["c2f"], cfg["L"])
    return oracle.posenc_features(uv, cfg["L"], w).reshape(-1, 2 + 4 * cfg["L"])


def step(cfg, params, warp, rgb, mask, progress, dz=False, **kw):
    return R.step(cfg, params, warp, rgb, mask, progress, recipe="k_step2dz" if dz else "k_step2",
                  features=features(cfg, warp, progress), **kw)


def kink_pixels(inputs, device="cpu", factor=4.0, dz=False):
    """bf16x3_tile_ref.kink_pixels on this recipe."""
    z64 = step(*inputs, dz=dz, device=device)["zs"]
    z32 = step(*inputs, dz=dz, acc=torch.float32, device=device)["zs"]
    thr = factor * max(float((a - b).abs().max()) for a, b in zip(z32, z64))
    near = torch.zeros(z64[0].shape[0], dtype=torch.bool, device=z64[0].device)
    for z in z64:
        near |= (z.abs() < thr).any(-1)
    return near.cpu().numpy().astype(np.float32).reshape(inputs[4].shape), thr


def flat(s):
    return [x for pair in s["grads"] for x in pair]


def mutate_pad_lo(width=40, lo=2.0 ** -9):
    """A perturbation for the mutation check, NOT a model of a padded-column defect in the kernel: the next
    layer's pre-activations get lo x the hi weights of the `width`-wide layer's last live column (width - 1),
    as if the first padded column (column `width`) held a lo word `lo` and met that live weight.  In the
    kernel a padded column's weights are zero in both planes, so a non-zero lo word there alone multiplies
    nothing (the recipe has no lo x lo term either) and may well be invisible to every test; what this
    shows is only that the bound sees a 2^-9 perturbation of z, which 1e-2 does not."""
    def f(l, a, W):
        if l == 0 or W[0].shape[1] != width:  # (W: this layer's (hi, lo) [out, in]; in = the padded layer's width)
            return torch.zeros((), dtype=torch.float32, device=a[0].device)
        return (lo * W[0][:, width - 1]).expand(a[0].shape[0], -1)
    return f


def held_bound(inputs, device="cpu", factor=4.0, dz=False):
    """The inputs and the bound of the kernel-against-emulation comparison, from the emulation alone
    (test_gpu_bf16x3_tile.test_step_vs_oracle_and_emulation's construction): the kink pixels' mask zeroed;
    E_sum = float32 against float64 accumulation, E_drop = W_l^T dz dropped against the full recipe, each
    the worst over the MLP gradient tensors.  Returns dict(inputs, emu, near, thr, e_sum, e_drop, held,
    bound): held is E_drop >= 10 E_sum, bound sqrt(E_sum E_drop)."""
    cfg, params, warp, rgb, mask, progress = inputs
    near, thr = kink_pixels(inputs, device, factor, dz)
    inputs2 = (cfg, params, warp, rgb, mask * (1 - near), progress)
    emu = step(*inputs2, dz=dz, device=device)
    e_sum = max(errors(step(*inputs2, dz=dz, acc=torch.float32, device=device), emu)["grads"])
    e_drop = max(errors(step(*inputs2, dz=dz, drop=("dgrad_wl",), device=device), emu)["grads"])
    return dict(inputs=inputs2, emu=emu, near=near, thr=thr, e_sum=e_sum, e_drop=e_drop, held=e_drop >= 10 * e_sum,
                bound=float(np.sqrt(e_sum * e_drop)), left=int((mask * (1 - near)).sum()), out=float(near.mean()))
