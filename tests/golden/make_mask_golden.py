"""Reference fixtures of the learned implicit mask (use_implicit_mask), from the REFERENCE itself on
the CPU through ref_harness.  Needs the reference checkout (MARF_REFERENCE); a few minutes:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_mask_golden.py

Writes tests/golden/mask_edges0.npz and mask_edges1.npz (use_edges off / on): data only.

Shape: patch 50 x 54 on a 100 x 108 canvas (Np = 2700 = 4 * 675: the reference's hard-coded
.view(180, 240, 3, -1) divides it), B = 3, seed 3, neural image [null, 64, 64, 3], L = 8.
The harness replaces inputs.compute_edges (cv2) by zeros: the edge *prediction* is zero, the edge
*target* is a random float64 tensor, so the edge term still carries its gradient into the mask.

Per file:
  inputs           rgb (some channels exactly 1.0, so both vocabulary rows occur), masks, edges, warp0
  init             checksums of every implicit_mask.* tensor and of embedding_view.weight, rows 0/1 of it
  step 0           m, rgb prediction, the losses, warp_param.grad, mask-net gradients (small tensors in
                   full; the 256 x 426 and 256 x 256 ones as a [::7, ::5] subset + row / column sums)
  traj_*           10 iterations: losses, warps, m checksums, the final m -- `base`, and `ulp1` where
                   the mask-net init was scaled by (1 + 2^-23)
  err32_*          fp32-vs-float64 error of tests/mask_ref.py per tensor on the step-0 state (the larger
                   of three float32 evaluation orders: see restatement_errors)
"""
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import ref_harness as R  # noqa: E402
import mask_ref  # noqa: E402

H, W, PH, PW, B, ITERS = 100, 108, 50, 54, 3, 10
LOSS_KEYS = ("render", "rgb", "mask", "edge", "all")
BIG_STRIDE = (7, 5)


def overrides(use_edges):
    return {"H": H, "W": W, "patch_H": PH, "patch_W": PW, "batch_size": B, "max_iter": 50,
            "use_implicit_mask": True, "build_single_masks": False, "use_edges": bool(use_edges),
            "alpha_initial": 0.25, "alpha_final": 0.75,
            "arch": {"layers": [None, 64, 64, 3], "skip": [], "posenc": {"L_2D": 8}}}


def make_inputs():
    rng = np.random.default_rng(7)
    rgb = rng.random((B, 3, PH, PW)).astype(np.float32)
    rgb[rng.random(rgb.shape) < 0.15] = 1.0
    masks = (rng.random((B, 1, PH, PW)) < 0.8).astype(np.float32)
    edges = (rng.random((B, 3, PH, PW)) * 0.5).astype(np.float64)
    warp0 = (rng.standard_normal((B, 8)) * 0.02).astype(np.float32)
    warp0[0] = 0
    return rgb, masks, edges, warp0


def big(name, g, out):
    g = g.detach().numpy()
    if g.ndim == 2 and g.shape[0] * g.shape[1] > 4096:
        out[name + "_sub"] = g[::BIG_STRIDE[0], ::BIG_STRIDE[1]].copy()
        out[name + "_rowsum"] = g.sum(1)
        out[name + "_colsum"] = g.sum(0)
        out[name + "_absmax"] = np.float64(np.abs(g).max())
    else:
        out[name] = g.copy()


def run(use_edges, scale_mask_init):
    _, planar, _, _ = R.import_reference()
    opt = R.make_opt(overrides(use_edges))
    rgb, masks, edges, warp0 = make_inputs()
    R.seed_all(opt.seed)
    graph = planar.Graph(opt)
    with torch.no_grad():
        graph.warp_param.weight.copy_(torch.from_numpy(warp0))
        if scale_mask_init:
            for p in graph.implicit_mask.parameters():
                p.mul_(1 + 2.0 ** -23)
    optim = torch.optim.Adam([
        dict(params=graph.neural_image.parameters(), lr=opt.optim.lr),
        dict(params=graph.warp_param.parameters(), lr=opt.optim.lr_warp),
        dict(params=graph.implicit_mask.parameters(), lr=opt.optim.lr_mask)])
    var = R.EasyDict(idx=torch.arange(B))
    var.images = R.EasyDict(rgb=torch.from_numpy(rgb), masks=torch.from_numpy(masks),
                            masks_eroded=torch.from_numpy(masks), edges=torch.from_numpy(edges))
    fake_model = R.EasyDict(opt=opt)
    out, traj = {}, {k: [] for k in LOSS_KEYS + ("warps", "m_sum", "m_sqsum")}
    if not scale_mask_init:
        sd = graph.state_dict()
        out["init_keys"] = np.array([k for k in sd if k.startswith(("implicit_mask.", "embedding_view."))])
        out["init_shapes"] = np.array([",".join(str(d) for d in sd[k].shape) for k in out["init_keys"]])
        out["init_sum"] = np.array([float(sd[k].double().sum()) for k in out["init_keys"]])
        out["init_abssum"] = np.array([float(sd[k].double().abs().sum()) for k in out["init_keys"]])
        out["embed_rows01"] = sd["embedding_view.weight"][:2].numpy().copy()
        out["state_keys"] = np.array(list(sd.keys()))
    for it in range(ITERS):
        optim.zero_grad()
        var = graph.forward(var, mode="train")
        loss = graph.compute_loss(var, mode="train")
        loss = planar.Model.summarize_loss(fake_model, loss)
        loss.all.backward()
        if it == 0 and not scale_mask_init:
            out["m0"] = var.mask_prediction.detach().numpy().copy()
            out["rgb_pred0"] = var.rgb_prediction.detach().numpy().copy()
            for k in LOSS_KEYS:
                out["loss0_" + k] = np.float64(float(loss[k]))
            out["grad0_warp"] = graph.warp_param.weight.grad.numpy().copy()
            for k, p in graph.implicit_mask.named_parameters():
                big("grad0_" + k, p.grad, out)
            out["embed_grad_absmax"] = np.float64(float(graph.embedding_view.weight.grad.abs().max()))
            out.update(restatement_errors(graph, var, opt, use_edges, loss))
        optim.step()
        graph.neural_image.progress.data.fill_((it + 1) / opt.max_iter)
        if opt.warp.fix_first:
            graph.warp_param.weight.data[0] = 0
        for k in LOSS_KEYS:
            traj[k].append(float(loss[k]))
        traj["warps"].append(graph.warp_param.weight.detach().numpy().copy())
        m = var.mask_prediction.detach().double()
        traj["m_sum"].append(float(m.sum()))
        traj["m_sqsum"].append(float((m ** 2).sum()))
    with torch.no_grad():
        var = graph.forward(var, mode="train")
    tag = "ulp1" if scale_mask_init else "base"
    for k, v in traj.items():
        out[f"traj_{tag}_{k}"] = np.asarray(v, dtype=np.float64 if k != "warps" else np.float32)
    out[f"traj_{tag}_m_final"] = var.mask_prediction.detach().numpy().copy()
    if not scale_mask_init:
        out.update(rgb=rgb, masks=masks, edges=edges, warp0=warp0,
                   cfg=np.array([H, W, PH, PW, B, ITERS, opt.max_iter, opt.alpha_initial, opt.alpha_final], np.float64))
    return out


def restatement_errors(graph, var, opt, use_edges, loss):
    """tests/mask_ref.py on the reference's step-0 state, float32 and float64: its agreement with the
    reference (rel, float32) and torch's own float32 error against float64, per tensor."""
    out = {}
    alpha = opt.alpha_initial if use_edges else 0
    weights = (opt.loss_weight.render, opt.loss_weight.rgb, opt.loss_weight.mask, opt.loss_weight.edge)
    res = {}
    # float32 three times: one patch at a time (the reference's order), all patches in one batch, and
    # the batch with each bias added after its product.  A hidden pre-activation within rounding of 0
    # falls on either side of the ReLU kink depending on the order of the float32 operations, and one
    # such flip moves a gradient entry by a whole pixel's contribution: the float32 error of a tensor
    # is a draw (4.5e-6 or 4.2e-5 for the same bias gradient), so the largest of the three is recorded.
    for tag, dt, batched in (("f32", torch.float32, 0), ("f32b", torch.float32, 1), ("f32c", torch.float32, 2),
                             ("f64", torch.float64, 0)):
        params = [p.detach().to(dt).requires_grad_() for p in graph.implicit_mask.parameters()]
        embed = graph.embedding_view.weight.detach().to(dt)
        index = var.images.rgb.long().reshape(B, 3, -1)
        xy = mask_ref.crop_grid(H, W, PH, PW, True, dt)
        if batched:
            m = mask_ref.mask_net(mask_ref.mask_input(index, embed, xy), params, bias_after=batched == 2)
        else:
            m = mask_ref.predict(index, embed, xy, params)
        m.retain_grad()
        m_map = m.view(B, PH, PW, 1).permute(0, 3, 1, 2)
        ep = var.edge_prediction.detach().to(dt) if use_edges else None
        eg = var.images.edges.to(dt) if use_edges else None
        ls = mask_ref.losses(var.rgb_prediction_map.detach().to(dt), var.images.rgb.to(dt), m_map, alpha, ep, eg, weights)
        ls["all"].backward()
        res[tag] = (m.detach(), m.grad.detach(), [p.grad for p in params], ls)

    def rel(a, b):
        return float((a.double() - b.double()).abs().max() / b.double().abs().max())
    m32, dm32, g32, l32 = res["f32"]
    m32b, dm32b, g32b, l32b = res["f32b"]
    m32c, dm32c, g32c, l32c = res["f32c"]
    m64, dm64, g64, l64 = res["f64"]
    out["err32_m"] = np.float64(max(float((x.double() - m64).abs().max()) for x in (m32, m32b, m32c)))
    out["err32_dm"] = np.float64(max(rel(x, dm64) for x in (dm32, dm32b, dm32c)))
    names = [k for k, _ in graph.implicit_mask.named_parameters()]
    out["err32_names"] = np.array(names)
    out["err32_grads_per_patch"] = np.array([rel(a, b) for a, b in zip(g32, g64)])
    out["err32_grads_batched"] = np.array([rel(a, b) for a, b in zip(g32b, g64)])
    out["err32_grads_bias_after"] = np.array([rel(a, b) for a, b in zip(g32c, g64)])
    out["err32_grads"] = np.maximum(np.maximum(out["err32_grads_per_patch"], out["err32_grads_batched"]),
                                    out["err32_grads_bias_after"])
    out["err32_losses"] = np.array([max(abs(float(l[k]) - float(l64[k])) for l in (l32, l32b, l32c))
                                    / abs(float(l64[k])) for k in LOSS_KEYS if l64[k] is not None])
    # the restatement against the reference itself (float32 both): the CPU test's <= 1e-6 rel check
    ref_g = [p.grad for p in graph.implicit_mask.parameters()]
    out["restate_vs_ref_m"] = np.float64(float((m32 - var.mask_prediction.detach()).abs().max()))
    out["restate_vs_ref_grads"] = np.array([rel(a, b) for a, b in zip(g32, ref_g)])
    out["restate_vs_ref_losses"] = np.array([abs(float(l32[k]) - float(loss[k])) / abs(float(loss[k]))
                                             for k in LOSS_KEYS if l32[k] is not None])
    out["dm0"] = dm64.numpy().astype(np.float32)
    return out


def main():
    torch.set_num_threads(int(os.environ.get("REF_THREADS", "8")))
    for use_edges in (0, 1):
        out = run(use_edges, False)
        out.update({k: v for k, v in run(use_edges, True).items() if k.startswith("traj_ulp1_")})
        path = os.path.join(HERE, f"mask_edges{use_edges}.npz")
        np.savez_compressed(path, **out)
        print(path, os.path.getsize(path), "bytes")
        for k in ("err32_m", "err32_dm", "err32_grads_per_patch", "err32_grads_batched", "err32_grads_bias_after", "err32_losses", "restate_vs_ref_m", "restate_vs_ref_grads",
                  "restate_vs_ref_losses", "embed_grad_absmax"):
            print("  ", k, out[k])
        for k in LOSS_KEYS:
            print("  ", k, out["traj_base_" + k][[0, -1]], out["traj_ulp1_" + k][[0, -1]])


if __name__ == "__main__":
    main()
