"""Timing of the learned implicit mask on the GPU (no pass / fail: correctness is tested elsewhere).

    python tools/bench_mask.py --part net  [--reps 20] [--out FILE] [--mask-precision fp32 bf16x3a]
    python tools/bench_mask.py --part step [--reps 20] [--out FILE] [--mask-precision fp32 bf16x3a]

At the C1 size (B = 5 patches of 180 x 240 on a 360 x 480 canvas):

  net    forward + backward of the mask network, alternating in one process
           marf        the library's kernels (input formation + MLP + weight gradients), fp32
           marf_bf16x3a  the same in the all-operands-split bf16 recipe (--mask-precision lists the recipes)
           stock_fp32  the same nn.Sequential through stock PyTorch on a pre-built [B*Np, 426] input
           stock_bf16  the same under torch.autocast(bfloat16)
           stock_full  stock fp32 including the input formation (embedding gather, uv features, cat)
  step   one full training iteration (forward, loss, backward, Adam) in fp32 with and without
         use_implicit_mask, and with the image net in bf16x3 beside each --mask-precision recipe of the
         mask net (step_bf16x3_mask_fp32, step_bf16x3_mask_bf16x3a), alternating

Every repetition is timed with device events after a warm-up; the JSON line gives median, min and
max per variant, so a difference can be read against the run-to-run spread.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "masking-bundle-adjusting-neural-radiance-fields_amd")
for p in (PKG, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

B, H, W, PH, PW = 5, 360, 480, 180, 240
DEV = "cuda:0"


def timed(fns, warmup, reps):
    """Alternate the callables: warm-up rounds, then `reps` rounds of one call each, device-event timed."""
    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    return {k: dict(median_ms=float(np.median(v)), min_ms=float(min(v)), max_ms=float(max(v)), reps=len(v))
            for k, v in ms.items()}


def part_net(reps, warmup, mask_precisions=("fp32",)):
    import marf_hip
    import mask_ref
    from model.planar import ImplicitMask
    torch.manual_seed(0)
    Np = PH * PW
    net = ImplicitMask().to(DEV)
    embed = torch.randn(1500, 128, device=DEV)
    index = (torch.rand(B, 3, Np, device=DEV) < 0.1).to(torch.int32)
    dm = torch.randn(B, Np, 1, device=DEV)
    codes = {"fp32": marf_hip.MARF_FP32, "bf16x3a": marf_hip.MARF_BF16X3A}
    engs = {mp: marf_hip.MaskEngine(1500, codes[mp], H, W, PH, PW) for mp in ("fp32",) + tuple(
        mp for mp in mask_precisions if mp != "fp32")}
    eng = engs["fp32"]
    ps = list(net.parameters())
    xy = mask_ref.crop_grid(H, W, PH, PW).to(DEV)
    x_fixed = mask_ref.mask_input(index, embed, xy).reshape(B * Np, -1).contiguous()
    seq = net.mask_mapping

    def marf_on(e):
        def run():
            for p in ps:
                p.grad = None
            marf_hip.mask_forward(e, index, embed, ps).backward(dm)
        return run

    marf = marf_on(eng)

    def stock(autocast):
        def run():
            for p in ps:
                p.grad = None
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
                m = seq(x_fixed)
            m.float().view(B, Np, 1).backward(dm)
        return run

    def stock_full():
        for p in ps:
            p.grad = None
        seq(mask_ref.mask_input(index, embed, xy).reshape(B * Np, -1)).view(B, Np, 1).backward(dm)

    fns = {"marf": marf}
    fns.update({"marf_" + mp: marf_on(e) for mp, e in engs.items() if mp != "fp32"})
    fns.update({"stock_fp32": stock(False), "stock_bf16": stock(True), "stock_full": stock_full})
    res = timed(fns, warmup, reps)
    # same parameters, same input: the two fp32 paths agree (m to rounding; the gradients up to the
    # ReLU-kink flips of a random-sign upstream gradient)
    marf()
    g1 = torch.cat([p.grad.reshape(-1) for p in ps])
    stock(False)()
    g2 = torch.cat([p.grad.reshape(-1) for p in ps])
    with torch.no_grad():
        m1 = marf_hip.mask_forward(eng, index, embed, [p.detach() for p in ps])
        m2 = seq(x_fixed).view(B, Np, 1)
    res["m_max_abs_diff_vs_stock_fp32"] = float((m1 - m2).abs().max())
    res["grad_cosine_vs_stock_fp32"] = float(torch.dot(g1.double(), g2.double()) / (g1.double().norm() * g2.double().norm()))
    res["grad_max_rel_diff_vs_stock_fp32"] = float((g1 - g2).abs().max() / g2.abs().max())
    for mp, e in engs.items():
        if mp == "fp32":
            continue
        marf_on(e)()
        g3 = torch.cat([p.grad.reshape(-1) for p in ps])
        with torch.no_grad():
            m3 = marf_hip.mask_forward(e, index, embed, [p.detach() for p in ps])
        res[f"m_max_abs_diff_{mp}_vs_marf_fp32"] = float((m3 - m1).abs().max())
        res[f"grad_max_rel_diff_{mp}_vs_marf_fp32"] = float((g3 - g1).abs().max() / g1.abs().max())
    return res


def part_step(reps, warmup, mask_precisions=("fp32",)):
    import options
    from model import planar
    from util import EasyDict as edict
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[0:PH, 0:PW].astype(np.float32)
    img = np.stack([0.5 + 0.4 * np.sin(xx / 17 + c) * np.cos(yy / 13 - c) for c in range(3)]).astype(np.float32)
    img[:, 40:60, 50:90] = 1.0
    rgb = torch.from_numpy(np.stack([np.roll(img, 3 * s, axis=2) for s in range(B)])).to(DEV)
    masks = torch.from_numpy((rng.random((B, 1, PH, PW)) < 0.9).astype(np.float32)).to(DEV)
    models = {}
    variants = [("step_plain", False, "fp32", None), ("step_implicit_mask", True, "fp32", None)]
    variants += [(f"step_bf16x3_mask_{mp}", True, "bf16x3", mp) for mp in mask_precisions]
    for name, implicit, prec, mp in variants:
        opt = options.override_options(options.load_options("options/planar.yaml"), edict({
            "model": "planar", "yaml": "planar", "seed": 3, "barf_c2f": [0, 0.4], "precision": prec, "H": H, "W": W,
            "patch_H": PH, "patch_W": PW, "batch_size": B, "max_iter": 3000, "use_edges": False,
            "use_implicit_mask": implicit, "mask_precision": mp}))
        opt.device = DEV
        opt.output_path = "/tmp/marf_bench_mask"
        torch.manual_seed(3)
        m = planar.Model(opt)
        m.images = edict(rgb=rgb, masks=masks, masks_eroded=None, edges=None, gt_hom=None, gt=None)
        m.build_networks()
        m.setup_optimizer()
        models[name] = (m, edict(idx=torch.arange(B), images=m.images))

    def step(name):
        def run():
            m, var = models[name]
            m.optim.zero_grad()
            v = m.graph.forward(var, mode="train")
            loss = m._loss_sum(m.graph.compute_loss(v, mode="train"))
            loss.all.backward()
            m.optim.step()
        return run

    return timed({k: step(k) for k in models}, warmup, reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["net", "step"], required=True)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out")
    ap.add_argument("--mask-precision", nargs="+", choices=["fp32", "bf16x3a"], default=["fp32", "bf16x3a"],
                    help="mask-net recipes timed beside the fp32 rows")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mask.py needs a GPU")
    res = dict(part=a.part, size=dict(B=B, H=H, W=W, patch_H=PH, patch_W=PW), device=torch.cuda.get_device_name(0))
    mps = tuple(a.mask_precision)
    res.update(part_net(a.reps, a.warmup, mps) if a.part == "net" else part_step(a.reps, a.warmup, mps))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
