"""Timing of the Levenberg-Marquardt iteration (warp_solver: lm, marf_gn_normal) against the frozen Adam
iteration (the warp-only fused step) of the same library on one GPU, and one end-to-end registration (no
pass / fail: correctness is tested in tests/test_gpu_gn.py and tests/test_gpu_gn_solver.py).

    python tools/bench_gn.py [--configs c1 c3] [--reps 20] [--warmup 5] [--robust huber cauchy] [--e2e] [--out FILE]

Per config (c1, c3) and precision (fp32, bf16x3) two seeded frozen models on the same inputs -- `adam`
(Model.train_iteration with freeze_image) and `lm` (the same with warp_solver: lm: one full and one
loss-only Gauss-Newton launch, the tangent chain and the batched solve) -- alternate in one process:
warm-up rounds, then `reps` rounds of one iteration each, timed with device events.  One JSON line per
(config, precision): median, min and max per variant, then the per-launch HIP-event times
(marf_profile_*: gn, gn_loss, gn_reduce beside mlp_step_warp, warp_bwd) of a few more iterations.
--robust huber cauchy adds a model per loss (`lm_huber`, `lm_cauchy`: lm.robust at --robust-delta, the
launches gn_robust and gn_robust_loss) to the same alternation, so the robust iteration stands beside the
plain lm iteration of the same build, process and inputs.

--e2e: the C1 problem (tests/golden/cat_batch3_c1.npz, seed 3, bf16x3) is trained for max_iter iterations
and checkpointed; the same patches are then registered on the frozen image from the trained warps plus
seeded noise, with adam (3000 iterations) and with lm.  The truth is the trained warps' homographies:
Model.homography_error against them after every iteration.  One JSON line: per solver the error's start
and end, and the iterations and the summed iteration wall time (host clock around a synchronised
iteration; the error's own evaluation left out) until the error first falls below the Adam run's final
value.  Nothing here decides what is a gain.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "masking-bundle-adjusting-neural-radiance-fields_amd")
for p in (PKG, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import bench_warp_step as W  # noqa: E402  (configs, inputs, the alternating timer, the per-launch times)

DEV = W.DEV
PRECISIONS = ["fp32", "bf16x3"]


def build(cfg, precision, solver, images, **over):
    import options
    from model import planar
    from util import EasyDict as edict
    H, Wd, ph, pw, B, L, hidden, _ = W.CONFIGS[cfg]
    base = {"model": "planar", "yaml": "planar", "seed": 3, "barf_c2f": [0, 0.4], "precision": precision, "H": H, "W": Wd,
            "patch_H": ph, "patch_W": pw, "batch_size": B, "max_iter": 3000, "use_edges": False, "freeze_image": True,
            "warp_solver": solver, "arch": {"layers": [None] + list(hidden) + [3], "skip": [], "posenc": {"L_2D": L}}}
    base.update(over)
    opt = options.override_options(options.load_options("options/planar.yaml"), edict(base))
    opt.device = DEV
    opt.output_path = W.OUT_DIR
    opt.freq.vis = 10 ** 9
    opt.freq.scalar = 10 ** 9
    torch.manual_seed(3)
    m = planar.Model(opt)
    m.images = images
    m.build_networks()
    if images.get("warp0") is not None:
        m.graph.warp_param.weight.data.copy_(images.warp0)
    m.graph.neural_image.progress.data.fill_(0.2)
    m.setup_optimizer()
    m.timer = edict(start=time.time(), it_mean=None)
    return m, edict(idx=torch.arange(B), images=images)


def bench(cfg, precision, reps, warmup, robust=(), delta=0.1):
    images = W.make_images(cfg)
    models = {s: build(cfg, precision, s, images) for s in ("adam", "lm")}
    for kind in robust:
        models["lm_" + kind] = build(cfg, precision, "lm", images, lm={"robust": kind, "robust_delta": delta})

    def it(name):
        def run():
            m, var = models[name]
            m.train_iteration(var, W._Loader())
        return run

    fns = {k: it(k) for k in models}
    res = dict(config=cfg, precision=precision, device=torch.cuda.get_device_name(0),
               step_kernel=models["adam"][0].graph.neural_image.engine(torch.device(DEV)).net.step_kernel)
    res.update(W.timed(fns, warmup, reps))
    res["kernels"] = {k: W.kernel_times(f, 5) for k, f in fns.items()}
    return res


def e2e(train_iters, adam_iters, lm_iters, noise):
    from model import planar
    from util import EasyDict as edict
    z = np.load(os.path.join(ROOT, "tests", "golden", "cat_batch3_c1.npz"))
    rgb = torch.from_numpy(z["rgb"].astype(np.float32) / np.float32(255)).to(DEV)
    mask = torch.from_numpy(z["mask"].astype(np.float32)).to(DEV)
    images = edict(rgb=rgb, masks=mask, masks_eroded=mask, edges=None, gt_hom=None, gt=None, warp0=None)
    W.CONFIGS["c1e"] = (360, 480, 180, 240, 5, 8, [256] * 4, ["bf16x3"])
    # ---- train, checkpoint
    m, var = build("c1e", "bf16x3", "adam", images, freeze_image=False, max_iter=train_iters)
    t0 = time.time()
    for _ in range(train_iters):
        m.train_iteration(var, W._Loader())
        m.graph.warp_param.weight.data[0] = 0
    torch.cuda.synchronize()
    train_s = time.time() - t0
    ck = os.path.join(tempfile.mkdtemp(prefix="marf_bench_gn_"), "model.ckpt")
    m.save_checkpoint(ck)
    truth = m.graph.warp_param.weight.detach().clone()
    gt_hom = m.lie.sl3_to_SL3(truth)
    start = truth + noise * torch.randn(truth.shape, device=DEV, generator=torch.Generator(DEV).manual_seed(3))
    start[0] = 0
    res = dict(e2e="c1", precision="bf16x3", train_iters=train_iters, train_s=train_s, noise=noise,
               device=torch.cuda.get_device_name(0))
    runs = {}
    for solver, iters in (("adam", adam_iters), ("lm", lm_iters)):
        r, v = build("c1e", "bf16x3", solver, images, load=ck, max_iter=iters)
        r.graph.warp_param.weight.data.copy_(start)
        r.graph.neural_image.progress.data.fill_(1.0)  # every band on: the trained image as it ended
        r.it = r.graph.it = 0
        errs, secs = [float(r.homography_error(r.graph.warp_param.weight.detach(), gt_hom))], [0.0]
        for i in range(iters):
            torch.cuda.synchronize()
            t0 = time.time()
            r.train_iteration(v, W._Loader())
            r.graph.warp_param.weight.data[0] = 0
            r.graph.neural_image.progress.data.fill_(1.0)
            torch.cuda.synchronize()
            secs.append(secs[-1] + time.time() - t0)
            errs.append(float(r.homography_error(r.graph.warp_param.weight.detach(), gt_hom)))
        runs[solver] = (errs, secs)
    final_adam = runs["adam"][0][-1]
    for solver, (errs, secs) in runs.items():
        hit = next((i for i, e in enumerate(errs) if e <= final_adam), None)
        marks = [i for i in (1, 2, 3, 5, 10, 20, 30, 50, 100, 300, 1000, 3000) if i < len(errs)]
        res[solver] = dict(iters=len(errs) - 1, err_start=errs[0], err_end=errs[-1], err_min=min(errs), total_s=secs[-1],
                           iters_to_adam_final=hit, s_to_adam_final=None if hit is None else secs[hit],
                           trace={str(i): [errs[i], secs[i]] for i in marks})  # iteration -> [error, seconds so far]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="*", choices=["c1", "c3"], default=["c1", "c3"])
    ap.add_argument("--precision", nargs="+", choices=PRECISIONS, default=PRECISIONS)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--robust", nargs="*", choices=["huber", "cauchy"], default=[])
    ap.add_argument("--robust-delta", type=float, default=0.1)
    ap.add_argument("--e2e", action="store_true")
    ap.add_argument("--train-iters", type=int, default=3000)
    ap.add_argument("--adam-iters", type=int, default=3000)
    ap.add_argument("--lm-iters", type=int, default=50)
    ap.add_argument("--noise", type=float, default=0.01)
    ap.add_argument("--out")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_gn.py needs a GPU")

    def emit(res):
        line = json.dumps(res)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")

    for cfg in a.configs:
        for prec in a.precision:
            emit(bench(cfg, prec, a.reps, a.warmup, a.robust, a.robust_delta))
            torch.cuda.empty_cache()
    if a.e2e:
        emit(e2e(a.train_iters, a.adam_iters, a.lm_iters, a.noise))


if __name__ == "__main__":
    main()
