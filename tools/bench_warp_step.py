"""Timing of the warp-only iteration (freeze_image) against the full training iteration of the same
library on one GPU (no pass / fail: correctness is tested in tests/test_gpu_warp_step.py).

    python tools/bench_warp_step.py [--configs c1 c3 c5] [--reps 20] [--warmup 5] [--out FILE]

Per config and precision (c1, c3: bf16x3; c5: bf16 and bf16x3) two seeded models on the same inputs --
`full` (Model.train_iteration as it is) and `frozen` (the same with freeze_image) -- alternate in one
process: warm-up rounds, then `reps` rounds of one iteration each, timed with device events.  One JSON
line per (config, precision): median, min and max per variant, then the per-kernel HIP-event times
(marf_profile_*) of a few more iterations of each.  Read a difference of the medians against the full
step's own min - max spread; nothing here decides what is a gain.
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
if PKG not in sys.path:
    sys.path.insert(0, PKG)

DEV = "cuda:0"
OUT_DIR = tempfile.mkdtemp(prefix="marf_bench_warp_step_")# name: (canvas H, W, patch h, w, patches, L, hidden widths, precisions)
CONFIGS = {
    "c1": (360, 480, 180, 240, 5, 8, [256] * 4, ["bf16x3"]),
    "c3": (512, 512, 256, 256, 64, 16, [256] * 4, ["bf16x3"]),
    "c5": (512, 512, 256, 256, 128, 16, [512] * 8, ["bf16", "bf16x3"]),
}


class _Loader:
    def set_postfix(self, **kw):
        pass


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


def build(cfg, precision, freeze, images):
    import options
    from model import planar
    from util import EasyDict as edict
    H, W, ph, pw, B, L, hidden, _ = CONFIGS[cfg]
    opt = options.override_options(options.load_options("options/planar.yaml"), edict({
        "model": "planar", "yaml": "planar", "seed": 3, "barf_c2f": [0, 0.4], "precision": precision, "H": H, "W": W,
        "patch_H": ph, "patch_W": pw, "batch_size": B, "max_iter": 3000, "use_edges": False, "freeze_image": freeze,
        "arch": {"layers": [None] + list(hidden) + [3], "skip": [], "posenc": {"L_2D": L}}}))
    opt.device = DEV
    opt.output_path = OUT_DIR
    opt.freq.vis = 10 ** 9
    opt.freq.scalar = 10 ** 9
    torch.manual_seed(3)
    m = planar.Model(opt)
    m.images = images
    m.build_networks()
    m.graph.warp_param.weight.data.copy_(images.warp0)
    m.graph.neural_image.progress.data.fill_(0.2)
    m.setup_optimizer()
    m.timer = edict(start=time.time(), it_mean=None)
    return m, edict(idx=torch.arange(B), images=images)


def make_images(cfg):
    from util import EasyDict as edict
    _, _, ph, pw, B, _, _, _ = CONFIGS[cfg]
    rng = np.random.default_rng(3)
    yy, xx = np.meshgrid(np.linspace(0, 1, ph, dtype=np.float32), np.linspace(0, 1, pw, dtype=np.float32), indexing="ij")
    rgb = np.stack([[0.5 + 0.4 * np.sin(2 * np.pi * (rng.uniform(1, 4) * xx + rng.uniform(1, 4) * yy) + rng.uniform(0, 6))
                     for _ in range(3)] for _ in range(B)]).astype(np.float32)
    mask = (rng.random((B, 1, ph, pw)) < 0.85).astype(np.float32)
    warp = (rng.standard_normal((B, 8)) * 0.01).astype(np.float32)
    mk = torch.from_numpy(mask).to(DEV)
    return edict(rgb=torch.from_numpy(rgb).to(DEV), masks=mk, masks_eroded=mk, edges=None, gt_hom=None, gt=None,
                 warp0=torch.from_numpy(warp).to(DEV))


def kernel_times(run, n):
    """Mean HIP-event milliseconds per launch name over n iterations of run()."""
    import marf_hip
    marf_hip.profile_enable(True)
    marf_hip.profile_reset()
    for _ in range(n):
        run()
    torch.cuda.synchronize()
    out = {k: dict(ms_per_iter=tot / n, launches_per_iter=cnt / n) for k, (tot, cnt) in marf_hip.profile_read().items()}
    marf_hip.profile_enable(False)
    return out


def bench(cfg, precision, reps, warmup):
    images = make_images(cfg)
    models = {"full": build(cfg, precision, False, images), "frozen": build(cfg, precision, True, images)}
    kernel = models["full"][0].graph.neural_image.engine(torch.device(DEV)).net.step_kernel

    def it(name):
        def run():
            m, var = models[name]
            m.train_iteration(var, _Loader())
        return run

    fns = {k: it(k) for k in models}
    res = dict(config=cfg, precision=precision, step_kernel=kernel, device=torch.cuda.get_device_name(0))
    res.update(timed(fns, warmup, reps))
    res["kernels"] = {k: kernel_times(f, 5) for k, f in fns.items()}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", choices=list(CONFIGS), default=list(CONFIGS))
    ap.add_argument("--precision", nargs="+", help="only these of a config's precisions")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_warp_step.py needs a GPU")
    for cfg in a.configs:
        for prec in CONFIGS[cfg][7]:
            if a.precision and prec not in a.precision:
                continue
            line = json.dumps(bench(cfg, prec, a.reps, a.warmup))
            print(line, flush=True)
            if a.out:
                with open(a.out, "a") as f:
                    f.write(line + "\n")
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
