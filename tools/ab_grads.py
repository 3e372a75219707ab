"""Dump two training iterations at C3 widths so two builds can be compared bit for bit:
    [MARF_LIB=<lib>] python tools/ab_grads.py out.npz [precision] [patches] [--mode M] [--mask] [--package DIR]
(default bf16, 8 patches; 4 or 12 patches give the step kernel an odd tile count per block), then
    python tools/ab_grads.py --compare a.npz b.npz
Two libraries: MARF_LIB.  Two Python layers on one library: --package, the package directory to import
(default: this tree's; e.g. a `git archive` of another commit's, with the same lib/libmarf.so in it).
--mode picks the path through the binding layer:
    step    the fused step (the default)
    render  the general forward + backward (fused_step: false)
    frozen  the warp-only fused step (freeze_image), the warps moved by Adam
    lm      Graph.lm_step on the frozen image (Gauss-Newton normal equations; fp32 or bf16x3)
--mask runs `step` with the learned mask network (use_implicit_mask, mask_precision fp32) at the shapes of
tests/mask_common.py's fixture.  Between the two iterations the library's Adam moves whatever has a
gradient, so the second one packs the weights again."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = {"step": {}, "render": {"fused_step": False}, "frozen": {"freeze_image": True},
         "lm": {"freeze_image": True, "warp_solver": "lm"}}


def _graph(mode, precision, B, mask, dev):
    """(graph, var) of the run: bench.py's C3 options and synthetic inputs, or the mask fixture's model."""
    import torch
    from util import EasyDict as edict
    if mask:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import mask_common
        z = np.load(os.path.join(ROOT, "tests", "golden", "mask_edges0.npz"), allow_pickle=False)
        import bench
        m = mask_common.fixture_model(z, 0, str(dev), bench._scratch_dir(), precision=precision, mask_precision="fp32",
                                      **MODES[mode])
        m.graph.neural_image.progress.data.fill_(0.2)
        return m.graph, edict(images=m.images)
    import bench
    from model import planar
    opt = bench.make_opt("c3", precision, B)
    opt.device = str(dev)
    for k, v in MODES[mode].items():
        opt[k] = v
    torch.manual_seed(3)
    graph = planar.Graph(opt).to(dev)
    graph.neural_image.progress.data.fill_(0.2)
    rgb, masks, warp = bench.synthetic_inputs(B, opt.patch_H, opt.patch_W, dev)
    with torch.no_grad():
        graph.warp_param.weight.copy_(warp)
    return graph, edict(images=edict(rgb=rgb, masks=masks, masks_eroded=masks, edges=None))


def dump(path, precision="bf16", B=8, mode="step", mask=False, package=None):
    sys.path.insert(0, ROOT)
    import bench  # noqa: F401  (puts this tree's package directory on sys.path; --package goes in front of it)
    if package:
        sys.path.insert(0, os.path.abspath(package))
    import torch
    import marf_hip
    print("package", os.path.relpath(os.path.dirname(os.path.abspath(marf_hip.__file__)), ROOT),
          "library", os.path.relpath(marf_hip.LIB_PATH, ROOT))
    dev = torch.device("cuda", 0)
    graph, var = _graph(mode, precision, B, mask, dev)
    graph.need_edges = False
    optim = marf_hip.Adam(list(graph.parameters()), lr=1e-3)
    out = {}
    for it in range(2):
        if mode == "lm":
            v, loss = graph.lm_step(var)
            out[f"loss{it}"] = np.array([float(loss.rgb)])
            for k in ("sse", "sse_trial", "msum", "accepted", "delta"):
                out[f"lm.{k}{it}"] = graph.lm_last[k].cpu().numpy()
        else:
            optim.zero_grad(set_to_none=True)
            v = graph.forward(var, mode="train")
            losses = graph.compute_loss(v, mode="train")
            loss = losses.render if mask else losses.rgb
            loss.backward()
            out[f"loss{it}"] = np.array([float(loss)])
            for n, p in graph.named_parameters():
                if p.grad is not None:
                    out[f"{n}.grad{it}"] = p.grad.cpu().numpy()
            optim.step()
        out[f"rgb{it}"] = v.rgb_prediction.detach().cpu().numpy()
        if mask:
            out[f"mask{it}"] = v.mask_prediction.detach().cpu().numpy()
    for n, p in graph.named_parameters():
        out[f"{n}.final"] = p.detach().cpu().numpy()
    np.savez(path, **out)
    print("wrote", path, len(out))


def compare(a, b):
    A, Bz = np.load(a), np.load(b)
    bad = 0
    if sorted(A.files) != sorted(Bz.files):
        bad += 1
        print("different arrays:", sorted(set(A.files) ^ set(Bz.files)))
    for k in A.files:
        if k not in Bz.files:
            continue
        same = A[k].shape == Bz[k].shape and A[k].dtype == Bz[k].dtype and A[k].tobytes() == Bz[k].tobytes()
        if not same:
            bad += 1
            if A[k].shape != Bz[k].shape:
                print(f"{k}: shapes {A[k].shape} and {Bz[k].shape}")
            else:
                print(f"{k}: max |diff| {np.abs(A[k].astype(np.float64) - Bz[k].astype(np.float64)).max():.3e}")
    print("identical" if bad == 0 else f"{bad} arrays differ")
    return bad


if __name__ == "__main__":
    if sys.argv[1] == "--compare":
        sys.exit(1 if compare(sys.argv[2], sys.argv[3]) else 0)
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("precision", nargs="?", default="bf16")
    ap.add_argument("patches", nargs="?", type=int, default=8)
    ap.add_argument("--mode", default="step", choices=list(MODES))
    ap.add_argument("--mask", action="store_true")
    ap.add_argument("--package", default=None)
    a = ap.parse_args()
    dump(a.out, a.precision, a.patches, a.mode, a.mask, a.package)
