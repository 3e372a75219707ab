"""Shared set-up of the implicit-mask tests: the options of the reference fixtures
(tests/golden/mask_edges{0,1}.npz, written by tests/golden/make_mask_golden.py) and a Model on them."""
import numpy as np
import torch

LOSS_KEYS = ("render", "rgb", "mask", "edge", "all")
MASK_PARAM_NAMES = [f"mask_mapping.{i}.{k}" for i in (0, 2, 4, 6, 8) for k in ("weight", "bias")]


def fixture_opt(z, use_edges, device, output_path, **extra):
    """options/planar.yaml with the fixture's overrides (make_mask_golden.overrides)."""
    import options
    from util import EasyDict as edict
    H, W, PH, PW, B, _, max_iter, a0, a1 = (float(v) for v in z["cfg"])
    over = {"model": "planar", "yaml": "planar", "seed": 3, "barf_c2f": [0, 0.4], "precision": "fp32",
            "H": int(H), "W": int(W), "patch_H": int(PH), "patch_W": int(PW), "batch_size": int(B),
            "max_iter": int(max_iter), "use_implicit_mask": True, "build_single_masks": False,
            "use_edges": bool(use_edges), "alpha_initial": a0, "alpha_final": a1,
            "arch": {"layers": [None, 64, 64, 3], "skip": [], "posenc": {"L_2D": 8}}}
    over.update(extra)
    opt = options.override_options(options.load_options("options/planar.yaml"), edict(over))
    opt.device = device
    opt.output_path = str(output_path)
    return opt


def fixture_model(z, use_edges, device, output_path, **extra):
    """A seed-3 Model on the fixture's inputs, the warps set to the fixture's (as the generator does)."""
    from model import planar
    from util import EasyDict as edict
    opt = fixture_opt(z, use_edges, device, output_path, **extra)
    torch.manual_seed(3)
    m = planar.Model(opt)
    t = lambda k: torch.from_numpy(np.ascontiguousarray(z[k])).to(device)  # noqa: E731
    m.images = edict(rgb=t("rgb"), masks=t("masks"), masks_eroded=t("masks"), edges=t("edges"), gt_hom=None, gt=None)
    m.build_networks()
    m.graph.warp_param.weight.data.copy_(t("warp0"))
    return m
