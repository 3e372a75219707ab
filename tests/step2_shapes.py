"""The shapes precision: bf16x3 reaches on the pixel-per-wave step kernel k_step2 (2 to 5 layers, hidden
widths 1..256, L = 0..32) beyond the ones the headline configs use, and their seeded inputs.  Nothing
here is used by the product; nothing here needs a GPU.

A case is (hidden widths, L, patches, patch h, patch w, c2f, progress).  Unless a row says otherwise:
2 patches of 24 x 20 on the 512 x 512 canvas -- 480 pixels per patch in 512 slots, so each patch ends
on a 128-slot tile with 96 valid slots -- seed 3, non-zero warps on every patch, Bernoulli(0.85) masks,
c2f [0, 0.4] at progress 0.2 (bands k >= L / 2 closed).  L = 0 is arch.posenc: None (the MLP reads the
two warped coordinates).  Rows that say otherwise, each for a reason settled on the host from the references
and the emulated recipe alone (tests/test_step2_shapes_cpu.py):
    seed 8      d2-L16, d3-L10, d4-L13, b-L0, b-L17, w-32x4: at seed 3 the emulated recipe itself is more than
                5e-3 from float64 on a gradient tensor (960 pixels: it moves between 5e-4 and 2.5e-2 with the
                seed); at seed 3, worst MLP tensor / d warp: 6.1e-3 / 6.4e-3, 1.9e-3 / 1.4e-2, 9.4e-3 / 1.3e-3,
                6.3e-3 / 2.6e-3, 3.2e-3 / 7.1e-3, 1.8e-2 / 7.7e-2 in that order
    progress    b-L32, n-L32 at 0.125 (bands below 10 open): at 0.2 bands up to 15 are open and the fp32 oracle
                is 6e-5 from float64 in rgb -- fp32 posenc arguments, not the kernel, would limit the 1e-5 bound
    c2f off     b-L20-noc2f: every band open, the four above 16 included; the reference's own fp32 is 5e-2 from
                float64 there, so its gradients and d warp are held against the fp32 oracle (whose prologue is the
                kernel's) and its gradients against the emulation

What each group is for (marf_abi.hip plan_step2_net / launch_s2 / l0_recompute / dzl_recompute,
marf_wgrad.hip marf_launch_wgrad):
    depth   every hidden layer 256 wide, so the compile-time instantiation (nk0, nta) of its L, at 2, 3
            and 4 layers: no hidden dgrad loop at 2; dz_{n-1} recomputed from 3 on, off at 2
    bands   nk0 = (L + 3) / 4 + 1 layer-0 k-steps, feat_0 rows of ldf0 = roundup(16 nk0, 32) bf16: 32 (L <= 4,
            stored), 64 / 96 (L = 5..16, recomputed by the layer-0 weight gradient), 96 (L = 17..20, stored:
            the recomputing stage builds 16 bands), >= 128 (L >= 21, stored); nk0 = 9 and r0 = 1 at L = 29..32
    widths  padded widths (no multiple of 32), one row tile, a last-layer input Kl != 256, a narrow first
            layer in front of a 256-wide one: each a different mix of weight-gradient launchers
    tiles   an odd tile count, one patch, three patches
"""
import numpy as np
import torch

CANVAS = 512
_D = dict(B=2, ph=24, pw=20, c2f=(0, 0.4), progress=0.2, seed=3)


def _c(hidden, L, **kw):
    return dict(_D, hidden=list(hidden), L=L, **kw)


DEPTH = {  # case -> (nk0, nta) of the instantiation it runs
    "d2-L8": (3, 2), "d2-L16": (5, 3), "d3-L10": (4, 2), "d4-L13": (5, 2),
}
CASES = {
    "d2-L8": _c([256], 8), "d2-L16": _c([256], 16, seed=8), "d3-L10": _c([256] * 2, 10, seed=8),
    "d4-L13": _c([256] * 3, 13, seed=8),
    "b-L0": _c([256, 256], 0, seed=8), "b-L17": _c([256, 256], 17, seed=8),
    **{f"b-L{L}": _c([256, 256], L) for L in (1, 4, 5, 12, 20, 21)},
    "b-L32": _c([256, 256], 32, progress=0.125),
    "b-L20-noc2f": _c([256, 256], 20, c2f=None),  # every band open, the four above 16 included
    "n-L0": _c([64, 64], 0), "n-L17": _c([64, 64], 17), "n-L32": _c([64, 64], 32, progress=0.125),
    "w-32": _c([32], 8), "w-32x4": _c([32] * 4, 8, seed=8), "w-48-40": _c([48, 40], 16), "w-100-33-7": _c([100, 33, 7], 8),
    "w-256-64-256": _c([256, 64, 256], 8), "w-256x3-32": _c([256, 256, 256, 32], 8), "w-64-256": _c([64, 256], 8),
    "t-3x16x20": _c([256] * 2, 10, B=3, ph=16, pw=20),  # 320 pixels = 3 tiles a patch, 9 tiles
    "t-1x24x20": _c([256] * 2, 10, B=1),                # one patch, 4 tiles
    "c1x2-64": _c([256] * 4, 8, ph=64, pw=64),          # the benchmarked instantiation (part 2 only)
}
BANDS = [k for k in CASES if k[:2] in ("b-", "n-")]
WIDTHS = [k for k in CASES if k.startswith("w-")]
TILES = ["t-3x16x20", "t-1x24x20"]
STEP_CASES = list(DEPTH) + BANDS + WIDTHS + TILES  # one step each against the oracle and float64
PLAIN16 = ["d2-L8", "b-L0", "b-L20", "b-L32"]      # also in plain bf16 and fp16
EMU_CASES = ["d2-L8", "d3-L10", "d4-L13", "w-256-64-256", "w-100-33-7", "b-L20", "b-L0", "c1x2-64"]
DZ_CASES = ["d3-L10", "w-256-64-256", "b-L20"]
PREDICT = ["d2-L8", "b-L20", "w-100-33-7"]
FULL = [k for k, c in CASES.items() if all(w == 256 for w in c["hidden"])]  # 256-wide hidden layers only


def dims(case):
    c = CASES[case]
    return [2 + 4 * c["L"]] + c["hidden"] + [3]


def arch(case):
    c = CASES[case]
    return {"layers": [None] + c["hidden"] + [3], "skip": [], "posenc": {"L_2D": c["L"]} if c["L"] > 0 else None}


def plan(case):
    """What marf_abi.hip's plan_step2_net and dzl_recompute decide for a case on the grid geometry, restated:
    (nk0, nta, dz_{n-1} recomputed).  Whether feat_0 is recomputed (l0_recompute: a 256-wide layer 0 at
    L = 5..16) is not here: no figure the ABI gives out shows it (marf_step_saved_bytes plans feat_0's rows
    either way), so no host test could compare it with the library; the GPU tests see it in results."""
    c = CASES[case]
    return (c["L"] + 3) // 4 + 1, (2 * c["L"] + 1 + 15) // 16, case in FULL and len(c["hidden"]) >= 2


def make_opt_for(case, tmp_path, precision, **over):
    from test_gpu_parity import make_opt
    c = CASES[case]
    return make_opt(tmp_path, H=CANVAS, W=CANVAS, patch_H=c["ph"], patch_W=c["pw"], batch_size=c["B"], precision=precision,
                    use_edges=False, arch=arch(case), barf_c2f=None if c["c2f"] is None else list(c["c2f"]), **over)


_INPUTS = {}


def inputs(case, seed=None):
    """(cfg, params, warp, rgb, mask, progress) of a case, as bf16x3_tile_ref.synthetic_inputs and
    test_gpu_parity._synthetic_setup make them: the seeded init of NeuralImageFunction (the first module Model
    builds under the seed), procedural targets, Bernoulli(0.85) masks, non-zero warps.  Built once per case
    and shared; the arrays are read-only."""
    c = CASES[case]
    seed = c["seed"] if seed is None else seed
    if (case, seed) in _INPUTS:
        return _INPUTS[case, seed]
    from model import planar
    B, ph, pw = c["B"], c["ph"], c["pw"]
    torch.manual_seed(seed)
    nif = planar.NeuralImageFunction(make_opt_for(case, None, "bf16x3"))
    params = [(l.weight.detach().numpy().copy(), l.bias.detach().numpy().copy()) for l in nif.mlp]
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.linspace(0, 1, ph), np.linspace(0, 1, pw), indexing="ij")
    rgb = np.stack([[0.5 + 0.4 * np.sin(2 * np.pi * (rng.uniform(1, 4) * xx + rng.uniform(1, 4) * yy) + rng.uniform(0, 6))
                     for _ in range(3)] for _ in range(B)]).astype(np.float32)
    mask = (rng.random((B, 1, ph, pw)) < 0.85).astype(np.float32)
    warp = (rng.standard_normal((B, 8)) * 0.01).astype(np.float32)
    cfg = dict(H=CANVAS, W=CANVAS, patch_H=ph, patch_W=pw, L=c["L"], c2f=None if c["c2f"] is None else list(c["c2f"]),
               max_iter=3000, lr=1e-3, lr_warp=1e-3, fix_first=True, use_edges=False, alpha_initial=0.0, alpha_final=1.0,
               skip=())
    _INPUTS[case, seed] = (cfg, params, warp, rgb, mask, c["progress"])
    return _INPUTS[case, seed]
