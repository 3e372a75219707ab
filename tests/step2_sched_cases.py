"""Small fused-step cases for the step kernel's register placement and instruction order (helper
module, not a test file; used by test_gpu_step2_sched.py and tools/make_step2_sched_bits.py).

A change of where k_step2's fragments and accumulators live, or of the issue order of independent
instructions, changes no arithmetic, so every result bit of a step stays what the parent commit's
library computed.  The cases are the smallest shapes that reach each body of the kernel:
MARF_STEP2_GRID (read at every launch) caps the persistent grid, so a few blocks take many tiles --
the last-layer weight gradient accumulates over them in LDS, groups of two tiles and a last single
tile both occur, and the dgrad runs with a sink set.

The tile-* cases pin the tile kernels (plain bf16, fp32, fp16, one skip net) in the same way; their
digests come from a build of the commit named under "tile_cases" in the fixture.  No candidate case
had to be left out: the parent library reproduced every one in three separate processes.

The split-*, plain-fwd-bwd, render-* and mask-* cases ("tile_view_cases" in the fixture, with their
parent commit) pin what had no bit fixture before the tile phases were written once over a tile view:
the split tile step k_mlp_step_split and its render, the separate k_mlp_fwd / k_mlp_bwd path and the
mask network's kernels in both recipes.  Kept on the same rule; none had to be left out.

The wg-* cases ("wgrad_cases" in the fixture, with their parent commit) reach the weight-gradient
paths that no case above does: the per-layer launches of the LDS-DMA kernel with and without its
recomputing instantiations, the register-staged kernel on T16 tensors, range mode (the pipelined
step), more than one output block per chunk under both block maps, and fp32 fragments in 128 x 64
blocks.  Same rule (the parent library, three separate processes); none had to be left out.

wg-fold ("backward_layer_cases" in the fixture, with its parent commit) pins the last-layer
reduction of a step above 1,024 partials, which folds them first.  Same rule; kept.

`case_launches` counts a case's launches per profile scope (tests/golden/backward_launches.json,
test_gpu_backward_launches.py).
"""
import hashlib
import os
import time

import numpy as np
import torch

import step_bits

HERE = os.path.dirname(os.path.abspath(__file__))
BITS_JSON = os.path.join(HERE, "golden", "step2_sched_bits.json")
DEV = step_bits.DEV

FULL = [256] * 4
# per-layer weight-gradient launches that read feat_0 and dz_{n-1} as the step kernel stored them
_STORED = {"MARF_WGRAD_FUSED": "0", "MARF_F0_RECOMPUTE": "0", "MARF_DZL_RECOMPUTE": "0"}
CASES = {
    # name: (patches, patch_H, patch_W, L, hidden widths, environment, model options)
    # 32 tiles on 3 blocks (11, 11, 10 tiles): (5, 3) instantiation
    "acc": (1, 64, 64, 16, FULL, {"MARF_STEP2_GRID": "3"}, {}),
    # 2,080 pixels per patch: padded pixel slots in each patch's last tile; (3, 2) instantiation
    "pad-L8": (2, 40, 52, 8, FULL, {"MARF_STEP2_GRID": "2"}, {}),
    "L10": (1, 64, 64, 10, FULL, {"MARF_STEP2_GRID": "5"}, {}),   # (4, 2)
    "L13": (1, 64, 64, 13, FULL, {"MARF_STEP2_GRID": "5"}, {}),   # (5, 2)
    # the generic kernel with an odd row-tile count (96 = 3 x 32)
    "narrow": (2, 64, 64, 8, [128, 96, 128], {"MARF_STEP2_GRID": "2"}, {}),
    # the generic kernel on the full-width net (the switch is read at net creation)
    "generic-full": (1, 64, 64, 16, FULL, {"MARF_STEP2_GRID": "3", "MARF_STEP2_GENERIC": "1"}, {}),
    # k_step2dz (read at net creation)
    "dz": (1, 64, 64, 16, FULL, {"MARF_STEP2_GRID": "3", "MARF_STEP2_DZ": "1"}, {}),
    # k_step2h
    "fp16x2": (1, 64, 64, 16, FULL, {"MARF_STEP2_GRID": "3"}, {"precision": "fp16x2"}),
    # the tile kernels (k_mlp_step, the k_wgrad family, marf_gemm.h), grid unconstrained: one block
    # per 64- or 128-pixel tile.  Their partials are reduced in a fixed order, so a step's bits are a
    # function of the build alone; each case was kept because the parent library reproduced its own
    # digests in three separate processes ("skip": opt.arch.skip, the SK instantiation).
    "tile-bf16": (1, 64, 64, 16, FULL, {}, {"precision": "bf16"}),
    "tile-fp32": (1, 64, 64, 8, FULL, {}, {"precision": "fp32"}),
    "tile-fp16": (1, 64, 64, 16, FULL, {}, {"precision": "fp16"}),
    "tile-skip": (1, 64, 64, 8, FULL, {}, {"precision": "bf16", "skip": [2]}),
    # k_mlp_step_split (bf16x3 on nets k_step2 cannot hold).  TP = 128: six layers force the tile
    # kernel, one row tile per wave
    "split-tp128": (1, 64, 64, 8, [128] * 6, {}, {}),
    # TP = 64 (width above 256), four row tiles per wave: the 2-deep ring of gemm_rows_split
    "split-tp64-ring": (1, 64, 64, 16, [512] * 2, {}, {}),
    # 288 = 9 x 32: waves get 3 and 2 row tiles; 9 k-steps: the GEMM's remainder
    "split-odd": (1, 64, 64, 8, [288, 512, 288], {}, {}),
    # 2,700 pixels per patch: the last tile of each patch is partly padding
    "split-pad": (2, 50, 54, 8, [128] * 6, {}, {}),
    # k_mlp_fwd + k_mlp_bwd: the differentiable forward / backward path (no fused step).  No fixture
    # of test_gpu_parity.py pinned their bits: its fused-against-separate test compares two paths of
    # one build
    "plain-fwd-bwd": (1, 64, 64, 8, FULL, {}, {"precision": "bf16", "fused_step": False}),
    # ---- the weight-gradient paths no case above reaches ("wgrad_cases" in the fixture)
    # the per-layer launches of the LDS-DMA kernel, its DZL and F0 instantiations among them
    "wg-perlayer": (1, 64, 64, 16, FULL, {"MARF_WGRAD_FUSED": "0"}, {}),
    # ... on stored T16 tensors: the 96-wide layer 0 and the 256-wide hidden layers
    "wg-stored": (1, 64, 64, 16, FULL, _STORED, {}),
    # ... and with the register-staged kernel reading T16 (t16_off), at 256 x 256 and 256 x 128
    "wg-staged-t16": (1, 64, 64, 16, FULL, dict(_STORED, MARF_WGRAD_DMA="0"), {}),
    # range mode: 2 x 17 tiles of 128 slots in pieces of 12 tiles -> 12, 12 and 10 tiles; 16 blocks
    # per piece (3 stages of 32 rows each), every CU's block on the last, shorter one
    "wg-ranged": (2, 40, 52, 16, FULL, {"MARF_PIPE": "1", "MARF_PIPE_WG": "16", "MARF_PIPE_PIECE": "12"}, {}),
    # k_wgrad_dma with 2 x 2 output blocks per chunk.  split_k: 2 patches of 2,080 pixels padded to the
    # tile give S = 4,224 (64-pixel tiles) or 4,352 (128), chunk 64, 66 or 68 chunks -- no multiple of
    # 8: the plain block map (block -> chunk block % n_chunks)
    "wg-wide-bf16": (2, 40, 52, 8, [512, 512], {}, {"precision": "bf16"}),
    # S = 4,096, chunk 64, 64 chunks -- a multiple of 8: the XCD-grouped block map
    "wg-wide-bf16-x8": (1, 64, 64, 8, [512, 512], {}, {"precision": "bf16"}),
    # fp32 fragments in 128 x 64 output blocks (M = 128 and M = 96)
    "wg-fp32-narrow": (1, 64, 64, 8, [128, 96, 128], {}, {"precision": "fp32"}),
    # ---- "backward_layer_cases" in the fixture
    # the last-layer reduction above 1,024 partials: k_fold_partials into the step buffer's `part`, then
    # the reduction of its groups.  fp32 tiles hold 64 slots; 13,456 pixels per patch pad to 13,568
    # slots = 212 tiles (the 211th holds 16 pixels, the 212th none), 5 patches: 1,060 tiles
    "wg-fold": (5, 116, 116, 8, [128, 96, 128], {}, {"precision": "fp32"}),
}
# the FWD instantiation of k_mlp_step_split: Model.predict_entire_image of the 6 x 128 net on a
# 45 x 61 canvas (2,745 pixels: no multiple of 128)
RENDER_CASES = {"render-deep": (45, 61, 8, [128] * 6)}
# the mask network (k_mask_fwd / k_mask_bwd, fp32 and the all-operands-split recipe) on the seeded
# cases of mask_split_ref.py: m and every parameter gradient of marf_hip.mask_forward + backward
MASK_CASES = {f"mask-{prec}-{shape}": (prec, shape) for prec in ("fp32", "bf16x3a") for shape in ("ragged", "tiny", "exact")}
ALL_CASES = list(CASES) + list(RENDER_CASES) + list(MASK_CASES)
# the launch census (case_launches): the fused weight gradients (plain and with `post`), the per-layer
# launches on recomputed and on stored operands, the pipelined step, the tile step in bf16 and fp32, the
# split tile step, the separate forward / backward path and the mask network in both recipes
LAUNCH_CASES = ["acc", "fp16x2", "wg-perlayer", "wg-stored", "wg-ranged", "tile-bf16", "tile-fp32", "split-tp128",
                "plain-fwd-bwd", "mask-fp32-tiny", "mask-bf16x3a-tiny"]


def build(case, setenv, out="/tmp/marf_sched"):
    """The seeded model of `case` (as test_gpu_dzl_recompute._build) and its var bundle.
    setenv(name, value) sets the case's environment before the model is built."""
    from model import planar
    from util import EasyDict as edict
    B, ph, pw, L, hidden, env, over = CASES[case]
    for k, v in env.items():
        setenv(k, v)
    over = dict(over)
    skip = over.pop("skip", [])
    opt = step_bits._opt(out, H=512, W=512, patch_H=ph, patch_W=pw, batch_size=B, use_edges=False,
                         arch={"layers": [None] + list(hidden) + [3], "skip": skip, "posenc": {"L_2D": L}}, **over)
    torch.manual_seed(3)
    m = planar.Model(opt)
    rng = np.random.default_rng(3)
    yy, xx = np.meshgrid(np.linspace(0, 1, ph), np.linspace(0, 1, pw), indexing="ij")
    rgb = np.stack([[0.5 + 0.4 * np.sin(2 * np.pi * (rng.uniform(1, 4) * xx + rng.uniform(1, 4) * yy) + rng.uniform(0, 6))
                     for _ in range(3)] for _ in range(B)]).astype(np.float32)
    mask = (rng.random((B, 1, ph, pw)) < 0.85).astype(np.float32)
    warp = (rng.standard_normal((B, 8)) * 0.01).astype(np.float32)
    mk = torch.from_numpy(mask).to(DEV)
    m.images = edict(rgb=torch.from_numpy(rgb).to(DEV), masks=mk, masks_eroded=mk, edges=None, gt_hom=None, gt=None)
    m.build_networks()
    m.graph.warp_param.weight.data.copy_(torch.from_numpy(warp).to(DEV))
    m.graph.neural_image.progress.data.fill_(0.2)
    m.setup_optimizer()
    m.timer = edict(start=time.time(), it_mean=None)
    return m, edict(idx=torch.arange(B), images=m.images)


def step(m, var, info=None):
    """rgb, loss, every MLP gradient and bias gradient, and d warp of one fused step (the state is
    left as it was).  info["fused"]: whether the forward ran the fused step kernel."""
    m.optim.zero_grad()
    v = m.graph.forward(var, mode="train")
    if info is not None:
        info["fused"] = v.fused_loss is not None
    loss = m.summarize_loss(m.graph.compute_loss(v, mode="train"))
    loss.all.backward()
    out = {"rgb": v.rgb_prediction.detach().clone(), "loss": loss.rgb.detach().reshape(1).clone(),
           "dh": m.graph.warp_param.weight.grad.detach().clone()}
    for i, lay in enumerate(m.graph.neural_image.mlp):
        out[f"dW{i}"] = lay.weight.grad.detach().clone()
        out[f"db{i}"] = lay.bias.grad.detach().clone()
    return out


def digest(t):
    a = t.detach().contiguous().cpu()
    return hashlib.sha1(a.view(torch.uint8).numpy().tobytes()).hexdigest()


def render_bits(case, out="/tmp/marf_sched"):
    from model import planar
    H, W, L, hidden = RENDER_CASES[case]
    opt = step_bits._opt(out, H=H, W=W, patch_H=32, patch_W=32, batch_size=2, use_edges=False,
                         arch={"layers": [None] + list(hidden) + [3], "skip": [], "posenc": {"L_2D": L}})
    torch.manual_seed(3)
    m = planar.Model(opt)
    m.build_networks()
    m.graph.neural_image.progress.data.fill_(0.2)
    kernel = m.graph.neural_image.engine(torch.device(DEV)).net.step_kernel
    img = m.predict_entire_image()
    assert tuple(img.shape) == (3, H, W) and torch.isfinite(img).all(), case
    return {"kernel": kernel, "bits": {"rgb": digest(img)}}


def mask_bits(case):
    import marf_hip
    import mask_split_ref as sr
    from mask_common import MASK_PARAM_NAMES
    prec, shape = MASK_CASES[case]
    B, ph, pw = sr.SHAPES[shape]
    c = sr.case(shape)
    code = {"fp32": marf_hip.MARF_FP32, "bf16x3a": marf_hip.MARF_BF16X3A}[prec]
    eng = marf_hip.MaskEngine(sr.N_VOCAB, code, 2 * ph, 2 * pw, ph, pw)
    ps = [p.to(DEV).requires_grad_() for p in c["params"]]
    m = marf_hip.mask_forward(eng, c["index"].to(torch.int32).to(DEV), c["embed"].to(DEV), ps)
    m.backward(c["dm"].to(DEV))
    torch.cuda.synchronize()
    out = {"m": m.detach()}
    out.update({name: p.grad for name, p in zip(MASK_PARAM_NAMES, ps)})
    assert all(torch.isfinite(v).all() for v in out.values()), case
    return {"kernel": "k_mask_fwd+k_mask_bwd " + prec, "bits": {k: digest(v) for k, v in out.items()}}


def case_launches(case, setenv):
    """{profile scope: launches} of one step of `case` (the mask network's forward + backward), counted
    by the library's profile hooks; profiling is off again and reset afterwards."""
    import marf_hip
    marf_hip.profile_enable(True)
    try:
        if case in MASK_CASES:
            marf_hip.profile_reset()
            mask_bits(case)
        else:
            m, var = build(case, setenv)
            marf_hip.profile_reset()
            step(m, var)
        torch.cuda.synchronize()
        return {name: int(n) for name, (_, n) in marf_hip.profile_read().items()}
    finally:
        marf_hip.profile_enable(False)
        marf_hip.profile_reset()


def case_bits(case, setenv):
    """{"kernel": the step kernel's name, "bits": {tensor: sha1 of its bytes}} of one step of `case`
    (of the render / the mask network's forward + backward for those cases)."""
    if case in RENDER_CASES:
        return render_bits(case)
    if case in MASK_CASES:
        return mask_bits(case)
    m, var = build(case, setenv)
    kernel = m.graph.neural_image.engine(torch.device(DEV)).net.step_kernel
    info = {}
    out = step(m, var, info)
    assert all(torch.isfinite(v).all() for v in out.values()), case
    if not CASES[case][6].get("fused_step", True):  # the separate kernels ran, not the net's step kernel
        assert not info["fused"], case
        kernel = "k_mlp_fwd+k_mlp_bwd"
    return {"kernel": kernel, "bits": {k: digest(v) for k, v in out.items()}}
