"""The smallest shapes that reach each path of the plain 16-bit tile step (precision: bf16 / fp16:
k_mlp_step<PrecBF16 | PrecF16, TP, BL, NW, SK> and the 16-bit weight-gradient kernels), and their seeded
inputs.  Nothing here is used by the product; nothing here needs a GPU.  Every row runs in bf16 and in fp16.

Unless a row says otherwise, as tests/step2_shapes.py: 2 patches of 24 x 20 on the 512 x 512 canvas -- 480
pixels a patch in 512 slots, so each patch's last 128-slot tile has 96 valid slots (the last 64-slot tile
32) -- Bernoulli(0.85) masks, warps 0.01 randn, c2f [0, 0.4] at progress 0.2.  S = 1024 pixel slots, so the
weight gradients split them into 16 chunks of 64 (split_k(S, 256)).

What a row reaches, read off net_create (marf_abi.hip: TP, the 8-wave tile), launch_step_b / launch_step_t
(marf_step.hip: BL = the hidden widths padded to 32 sum to <= 1024, SK = a skip layer) and wg_pick
(marf_args.h) on wg_shape (M = Mp[l], K = ldf = Kp[l], ldz = Kp[l + 1]); plan() below restates those rules
and tests/test_plain16_cpu.py holds the table to it and plan() to the library's marf_step_saved_bytes.
The last layer's weight gradient is the step kernel's own (step_wlast_grad on Kp[n-1] columns).

    case          step kernel              weight gradients, layer 0 upwards (rows x cols of M x K blocks)
    p-tp128       TP128 NW4 BL             staged 256x64 (1x1); DMA256 (1x1)
    p-L16         TP128 NW4 BL             DMA96 (1x1); DMA256
    p-L16-nodma   the same, MARF_WGRAD_DMA=0: staged 256x128 (one 96-column block); staged 256x256
    p-narrow      TP128 NW4 BL             staged 128x64 on 128 x 64 (1x1); on 96 x 128 (a partial row block, 2
                                           column blocks); on 128 x 96 (64 + 32 columns)
    p-mid         TP128 NW4 BL             staged 256x64 (1x1); staged 128x64 on 160 x 256 (128 + 32 rows, 4
                                           column blocks -- M < 256 never takes the 256-row kernels); staged
                                           256x128 on 256 x 160 (128 + 32 columns)
    p-288         TP128 NW8 BL             Kmax = 288 > 256: the 8-wave tile.  staged 256x64 on 288 x 64 (256 + 32
                                           rows); staged 256x256 on 288 x 288 (2 x 2 blocks, both remainders)
    p-288-nw4     TP64 NW4 BL              the same net with MARF_STEP_NW=4 at net creation
    p-wide8       TP128 NW8, BL off        biases 512 + 512 + 32 = 1056 > 1024.  DMA96 on 512 x 96 (2 row blocks);
                                           DMA256 on 512 x 512 (2 x 2); staged 128x64 on 32 x 512 (M = 32, 8
                                           column blocks); the last layer's K = 32
    p-skip        TP128 NW4 BL SK          [64, 64, 64], skip [2]: Kp = 64, 64, 128, 64.  staged 128x64 x 3 (layer 1
                                           reads dz rows of stride 128, layer 2 two column blocks)
    p-skip-wide   TP128 NW8 BL SK          [256] x 3, skip [2], L = 16: layer 2 reads 256 + 96 = 352 columns.  DMA96;
                                           DMA256 on dz rows of stride 352; staged 256x256 on 256 x 352 (256 + 96)
    p-skip-tp64   TP64 NW4 BL SK           [416, 416], skip [1], L = 16: Kmax = 512 and the skip image: the 8-wave
                                           tile does not fit LDS.  staged 256x128 on 416 x 96 (256 + 160 rows, dz
                                           rows of stride 512); staged 256x256 on 416 x 512 (2 x 2)
    p-1patch      p-tp128's net, B = 1     4 tiles, one patch
    p-3patch      p-tp128's net, B = 3 of 16 x 20: 320 pixels in 384 slots a patch, 9 tiles; S = 1152, 18 chunks
    p-noc2f       p-tp128's net, c2f off   every band open

Against the issue's table: p-mid's layer 1 (M = 160) runs the 128-row staged kernel, not a 256 x 128 one;
the 256 x 128 kernel with a 32-column remainder is its layer 2.  Added: p-L16-nodma (the staged kernels
on DMA-shaped layers).  Reached by no row: BL off on 4 waves (more than 1024 bias floats at <= 256 wide: five
hidden layers, where the rounding-flip rule of plain16_ref.kink_pixels marks over half of 960 pixels) and BL
off at TP64 (a third 416-wide skip-net layer); BL only moves where a forward bias is read from.

REACHES and plan() are two restatements, by hand, of rules read in the library's source.  Only (TP, NW) is
tied to the library itself, through marf_step_saved_bytes; BL, SK and every weight-gradient pick are
UNVERIFIED AGAINST THE LIBRARY -- it gives out no figure that shows them -- and are checked against each
other only: a later change of wg_pick or launch_step_b leaves these tests green while a row stops reaching
the kernel it names.  Whoever changes those rules re-derives this table.

Seeds.  On the statement alone (tests/test_plain16_cpu.py) a row must have every defect move every tensor it
touches by >= 10 x the tensor's accumulation error E_sum and by >= 3 x the bound the GPU test asserts on it,
and at most 6 % of its pixels left out.  It takes the first seed from 3 upwards that does, per type (seeds
tried = seed - 2): CASES below; the two entries of NOT_HELD are the exceptions.  The narrow margins are dW_last and the dgrad's start: dropping g_l and
starting from unrounded g are worth 2^-9 (bf16) / 2^-12 (fp16) of a term, 3 to 4 x the bound at the seeds
taken and less at most others; the nets with L = 16 needed 53 to 85 tries.  E_sum is taken in a summation
order that is the same on every host (plain16_ref._mm), since torch's own float32 matmul blocks by CPU.
"""
import numpy as np
import torch

CANVAS = 512
_D = dict(B=2, ph=24, pw=20, c2f=(0, 0.4), progress=0.2, skip=(), env={})


def _c(hidden, L, bf16=3, fp16=3, **kw):
    return dict(_D, hidden=list(hidden), L=L, seed={"bf16": bf16, "fp16": fp16}, **kw)


CASES = {
    "p-tp128": _c([256, 256], 8, bf16=9, fp16=3),
    "p-L16": _c([256, 256], 16, bf16=55, fp16=80),
    "p-L16-nodma": _c([256, 256], 16, bf16=55, fp16=80, env={"MARF_WGRAD_DMA": "0"}),
    "p-narrow": _c([128, 96, 128], 8, bf16=9, fp16=10),
    "p-mid": _c([256, 160, 256], 8, bf16=5, fp16=6),
    "p-288": _c([288, 288], 8, bf16=7, fp16=5),
    "p-288-nw4": _c([288, 288], 8, bf16=7, fp16=5, env={"MARF_STEP_NW": "4"}),
    "p-wide8": _c([512, 512, 32], 16, bf16=69, fp16=7),
    "p-skip": _c([64, 64, 64], 8, bf16=5, fp16=6, skip=(2,)),
    "p-skip-wide": _c([256, 256, 256], 16, bf16=8, fp16=95, skip=(2,)),
    "p-skip-tp64": _c([416, 416], 16, bf16=4, fp16=87, skip=(1,)),
    "p-1patch": _c([256, 256], 8, bf16=6, fp16=36, B=1),
    "p-3patch": _c([256, 256], 8, bf16=4, fp16=5, B=3, ph=16, pw=20),
    "p-noc2f": _c([256, 256], 8, bf16=8, fp16=5, c2f=None),
}
# (case, type) -> the tensors exempt from the HOST test's separation conditions: no seed of 150 meets them there
# (the three-layer nets in fp16: the weakest defect on these tensors is 2.0, just under 3 and 2.5 x above the
# bound, or under 10 x E_sum).  tests/test_plain16_cpu.py holds this table to the statement, no more and no
# fewer.  The GPU test knows no exemption: the kernel is held to the bound on these tensors as on every other.
NOT_HELD = {("p-wide8", "fp16"): ("dh",), ("p-skip-wide", "fp16"): ("dW2", "dW3")}
ALL = list(CASES)
TYPES = ["bf16", "fp16"]
SWITCHES = ("MARF_STEP_NW", "MARF_WGRAD_DMA")  # what a row's env may set; unset everywhere else
WARP_ONLY = ["p-tp128", "p-wide8", "p-skip"]

# case -> (TP, NW, BL, SK) and per hidden-side layer (kernel, bm, bn, row blocks, column blocks): the table above
REACHES = {
    "p-tp128": ((128, 4, True, False), [("staged", 256, 64, 1, 1), ("dma256", 256, 256, 1, 1)]),
    "p-L16": ((128, 4, True, False), [("dma96", 256, 96, 1, 1), ("dma256", 256, 256, 1, 1)]),
    "p-L16-nodma": ((128, 4, True, False), [("staged", 256, 128, 1, 1), ("staged", 256, 256, 1, 1)]),
    "p-narrow": ((128, 4, True, False), [("staged", 128, 64, 1, 1), ("staged", 128, 64, 1, 2), ("staged", 128, 64, 1, 2)]),
    "p-mid": ((128, 4, True, False), [("staged", 256, 64, 1, 1), ("staged", 128, 64, 2, 4), ("staged", 256, 128, 1, 2)]),
    "p-288": ((128, 8, True, False), [("staged", 256, 64, 2, 1), ("staged", 256, 256, 2, 2)]),
    "p-288-nw4": ((64, 4, True, False), [("staged", 256, 64, 2, 1), ("staged", 256, 256, 2, 2)]),
    "p-wide8": ((128, 8, False, False), [("dma96", 256, 96, 2, 1), ("dma256", 256, 256, 2, 2), ("staged", 128, 64, 1, 8)]),
    "p-skip": ((128, 4, True, True), [("staged", 128, 64, 1, 1), ("staged", 128, 64, 1, 1), ("staged", 128, 64, 1, 2)]),
    "p-skip-wide": ((128, 8, True, True), [("dma96", 256, 96, 1, 1), ("dma256", 256, 256, 1, 1), ("staged", 256, 256, 1, 2)]),
    "p-skip-tp64": ((64, 4, True, True), [("staged", 256, 128, 2, 1), ("staged", 256, 256, 2, 2)]),
}
for _k in ("p-1patch", "p-3patch", "p-noc2f"):
    REACHES[_k] = REACHES["p-tp128"]


def dims(case):
    c = CASES[case]
    return [2 + 4 * c["L"]] + c["hidden"] + [3]


def arch(case):
    c = CASES[case]
    return {"layers": [None] + c["hidden"] + [3], "skip": list(c["skip"]), "posenc": {"L_2D": c["L"]}}


def _rup(x, m):
    return -(-x // m) * m


def plan(case):
    """net_create's, launch_step_b / _t's, wg_pick's and plan_step's rules restated for a 16-bit net (2-byte
    elements): dict(TP, NW, BL, SK, Kp, Mp, picks, step_saved_bytes)."""
    c = CASES[case]
    d = dims(case)
    n = len(d) - 1
    skip = set(c["skip"])
    Kp, Mp = [_rup(d[0], 32)], []
    for l in range(n - 1):
        Mp.append(_rup(d[l + 1], 32))
        Kp.append(Mp[l] + (Kp[0] if l + 1 in skip else 0))
    Kmax = max(Kp)
    TP, NW = (128 if Kmax <= 256 else 64), 4
    lda = Kmax + 8
    lds8 = max(128 * lda * 2, 128 * (Kp[0] + 1) * 4) + (128 * Kp[0] * 4 if skip else 0)
    if c["env"].get("MARF_STEP_NW") != "4" and Kmax > 256 and lds8 + 16 * 1024 <= 160 * 1024:
        TP, NW = 128, 8
    S = c["B"] * _rup(c["ph"] * c["pw"], 128)
    chunk = max(64, _rup(-(-S // 256), 64))
    n_chunks = -(-S // chunk)
    dma_on = c["env"].get("MARF_WGRAD_DMA") != "0"
    picks = []
    for l in range(n - 1):
        M, K, ldz = Mp[l], Kp[l], Kp[l + 1]
        dma = M % 256 == 0 and ldz % 8 == 0 and ldz >= M and S % 32 == 0 and chunk % 32 == 0 and dma_on
        if dma and K % 256 == 0:
            k, bm, bn = "dma256", 256, 256
        elif dma and K == 96:
            k, bm, bn = "dma96", 256, 96
        elif M >= 256 and K >= 192:
            k, bm, bn = "staged", 256, 256
        elif M >= 256 and K > 64:
            k, bm, bn = "staged", 256, 128
        else:
            k, bm, bn = "staged", (256 if M >= 256 else 128), 64
        picks.append((k, bm, bn, -(-M // bm), -(-K // bn)))
    # plan_step (STEP_FULL): every region rounded up to 256 B
    tiles = S // TP
    regions = [S * Kp[l] * 2 for l in range(n - 1)]
    for l in range(1, n):
        regions += [S * Kp[l] * 2, tiles * NW * 1024]
    regions += [tiles * 3 * Kp[n - 1] * 4, tiles * 3 * 4, tiles * 9 * 4, tiles * 2 * 8, 256]
    mxo, mxm = max(Mp[l] * Kp[l] for l in range(n - 1)), max(Mp)
    regions += [max(n_chunks * mxo, 256 * (3 * Kp[n - 1] + 3)) * 4, n_chunks * mxm * 4]
    offs = [0]
    for r in regions:
        offs.append(offs[-1] + _rup(r, 256))
    # byte offsets of the saved tensors: feat_l [S][Kp[l]] (l <= n-2), then dz_l [S][Kp[l]] (the gradient at
    # layer l-1's output; l = 1 .. n-1), each followed by layer l's ReLU records
    return dict(TP=TP, NW=NW, BL=sum(Mp) <= 1024, SK=bool(skip), Kp=Kp, Mp=Mp, picks=picks, S=S,
                feat_off=offs[:n - 1], dz_off={l: offs[n - 1 + 2 * (l - 1)] for l in range(1, n)},
                step_saved_bytes=offs[-1])


def seed_of(case, T):
    s = CASES[case]["seed"]
    return s[T] if isinstance(s, dict) else s


def make_opt_for(case, tmp_path, precision, **over):
    from test_gpu_parity import make_opt
    c = CASES[case]
    return make_opt(tmp_path, H=CANVAS, W=CANVAS, patch_H=c["ph"], patch_W=c["pw"], batch_size=c["B"], precision=precision,
                    use_edges=False, arch=arch(case), barf_c2f=None if c["c2f"] is None else list(c["c2f"]), **over)


_INPUTS, _FEATS = {}, {}


def inputs(case, T):
    """(cfg, params, warp, rgb, mask, progress) of a case in type T ("bf16" / "fp16": a row's seed may differ
    between them), as step2_shapes.inputs makes them: the seeded init of NeuralImageFunction (the first module
    Model builds under the seed), procedural targets, Bernoulli(0.85) masks, non-zero warps.  Built once per
    (case, seed) and shared; the arrays are read-only."""
    seed = seed_of(case, T)
    if (case, seed) in _INPUTS:
        return _INPUTS[case, seed]
    from model import planar
    c = CASES[case]
    B, ph, pw = c["B"], c["ph"], c["pw"]
    torch.manual_seed(seed)
    nif = planar.NeuralImageFunction(make_opt_for(case, None, "bf16"))
    params = [(l.weight.detach().numpy().copy(), l.bias.detach().numpy().copy()) for l in nif.mlp]
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.linspace(0, 1, ph), np.linspace(0, 1, pw), indexing="ij")
    rgb = np.stack([[0.5 + 0.4 * np.sin(2 * np.pi * (rng.uniform(1, 4) * xx + rng.uniform(1, 4) * yy) + rng.uniform(0, 6))
                     for _ in range(3)] for _ in range(B)]).astype(np.float32)
    mask = (rng.random((B, 1, ph, pw)) < 0.85).astype(np.float32)
    warp = (rng.standard_normal((B, 8)) * 0.01).astype(np.float32)
    cfg = dict(H=CANVAS, W=CANVAS, patch_H=ph, patch_W=pw, L=c["L"], c2f=None if c["c2f"] is None else list(c["c2f"]),
               max_iter=3000, lr=1e-3, lr_warp=1e-3, fix_first=True, use_edges=False, alpha_initial=0.0, alpha_final=1.0,
               skip=tuple(c["skip"]))
    _INPUTS[case, seed] = (cfg, params, warp, rgb, mask, c["progress"])
    return _INPUTS[case, seed]


def features(case, T):
    """The prologue's float32 values by the oracle (step2_ref.features), [pixels, 2 + 4L]."""
    key = (case, seed_of(case, T))
    if key not in _FEATS:
        import step2_ref
        cfg, _, warp, _, _, progress = inputs(case, T)
        _FEATS[key] = step2_ref.features(cfg, warp, progress)
    return _FEATS[key]
