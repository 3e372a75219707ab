"""Reference statement of the Gauss-Newton registration on a frozen image, for the
tests.  Nothing in the product imports it.

Per patch b and pixel q, with p the sigmoid output, g the target and m the mask:
    r_qc = m_q (p_qc - g_qc)        J_qc = m_q d p_qc / d vec(H_b)   (vec row-major)
    sse_b = sum r^2   msum_b = sum m   g9_b = sum_qc J_qc^T r_qc   N_b = sum_qc J_qc^T J_qc

normal(): torch (float64 by default) with the ops of oracle/cpu_ref.py as they are (pixel_grid,
sl3_to_SL3, positional_encoding, CpuRefStep.render) and H expanded to a per-pixel leaf [B][Np][3][3];
three backward passes, one per channel, give d p_qc / d H_q per pixel by autograd alone -- no analytic
warp derivative appears here.  emu_normal(): the same quantities in the bf16x3 tile recipe's operand
rounding (bf16x3_tile_ref.split / mm3: three-term forward and dgrad, float32 prologue), accumulated in
float64.  lm(): the Levenberg-Marquardt loop of Graph.lm_step restated in float64 on normal().
"""
import numpy as np
import torch

import bf16x3_tile_ref as R
import cpu_ref

SHAPES = dict(R.SHAPES)
SHAPES["small"] = ([64, 64], 8, 50, 54)  # a k_step2-shaped net (<= 5 layers x 256)
TRIU = np.triu_indices(9)


def synthetic_inputs(case, **kw):
    """bf16x3_tile_ref.synthetic_inputs, the new case built the same way (its table holds the case for
    the call only: other tests parametrise over it)."""
    if case in R.SHAPES:
        return R.synthetic_inputs(case, **kw)
    R.SHAPES[case] = SHAPES[case]
    try:
        return R.synthetic_inputs(case, **kw)
    finally:
        del R.SHAPES[case]


def _T(a, dtype, dev="cpu"):
    return torch.as_tensor(np.asarray(a, np.float32)).to(device=dev, dtype=dtype)


def _uv_from_H(cfg, Hq, dtype):
    """The reference's point warp (cpu_ref.warp_grid's two lines) with a homography per pixel."""
    xy = cpu_ref.pixel_grid(cfg["H"], cfg["W"], cfg["patch_H"], cfg["patch_W"], crop=True, dtype=dtype).to(Hq.device)
    hom = torch.cat([xy, torch.ones_like(xy[..., :1])], -1)
    Xw = (Hq @ hom[None, :, :, None])[..., 0]
    return Xw[..., :2] / (Xw[..., 2:] + 1e-8)


def _sums(p, dp, tgt, m):
    """sse, msum, g9, N from p [B, Np, 3], dp [3][B, Np, 9], tgt [B, Np, 3], m [B, Np, 1] (float64 sums)."""
    f64 = torch.float64
    r = ((p - tgt) * m).to(f64)
    J = torch.stack([d.to(f64) * m.to(f64) for d in dp], 2)  # [B, Np, 3, 9]
    sse = (r * r).sum((1, 2))
    msum = m.to(f64).sum((1, 2))
    g9 = (J * r[..., None]).sum((1, 2))
    N = torch.einsum("bqci,bqcj->bij", J, J)
    return dict(sse=sse.cpu().numpy(), msum=msum.cpu().numpy(), g9=g9.cpu().numpy(), N=N.cpu().numpy(),
                rgb=p.detach().to(f64).cpu().numpy())


def normal(inputs, dtype=torch.float64, warp=None, device="cpu"):
    """The normal equations of `inputs` at its warps (or `warp`), reference ops in `dtype`."""
    cfg, params, warp0, rgb, mask, progress = inputs
    warp = warp0 if warp is None else warp
    s = cpu_ref.CpuRefStep(cfg, params, warp0, rgb, mask, dtype=dtype, device=device)
    s.progress.data.fill_(progress)
    B, Np = s.B, s.h * s.w
    h = torch.as_tensor(np.asarray(warp)).to(device=device, dtype=dtype)
    Hq = cpu_ref.sl3_to_SL3(h)[:, None].expand(B, Np, 3, 3).clone().requires_grad_()
    p = s.render(_uv_from_H(cfg, Hq, dtype))
    dp = [torch.autograd.grad(p[..., c].sum(), Hq, retain_graph=c < 2)[0].reshape(B, Np, 9) for c in range(3)]
    tgt = s.rgb.permute(0, 2, 3, 1).reshape(B, Np, 3)
    return _sums(p.detach(), dp, tgt, s.mask.reshape(B, Np, 1))


def emu_normal(inputs, acc=torch.float64, device="cpu"):
    """normal() in the bf16x3 tile recipe (bf16x3_tile_ref.step's forward and dgrad, one dgrad pass per
    channel started at sigma'_c alone, the layer-0 adjoint by autograd through the float32 prologue)."""
    cfg, params, warp, rgb, mask, progress = inputs
    f32 = torch.float32
    L, n = cfg["L"], len(params)
    B, _, h, w = rgb.shape
    Np = h * w
    Hq = cpu_ref.sl3_to_SL3(_T(warp, f32, device))[:, None].expand(B, Np, 3, 3).clone().requires_grad_()
    uv = _uv_from_H(cfg, Hq, f32)
    x = uv
    if L > 0:
        x = torch.cat([uv, cpu_ref.positional_encoding(uv, L, torch.tensor(progress, dtype=f32, device=device), cfg["c2f"])], -1)
    x = x.reshape(B * Np, -1)
    Ws = [R.split(_T(W, f32, device)) for W, _ in params]
    bs = [_T(b, f32, device) for _, b in params]
    a = R.split(x.detach())
    zs = []
    for l in range(n):
        z = (R.mm3(a, (Ws[l][0].t(), Ws[l][1].t()), acc) + bs[l].to(acc)).to(f32)
        zs.append(z)
        if l < n - 1:
            a = R.split(torch.relu(z))
    y = torch.sigmoid(zs[-1])
    dp = []
    for c in range(3):
        g = torch.zeros_like(y)
        g[:, c] = (1.0 - y[:, c]) * y[:, c]
        dz = R.split(g)
        for l in range(n - 1, -1, -1):
            da = R.mm3(dz, Ws[l], acc).to(f32)
            if l > 0:
                dz = R.split(da * (zs[l - 1] > 0))
        dp.append(torch.autograd.grad(x, Hq, da, retain_graph=c < 2)[0].reshape(B, Np, 9))
    tgt = _T(rgb, f32, device).permute(0, 2, 3, 1).reshape(B, Np, 3)
    return _sums(y.reshape(B, Np, 3), dp, tgt, _T(mask, f32, device).reshape(B, Np, 1))


def pack56(nm):
    """[B, 56] as marf_gn_normal writes it: sse, msum, g9, N's upper triangle row-major."""
    return np.concatenate([nm["sse"][:, None], nm["msum"][:, None], nm["g9"], nm["N"][:, TRIU[0], TRIU[1]]], 1)


def tangent(h, se2_p=None):
    """E_b = d vec(H_b) / d h_b [B, 9, 8] in float64 by autograd (se2_p: [B, 3] se(2) parameters p with
    h = embed(p): E [B, 9, 3])."""
    def f(v):
        if se2_p is not None:  # [[0, -theta, tx], [theta, 0, ty], [0, 0, 0]] in warp.py:101-104's layout
            z = torch.zeros_like(v[0])
            v = torch.stack([v[0], v[1], -v[2], v[2], z, z, z, z])
        return cpu_ref.sl3_to_SL3(v).reshape(9)
    src = h if se2_p is None else se2_p
    return torch.stack([torch.autograd.functional.jacobian(f, torch.as_tensor(np.asarray(v), dtype=torch.float64))
                        for v in src]).numpy()


def solve(A, rhs, lam, eps=1e-12):
    """delta_b = -(A_b + lam_b diag(A_b) + eps I)^-1 rhs_b; a patch that cannot be solved gets 0."""
    out = np.zeros_like(rhs)
    for b in range(A.shape[0]):
        M = A[b] + lam[b] * np.diag(np.diag(A[b])) + eps * np.eye(A.shape[1])
        try:
            d = -np.linalg.solve(M, rhs[b])
        except np.linalg.LinAlgError:
            continue
        if np.all(np.isfinite(d)):
            out[b] = d
    return out


LM_DEFAULT = dict(lambda0=1e-3, up=10.0, down=10.0, lambda_min=1e-9, lambda_max=1e9)


def lm(inputs, h0, iters, fix_first=True, opts=LM_DEFAULT):
    """The LM loop of Graph.lm_step in float64: returns (h [B, 8], the accepted point's per-patch sse
    before every iteration [iters, B]).  The warps are kept in float64 (the product stores float32)."""
    h = np.asarray(h0, np.float64).copy()
    B = h.shape[0]
    lam = np.full(B, opts["lambda0"])
    hist = []
    for _ in range(iters):
        nm = normal(inputs, warp=h)
        E = tangent(h)
        A = np.einsum("bki,bkl,blj->bij", E, nm["N"], E)
        rhs = np.einsum("bki,bk->bi", E, nm["g9"])
        d = solve(A, rhs, lam)
        if fix_first:
            d[0] = 0
        trial = normal(inputs, warp=h + d)["sse"]
        better = trial < nm["sse"]
        h = np.where(better[:, None], h + d, h)
        lam = np.where(better, np.maximum(lam / opts["down"], opts["lambda_min"]), np.minimum(lam * opts["up"], opts["lambda_max"]))
        hist.append(nm["sse"])
    return h, np.array(hist)


def realisable(seed=3, dtype="fp32", B=3, hidden=(64, 64), L=2, H=64, W=64, ph=48, pw=48, noise=0.01):
    """The solver tests' problem: a frozen random image ([64, 64], L = 2, c2f off) whose targets are its
    own render at known warps h* (so the residual at the solution is zero), the start h* + 0.01 noise
    (seeded), patch 0 at the identity in both (fix_first).  Returns (inputs without targets, h*, h0):
    the caller renders the targets (marf_render on the GPU, normal()'s rgb on the CPU)."""
    from model import planar
    from test_gpu_parity import make_opt
    opt = make_opt(None, H=H, W=W, patch_H=ph, patch_W=pw, batch_size=B, precision=dtype, use_edges=False,
                   arch={"layers": [None] + list(hidden) + [3], "skip": [], "posenc": {"L_2D": L}}, barf_c2f=None)
    torch.manual_seed(seed)
    nif = planar.NeuralImageFunction(opt)
    params = [(l.weight.detach().numpy().copy(), l.bias.detach().numpy().copy()) for l in nif.mlp]
    rng = np.random.default_rng(seed)
    hstar = (rng.standard_normal((B, 8)) * 0.02).astype(np.float32)
    h0 = (hstar + noise * rng.standard_normal((B, 8))).astype(np.float32)
    hstar[0] = 0
    h0[0] = 0
    mask = np.ones((B, 1, ph, pw), np.float32)
    cfg = dict(H=H, W=W, patch_H=ph, patch_W=pw, L=L, c2f=None, max_iter=3000, lr=1e-3, lr_warp=1e-3,
               fix_first=True, use_edges=False, alpha_initial=0.0, alpha_final=1.0, skip=())
    rgb0 = np.zeros((B, 3, ph, pw), np.float32)
    return (cfg, params, hstar, rgb0, mask, 0.0), hstar, h0


def with_targets(inputs, rgb_bn3):
    """`inputs` with the targets rgb [B, Np, 3] (a render) in the [B, 3, h, w] layout."""
    cfg, params, warp, rgb, mask, progress = inputs
    B, _, h, w = rgb.shape
    tg = np.asarray(rgb_bn3, np.float32).reshape(B, h, w, 3).transpose(0, 3, 1, 2).copy()
    return cfg, params, warp, tg, mask, progress
