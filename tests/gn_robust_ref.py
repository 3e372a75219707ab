"""Reference statement of the robust Gauss-Newton registration (marf_gn_normal_robust, lm.robust; DESIGN.md
§13), for the tests.  Nothing in the product imports it.

With r_qc = m_q (p_qc - g_qc) and J_qc of gn_ref, e_q = sum_c r_qc^2, s_q = sqrt(e_q) and the scale delta:
    huber :  rho(e) = e if e <= delta^2, else 2 delta s - delta^2        w = 1, else delta / s
    cauchy:  rho(e) = delta^2 log1p(e / delta^2)                         w = 1 / (1 + e / delta^2)
    cost_b = sum_q rho(e_q)   msum_b = sum_q m_q   g9_b = sum_q w_q sum_c J_qc^T r_qc   N_b = sum_q w_q sum_c J_qc^T J_qc

normal() / emu_normal(): gn_ref's per-pixel p and d p / d H (float64 autograd, or the bf16x3 tile recipe's
emulation) under these weights; the residual, e, w and rho are evaluated in the render's dtype (so the
float32 evaluation is one), the sums in float64.  lm(): gn_ref.lm with the cost in sse's place.  occluded():
the solver tests' problem -- gn_ref.realisable() with a constant-colour rectangle painted into each target.
"""
import numpy as np
import torch

import cpu_ref
import gn_ref

KINDS = ("huber", "cauchy")
RECT = (16, 20)  # rows x columns of the occluder: 320 of 2,304 pixels, 13.9 %


def weights(e, kind, delta):
    """(rho, w) of e = sum_c r_c^2 (a tensor), in e's dtype."""
    d2 = delta * delta
    if kind == "huber":
        far = e > d2
        s = torch.sqrt(torch.where(far, e, torch.ones_like(e)))  # (no sqrt at 0: autograd goes through here)
        return torch.where(far, 2 * delta * s - d2, e), torch.where(far, delta / s, torch.ones_like(e))
    if kind == "cauchy":
        return d2 * torch.log1p(e / d2), 1 / (1 + e / d2)
    raise ValueError(kind)


def _pixels(fn, *args, **kw):
    """What gn_ref.normal / gn_ref.emu_normal hand to their summation: p [B, Np, 3], dp [3][B, Np, 9], tgt
    [B, Np, 3], m [B, Np, 1] (gn_ref's own per-pixel code, its last line swapped for the call only)."""
    got = {}
    keep = gn_ref._sums
    gn_ref._sums = lambda p, dp, tgt, m: got.update(p=p, dp=dp, tgt=tgt, m=m)
    try:
        fn(*args, **kw)
    finally:
        gn_ref._sums = keep
    return got


def _sums(px, kind, delta):
    f64 = torch.float64
    p, dp, tgt, m = px["p"].detach(), px["dp"], px["tgt"], px["m"]
    r = (p - tgt) * m
    e = (r * r).sum(-1)
    rho, w = weights(e, kind, delta)
    r, w64 = r.to(f64), w.to(f64)
    J = torch.stack([d.to(f64) * m.to(f64) for d in dp], 2)  # [B, Np, 3, 9]
    g9 = (w64[..., None, None] * J * r[..., None]).sum((1, 2))
    N = torch.einsum("bq,bqci,bqcj->bij", w64, J, J)
    n = lambda x: x.to(f64).cpu().numpy()  # noqa: E731
    return dict(cost=n(rho.to(f64).sum(1)), msum=n(m.to(f64).sum((1, 2))), g9=n(g9), N=n(N), rgb=n(p), weight=n(w), e=n(e))


def normal(inputs, kind, delta, dtype=torch.float64, warp=None, device="cpu"):
    """The robust normal equations of `inputs` at its warps (or `warp`): cost, msum, g9, N [B, ...], rgb [B,
    Np, 3], and per pixel the weight and e [B, Np]."""
    return _sums(_pixels(gn_ref.normal, inputs, dtype=dtype, warp=warp, device=device), kind, delta)


def emu_normal(inputs, kind, delta):
    """normal() on the bf16x3 tile recipe's emulation (gn_ref.emu_normal's p and dp, float32)."""
    return _sums(_pixels(gn_ref.emu_normal, inputs), kind, delta)


def pack56(nm):
    return np.concatenate([nm["cost"][:, None], nm["msum"][:, None], nm["g9"], nm["N"][:, gn_ref.TRIU[0], gn_ref.TRIU[1]]], 1)


def cost_gradient(inputs, kind, delta):
    """d cost_b / d vec(H_b) [B, 9] by autograd through the reference's render (float64), one H per patch."""
    cfg, params, warp, rgb, mask, progress = inputs
    f64 = torch.float64
    s = cpu_ref.CpuRefStep(cfg, params, warp, rgb, mask, dtype=f64)
    s.progress.data.fill_(progress)
    B, Np = s.B, s.h * s.w
    Hb = cpu_ref.sl3_to_SL3(torch.as_tensor(np.asarray(warp)).to(f64)).clone().requires_grad_()
    p = s.render(gn_ref._uv_from_H(cfg, Hb[:, None].expand(B, Np, 3, 3), f64))
    r = (p - s.rgb.permute(0, 2, 3, 1).reshape(B, Np, 3)) * s.mask.reshape(B, Np, 1)
    rho, _ = weights((r * r).sum(-1), kind, delta)
    return torch.autograd.grad(rho.sum(), Hb)[0].reshape(B, 9).numpy()


def lm(inputs, h0, iters, kind=None, delta=None, fix_first=True, opts=gn_ref.LM_DEFAULT):
    """gn_ref.lm under the robust cost (kind None: the plain sse): (h [B, 8], the accepted point's per-patch
    cost before every iteration [iters, B], the weights at the final warps [B, Np] or None)."""
    if kind is None:
        fn, key = (lambda h: gn_ref.normal(inputs, warp=h)), "sse"
    else:
        fn, key = (lambda h: normal(inputs, kind, delta, warp=h)), "cost"
    h = np.asarray(h0, np.float64).copy()
    lam = np.full(h.shape[0], opts["lambda0"])
    hist = []
    for _ in range(iters):
        nm = fn(h)
        E = gn_ref.tangent(h)
        A = np.einsum("bki,bkl,blj->bij", E, nm["N"], E)
        rhs = np.einsum("bki,bk->bi", E, nm["g9"])
        d = gn_ref.solve(A, rhs, lam)
        if fix_first:
            d[0] = 0
        better = fn(h + d)[key] < nm[key]
        h = np.where(better[:, None], h + d, h)
        lam = np.where(better, np.maximum(lam / opts["down"], opts["lambda_min"]), np.minimum(lam * opts["up"], opts["lambda_max"]))
        hist.append(nm[key])
    return h, np.array(hist), (None if kind is None else fn(h)["weight"])


def occlude(rgb_bn3, ph=48, pw=48):
    """The render rgb [B, Np, 3] with one RECT rectangle of a constant random colour (default_rng(7), one
    colour per patch) painted into each patch at y0 = 6 + 5 b, x0 = 10 + 4 b: (painted float32 [B, Np, 3],
    inside [B, Np] bool)."""
    img = np.asarray(rgb_bn3, np.float32).reshape(-1, ph, pw, 3).copy()
    B = img.shape[0]
    colour = np.random.default_rng(7).random((B, 3)).astype(np.float32)
    inside = np.zeros((B, ph, pw), bool)
    for b in range(B):
        y0, x0 = 6 + 5 * b, 10 + 4 * b
        img[b, y0:y0 + RECT[0], x0:x0 + RECT[1]] = colour[b]
        inside[b, y0:y0 + RECT[0], x0:x0 + RECT[1]] = True
    return img.reshape(B, ph * pw, 3), inside.reshape(B, ph * pw)


def occluded(seed=3):
    """gn_ref.realisable() with its defaults (3 patches of 48 x 48, [64, 64], L = 2, start h* + 0.01 noise,
    mask all ones), the targets the image's own float64 render at h* with the occluders painted in:
    (inputs, h*, h0, inside [B, Np])."""
    inputs, hstar, h0 = gn_ref.realisable(seed=seed)
    rgb, inside = occlude(gn_ref.normal(inputs, warp=hstar)["rgb"])
    return gn_ref.with_targets(inputs, rgb), hstar, h0, inside
