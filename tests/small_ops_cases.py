"""Inputs and plain-torch references for the small kernels around the fused step: the Lie
exponential (csrc/marf_lie.hip), the point warp, Adam and the masked MSE (csrc/marf_misc.hip,
k_mse_mask_bwd in csrc/marf_mask.hip).

Nothing here touches the GPU or the library (cpu_ref is the torch-CPU restatement of the reference's
ops).  The Lie case builders classify every input by the branch torch.linalg.matrix_exp must take
for it, from the six published float32 thresholds and float32 arithmetic alone, and assert that every branch and every squaring count is populated, so the
tests that consume them (tests/test_small_ops_cpu.py, tests/test_gpu_lie_branches.py) cannot quietly
lose a branch.  Expected values are never stored: the tests compute them from torch on the CPU.

torch's algorithm (aten/src/ATen/native/LinearAlgebra.cpp, mexp_impl), restated:
  * a batch of one picks the Taylor degree by the matrix 1-norm: norm <= theta[0] -> T1, <= theta[1] ->
    T2, <= theta[2] -> T4, <= theta[3] -> T8, < theta[4] -> T12, >= theta[4] -> T18 with
    s = max(0, ceil(log2(norm / theta[5]))) scalings and squarings; a NaN norm gives an all-NaN result;
  * a larger batch always takes T18 with the same s;
  * the backward is the same function of the 2n x 2n block matrix [[A^T, G], [0, A^T]].
"""
from types import SimpleNamespace

import numpy as np
import torch

import cpu_ref

F = np.float32

# thresholds_float of mexp_impl (degrees 1, 2, 4, 8, 12, 18), as float32
THETA = np.array([1.192092800768788e-07, 5.978858893805233e-04, 5.116619363445086e-02,
                  5.800524627688768e-01, 1.461661507209034e+00, 3.010066362817634e+00], F)

# the seven batch-of-one paths ("T18s" = T18 with at least one scaling and squaring)
PATHS = ("T1", "T2", "T4", "T8", "T12", "T18", "T18s")

WARP_N = (1, 44, 45, 63, 65, 1023, 1024, 1025, 4100)


# ---------------------------------------------------------------------------- float32 helpers

def ulp_step(x, k):
    """The float32 k representable values above (k > 0) or below (k < 0) x."""
    x = F(x)
    for _ in range(abs(k)):
        x = np.nextafter(x, F(np.inf) if k > 0 else F(-np.inf), dtype=F)
    return x


def generator_np(h):
    """h [8] float32 -> the generator [[h5,h3,h1],[h4,-h5-h6,h2],[h7,h8,h6]] (1-based), float32; the
    middle entry is the float32 sum (-h5) + (-h6), as torch evaluates -h5-h6."""
    h = np.asarray(h, F)
    return np.array([[h[4], h[2], h[0]], [h[3], F(-h[4]) + F(-h[5]), h[1]], [h[6], h[7], h[5]]], F)


def block_matrix_np(h, dH):
    """The 6x6 matrix whose exponential is the backward: [[A^T, G], [0, A^T]]."""
    At = generator_np(h).T
    M = np.zeros((6, 6), F)
    M[:3, :3] = At
    M[3:, 3:] = At
    M[:3, 3:] = np.asarray(dH, F).reshape(3, 3)
    return M


def one_norm_f32(M):
    """max over columns of the float32 sum of |entries|, rows added in order from 0."""
    M = np.asarray(M, F)
    best = None
    for j in range(M.shape[1]):
        s = F(0)
        for i in range(M.shape[0]):
            s = F(s + np.abs(M[i, j]))
        if np.isnan(s):
            return F(np.nan)
        best = s if best is None or s > best else best
    return best


def squarings(norm):
    """s = max(0, ceil(log2(norm / theta[5]))) with the quotient in float32 and a correctly rounded
    float32 log2 (float64 log2 rounded once)."""
    q = F(F(norm) / THETA[5])
    if not q > 0:
        return 0
    l = np.ceil(F(np.log2(np.float64(q))))
    return int(l) if l > 0 else 0


def classify(norm):
    """(path of a batch of one, squaring count of T18 at this norm -- which a batch >= 2 uses)."""
    norm = F(norm)
    if np.isnan(norm):
        return "nan", 0
    s = squarings(norm)
    if norm >= THETA[4]:
        return ("T18s" if s > 0 else "T18"), s
    for i, name in enumerate(("T1", "T2", "T4", "T8")):
        if norm <= THETA[i]:
            return name, s
    return "T12", s


# interiors of the norm intervals the dense rows aim at: (path, low, high)
_BANDS = (("T1", 1e-10, 1.0e-7), ("T2", 2e-7, 5e-4), ("T4", 7e-4, 4.5e-2), ("T8", 6e-2, 0.5), ("T12", 0.65, 1.4),
          ("T18", 1.5, 2.9), ("T18s", 3.2, 5.8), ("T18s", 6.3, 11.5), ("T18s", 12.5, 23.0), ("T18s", 25.0, 46.0))


def _boundary_norms():
    """(tag, norm): each theta with its float32 neighbours, and theta[5] * 2^k with three on each side."""
    out = []
    for i in range(6):
        for d in (-1, 0, 1):
            out.append((f"theta{i}{d:+d}", ulp_step(THETA[i], d)))
    for k in range(5):
        for d in range(-3, 4):
            out.append((f"theta5*2^{k}{d:+d}", ulp_step(F(np.ldexp(THETA[5], k)), d)))
    return out


def _coverage(paths, ss, min_s, what):
    for p in PATHS:
        n = sum(1 for q in paths if q == p)
        assert n >= 8, f"{what}: path {p} has {n} cases (< 8)"
    t18 = [s for p, s in zip(paths, ss) if p in ("T18", "T18s")]
    for s in min_s:
        n = sum(1 for q in t18 if q == s)
        assert n >= 4, f"{what}: squaring count {s} has {n} batch-of-one cases (< 4)"


def lie_forward_cases():
    """h [N, 8] float32 with, per row, the float32 1-norm of its generator, the batch-of-one path, the
    T18 squaring count at that norm and a tag.  Dense rows (random h rescaled into every path's
    interval), exact-boundary rows (only h3 = a, h4 = b non-zero: the norm is max(|a|, |b|) exactly
    and A^2 = diag(ab, ab, 0) != 0, so a wrong degree or squaring count changes the result), h = 0 and
    one row with a NaN."""
    rng = np.random.default_rng(20240611)
    hs, tags, want = [], [], {}
    for name, lo, hi in _BANDS:
        for target in np.geomspace(lo, hi, 8):
            h = rng.standard_normal(8).astype(F)
            h = (h * F(target / one_norm_f32(generator_np(h)))).astype(F)
            hs.append(h)
            tags.append(f"dense {name} {target:.3g}")
    for i, (tag, nv) in enumerate(_boundary_norms()):
        small = F(nv * F(0.5 + 0.25 * (i % 2)))
        big = nv if i % 4 < 2 else F(-nv)
        h = np.zeros(8, F)
        h[2], h[3] = (big, small) if i % 3 else (small, big)
        want[len(hs)] = nv
        hs.append(h)
        tags.append("edge " + tag)
    hs.append(np.zeros(8, F))
    tags.append("zero")
    h = rng.standard_normal(8).astype(F) * F(0.1)
    h[3] = np.nan
    hs.append(h)
    tags.append("nan")
    h = np.stack(hs)
    norm = np.array([one_norm_f32(generator_np(r)) for r in h], F)
    cl = [classify(v) for v in norm]
    c = SimpleNamespace(h=h, norm=norm, path=[p for p, _ in cl], s=np.array([s for _, s in cl]), tag=tags)
    for i, nv in want.items():
        assert norm[i] == nv, (tags[i], norm[i], nv)   # the boundary rows sit exactly where they claim
    _coverage(c.path, c.s, range(5), "lie_forward_cases")
    assert c.path.count("nan") == 1
    return c


H_SCALES = (0.0, 1e-3, 0.1, 0.5, 1.5)
DH_SCALES = (0.0, 1e-9, 1e-6, 1e-4, 1e-2, 1.0, 30.0)


def lie_backward_cases():
    """(h [N, 8], dH [N, 3, 3]) float32 with the float32 1-norm of the 6x6 block matrix, its path and
    squaring count.  Every |h| scale x every |dH| scale (entries uniform in [-scale, scale]; the
    training regime is a small dH), three draws each, and h = 0 with a two-entry dH that puts the
    norm on every theta, on theta[5] * 2^k (k <= 3) and on their float32 neighbours."""
    rng = np.random.default_rng(20240612)
    hs, gs, tags = [], [], []
    for sh in H_SCALES:
        for sg in DH_SCALES:
            for r in range(3):
                hs.append((rng.uniform(-1, 1, 8) * sh).astype(F))
                gs.append((rng.uniform(-1, 1, (3, 3)) * sg).astype(F))
                tags.append(f"h {sh:g} dH {sg:g} #{r}")
    for i, (tag, nv) in enumerate(_boundary_norms()):
        if tag.startswith("theta5*2^4"):
            continue
        G = np.zeros((3, 3), F)
        G[i % 3, (i + 1) % 3] = nv if i % 2 else F(-nv)      # two columns: the norm is the larger entry
        G[(i + 1) % 3, (i + 2) % 3] = F(nv * F(0.5))
        hs.append(np.zeros(8, F))
        gs.append(G)
        tags.append("edge " + tag)
    h, dH = np.stack(hs), np.stack(gs)
    norm = np.array([one_norm_f32(block_matrix_np(a, b)) for a, b in zip(h, dH)], F)
    cl = [classify(v) for v in norm]
    c = SimpleNamespace(h=h, dH=dH, norm=norm, path=[p for p, _ in cl], s=np.array([s for _, s in cl]), tag=tags)
    edge = [b for t_, b in _boundary_norms() if not t_.startswith("theta5*2^4")]
    assert np.array_equal(norm[len(norm) - len(edge):], np.array(edge, F))
    _coverage(c.path, c.s, range(4), "lie_backward_cases")
    return c


def one_row_per_path(c):
    """Indices of a subset with at least one row of every path (first and last of each), the NaN row
    included where there is one."""
    idx = []
    for p in PATHS + ("nan",):
        rows = [i for i, q in enumerate(c.path) if q == p]
        idx += rows[:1] + rows[-1:]
    return sorted(set(idx))


# ---------------------------------------------------------------------------- torch references

def torch_sl3(h, dtype=torch.float32):
    """matrix_exp of the generators of h [B, 8] (numpy) as ONE batch of B on the CPU -> numpy."""
    return cpu_ref.sl3_to_SL3(torch.from_numpy(np.asarray(h)).to(dtype)).numpy()


def torch_sl3_rows(h, dtype=torch.float32):
    """Every row as a batch of one (torch's degree-selecting path)."""
    return np.stack([torch_sl3(r[None], dtype)[0] for r in np.asarray(h)])


def torch_sl3_backward(h, dH, dtype=torch.float32):
    """d h of sum(matrix_exp(A(h)) * dH), the batch taken whole."""
    x = torch.from_numpy(np.asarray(h)).to(dtype).requires_grad_()
    cpu_ref.sl3_to_SL3(x).backward(torch.from_numpy(np.asarray(dH)).to(dtype))
    return x.grad.numpy()


def torch_sl3_backward_rows(h, dH, dtype=torch.float32):
    return np.stack([torch_sl3_backward(a[None], b[None], dtype)[0] for a, b in zip(np.asarray(h), np.asarray(dH))])


def warp_expr(xy, Hm):
    """The reference's Warp.warp_grid after the exponential: to_hom, @ H^T, perspective divide."""
    hom = torch.cat([xy, torch.ones_like(xy[..., :1])], dim=-1)
    X = hom @ Hm.transpose(-2, -1)
    return X[..., :2] / (X[..., 2:] + 1e-8)


def hom_product(xy, Hm, fma):
    """X = H [x, y, 1]^T in float32 torch with the sum written out, in the two roundings torch's CPU
    matmul [B, n, 3] @ [B, 3, 3]^T is seen to use: fma False = (x H0 + y H1) + H2 with every product and
    sum rounded (torch's own small-matrix kernel); fma True = fma(y, H1, x H0) + H2 (a BLAS kernel that
    fuses; the fused step is taken in float64, where the product is exact, and rounded once)."""
    x, y = xy[..., 0:1], xy[..., 1:2]
    H0, H1, H2 = (Hm[:, None, :, k] for k in range(3))
    acc = x * H0
    acc = (acc.double() + y.double() * H1.double()).float() if fma else acc + y * H1
    return acc + H2


def warp_expr_pinned(xy, Hm):
    """warp_expr with the rounding of the matmul pinned to what tests/golden holds (generated from the
    reference): torch's small-matrix kernel below 400 multiply-adds per patch (9 n < 400), a fusing BLAS
    kernel from there on.  torch's BLAS kernel depends on the host: an AVX-512 EPYC 9575F was seen to
    use the unfused sum at every n, where the host that generated tests/golden fuses; below the switch
    torch's result is the same everywhere.  The kernels and the oracle reproduce the pinned recipe."""
    X = hom_product(xy, Hm, fma=9 * xy.shape[-2] >= 400)
    return X[..., :2] / (X[..., 2:] + 1e-8)


def torch_matmul_roundings(xy, Hm):
    """Which of hom_product's roundings the installed torch's matmul shows on this input on this host
    (both, for an input on which they coincide; none would be a third recipe, which the tests refuse)."""
    hom = torch.cat([xy, torch.ones_like(xy[..., :1])], dim=-1)
    X = hom @ Hm.transpose(-2, -1)
    return {fma for fma in (False, True) if torch.equal(X, hom_product(xy, Hm, fma))}


def warp_reference(xy, Hm):
    """The expected warped points (numpy in, numpy out): warp_expr_pinned, after checking it against the
    installed torch -- torch's matmul must show one of the two known roundings, the unfused one below
    the switch, and wherever it shows the pinned one, the reference's plain expression (warp_expr, with
    torch's own matmul) must give the very same bits."""
    xy, Hm = torch.from_numpy(xy), torch.from_numpy(Hm)
    pinned = 9 * xy.shape[-2] >= 400
    kinds = torch_matmul_roundings(xy, Hm)
    assert kinds, "torch's CPU matmul rounds in neither known way on this host"
    assert pinned or False in kinds, "torch's small-matrix kernel no longer rounds every product and sum"
    want = warp_expr_pinned(xy, Hm)
    if pinned in kinds:
        assert torch.equal(warp_expr(xy, Hm), want)
    return want.numpy()


def warp_case(B, n):
    """Points uniform in [-1, 1], H = identity + N(0, 0.05), an upstream gradient; float32 numpy."""
    rng = np.random.default_rng(1000 * B + n)
    xy = rng.uniform(-1, 1, (B, n, 2)).astype(F)
    Hm = (np.eye(3) + rng.standard_normal((B, 3, 3)) * 0.05).astype(F)
    G = rng.standard_normal((B, n, 2)).astype(F)
    return xy, Hm, G


def warp_backward_ref(xy, Hm, G, dtype):
    """(d xy, d H) by torch CPU autograd of warp_expr in dtype."""
    x = torch.from_numpy(xy).to(dtype).requires_grad_()
    Hh = torch.from_numpy(Hm).to(dtype).requires_grad_()
    warp_expr(x, Hh).backward(torch.from_numpy(G).to(dtype))
    return x.grad.numpy(), Hh.grad.numpy()


def adam_ref(p, g, m, v, lr, b1, b2, eps, step, dtype):
    """torch.optim.Adam's single-tensor update (torch/optim/adam.py, _single_tensor_adam: no weight
    decay, no amsgrad, bias corrections in python float64) on numpy inputs in dtype -> (p, m, v)."""
    p, g, m, v = (torch.from_numpy(np.array(a)).to(dtype) for a in (p, g, m, v))
    m.lerp_(g, 1 - b1)
    v.mul_(b2).addcmul_(g, g, value=1 - b2)
    bc1 = 1 - b1 ** step
    bc2 = 1 - b2 ** step
    denom = (v.sqrt() / (bc2 ** 0.5)).add_(eps)
    p.addcdiv_(m, denom, value=-(lr / bc1))
    return p.numpy(), m.numpy(), v.numpy()


def mse_ref(pred, gt, mask, gout, denom=None):
    """The two branches of the reference's mse_loss in float64 with autograd.  pred [B, Np, 3] (the
    MLP's layout), gt [B, 3, Np], mask [B, 1, Np] or None (numpy); denom replaces 3 * sum(mask) as a
    constant.  Returns (loss, d (gout * loss) / d pred [B, Np, 3], d / d mask or None)."""
    p = torch.from_numpy(pred).double().requires_grad_()
    labels = torch.from_numpy(gt).double()
    x = p.permute(0, 2, 1)
    mk = None
    if mask is None:
        loss = ((x.contiguous() - labels) ** 2).mean()
    else:
        mk = torch.from_numpy(mask).double().requires_grad_()
        masked = ((x.contiguous() - labels) * mk) ** 2
        loss = masked.sum() / ((mk.sum() * 3) if denom is None else float(denom))
    (loss * gout).backward()
    return float(loss.detach()), p.grad.numpy(), None if mk is None else mk.grad.numpy()


def abs_err(a, ref):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(ref, np.float64)).max())


def ulp_of_max(ref):
    """One float32 ulp at the largest magnitude of ref."""
    return float(np.spacing(F(np.abs(ref).max())))
