"""Reference statement of the mosaic of the registered patches (include/marf.h marf_compose),
for the tests.  Nothing in the product imports it.

compose(): torch, float64 by default, the definition line by line with a two-pass disagreement (mean first,
then the weighted squared deviations); dtype=torch.float32 gives torch's own float32 evaluation of the same
statement.  Beside the outputs it returns, per patch and canvas pixel, the distance of (r, c) to the four
validity lines c = -E, c = w - 1 + E, r = -E, r = h - 1 + E, so a test can leave out exactly the pixels whose
membership rounding may decide.  The Lie exponential is oracle/cpu_ref.py's.
"""
import numpy as np
import torch

import cpu_ref

E = 2.0 ** -10


def geometry(H, W, ph, pw, crop):
    """(h, w, y0, x0, norm_h, norm_w) of marf_pixel_grid's integer crop window (or the canvas)."""
    norm_h, norm_w = H / max(H, W), W / max(H, W)
    if not crop:
        return H, W, 0, 0, norm_h, norm_w
    y0, x0 = H // 2 - ph // 2, W // 2 - pw // 2
    return (H // 2 + ph // 2) - y0, (W // 2 + pw // 2) - x0, y0, x0, norm_h, norm_w


def se2_embed(p):
    """se(2) parameters [B, 3] = (tx, ty, theta) in the sl(3) layout of warp.py:101-104."""
    p = np.asarray(p, np.float64)
    z = np.zeros_like(p[:, 0])
    return np.stack([p[:, 0], p[:, 1], -p[:, 2], p[:, 2], z, z, z, z], 1)


def hmat(h):
    """expm(A(h)) in float64: [B, 3, 3]."""
    return cpu_ref.sl3_to_SL3(torch.as_tensor(np.asarray(h, np.float64)))


def hinv(h):
    """The inverse homographies as the product forms them: expm(A(-h)) in float64."""
    return hmat(-np.asarray(h, np.float64))


def _bilinear(plane, r, c):
    """plane [..., h, w] sampled at r, c [H, W] (already clamped to the patch) -> [..., H, W]."""
    h, w = plane.shape[-2:]
    r0 = torch.floor(r).long().clamp(0, h - 1)
    c0 = torch.floor(c).long().clamp(0, w - 1)
    r1, c1 = (r0 + 1).clamp(max=h - 1), (c0 + 1).clamp(max=w - 1)
    fy, fx = r - r0.to(r.dtype), c - c0.to(c.dtype)
    top = plane[..., r0, c0] * (1 - fx) + plane[..., r0, c1] * fx
    bot = plane[..., r1, c0] * (1 - fx) + plane[..., r1, c1] * fx
    return top * (1 - fy) + bot * fy


def patch_coords(H, W, ph, pw, crop, Hinv, dtype=torch.float64):
    """(r, c, X2) [B, H, W] of every canvas pixel in every patch, unclamped."""
    h, w, y0, x0, norm_h, norm_w = geometry(H, W, ph, pw, crop)
    Hi = torch.as_tensor(np.asarray(Hinv)).to(dtype).reshape(-1, 3, 3)
    gx = ((torch.arange(W, dtype=dtype) + 0.5) / W * 2 - 1) * norm_w
    gy = ((torch.arange(H, dtype=dtype) + 0.5) / H * 2 - 1) * norm_h
    Y, X = torch.meshgrid(gy, gx, indexing="ij")
    a = Hi[:, :, 0, None, None] * X + Hi[:, :, 1, None, None] * Y + Hi[:, :, 2, None, None]  # [B, 3, H, W]
    d = a[:, 2] + 1e-8
    c = (a[:, 0] / d / norm_w + 1) * W / 2 - 0.5 - x0
    r = (a[:, 1] / d / norm_h + 1) * H / 2 - 0.5 - y0
    return r, c, a[:, 2]


def compose(H, W, ph, pw, crop, Hinv, img, weight=None, feather=False, dtype=torch.float64):
    """The definition.  Hinv [B, 3, 3], img [B, 3, h, w], weight [B, 1, h, w] or None -> dict(image [3, H, W],
    wsum, count, var [H, W], valid [B, H, W] bool, dist [B, H, W, 4]) as numpy arrays."""
    h, w, y0, x0, norm_h, norm_w = geometry(H, W, ph, pw, crop)
    img = torch.as_tensor(np.asarray(img)).to(dtype).reshape(-1, 3, h, w)
    B = img.shape[0]
    wgt = None if weight is None else torch.as_tensor(np.asarray(weight)).to(dtype).reshape(B, h, w)
    r, c, X2 = patch_coords(H, W, ph, pw, crop, Hinv, dtype)
    valid = (X2 > 0) & (c >= -E) & (c <= w - 1 + E) & (r >= -E) & (r <= h - 1 + E)
    dist = torch.stack([(c + E).abs(), (c - (w - 1 + E)).abs(), (r + E).abs(), (r - (h - 1 + E)).abs()], -1)
    vs, oms = [], []
    for b in range(B):
        cc = torch.nan_to_num(c[b]).clamp(0, w - 1)
        rr = torch.nan_to_num(r[b]).clamp(0, h - 1)
        v = _bilinear(img[b], rr, cc)  # [3, H, W]
        m = torch.ones_like(cc) if wgt is None else _bilinear(wgt[b], rr, cc)
        f = torch.ones_like(cc)
        if feather:
            f = ((1 - (2 * cc / (w - 1) - 1).abs()) * (1 - (2 * rr / (h - 1) - 1).abs())).clamp(min=E)
        vs.append(v)
        oms.append(torch.where(valid[b], f * m, torch.zeros_like(m)))
    v, om = torch.stack(vs), torch.stack(oms)  # [B, 3, H, W], [B, H, W]
    count = (valid & (om > 0)).sum(0)
    wsum = om.sum(0)
    safe = torch.where(wsum > 0, wsum, torch.ones_like(wsum))
    image = (om[:, None] * v).sum(0) / safe * (wsum > 0)
    var = (om[:, None] * (v - image[None]) ** 2).sum((0, 1)) / (3 * safe)
    var = torch.where(count >= 2, var, torch.zeros_like(var))
    return dict(image=image.numpy(), wsum=wsum.numpy(), count=count.numpy().astype(np.float64), var=var.numpy(),
                valid=valid.numpy(), dist=dist.numpy())


def scores(res):
    """coverage, overlap, seam_rmse of a compose() result (Model.evaluate's three)."""
    over = res["count"] >= 2
    return dict(coverage=float((res["wsum"] > 0).mean()), overlap=float(over.mean()),
                seam_rmse=float(np.sqrt(res["var"][over].mean())) if over.any() else float("nan"))


# ---- the smooth analytic image of the tests: 0.5 + sum_k a_k sin(2 pi (p_k s + q_k t) + phase_kc) with (s, t)
# in [0, 1]^2 the position on the canvas; at most 2 periods across it
TERMS = ((1.0, 0.0, 0.15), (0.0, 1.0, 0.10), (2.0, 1.0, 0.05))  # (p, q, amplitude)
PHASES = ((0.3, 1.1, 2.0), (1.7, 0.2, 0.9), (2.9, 2.3, 0.5))    # per term, per channel


def smooth_image(u, v, H, W):
    """The image at normalised canvas coordinates (u, v) (arrays of one shape) -> [3, ...] float64."""
    norm_h, norm_w = H / max(H, W), W / max(H, W)
    s, t = (np.asarray(u, np.float64) / norm_w + 1) / 2, (np.asarray(v, np.float64) / norm_h + 1) / 2
    out = np.full((3,) + s.shape, 0.5)
    for (p, q, a), ph in zip(TERMS, PHASES):
        for ch in range(3):
            out[ch] += a * np.sin(2 * np.pi * (p * s + q * t) + ph[ch])
    return out


def smooth_slope(H, W):
    """An upper bound of |grad I| per canvas pixel."""
    return sum(a * 2 * np.pi * np.hypot(p / W, q / H) for p, q, a in TERMS)


def smooth_curvature(H, W):
    """An upper bound of the Hessian's operator norm per canvas pixel squared (each term's Hessian is rank
    one with eigenvalue a (2 pi)^2 ((p / W)^2 + (q / H)^2))."""
    return sum(a * (2 * np.pi) ** 2 * ((p / W) ** 2 + (q / H) ** 2) for p, q, a in TERMS)


def sample_patches(H, W, ph, pw, crop, h):
    """The B patches of the smooth image at the warps h [B, 8] (float64): img [B, 3, h, w]."""
    hh, ww, _, _, _, _ = geometry(H, W, ph, pw, crop)
    xy = cpu_ref.pixel_grid(H, W, ph, pw, crop=crop, dtype=torch.float64)
    uv = cpu_ref.warp_grid(xy[None].expand(len(h), -1, -1), torch.as_tensor(np.asarray(h, np.float64))).numpy()
    return smooth_image(uv[..., 0], uv[..., 1], H, W).transpose(1, 0, 2).reshape(len(h), 3, hh, ww)


def case(H, W, ph, pw, B, noise, seed=0, crop=True, special=None, misreg=0.0):
    """One GPU test case: warps h [B, 8] (h_0 = 0, the rest noise * N(0, 1)), patches of the smooth image
    (float32), weights random in [0, 1] with a zero rectangle.  special: "off" = the last patch translated
    wholly off the canvas, "zero" = the last patch's weight map all zero, "se2" = se(2) warps embedded.

    misreg: the patches b >= 1 are sampled at h_b + misreg * N(0, 1), not at h_b -- a registration error, so
    that overlapping patches disagree by a few percent of the value range.  Patches sampled at the very warps
    they are composed with agree to ~3e-4 (var ~1e-7), and an fp32 sampler's own rounding of a value (~1e-7)
    is then 1e-4 of var's max: torch's float32 evaluation of the statement misses 1e-5 on such input.
    The zero rectangle is in the patches b >= 1 only: under patch 0's identity warp a canvas pixel lands on a
    patch pixel centre to rounding, where the bilinear weight next to a zero region is 0 or 1e-7 -- and count
    flips -- by the last bit of c; float32 torch and float64 disagree there."""
    rng = np.random.default_rng(seed)
    hh, ww, _, _, _, _ = geometry(H, W, ph, pw, crop)
    p = None
    if special == "se2":
        p = (noise * rng.standard_normal((B, 3))).astype(np.float32)
        p[0] = 0
        h = se2_embed(p)
    else:
        h = noise * rng.standard_normal((B, 8))
        h[0] = 0
    if special == "off":
        h[-1] = 0
        h[-1, 0] = 3.0  # three canvas widths to the side
    h = h.astype(np.float32)
    hs = h.astype(np.float64)
    if misreg:
        if special == "se2":
            d = se2_embed(misreg * rng.standard_normal((B, 3)))
        else:
            d = misreg * rng.standard_normal((B, 8))
        d[0] = 0
        hs = hs + d
    img = sample_patches(H, W, ph, pw, crop, hs).astype(np.float32)
    weight = rng.random((B, 1, hh, ww)).astype(np.float32)
    weight[1:, :, hh // 4:hh // 2, ww // 3:2 * ww // 3] = 0
    if special == "zero":
        weight[-1] = 0
    return dict(H=H, W=W, ph=ph, pw=pw, crop=crop, B=B, h=h, p=p, img=img, weight=weight)
