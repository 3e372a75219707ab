"""Torch restatement of the learned implicit mask (reference model/planar.py:340-391, 475-518), in
float32 or float64, for the implicit-mask tests.  Plain tensor ops on any device; nothing here is
used by the product.

    crop_grid        the unwarped pixel grid the mask net sees (warp.py:33-68)
    uv_features      [x, y, sin(f_0 x), sin(f_0 y), cos(f_0 x), cos(f_0 y), sin(f_1 x), ...], f_k = 2^k
    mask_input       [E[r] ; E[g] ; E[b] ; uv] per pixel, 3 * 128 + 42 = 426 columns
    mask_net         426 -> 256 -> 256 -> 256 -> 256 -> 1, ReLU between, sigmoid at the end
    predict          the net on every patch's input, stacked to m [B, Np, 1]
    masked_mse       sum(((p - g) m)^2) / (3 sum m)
    losses           rgb / edge / mask terms, render and the weighted sum `all`
"""
import torch


def crop_grid(H, W, patch_H, patch_W, crop=True, dtype=torch.float32):
    """[h*w, 2] (x, y) of the centre crop (or of the whole canvas), row-major, computed in float32 as
    the reference does and then cast."""
    if crop:
        ys = torch.arange(H // 2 - patch_H // 2, H // 2 + patch_H // 2, dtype=torch.float32)
        xs = torch.arange(W // 2 - patch_W // 2, W // 2 + patch_W // 2, dtype=torch.float32)
    else:
        ys = torch.arange(H, dtype=torch.float32)
        xs = torch.arange(W, dtype=torch.float32)
    m = max(H, W)
    y = ((ys + 0.5) / H * 2 - 1) * (H / m)
    x = ((xs + 0.5) / W * 2 - 1) * (W / m)
    grid = torch.stack([x[None, :].expand(len(ys), len(xs)), y[:, None].expand(len(ys), len(xs))], dim=-1)
    return grid.reshape(-1, 2).to(dtype)


def uv_features(xy, n_freqs=10):
    """[N, 2] -> [N, 2 + 4 n_freqs]; frequencies 2^k without pi, band-major, sin before cos."""
    cols = [xy]
    for k in range(n_freqs):
        cols.append(torch.sin((2.0 ** k) * xy))
        cols.append(torch.cos((2.0 ** k) * xy))
    return torch.cat(cols, dim=-1)


def mask_input(index, embed, xy, n_freqs=10):
    """index [B, 3, Np] (integer rows of embed [V, 128]), xy [Np, 2] -> [B, Np, 3 * 128 + 2 + 4 n_freqs]."""
    B, _, Np = index.shape
    rows = embed[index.long()]                      # [B, 3, Np, 128]
    rows = rows.permute(0, 2, 1, 3).reshape(B, Np, -1)
    uv = uv_features(xy, n_freqs).to(embed.dtype)
    return torch.cat([rows, uv[None].expand(B, -1, -1)], dim=-1)


def mask_net(x, params, bias_after=False):
    """params: [W0, b0, W1, b1, ...] in nn.Linear layout.  Returns m [..., 1].  bias_after: the bias
    added to the finished product instead of inside it (another float32 rounding of the same sum)."""
    n = len(params) // 2
    for l in range(n):
        if bias_after:
            x = x @ params[2 * l].t() + params[2 * l + 1]
        else:
            x = torch.nn.functional.linear(x, params[2 * l], params[2 * l + 1])
        if l < n - 1:
            x = torch.relu(x)
    return torch.sigmoid(x)


def predict(index, embed, xy, params, n_freqs=10):
    """m [B, Np, 1]: the shared net on each patch's [Np, 426] input in turn, stacked (one patch at a
    time, as the reference evaluates it: the float32 sums then run in the same order)."""
    x = mask_input(index, embed, xy, n_freqs)
    return torch.stack([mask_net(x[i], params) for i in range(x.shape[0])])


def masked_mse(pred, target, m):
    d = (pred - target) * m
    return (d ** 2).sum() / (m.sum() * 3)


def losses(rgb_pred, rgb_gt, m_map, alpha=0.0, edge_pred=None, edge_gt=None, weights=(0, 0, 0, 0)):
    """rgb_pred / rgb_gt [B, 3, h, w], m_map [B, 1, h, w]; edge_* [B, C, h, w] or None (no edge term).
    weights: log10 weights of (render, rgb, mask, edge).  Returns a dict of 0-d tensors."""
    out = {}
    out["rgb"] = masked_mse(rgb_pred, rgb_gt, m_map)
    out["mask"] = ((1 - m_map) ** 2).mean()
    if edge_pred is not None:
        out["edge"] = masked_mse(edge_pred, edge_gt, m_map)
        out["render"] = (1 - alpha) * out["rgb"] + 0.5 * out["mask"] + alpha * out["edge"]
    else:
        out["edge"] = None
        out["render"] = (1 - alpha) * out["rgb"] + 0.5 * out["mask"]
    total = 0.0
    for key, w in zip(("render", "rgb", "mask", "edge"), weights):
        if w is not None and out[key] is not None:
            total = total + 10 ** float(w) * out[key]
    out["all"] = total
    return out
