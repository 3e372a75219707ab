"""Torch statement of the mask network's all-operands-split bf16 recipe (MARF_BF16X3A), for the tests.
Nothing here is used by the product.

    split(x)      hi = bf16_rne(x), lo = bf16_rne(x - float(hi)), both returned as float32
    mm3(a, b)     a_h b_h + a_h b_l + a_l b_h with float32 accumulation (lo * lo dropped)
    forward       z = W a + b through mm3, a = relu(z) split before it is the next operand, sigmoid in float32
    backward      g = dm (1 - m) m in float32; da = dz W, dW = dz^T a, both through mm3; db = sum(dz_h + dz_l);
                  relu' from the forward's own pre-activations

`single` names operand classes left as one bf16 (their lo dropped): "dz" is the image net's bf16x3
recipe, the one the mask net's 1e-2 gradient bound rules out.

    case(shape)   the seeded random-weight case of test_gpu_implicit_mask._case with the kink threshold of
                  this recipe: pixels with any hidden float64 pre-activation within 3e-5 of 0 (2.3 x the
                  recipe's emulated pre-activation error, 1.3e-5) get a zero upstream gradient
"""
import numpy as np
import torch

import mask_ref

N_VOCAB = 7
SHAPES = {"ragged": (3, 50, 54), "tiny": (1, 6, 10), "exact": (2, 16, 16)}
LAYER_DIMS = [(256, 426), (256, 256), (256, 256), (256, 256), (1, 256)]
KINK = 3e-5


def split(x, single=False):
    hi = x.to(torch.bfloat16).to(torch.float32)
    lo = torch.zeros_like(hi) if single else (x - hi).to(torch.bfloat16).to(torch.float32)
    return hi, lo


def mm3(a, b):
    """a, b: (hi, lo) pairs of float32 matrices [M, K], [K, N]."""
    return a[0] @ b[0] + a[0] @ b[1] + a[1] @ b[0]


def forward(x, params, single=()):
    """x [N, D] float32, params [W0, b0, ...] float32.  Returns m [N, 1] and what the backward needs."""
    n = len(params) // 2
    acts, zs = [], []
    a = split(x, "act" in single)
    for l in range(n):
        w = split(params[2 * l], "w" in single)
        z = mm3(a, (w[0].t(), w[1].t())) + params[2 * l + 1]
        acts.append(a)
        zs.append(z)
        if l < n - 1:
            a = split(torch.relu(z), "act" in single)
    return torch.sigmoid(zs[-1]), (acts, zs)


def backward(dm, m, params, saved, single=()):
    """Gradients [dW0, db0, ...] for the upstream dm [N, 1]."""
    acts, zs = saved
    n = len(params) // 2
    grads = [None] * (2 * n)
    dz = split((dm * (1 - m)) * m, "dz" in single)
    for l in range(n - 1, -1, -1):
        grads[2 * l] = mm3((dz[0].t(), dz[1].t()), acts[l])
        grads[2 * l + 1] = (dz[0] + dz[1]).sum(0)
        if l > 0:
            da = mm3(dz, split(params[2 * l], "w" in single))
            dz = split(da * (zs[l - 1] > 0), "dz" in single)
    return grads


_CASES = {}


def case(shape):
    """Seeded weights, embedding table, indices and upstream gradient with the float64 reference (m64, g64),
    the float32 input x of every patch and the share of pixels the kink rule excluded."""
    if shape in _CASES:
        return _CASES[shape]
    B, ph, pw = SHAPES[shape]
    g = torch.Generator().manual_seed(11 + len(shape))
    params = []
    for mo, k in LAYER_DIMS:
        bound = 1.0 / np.sqrt(k)
        params.append((torch.rand(mo, k, generator=g) * 2 - 1) * bound)
        params.append((torch.rand(mo, generator=g) * 2 - 1) * bound)
    embed = torch.randn(N_VOCAB, 128, generator=g)
    index = torch.randint(0, N_VOCAB, (B, 3, ph * pw), generator=g)
    dm = torch.randn(B, ph * pw, 1, generator=g)
    p64 = [p.double().requires_grad_() for p in params]
    xy = mask_ref.crop_grid(2 * ph, 2 * pw, ph, pw, True, torch.float64)
    with torch.no_grad():
        x = mask_ref.mask_input(index, embed.double(), xy)
        near = torch.zeros(B, ph * pw, dtype=torch.bool)
        for l in range(len(LAYER_DIMS) - 1):
            zl = torch.nn.functional.linear(x, p64[2 * l], p64[2 * l + 1])
            near |= (zl.abs() < KINK).any(-1)
            x = torch.relu(zl)
    dm[near] = 0
    m64 = mask_ref.predict(index, embed.double(), xy, p64)
    (m64 * dm.double()).sum().backward()
    x32 = mask_ref.mask_input(index, embed, mask_ref.crop_grid(2 * ph, 2 * pw, ph, pw))
    c = dict(params=params, embed=embed, index=index, dm=dm, m64=m64.detach(), g64=[p.grad for p in p64], x32=x32,
             excluded=float(near.double().mean()))
    _CASES[shape] = c
    return c
