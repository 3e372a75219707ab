"""Torch statement of the plain 16-bit tile recipe (precision: bf16 / fp16 on k_mlp_step<PrecBF16 | PrecF16>
and the 16-bit k_wgrad / k_wgrad_dma family), for the tests.  Nothing here is used by the product.

T(x) is the storage type's round-to-nearest-even conversion (P::cvt / P::pk2 in marf_common.h: the
hardware v_cvt_pk_bf16_f32 and v_cvt_f16_f32, torch's .to(bfloat16) / .to(float16)).

    prologue   grid, warp, sin / cos and the c2f band weight multiplied in, all float32, then T
               (tile_prologue, TileView::put).  The 16-bit kernels take sin / cos from the hardware
               v_sin_f32 / v_cos_f32 on a double-float reduced argument (band_sincos<true>), not from
               sincosf: a feature can land on the neighbouring T value.  The statement uses exact
               sin / cos; the GPU test leaves the pixels out whose saved feat_0 row differs.  The
               prologue's adjoint is autograd through the float32 prologue (warp_adjoint_tail is float32
               on the float32 accumulators).
    weights    T once (the packed image); biases stay float32
    forward    z_l = W_l a_l + b_l in one float32 accumulator; a_{l+1} = T(relu(z_l)); the ReLU record is
               z_l > 0; a skip layer's input is [a ; T(features)] (marf_step.hip hidden()); the last layer
               the same; sigmoid, masked MSE and g = ((2 x m)(1 - y)) y in float32 (step_loss_slots)
    last layer dW = (g_h + g_l)^T a_{n-1}, g_h = T(g), g_l = T(g - g_h) (step_wlast_grad); db = sum g in
               float32 (step_tile_partials)
    dgrad      starts from T(g) alone (step_fill_d); da = W_l^T dz in float32; dz_l = T(da * relu'); a skip
               layer's posenc columns of da are added, unrounded, into a float32 image (dsk) that joins
               layer 0's da before the prologue's adjoint
    wgrad      dW_l = dz_{l+1}^T a_l, db_l = sum dz_{l+1}: the saved T tensors, float32 accumulators
    scaling    2 / denom at the end (loss.all = 2 loss.rgb with use_edges off)

    fp16       subnormals are kept (torch's conversion; 2^-24 .. 2^-14, where g and dz of masked-MSE size often
               lie).  A conversion or MFMA that flushed them would move the gradient tensors by 1e-4 .. 8e-3
               (ftz=True below: 3 to 90 x the GPU test's bounds); the kernel is inside the bounds on every
               case, so v_cvt_f16_f32 and the f16 MFMA keep them.

step(...) returns what cpu_ref.CpuRefStep.step() returns (loss_rgb, rgb, grads, dh) plus the hidden
pre-activations zs, every layer's input acts and the gradient at every layer's output dzs.  Switches:
    T         "bf16", "fp16", or None: no rounding anywhere and float64 throughout (the structure check
              against cpu_ref.CpuRefStep)
    acc       torch.float64 (default: the recipe's operand rounding alone; every GEMM result rounded to
              float32, as the kernel's accumulators are), or ("f32", k): float32 in the k-th of several
              summation orders on top (k = 0: torch's own)
    prologue  dtype of the prologue the adjoint runs through: torch.float32 (default) or torch.float64
    features  the prologue's float32 values from elsewhere, [pixels, 2 + 4L]; the adjoint stays torch's.
              held() and contract() pass the oracle's (step2_ref.features), as step2_ref.step does and for
              its reason
    mutate    a defect of MUTATIONS put into the statement (tests/test_plain16_cpu.py)
    ftz       fp16 results below 2^-14 flushed to zero (a diagnosis aid: what a flushing conversion would do)
"""
import numpy as np
import torch

import bf16x3_tile_ref as R
import cpu_ref

err, errors, truth = R.err, R.errors, R.truth

TYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}

# defect -> the gradient tensors it can move ("hidden": dW_l, db_l below the last layer; "wlast", "blast":
# the last layer's; "dh": d warp).  By construction, not by measurement.
MUTATIONS = {
    "wlast_no_gl": ("wlast",),                # (a) dW_last from g_h alone
    "dgrad_full_g": ("hidden", "dh"),         # (b) the dgrad chain started from g, not T(g)
    "wgrad_drop_rows": ("hidden",),           # (c) hidden weight gradients without their last 32 pixel rows
    "dz_trunc": ("hidden", "dh"),             # (d) bf16: dz truncated, not rounded
    "edge_rows": ("hidden",),                 # (e) the last 32 output rows of a hidden gradient's last row block zeroed
    "blast_rounded": ("blast",),              # (f) db_last summed from T(g), not from float32 g
}


def touched(mutation, n_layers):
    """Indices into flat(grads) + [dh] (2 l: dW_l, 2 l + 1: db_l, 2 n: d warp) a defect can move."""
    kinds = MUTATIONS[mutation]
    out = []
    if "hidden" in kinds:
        out += [i for l in range(n_layers - 1) for i in (2 * l, 2 * l + 1)]
    if "wlast" in kinds:
        out.append(2 * n_layers - 2)
    if "blast" in kinds:
        out.append(2 * n_layers - 1)
    if "dh" in kinds:
        out.append(2 * n_layers)
    return out


def mutations_for(T):
    return [m for m in MUTATIONS if m != "dz_trunc" or T == "bf16"]


def _round(T, ftz):
    if T is None:
        return lambda x: x
    dt = TYPES[T]

    def f(x):
        y = x.to(dt).to(torch.float32)
        if ftz and T == "fp16":
            y = torch.where(y.abs() < 2.0 ** -14, torch.zeros_like(y), y)
        return y
    return f


def _trunc_bf16(x):
    return (x.contiguous().view(torch.int32) & -65536).view(torch.float32)


def _mm(a, b, acc):
    """a @ b accumulated in `acc`: a dtype, or ("f32", k) for float32 in the k-th summation order: the
    contraction axis in steps of 32 (k = 0: as it lies; k > 0: permuted by the generator seeded k), each step's
    sum formed exactly (in float64: 32 products of 16-bit values), rounded to float32 and added to a float32
    accumulator in turn -- an MFMA chain's shape, and the same bits on every host, which torch's own float32
    matmul is not (its blocking follows the CPU: E_sum moved by 2 x between two hosts)."""
    if isinstance(acc, tuple):
        K = a.shape[1]
        p = torch.arange(K) if acc[1] == 0 else torch.randperm(K, generator=torch.Generator().manual_seed(acc[1]))
        p = p.to(a.device)
        a64, b64 = a.to(torch.float64), b.to(torch.float64)
        out = torch.zeros(a.shape[0], b.shape[1], dtype=torch.float32, device=a.device)
        for c in range(0, K, 32):
            i = p[c:c + 32]
            out = out + (a64[:, i] @ b64[i]).to(torch.float32)
        return out
    return a.to(acc) @ b.to(acc)


def _colsum(x, acc):
    """Sum over the rows of x in `acc` (the bias gradients), by the same rule."""
    if not isinstance(acc, tuple):
        return x.to(acc).sum(0)
    return _mm(torch.ones(1, x.shape[0], dtype=x.dtype, device=x.device), x, acc)[0]


def _acc_dtype(acc):
    return torch.float32 if isinstance(acc, tuple) else acc


def step(cfg, params, warp, rgb, mask, progress, T="bf16", acc=torch.float64, device="cpu", mutate=None, features=None,
         prologue=torch.float32, ftz=False, _dz_out=None):
    assert T is None or T in TYPES, T
    assert mutate is None or mutate in MUTATIONS, mutate
    dev = torch.device(device)
    wd = torch.float64 if T is None else torch.float32  # the "float32" of the recipe
    if T is None:
        acc = prologue = torch.float64
    rnd = _round(T, ftz)
    ad = _acc_dtype(acc)

    def A(a):
        return torch.as_tensor(np.asarray(a, np.float32)).to(dev)
    L, n = cfg["L"], len(params)
    skip = tuple(cfg.get("skip", ()))
    B, _, h, w = rgb.shape
    # ---- the prologue (autograd keeps its adjoint)
    wp = A(warp).to(prologue).clone().requires_grad_()
    xy = cpu_ref.pixel_grid(cfg["H"], cfg["W"], cfg["patch_H"], cfg["patch_W"], crop=True, dtype=prologue).to(dev)
    uv = cpu_ref.warp_grid(xy.repeat(B, 1, 1), wp)
    x = uv
    if L > 0:
        x = torch.cat([uv, cpu_ref.positional_encoding(uv, L, torch.tensor(progress, dtype=prologue, device=dev), cfg["c2f"])], -1)
    x = x.reshape(B * h * w, -1)
    D = x.shape[1]
    Ws = [rnd(A(W).to(wd)) for W, _ in params]
    bs = [A(b).to(wd) for _, b in params]
    # ---- forward
    f0 = rnd((x.detach() if features is None else A(features).reshape(x.shape)).to(wd))
    a = f0
    acts, zs = [], []
    for l in range(n):
        if l in skip:
            a = torch.cat([a, f0], -1)
        z = (_mm(a, Ws[l].t(), acc) + bs[l].to(ad)).to(wd)
        acts.append(a)
        zs.append(z)
        if l < n - 1:
            a = rnd(torch.relu(z))
    y = torch.sigmoid(zs[-1])
    tgt = A(rgb).permute(0, 2, 3, 1).reshape(-1, 3).to(wd)
    m = A(mask).reshape(-1, 1).to(wd)
    xm = (y - tgt) * m
    denom = m.sum() * 3
    loss = (xm * xm).to(ad).sum().to(wd) / denom
    g = ((2.0 * xm) * m * (1.0 - y)) * y  # unit upstream gradient; 2 / denom is applied to the sums below
    scale = (2.0 / denom).to(wd)
    # ---- backward
    g_h = rnd(g)
    g_l = rnd(g - g_h)
    if mutate == "wlast_no_gl":
        g_l = torch.zeros_like(g_l)
    grads = [None] * n
    b_src = g_h if mutate == "blast_rounded" else g
    grads[n - 1] = ((_mm(g_h.t(), acts[n - 1], acc) + _mm(g_l.t(), acts[n - 1], acc)).to(wd), _colsum(b_src, acc).to(wd))
    dz = g if mutate == "dgrad_full_g" else g_h
    dsk = None
    dzs = [None] * n  # the gradient at layer l's output, as layer l's weight gradient reads it
    for l in range(n - 1, -1, -1):
        if _dz_out is not None and l in _dz_out:  # (warp_grad_from_dz: the gradient at layer l's output, given)
            dz = torch.as_tensor(np.asarray(_dz_out[l], np.float32)).to(dev)
        dzs[l] = dz
        if l < n - 1:
            d_, a_ = dz, acts[l]
            if mutate == "wgrad_drop_rows":
                d_, a_ = dz[:-32], a_[:-32]
            gw, gb = _mm(d_.t(), a_, acc).to(wd), _colsum(d_, acc).to(wd)
            if mutate == "edge_rows":
                gw, gb = gw.clone(), gb.clone()
                gw[-32:] = 0
                gb[-32:] = 0
            grads[l] = (gw, gb)
        da = _mm(dz, Ws[l], acc).to(wd)
        if l in skip:  # [a ; features]: the features' share waits, unrounded, for layer 0's
            dsk = da[:, -D:] if dsk is None else dsk + da[:, -D:]
            da = da[:, :-D]
        if l > 0:
            dz = da * (zs[l - 1] > 0)
            dz = _trunc_bf16(dz) if mutate == "dz_trunc" else rnd(dz)
    if dsk is not None:
        da = da + dsk
    x.backward(da.to(prologue))
    return dict(loss_rgb=float(loss), rgb=y.cpu().numpy(), zs=zs[:-1], acts=acts, dzs=dzs, Ws=Ws, scale=float(scale),
                grads=[((gw * scale).cpu().numpy(), (gb * scale).cpu().numpy()) for gw, gb in grads],
                dh=(wp.grad.to(wd) * scale).cpu().numpy())


def flat(s):
    """dW_0, db_0, ..., dW_{n-1}, db_{n-1}, d warp."""
    return [x for pair in s["grads"] for x in pair] + [s["dh"]]


def errs(got, ref):
    """Per tensor of flat(): max error relative to the reference tensor's max."""
    return [err(a, b) for a, b in zip(flat(got), flat(ref))]


def kink_pixels(inputs, T, factor=4.0, device="cpu", features=None, propagate=True):
    """Pixels whose ReLU decision the accumulation order can flip, by the per-layer rule: a hidden
    pre-activation of the float64-accumulated statement within `factor` x the largest per-layer accumulation
    difference of 0.  That difference is float32 against float64 accumulation of each layer's GEMM on the SAME
    inputs (the float64-accumulated statement's activations) -- not the end-to-end difference
    bf16x3_tile_ref.kink_pixels takes: in plain 16 bit one flipped rounding of an activation moves the next
    layer's z by about 1e-3, and the end-to-end rule then marks a third of the pixels or more.
    propagate (default): also the pixels where exactly such a flipped rounding can reach a kink
    (_flip_kinks).  The per-layer rule alone marks <= 0.31 % of the pixels and is not enough: measured in
    torch's own float32 matmul, at 1 seed in 4 the statement's float32 and float64 accumulation differed in
    one ReLU decision of a pixel with |z| = 1e-4 .. 1e-5, which moved a weight gradient by up to 2.3e-2 of
    its max (p-288, seed 4).  With both: 0 to 5.3 % of the pixels on the two- and three-layer nets of
    plain16_cases, and no differing decision in any of eight orders (tests/test_plain16_cpu.py).
    Returns the pixels as a [B, 1, h, w] float array of 0 / 1 and the threshold."""
    s = step(*inputs, T=T, device=device, features=features)
    params = inputs[1]
    rnd = _round(T, False)
    Wts, d = [], 0.0
    for l in range(len(params) - 1):
        Wts.append(rnd(torch.as_tensor(np.asarray(params[l][0], np.float32)).to(s["acts"][l].device)).t())
        z32, z64 = _mm(s["acts"][l], Wts[l], ("f32", 0)), _mm(s["acts"][l], Wts[l], torch.float64).to(torch.float32)
        d = max(d, float((z32 - z64).abs().max()))
    thr = factor * d
    near = torch.zeros(s["zs"][0].shape[0], dtype=torch.bool, device=s["zs"][0].device)
    for z in s["zs"]:
        near |= (z.abs() < thr).any(-1)
    if propagate:
        near |= _flip_kinks(s, Wts, T, thr, tuple(inputs[0].get("skip", ())))
    return near.cpu().numpy().astype(np.float32).reshape(inputs[4].shape), thr


def _flip_kinks(s, Wts, T, thr, skip):
    """The pixels a flipped ROUNDING can push over a ReLU kink.  Two runs of the recipe whose accumulation
    orders differ agree on layer 0's input; a pre-activation within thr of a rounding midpoint of T may round
    to either neighbour, the next layer then sees that activation one ulp_T away, and its pre-activations move
    by |w| ulp_T -- about 1e-3 in bf16, far more than thr.  Per pixel and unit: delta_0 = thr; unit k of
    layer l is at risk if relu(z_lk) is within delta_lk of a midpoint; delta_{l+1, j} = thr + sum over the
    units at risk of |W_{l+1}[j, k]| ulp_T(a_k); a pixel is marked if |z_lj| < delta_lj anywhere.  (A bound,
    not an estimate: every flip at risk is taken to happen and to push the same way.)"""
    bits = torch.int16
    dt = TYPES[T]
    near = torch.zeros(s["zs"][0].shape[0], dtype=torch.bool, device=s["zs"][0].device)
    delta = None
    for l, z in enumerate(s["zs"]):
        dl = torch.full_like(z, thr) if delta is None else delta
        near |= (z.abs() < dl).any(-1)
        if l + 1 >= len(Wts):
            break
        r = torch.relu(z)
        a = r.to(dt)
        up = (a.view(bits) + 1).view(dt).to(torch.float32)
        dn = torch.where(a > 0, (a.view(bits) - 1).view(dt).to(torch.float32), torch.zeros_like(r))
        af = a.to(torch.float32)
        mid = torch.minimum((af + up) / 2 - r, r - (af + dn) / 2)
        risk = ((mid < dl) & (z > 0)).to(torch.float32) * (up - af)
        if (l + 1) in skip:  # [a ; features]: the features' columns are the same in both runs
            risk = torch.cat([risk, torch.zeros(risk.shape[0], Wts[l + 1].shape[0] - risk.shape[1], device=risk.device)], -1)
        delta = thr + risk @ Wts[l + 1].abs()
    return near


_HELD, _CONTRACT = {}, {}


def contract(case, T):
    """The contract comparison's host side, once per (case, type): the reference in float64 on the case's
    inputs (t64) and E_emu, the statement's own error against it per tensor of flat()."""
    if (case, T) not in _CONTRACT:
        import plain16_cases as C
        inputs = C.inputs(case, T)
        t64 = truth(inputs)
        emu = step(*inputs, T=T, features=C.features(case, T))
        _CONTRACT[case, T] = dict(t64=t64, emu=emu, e_emu=errs(emu, t64), rgb=float(np.abs(emu["rgb"] - t64["rgb"]).max()))
    return _CONTRACT[case, T]


ORDERS = 8  # float32 summation orders d warp's noise is the worst of (and none may take another ReLU decision)
ULP = {"bf16": 2.0 ** -8, "fp16": 2.0 ** -11}  # one step to the neighbouring value, relative (at least)


def one_flip(s, T):
    """What ONE value of ONE pixel landing on the neighbouring T value is worth, from the number format alone
    (u = 2^-8 bf16 / 2^-11 fp16), relative to the tensor's max, per MLP gradient tensor of flat():
        dW_l        u x the largest single-pixel term max_p max|dz_l(p)| max|a_l(p)| (a_l and dz_l are T values)
        db_l, l < n-1   u x max|dz_l|
        db_last     the sum of float32 g, nothing in it is rounded to T: a flipped a_{n-1}(p, k) moves z_last by
                    dz = u max|W_last(c, k) a_{n-1}(p, k)| and g by at most 0.3 dz (|dg/dz| = 2 m^2 |(y(1-y))^2 +
                    (y-t) y(1-y)(1-2y)| <= 0.3)
    and for rgb 0.25 dz (sigmoid' <= 1/4).  Two correct runs of the recipe that differ in summation order
    differ by a handful of such steps (an activation within 1e-6 of a rounding midpoint); in bf16 they are few
    and large, so one pair of runs may show none on a tensor (E_sum = 0) where another pair shows one."""
    u, sc, out = ULP[T], s["scale"], []
    n = len(s["acts"])
    dzl = u * float((s["acts"][-1].abs().max(0).values * s["Ws"][-1].abs().max(0).values).max())
    for l, (dz, a) in enumerate(zip(s["dzs"], s["acts"])):
        gw, gb = s["grads"][l]
        pd, pa = dz.abs().max(-1).values, a.abs().max(-1).values
        fb = 0.3 * dzl if l == n - 1 else u * float(pd.max())
        out += [u * float((pd * pa).max()) * sc / (float(np.abs(gw).max()) + 1e-30), fb * sc / (float(np.abs(gb).max()) + 1e-30)]
    return out, 0.25 * dzl


def one_flip_dh(inputs, s, T):
    """one_flip() for d warp: the dgrad's last T values are dz at layer 0's output; one of them, of one pixel,
    on its neighbour moves layer 0's da of that pixel by u |dz(p, j)| W_0[j, :] and d warp by that through the
    pixel's prologue Jacobian J_p = d features(p) / d warp (float64 central differences; a pixel depends on its
    own patch's eight parameters only).  The largest such term, relative to d warp's max."""
    cfg, params, warp, rgb = inputs[0], inputs[1], inputs[2], inputs[3]
    B, _, h, w = rgb.shape
    f64 = torch.float64
    xy = cpu_ref.pixel_grid(cfg["H"], cfg["W"], cfg["patch_H"], cfg["patch_W"], crop=True, dtype=f64)

    def feats(wp):
        uv = cpu_ref.warp_grid(xy.repeat(B, 1, 1), wp)
        if cfg["L"] > 0:
            uv = torch.cat([uv, cpu_ref.positional_encoding(uv, cfg["L"], torch.tensor(inputs[5], dtype=f64), cfg["c2f"])], -1)
        return uv.reshape(B * h * w, -1)
    w0, eps = torch.as_tensor(np.asarray(warp, np.float64)), 1e-5
    J = []
    for k in range(8):
        d = torch.zeros_like(w0)
        d[:, k] = eps
        J.append((feats(w0 + d) - feats(w0 - d)) / (2 * eps))
    J = torch.stack(J, -1)  # [pixels, D, 8]
    G = torch.einsum("md,ndk->nmk", s["Ws"][0].to(f64), J).abs()
    worst = float((s["dzs"][0].abs().to(f64)[:, :, None] * G).max())
    return ULP[T] * worst * s["scale"] / (float(np.abs(s["dh"]).max()) + 1e-30)


def warp_grad_from_dz(inputs, T, dz_out, features=None, prologue=torch.float32):
    """d warp of the statement's layer-0 dgrad and adjoint started from GIVEN gradients dz_out[l] at the
    output of layer l (l = 0, and l for every skip layer l: their posenc share), float64 accumulation: what
    the kernel's last stage computes from the dz it saved."""
    cfg, params, warp, rgb, mask, progress = inputs
    s = step(cfg, params, warp, rgb, mask, progress, T=T, features=features, prologue=prologue, _dz_out=dz_out)
    return s["dh"]


def held(case, T, drop=None):
    """Everything the kernel-against-statement comparison of a case needs, from the statement alone; without
    `drop` computed once per (case, type) and shared by the CPU and the GPU tests (read-only).  drop: further
    pixels ([B, 1, h, w] of 0 / 1) whose mask is zeroed before anything is computed, so that bounds and
    comparison are on the same input.
        inputs   the case's inputs with the kink pixels' (and drop's) mask zeroed; near, thr, out (kink share;
                 out_layer: the per-layer rule's alone), left
        emu      the statement on them (float64 accumulation)
        e_sum    per tensor of flat(): the statement in the first float32 summation order against emu
        e_mut    defect -> per-tensor change against emu;  e_min: per tensor, the least over the defects touching it
        bound    per tensor, what the kernel is held to:
                 MLP tensors  sqrt(max(e_sum, one_flip) e_min): E_sum, but no less than one rounding flip's worth
                 d warp       max(1e-5, 3 e32, 3 max(dh_noise, one_flip_dh)), dh_noise the worst of ORDERS orders
                              against emu
                 rgb_bound    max(1e-6, 3 max(rgb32, one flip's worth)), rgb32 the first order against emu (abs)
        e32      d warp of emu with its adjoint through a float64 prologue against the float32 one
        loss32   the first float32 order against emu, rel"""
    if drop is None and (case, T) in _HELD:
        return _HELD[case, T]
    import plain16_cases as C
    inputs, feats = C.inputs(case, T), C.features(case, T)
    cfg, params, warp, rgb, mask, progress = inputs
    near, thr = kink_pixels(inputs, T, features=feats)
    out_layer = float(kink_pixels(inputs, T, features=feats, propagate=False)[0].mean())
    keep = (1 - near) if drop is None else (1 - near) * (1 - drop)
    inputs2 = (cfg, params, warp, rgb, mask * keep, progress)
    emu = step(*inputs2, T=T, features=feats)
    nl = len(params)
    draws = [step(*inputs2, T=T, features=feats, acc=("f32", k)) for k in range(ORDERS)]
    e_draw = [errs(d, emu) for d in draws]
    live = torch.as_tensor(inputs2[4].reshape(-1)) > 0
    relu_flips = sum(int((((a > 0) != (b > 0)).any(-1) & live).sum()) for d in draws for a, b in zip(d["zs"], emu["zs"]))
    e_sum = e_draw[0]
    flip, flip_rgb = one_flip(emu, T)
    e_mut = {mu: errs(step(*inputs2, T=T, features=feats, mutate=mu), emu) for mu in mutations_for(T)}
    e_min = [min(e_mut[mu][i] for mu in e_mut if i in touched(mu, nl)) for i in range(2 * nl + 1)]
    e32 = err(emu["dh"], step(*inputs2, T=T, features=feats, prologue=torch.float64)["dh"])
    dh_noise, dh_flip = max(e[-1] for e in e_draw), one_flip_dh(inputs2, emu, T)
    rgb32 = float(np.abs(draws[0]["rgb"] - emu["rgb"]).max())
    ok = [all(e_mut[mu][i] >= 10 * e_sum[i] for mu in e_mut if i in touched(mu, nl)) for i in range(2 * nl + 1)]
    h = dict(
        ok10=ok, inputs=inputs2, features=feats, near=near, keep=keep, thr=thr, out=float(near.mean()), out_layer=out_layer,
        left=int((mask * keep).sum()), emu=emu, e_sum=e_sum, e_mut=e_mut, e_min=e_min, e_flip=flip, relu_flips=relu_flips,
        bound=[float(np.sqrt(max(e_sum[i], flip[i]) * e_min[i])) for i in range(2 * nl)] + [max(1e-5, 3 * e32, 3 * max(dh_noise, dh_flip))],
        e32=e32, dh_noise=dh_noise, dh_flip=dh_flip, rgb32=rgb32, rgb_flip=flip_rgb, rgb_bound=max(1e-6, 3 * max(rgb32, flip_rgb)),
        loss32=abs(draws[0]["loss_rgb"] / emu["loss_rgb"] - 1))
    # held: per tensor, every defect touching it is >= 10 x e_sum and >= 3 x the bound
    h["held"] = [h["ok10"][i] and all(e_mut[mu][i] >= 3 * h["bound"][i] for mu in e_mut if i in touched(mu, nl)) for i in range(2 * nl + 1)]
    if drop is None:
        _HELD[case, T] = h
    return h
