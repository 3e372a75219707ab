"""The Gauss-Newton normal equations of marf_gn_normal on the GPU, against the float64
reference of tests/gn_ref.py, against the kernels that exist (the warp-only step's gradient and loss,
marf_render's rgb), and for determinism and honest buffer plans.

Inputs: bf16x3_tile_ref.synthetic_inputs (2 patches on the 512 canvas, seed 3, non-zero warps, c2f [0, 0.4]
at progress 0.2, and once off, on "odd"): "ragged" ([128] x 6, 50 x 54: TP = 128 split / TP = 64 fp32, 21.1 tiles per
patch, a padded last tile), "odd" ([288, 512, 288]: TP = 64 split) and the k_step2-shaped "small" ([64, 64],
50 x 54) of gn_ref.  Pixels at a ReLU kink (bf16x3_tile_ref.kink_pixels, factor 4) get mask 0 on both
sides, the project's precedent; their share must stay <= 8 %."""
import ctypes

import numpy as np
import pytest
import torch

import bf16x3_tile_ref as R
import gn_ref
from test_gpu_parity import DEV, gpu, make_opt, t  # noqa: F401 (gpu: fixture)

pytestmark = pytest.mark.gpu

CASES = ["ragged", "odd", "small"]
_REF = {}


def reference(case, c2f=True):
    """(inputs with the kink pixels masked, kink share, float64 normal equations) of a case: computed
    once, shared by the tests, never changed."""
    key = (case, c2f)
    if key not in _REF:
        inputs = gn_ref.synthetic_inputs(case)
        if not c2f:
            inputs = (dict(inputs[0], c2f=None),) + tuple(inputs[1:])
        near, _ = R.kink_pixels(inputs)
        cfg, params, warp, rgb, mask, progress = inputs
        inputs = (cfg, params, warp, rgb, mask * (1 - near), progress)
        _REF[key] = (inputs, float(near.mean()), gn_ref.normal(inputs))
    return _REF[key]


def setup(inputs, prec, tmp_path, **over):
    """A frozen Model on `inputs` (the image's parameters copied in), its var bundle and engine."""
    from model import planar
    from util import EasyDict as edict
    cfg, params, warp, rgb, mask, progress = inputs
    B = rgb.shape[0]
    hidden = [W.shape[0] for W, _ in params[:-1]]
    base = dict(H=cfg["H"], W=cfg["W"], patch_H=cfg["patch_H"], patch_W=cfg["patch_W"], batch_size=B, precision=prec,
                use_edges=False, freeze_image=True, barf_c2f=list(cfg["c2f"]) if cfg["c2f"] else None,
                arch={"layers": [None] + hidden + [3], "skip": [], "posenc": {"L_2D": cfg["L"]}})
    base.update(over)
    opt = make_opt(tmp_path, **base)
    torch.manual_seed(3)
    m = planar.Model(opt)
    m.images = edict(rgb=t(rgb), masks=t(mask), masks_eroded=t(mask), edges=None, gt_hom=None, gt=None)
    m.build_networks()
    with torch.no_grad():
        for lay, (W, b) in zip(m.graph.neural_image.mlp, params):
            lay.weight.copy_(t(W))
            lay.bias.copy_(t(b))
    if tuple(m.graph.warp_param.weight.shape) == tuple(np.shape(warp)):  # (se2: the caller sets its 3 dof)
        m.graph.warp_param.weight.data.copy_(t(warp))
    m.graph.neural_image.progress.data.fill_(progress)
    m.setup_optimizer()
    return m, edict(idx=torch.arange(B), images=m.images), m.graph.neural_image.engine(torch.device(DEV))


def launch(m, loss_only=False, warp=None):
    g = m.graph
    h = g.warp_h().detach() if warp is None else t(np.asarray(warp, np.float32))
    out, rgb = g.neural_image.render_gn(h, m.images.rgb, m.images.masks, loss_only=loss_only)
    torch.cuda.synchronize()
    return out, rgb


def unpack(out):
    o = out.cpu().numpy()
    N = np.zeros((o.shape[0], 9, 9))
    N[:, gn_ref.TRIU[0], gn_ref.TRIU[1]] = o[:, 11:]
    N = N + np.triu(N, 1).transpose(0, 2, 1)
    return dict(sse=o[:, 0], msum=o[:, 1], g9=o[:, 2:11], N=N)


@pytest.mark.parametrize("case,c2f", [(c, True) for c in CASES] + [("odd", False)])
def test_fp32_against_float64(case, c2f, tmp_path):
    """fp32: sse, msum, g9 and N within 1e-5 of each tensor's max (the project's fp32 bound), rgb within
    1e-5.  The §11 rule: a tensor for which torch's own float32 evaluation of gn_ref differs from float64
    by more than a third of 1e-5 is held to three times that recorded error (printed).  Recorded: with c2f
    torch's float32 error is below 3.3e-6 for every tensor on the three inputs (largest: N on "odd",
    5.2e-7; the kernel's 5.2e-7), so 1e-5 holds there.  c2f is off once, on "odd": the reference alone puts
    3.2 % of its pixels at a kink there (0.4 % on "small"; 10.3 % on "ragged", above the 8 % allowed, so
    not that one).  With every band on, the float32 posenc argument 2^k pi u carries u's rounding 2^k
    times: torch's float32 g9 is off by 1.9e-3 and its N by 4.3e-5 (sse 3.8e-9), so those two are held to
    5.7e-3 and 1.3e-4; measured on one MI355X: 1.90e-3 and 4.30e-5, torch's own figures to three digits."""
    inputs, share, ref = reference(case, c2f)
    assert share <= 0.08, share
    e32 = gn_ref.normal(inputs, dtype=torch.float32)
    m, var, eng = setup(inputs, "fp32", tmp_path)
    out, rgb = launch(m)
    got = unpack(out)
    assert np.abs(rgb.cpu().numpy().astype(np.float64) - ref["rgb"]).max() <= 1e-5
    for k in ("sse", "msum", "g9", "N"):
        rec = R.err(e32[k], ref[k])
        bound = 3 * rec if rec > 1e-5 / 3 else 1e-5
        e = R.err(got[k], ref[k])
        print(case, "c2f" if c2f else "no c2f", k, "kernel %.2e | torch float32 %.2e | bound %.2e" % (e, rec, bound))
        assert e <= bound, (case, k, e, bound)
    assert np.array_equal(got["msum"], ref["msum"])


@pytest.mark.parametrize("case", CASES)
def test_bf16x3_against_float64(case, tmp_path):
    """bf16x3 on all three shapes (the split tile recipe; "small" is a k_step2 net in training): rgb within
    1e-5; g9 within max(1e-2, twice the float64-accumulated emulation's own error) of its max, the rule of
    tests/test_gpu_bf16x3_tile.py; N within 2e-2 of its max (a product of two factors each inside 1e-2,
    and its diagonal does not cancel); msum exact; sse within the first-order effect of rgb's 1e-5,
    2e-5 sum |r| over the patch.  The measured values are printed (profiles/gn/README.md records them);
    on one MI355X, kernel / emulation: g9 4.4e-6 / 5.2e-6 (ragged), 9.4e-6 / 9.0e-6 (odd), 9.1e-6 / 9.3e-6
    (small); N 2.0e-6, 1.2e-6, 2.2e-6; rgb 1.3e-7, 6.9e-7, 1.2e-6; kink shares 5.8 %, 3.1 %, 0.3 %."""
    inputs, share, ref = reference(case)
    assert share <= 0.08, share
    emu = gn_ref.emu_normal(inputs)
    m, var, eng = setup(inputs, "bf16x3", tmp_path)
    assert eng.net.step_kernel == ("k_step2" if case == "small" else "k_mlp_step_split")
    out, rgb = launch(m)
    got = unpack(out)
    e_rgb = np.abs(rgb.cpu().numpy().astype(np.float64) - ref["rgb"]).max()
    e_emu = R.err(emu["g9"], ref["g9"])
    e_g9, e_N = R.err(got["g9"], ref["g9"]), R.err(got["N"], ref["N"])
    cfg, _, _, tgt, mask, _ = inputs
    B = tgt.shape[0]
    r = np.abs((ref["rgb"].reshape(B, -1, 3) - tgt.transpose(0, 2, 3, 1).reshape(B, -1, 3)) * mask.reshape(B, -1, 1))
    e_sse = np.abs(got["sse"] - ref["sse"])
    print(case, "kink share %.1f %% | rgb %.2e | g9 kernel %.2e emulation %.2e | N kernel %.2e emulation %.2e | sse rel %.2e"
          % (100 * share, e_rgb, e_g9, e_emu, e_N, R.err(emu["N"], ref["N"]), (e_sse / ref["sse"]).max()))
    assert e_rgb <= 1e-5
    assert e_g9 <= max(1e-2, 2 * e_emu), (e_g9, e_emu)
    assert e_N <= 2e-2, e_N
    assert np.array_equal(got["msum"], ref["msum"])
    assert (e_sse <= 2e-5 * r.sum((1, 2)) + 1e-12).all(), (e_sse, r.sum((1, 2)))


@pytest.mark.parametrize("prec,bound", [("fp32", 1e-5), ("bf16x3", 1e-2)])
def test_against_the_kernels_that_exist(prec, bound, tmp_path):
    """On "small" (bf16x3: a k_step2 net, whose own warp-only step is the two-term k_step2w):
    2 E^T g9 / (3 sum msum) is render_warp_step's warp gradient within `bound` of its max (fp32 1e-5,
    bf16x3 1e-2); sum sse / (3 sum msum) its loss within 1e-6 relative; the launch's rgb is marf_render's
    within 1e-5."""
    import marf_hip
    inputs, _, _ = reference("small")
    m, var, eng = setup(inputs, prec, tmp_path)
    ni = m.graph.neural_image
    w = m.graph.warp_param.weight.detach().clone().requires_grad_()
    _, loss = marf_hip.render_warp_step(w, ni.progress.detach(), eng, ni._params(), m.images.rgb, m.images.masks)
    loss.backward()
    loss = loss.detach()
    with torch.no_grad():
        rgb_render = m.graph.forward(var).rgb_prediction.clone()
    out, rgb = launch(m)
    E = marf_hip.gn_tangent(w.detach(), eng.lie_batch(w.shape[0]))
    _, rhs = marf_hip.gn_system(out, E)
    dh = (2 * rhs / (3 * out[:, 1].sum())).cpu().numpy()
    want = w.grad.cpu().numpy().astype(np.float64)
    e_dh = R.err(dh, want)
    l = float(out[:, 0].sum() / (3 * out[:, 1].sum()))
    e_rgb = float((rgb - rgb_render).abs().max())
    print(prec, "dh %.2e | loss rel %.2e | rgb %.2e" % (e_dh, abs(l - float(loss)) / float(loss), e_rgb))
    assert e_dh <= bound, e_dh
    assert abs(l - float(loss)) <= 1e-6 * float(loss)
    assert e_rgb <= 1e-5
    # E against autograd of the reference's matrix exponential
    assert np.abs(E.cpu().numpy() - gn_ref.tangent(inputs[2])).max() <= 1e-5


@pytest.mark.parametrize("prec,case", [("fp32", "ragged"), ("bf16x3", "ragged"), ("bf16x3", "odd")])
def test_determinism_and_guards(prec, case, tmp_path):
    """marf_gn_normal through ctypes: two launches give bit-identical d_out; loss_only gives the full
    launch's sse / msum bits and writes nothing else; 1 MiB of guard bytes behind marf_gn_scratch_bytes
    and behind d_out stays untouched; an all-zero mask on one patch gives zeros for that patch and a
    finite delta = 0 from the solver."""
    import marf_hip
    inputs, _, _ = reference(case)
    cfg, params, warp, rgb, mask, progress = inputs
    mask = mask.copy()
    mask[1] = 0
    m, var, eng = setup((cfg, params, warp, rgb, mask, progress), prec, tmp_path)
    L = marf_hip.lib()
    dev = torch.device(DEV)
    w = m.graph.warp_param.weight.detach().contiguous()
    B = w.shape[0]
    st = marf_hip._stream(w)
    Hm = torch.empty(B, 3, 3, device=dev)
    marf_hip._check(L.marf_sl3_to_SL3(w.data_ptr(), Hm.data_ptr(), B, eng.lie_batch(B), st))
    geo = eng.grid_geo(B, Hm)
    Np = marf_hip.geo_np(eng)
    n = L.marf_gn_scratch_bytes(eng.net.handle, ctypes.byref(geo))
    assert n > 0
    guard = 1 << 20
    packed = eng.gn_packed_for(m.graph.neural_image._params())
    gt = m.images.rgb.reshape(B, 3, Np).contiguous()
    mk = m.images.masks.reshape(B, 1, Np).contiguous()
    cf = marf_hip.make_c2f(m.graph.neural_image.progress.detach(), eng.c2f)
    outs = []
    for loss_only in (0, 0, 1):
        buf = torch.full((n + guard,), 0xA5, dtype=torch.uint8, device=dev)
        out = torch.full((B * 56 * 8 + guard,), 0xA5, dtype=torch.uint8, device=dev)
        marf_hip._check(L.marf_gn_normal(eng.net.handle, ctypes.byref(geo), ctypes.byref(cf), packed.data_ptr(), gt.data_ptr(),
                                         mk.data_ptr(), loss_only, None, out.data_ptr(), buf.data_ptr(), st))
        torch.cuda.synchronize()
        assert bool((buf[n:] == 0xA5).all()) and bool((out[B * 56 * 8:] == 0xA5).all()), (prec, case, loss_only)
        outs.append(out[:B * 56 * 8].view(torch.int64).view(B, 56).clone())
    assert torch.equal(outs[0], outs[1])
    assert torch.equal(outs[2][:, :2], outs[0][:, :2])
    assert bool((outs[2][:, 2:].view(torch.uint8) == 0xA5).all())
    o = outs[0].view(torch.float64)
    assert bool(torch.isfinite(o).all()) and bool((o[1] == 0).all()) and bool(o[0, 0] > 0)
    E = marf_hip.gn_tangent(w, eng.lie_batch(B))
    A, rhs = marf_hip.gn_system(o, E)
    delta = marf_hip.gn_solve(A, rhs, torch.full((B,), 1e-3, dtype=torch.float64, device=dev))
    assert bool(torch.isfinite(delta).all()) and bool((delta[1] == 0).all()) and bool(delta[0].abs().sum() > 0)


def test_lm_iteration_launches(tmp_path):
    """One train_iteration under warp_solver: lm: marf_profile_* shows one `gn` launch (the full one), one
    `gn_loss` (the trial) and their reductions, and no mlp_step* / wgrad_* launch; var.rgb_prediction and
    the loss dict are filled."""
    import marf_hip
    import step_bits
    import time
    from util import EasyDict as edict
    inputs, _, _ = reference("small")
    m, var, eng = setup(inputs, "bf16x3", tmp_path, warp_solver="lm")
    m.timer = edict(start=time.time(), it_mean=None)
    m.train_iteration(var, step_bits._Loader())  # (packs, sizes the buffers)
    marf_hip.profile_enable(True)
    try:
        marf_hip.profile_reset()
        loss = m.train_iteration(var, step_bits._Loader())
        torch.cuda.synchronize()
        ran = marf_hip.profile_read()
    finally:
        marf_hip.profile_enable(False)
    print(sorted((k, c) for k, (_, c) in ran.items()))
    assert ran.get("gn", (0, 0))[1] == 1 and ran.get("gn_loss", (0, 0))[1] == 1 and ran.get("gn_reduce", (0, 0))[1] == 2, ran
    assert not [k for k in ran if k.startswith("mlp_step") or k.startswith("wgrad")], ran
    assert set(loss) >= {"render", "rgb", "mask", "edge", "all"} and bool(torch.isfinite(loss.all))
    assert var.rgb_prediction.shape == (2, 50 * 54, 3) and m.it == 2 and m.graph.it == 2
