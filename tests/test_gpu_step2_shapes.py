"""precision: bf16x3 on the pixel-per-wave step kernel k_step2 at the depths, band counts, widths and tile
counts it accepts beside the headline configs' (tests/step2_shapes.py), on the GPU.

The cases are small (2 patches of 24 x 20 unless a row says otherwise: 1024 pixel slots, 8 tiles, each
patch's last tile with 96 of 128 slots valid).  Their inputs, seeds and the bounds' conditions are settled
without the kernel in tests/test_step2_shapes_cpu.py; the recipe's statement is tests/step2_ref.py.
Measured values: profiles/step2_shapes/gpu_tests.log."""
import numpy as np
import pytest
import torch

import oracle
import step2_ref as E
import step2_shapes as S
from test_gpu_bf16x3_tile import _cos, _grads
from test_gpu_dzl_recompute import _assert_equal, _saved_bytes, _step
from test_gpu_parity import DEV, _compare_step, gpu, one_step_grads, t  # noqa: F401 (gpu: fixture)

pytestmark = pytest.mark.gpu

NOC2F = "b-L20-noc2f"
KERNEL = {"bf16x3": "k_step2", "fp32": "k_mlp_step", "bf16": "k_mlp_step", "fp16": "k_mlp_step"}


def _setup(case, tmp_path, precision="bf16x3"):
    """The product's model of a case on step2_shapes.inputs(case): the same seeded init (checked), targets,
    masks, warps and progress."""
    import time
    from model import planar
    from util import EasyDict as edict
    inputs = S.inputs(case)
    cfg, params, warp, rgb, mask, progress = inputs
    c = S.CASES[case]
    torch.manual_seed(c["seed"])
    m = planar.Model(S.make_opt_for(case, tmp_path, precision))
    m.images = edict(rgb=t(rgb), masks=t(mask), masks_eroded=t(mask), edges=None, gt_hom=None, gt=None)
    m.build_networks()
    for i, (W, b) in enumerate(params):
        assert np.array_equal(m.graph.neural_image.mlp[i].weight.detach().cpu().numpy(), W)
        assert np.array_equal(m.graph.neural_image.mlp[i].bias.detach().cpu().numpy(), b)
    m.graph.warp_param.weight.data.copy_(t(warp))
    m.graph.neural_image.progress.data.fill_(progress)
    m.setup_optimizer()
    m.timer = edict(start=time.time(), it_mean=None)
    assert m.graph.neural_image.engine(torch.device(DEV)).net.step_kernel == KERNEL[precision]
    return m, edict(idx=torch.arange(c["B"]), images=m.images), inputs


def _bits_again(m, var, nl):
    """A second step repeats every bit; a no_grad eval forward returns the training forward's rgb."""
    v1, l1 = one_step_grads(m, var)
    g1, d1 = _grads(m, nl)
    rgb1 = v1.rgb_prediction.detach().clone()
    v2, l2 = one_step_grads(m, var)
    g2, d2 = _grads(m, nl)
    assert torch.equal(v2.rgb_prediction.detach().view(torch.int32), rgb1.view(torch.int32))
    assert float(l1.rgb) == float(l2.rgb)
    assert all(np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in zip(g1 + [d1], g2 + [d2]))
    with torch.no_grad():
        got = m.graph.forward(var, mode="eval").rgb_prediction
    assert torch.equal(got.reshape(-1).view(torch.int32), rgb1.reshape(-1).view(torch.int32))


# ---------------------------------------------------------------- 1. each case against the oracle and float64

@pytest.mark.parametrize("case", S.STEP_CASES)
def test_step_vs_oracle_and_float64(case, tmp_path):
    """One k_step2 step per case with the bounds of test_bf16x3_odd_width_vs_oracle / test_bf16x3_step_c2f_settings:
    rgb <= 1e-5 abs and loss <= 1e-5 rel against oracle.PlanarStep; every MLP gradient tensor and d warp <= 1e-2
    of its max against cpu_ref.CpuRefStep in float64, cosine >= 0.9999; a second step repeats every bit and the
    no_grad eval forward returns the same rgb.

    b-L20-noc2f (c2f off: every band open, the only case where bands 10..19 of the generic nk0 = 6 kernel and
    its posenc / warp adjoint carry anything): float64 cannot referee fp32 posenc arguments at open bands
    16..19 -- the reference's own fp32 arithmetic is 5.3e-2 (MLP) / 7.5e-2 (d warp) from float64 there
    (tests/test_step2_shapes_cpu.py), and so is the kernel (reported in the table, not asserted).  That case's
    MLP gradients AND d warp are held at the same 1e-2 / cosine 0.9999 against the fp32 oracle
    (oracle.PlanarStep), whose prologue is the kernel's; its MLP gradients again in test_kernel_vs_emulation.

    Measured on one MI355X: rgb against the oracle; then the worst MLP gradient tensor and d warp against
    float64 as kernel / emulated recipe (host) / the reference's own fp32:
        d2-L8         2.1e-06   4.1e-04 / 4.1e-04 / 6.8e-07   4.7e-04 / 4.7e-04 / 1.9e-07
        d2-L16        3.0e-06   5.9e-04 / 5.9e-04 / 7.7e-07   2.4e-03 / 2.4e-03 / 3.3e-06
        d3-L10        1.6e-06   7.2e-04 / 7.2e-04 / 6.8e-07   2.1e-03 / 2.0e-03 / 2.5e-07
        d4-L13        7.7e-07   2.9e-03 / 3.0e-03 / 9.5e-07   4.9e-04 / 5.3e-04 / 9.9e-07
        b-L0          4.8e-07   1.9e-03 / 1.9e-03 / 8.0e-07   2.1e-03 / 2.0e-03 / 3.5e-07
        b-L1          5.4e-07   1.6e-03 / 1.6e-03 / 1.2e-06   4.2e-03 / 4.1e-03 / 5.8e-07
        b-L4          8.9e-07   1.0e-03 / 1.0e-03 / 6.9e-07   1.1e-03 / 1.1e-03 / 4.0e-07
        b-L5          9.5e-07   4.0e-03 / 4.0e-03 / 9.5e-07   1.8e-03 / 1.8e-03 / 6.0e-07
        b-L12         1.4e-06   3.2e-03 / 3.2e-03 / 3.7e-07   1.6e-03 / 1.6e-03 / 6.9e-07
        b-L17         1.8e-06   4.7e-04 / 4.7e-04 / 7.9e-07   1.6e-03 / 1.9e-03 / 2.4e-06
        b-L20         2.0e-06   8.0e-04 / 8.0e-04 / 2.0e-06   3.3e-03 / 3.3e-03 / 2.0e-05
        b-L21         2.0e-06   9.1e-04 / 9.1e-04 / 3.5e-06   4.4e-04 / 5.9e-04 / 7.1e-06
        b-L32         1.9e-06   8.8e-04 / 9.6e-04 / 1.9e-06   1.6e-03 / 1.5e-03 / 4.1e-06
        b-L20-noc2f   4.5e-07   5.3e-02 / 5.3e-02 / 5.3e-02   7.7e-02 / 7.8e-02 / 5.4e-02   (reported; held against
                                  the fp32 oracle: kernel 1.8e-3 / 1.4e-3, cosine 0.999998 / 1.000000)
        n-L0          4.5e-07   2.4e-03 / 2.4e-03 / 8.1e-07   1.2e-03 / 1.2e-03 / 4.8e-07
        n-L17         2.0e-06   1.0e-03 / 1.0e-03 / 4.8e-07   2.1e-03 / 2.2e-03 / 2.1e-06
        n-L32         2.0e-06   1.0e-03 / 1.0e-03 / 2.6e-06   1.3e-03 / 1.3e-03 / 2.3e-06
        w-32          2.3e-06   2.8e-04 / 2.8e-04 / 6.3e-07   2.4e-04 / 2.5e-04 / 5.1e-07
        w-32x4        3.3e-07   8.5e-04 / 8.5e-04 / 5.5e-07   3.6e-03 / 3.7e-03 / 5.7e-07
        w-48-40       2.1e-06   1.5e-03 / 1.5e-03 / 3.8e-07   2.3e-03 / 2.3e-03 / 9.5e-07
        w-100-33-7    6.0e-07   9.9e-04 / 9.9e-04 / 2.1e-07   1.9e-03 / 1.9e-03 / 3.9e-07
        w-256-64-256  6.0e-07   5.0e-03 / 1.8e-03 / 5.1e-07   3.9e-03 / 4.0e-03 / 7.8e-07   (2.5 % of its pixels
                                                       at a ReLU kink; 8.2e-5 of the emulation once those are masked)
        w-256x3-32    3.0e-07   3.4e-03 / 4.1e-03 / 6.7e-07   1.9e-03 / 1.9e-03 / 5.9e-07
        w-64-256      1.0e-06   3.2e-03 / 3.2e-03 / 8.3e-07   1.7e-03 / 1.8e-03 / 3.4e-07
        t-3x16x20     1.3e-06   1.6e-03 / 1.6e-03 / 9.0e-07   1.8e-03 / 1.6e-03 / 5.0e-07
        t-1x24x20     1.1e-06   2.2e-03 / 2.4e-03 / 8.1e-07   1.9e-03 / 1.9e-03 / 1.4e-07
    loss <= 2.6e-7 rel, cosine >= 0.999994 everywhere but the c2f-off case."""
    nl = len(S.CASES[case]["hidden"]) + 1
    m, var, inputs = _setup(case, tmp_path)
    o = _compare_step(m, var, inputs, "bf16x3", nl)
    print("STEP", case, "rgb %.2e loss %.2e | kernel grads %.2e dh %.2e cos %.6f / %.6f | ref32 grads %.2e dh %.2e" %
          (o["rgb"], o["loss"], o["grad_err"], o["dh_err"], o["grad_cos"], o["dh_cos"], o["grad_err_ref32"], o["dh_err_ref32"]))
    assert o["rgb"] <= 1e-5 and o["loss"] <= 1e-5, o
    if case != NOC2F:
        assert o["grad_err"] <= 1e-2 and o["dh_err"] <= 1e-2, o
        assert o["grad_cos"] >= 0.9999 and o["dh_cos"] >= 0.9999, o
    else:  # (the fp32 oracle, whose prologue is the kernel's, in float64's place: the docstring)
        cfg, params, warp, rgb, mask, progress = inputs
        st = oracle.PlanarStep(cfg, params, warp, rgb, mask)
        st.progress = np.float32(progress)
        r = st.step()
        ours, dh = _grads(m, nl)
        ref = E.flat(r)
        ge, gc = max(E.err(a, b) for a, b in zip(ours, ref)), min(_cos(a, b) for a, b in zip(ours, ref))
        de, dc = E.err(dh, r["dh"]), _cos(dh, r["dh"])
        print("STEP", case, "against the fp32 oracle: kernel grads %.2e dh %.2e cos %.6f / %.6f" % (ge, de, gc, dc))
        assert ge <= 1e-2 and de <= 1e-2, (ge, de)
        assert gc >= 0.9999 and dc >= 0.9999, (gc, dc)
    _bits_again(m, var, nl)


@pytest.mark.parametrize("case", S.STEP_CASES)
def test_fp32_control(case, tmp_path):
    """The same case in fp32 on the tile kernel k_mlp_step with test_c3_two_patch_step_vs_oracle's fp32 bounds:
    rgb <= 1e-5, loss <= 1e-6, gradients <= max(1e-5, 2 x the reference's own fp32 error).  A failure here is a
    finding about the tile kernel or the checker, not about k_step2.  (The tile kernels' first 2-layer,
    L > 16 and L = 0 shapes.)  Measured: rgb <= 1.8e-7, loss <= 9.2e-8; gradients under 1e-5 or about at the reference's
    own fp32 error (kernel / reference, worst MLP tensor: 1.3e-7..4.0e-7 / 2.1e-7..1.2e-6 up to L = 17;
    2.1e-6 / 2.0e-6 at L = 20, 3.4e-6 / 3.5e-6 at L = 21, 5.3e-2 / 5.3e-2 with c2f off at L = 20; d warp at most
    1.5 x the reference's: 3.4e-6 / 2.3e-6 at n-L32)."""
    nl = len(S.CASES[case]["hidden"]) + 1
    m, var, inputs = _setup(case, tmp_path, "fp32")
    o = _compare_step(m, var, inputs, "fp32", nl)
    print("FP32", case, "rgb %.2e loss %.2e | kernel grads %.2e dh %.2e | ref32 grads %.2e dh %.2e" %
          (o["rgb"], o["loss"], o["grad_err"], o["dh_err"], o["grad_err_ref32"], o["dh_err_ref32"]))
    assert o["rgb"] <= 1e-5 and o["loss"] <= 1e-6, o
    assert o["grad_err"] <= max(1e-5, 2 * o["grad_err_ref32"]), o
    assert o["dh_err"] <= max(1e-5, 2 * o["dh_err_ref32"]), o


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
@pytest.mark.parametrize("case", S.PLAIN16)
def test_plain_16_bit(case, precision, tmp_path):
    """d2-L8 and L = 0, 20, 32 on [256, 256] in plain bf16 / fp16 (k_mlp_step) with test_small_step_bf16's bounds
    against the fp32 oracle: rgb 1e-2 abs, loss 2e-2 rel, every MLP weight gradient's cosine > 0.99.  Measured
    (rgb / loss / smallest cosine), bf16: d2-L8 9.3e-4 / 1.5e-4 / 0.99999, b-L0 2.2e-4 / 1.1e-5 / 0.99902, b-L20
    9.4e-4 / 7.5e-6 / 0.99990, b-L32 9.5e-4 / 1.3e-4 / 0.99974; fp16: 1.3e-4 / 2.2e-5 / 1.00000, 2.7e-5 / 1.2e-6 /
    0.99993, 1.2e-4 / 7.8e-6 / 0.99999, 1.6e-4 / 1.4e-5 / 0.99995."""
    nl = len(S.CASES[case]["hidden"]) + 1
    m, var, inputs = _setup(case, tmp_path, precision)
    cfg, params, warp, rgb, mask, progress = inputs
    var, loss = one_step_grads(m, var)
    st = oracle.PlanarStep(cfg, params, warp, rgb, mask)
    st.progress = np.float32(progress)
    r = st.step()
    got = var.rgb_prediction.detach().cpu().numpy().reshape(-1, 3)
    cos = [_cos(m.graph.neural_image.mlp[i].weight.grad.cpu().numpy(), r["grads"][i][0]) for i in range(nl)]
    print("P16", case, precision, "rgb %.2e loss %.2e min cos %.5f" %
          (np.abs(got - r["rgb"]).max(), abs(float(loss.rgb) / float(r["loss_rgb"]) - 1), min(cos)))
    np.testing.assert_allclose(got, r["rgb"], atol=1e-2, rtol=0)
    np.testing.assert_allclose(float(loss.rgb), r["loss_rgb"], rtol=2e-2)
    assert min(cos) > 0.99, (case, precision, cos)


@pytest.mark.parametrize("case", S.PREDICT)
def test_predict_entire_image_vs_oracle(case, tmp_path):
    """Model.predict_entire_image (explicit coordinates, the forward-only launch) on a 13 x 11 canvas: 143
    pixels, one ragged tile; 1e-5 abs against the oracle's forward (test_predict_entire_image_deep_vs_oracle).
    Measured: d2-L8 2.0e-6, b-L20 1.6e-6, w-100-33-7 4.2e-7."""
    import cpu_ref
    from model import planar
    from test_gpu_parity import make_opt
    c = S.CASES[case]
    opt = make_opt(tmp_path, H=13, W=11, patch_H=8, patch_W=8, batch_size=2, precision="bf16x3", use_edges=False,
                   arch=S.arch(case), barf_c2f=None if c["c2f"] is None else list(c["c2f"]))
    torch.manual_seed(c["seed"])
    m = planar.Model(opt)
    m.build_networks()
    m.graph.neural_image.progress.data.fill_(c["progress"])
    assert m.graph.neural_image.engine(torch.device(DEV)).net.step_kernel == "k_step2"
    img = m.predict_entire_image()
    assert tuple(img.shape) == (3, 13, 11)
    params = [(l.weight.detach().cpu().numpy(), l.bias.detach().cpu().numpy()) for l in m.graph.neural_image.mlp]
    xy = cpu_ref.pixel_grid(13, 11, 0, 0, crop=False).numpy()
    w = oracle.c2f_weights(np.float32(c["progress"]), None if c["c2f"] is None else list(c["c2f"]), c["L"])
    _, ref = oracle.mlp_forward(oracle.posenc_features(xy, c["L"], w), params)
    got = img.permute(1, 2, 0).reshape(-1, 3).cpu().numpy()
    print("PREDICT", case, "%.2e" % np.abs(got - ref).max())
    assert np.abs(got - ref).max() <= 1e-5, np.abs(got - ref).max()


# ---------------------------------------------------------------- 2. the kernel against a statement of its recipe

@pytest.mark.parametrize("case", S.EMU_CASES + [NOC2F])
def test_kernel_vs_emulation(case, tmp_path):
    """The kernel against the emulated recipe (tests/step2_ref.py), as test_gpu_bf16x3_tile's
    test_step_vs_oracle_and_emulation holds the tile kernel: the mask of the emulation's kink pixels (factor 4)
    zeroed, kernel and emulation on that mask, and on every MLP gradient tensor kernel-vs-emulation <=
    sqrt(E_sum E_drop), E_sum the emulation's float32 against float64 accumulation and E_drop the emulation
    without W_l^T dz in the dgrad, both from the emulation alone.  Every case is held (E_drop >= 10 E_sum,
    >= 256 pixels left, <= 50 % left out: asserted here and, without the kernel, in
    tests/test_step2_shapes_cpu.py; a case that were not held fails).  Not applied to d warp (its float32 sum
    over the tile's pixels and the dH partials has no counterpart in E_sum).  c1x2-64 is [256] * 4 at L = 8 on
    2 patches of 64 x 64: the benchmarked instantiation.  b-L20-noc2f, beyond the eight: the open bands 16..19
    (columns 64..79 of feat_0, which the layer-0 weight gradient read unwritten before it refused L > 16).

    The emulation runs on the host, so its inputs and bound are the ones tests/test_step2_shapes_cpu.py checks,
    and takes the prologue's values from the oracle (step2_ref.features): torch's float32 prologue differs
    from the kernel's on some hosts by an amount that doubles per band, as a last-place difference of a warped
    coordinate would (measured at b-L20-noc2f on torch's prologue: 2.3e-2 on the gradients against 4.7e-4 of bound).

    Measured on one MI355X (kink share / pixels left / E_sum / E_drop / bound / kernel vs emulation):
        d2-L8         0.0 % /  822 / 4.8e-6 / 1.9e-3 / 9.5e-5 / 4.6e-6
        d3-L10        0.6 % /  841 / 4.2e-5 / 2.5e-3 / 3.3e-4 / 4.4e-5
        d4-L13        0.5 % /  842 / 3.1e-4 / 4.3e-3 / 1.2e-3 / 2.4e-4
        w-256-64-256  2.5 % /  798 / 5.4e-5 / 2.6e-3 / 3.7e-4 / 8.2e-5
        w-100-33-7    0.1 % /  821 / 3.3e-5 / 4.5e-3 / 3.8e-4 / 5.6e-5
        b-L20         0.6 % /  817 / 4.4e-5 / 2.3e-3 / 3.2e-4 / 5.0e-5
        b-L0          0.5 % /  842 / 1.1e-4 / 4.3e-3 / 6.8e-4 / 2.7e-4
        c1x2-64       6.0 % / 6548 / 6.7e-5 / 4.0e-3 / 5.1e-4 / 8.5e-5
        b-L20-noc2f   0.7 % /  815 / 7.8e-5 / 2.4e-3 / 4.4e-4 / 7.1e-5
    all held; the kernel is 1 to 2.5 times E_sum from the emulation (its own fp32 summation order) and 2.5 to
    20 times inside the bound.  b-L0 has the least headroom (2.7e-4 against 6.8e-4, 2.5 x E_sum).  E_sum, and
    with it the bound, depends on the host's torch: at b-L0 1.46e-4 on one host and 1.08e-4 on another (bound
    8.0e-4 / 6.8e-4)."""
    nl = len(S.CASES[case]["hidden"]) + 1
    m, var, inputs = _setup(case, tmp_path)
    hb = E.held_bound(inputs, "cpu")
    assert hb["left"] >= 256 and hb["out"] <= 0.5, (case, hb["left"], hb["out"])
    m.images.masks = m.images.masks_eroded = t(hb["inputs"][4])
    one_step_grads(m, var)
    ours, _ = _grads(m, nl)
    per = [E.err(a, b) for a, b in zip(ours, E.flat(hb["emu"]))]
    print("EMU", case, "kink %.3f left %d E_sum %.2e E_drop %.2e bound %.2e kernel vs emulation %.2e" %
          (hb["out"], hb["left"], hb["e_sum"], hb["e_drop"], hb["bound"], max(per)), ["%.1e" % x for x in per])
    assert hb["held"], ("not held", case, hb["e_sum"], hb["e_drop"])
    assert max(per) <= hb["bound"], (case, per, hb["bound"])


# ---------------------------------------------------------------- 3. the A/B switches at the new shapes

_DZL = [("d3-L10", True), ("d4-L13", True), ("d2-L8", False)]
_F0 = [(c, True) for c in ("d2-L8", "b-L5")] + [(c, False) for c in ("b-L17", "b-L20", NOC2F, "b-L4", "b-L21")]
SWITCHES = ([("MARF_DZL_RECOMPUTE", "0", c, mv) for c, mv in _DZL] + [("MARF_F0_RECOMPUTE", "0", c, mv) for c, mv in _F0] +
            [("MARF_WGRAD_FUSED", "0", c, None) for c in ("d2-L8", "d3-L10", "w-256-64-256")] +
            [("MARF_STEP2_GENERIC", "1", c, None) for c in S.DEPTH])


@pytest.mark.parametrize("switch,value,case,moves", SWITCHES, ids=[f"{s[5:]}-{c}" for s, _, c, _ in SWITCHES])
def test_switch_gives_the_default_bits(switch, value, case, moves, tmp_path, monkeypatch):
    """Each A/B switch of the library gives the default path's bits at the new shapes: torch.equal on rgb, loss,
    every MLP gradient and d warp.  MARF_DZL_RECOMPUTE=0 moves dz_{n-1} into the saved bytes at 3 and 4 layers
    (asserted: the two runs took different paths) and nothing at 2 (the mode is off there).  MARF_F0_RECOMPUTE=0
    changes no saved byte at any shape (feat_0's rows are planned either way), so its paths show in the results
    alone: feat_0 is recomputed by default at d2-L8 and L = 5, and stored with or without the switch at L = 4,
    21 and, since the recomputing stage builds 16 bands only, at L = 17 and 20 -- there the switch is the
    regression test of that refusal (before it, the default path's layer-0 gradient read columns 64..79
    unwritten and was NaN: profiles/step2_shapes/parent_ab.log)."""
    for v in ("MARF_DZL_RECOMPUTE", "MARF_F0_RECOMPUTE", "MARF_WGRAD_FUSED", "MARF_STEP2_GENERIC"):
        monkeypatch.delenv(v, raising=False)
    m, var, _ = _setup(case, tmp_path)
    ref, b0 = _step(m, var), _saved_bytes(m)
    monkeypatch.setenv(switch, value)
    b1 = _saved_bytes(m)
    got = _step(m, var)
    _assert_equal(got, ref, (switch, case))
    if switch == "MARF_DZL_RECOMPUTE" and moves:
        c = S.CASES[case]
        slots = c["B"] * -(-c["ph"] * c["pw"] // 128) * 128
        assert b1 - b0 >= slots * (512 - 48) - 65536, (b0, b1, slots)
    else:
        assert b1 == b0, (switch, case, b0, b1)


@pytest.mark.parametrize("grid", [1, 2])
def test_tile_grouping_invariance_nine_tiles(grid, tmp_path, monkeypatch):
    """d3-L10 on 3 patches of 16 x 20 (9 tiles) with every tile on one block and on two (MARF_STEP2_GRID): as
    test_step2_tile_grouping_invariance, rgb, d warp and every gradient but the last layer's are bit-identical
    to the one-tile-per-block default; the last layer's gradients and the loss, block-partial sums, agree to
    summation order under that test's bounds."""
    monkeypatch.delenv("MARF_STEP2_GRID", raising=False)
    m, var, _ = _setup("t-3x16x20", tmp_path)
    a = _step(m, var)
    monkeypatch.setenv("MARF_STEP2_GRID", str(grid))
    b = _step(m, var)
    last = ("dW2", "db2", "loss")
    bad = sorted(k for k in a if k not in last and not torch.equal(a[k], b[k]))
    assert not bad, (grid, bad)
    for k in last[:2]:
        assert torch.allclose(a[k], b[k], rtol=1e-4, atol=1e-7 * float(a[k].abs().max())), (k, (a[k] - b[k]).abs().max().item())
    assert abs(float(a["loss"]) - float(b["loss"])) <= 1e-6 * abs(float(a["loss"]))


@pytest.mark.parametrize("case", S.DZ_CASES)
def test_split_dz_kernel(case, tmp_path, monkeypatch):
    """k_step2dz (MARF_STEP2_DZ=1 at net creation) at 3 layers, at Kl = 64 between 256-wide layers and at L = 20:
    rgb and loss bit-identical to the default recipe's; the gradients within part 1's bounds (1e-2 of the
    tensor's max against float64, cosine >= 0.9999).  Measured (worst MLP tensor / d warp; k_step2's in
    brackets): d3-L10 7.4e-4 / 1.4e-3 (7.2e-4 / 2.1e-3), w-256-64-256 5.0e-3 / 2.2e-3 (5.0e-3 / 3.9e-3), b-L20
    7.7e-4 / 2.3e-3 (8.0e-4 / 3.3e-3)."""
    nl = len(S.CASES[case]["hidden"]) + 1
    monkeypatch.delenv("MARF_STEP2_DZ", raising=False)
    m0, var0, _ = _setup(case, tmp_path / "a")
    ref = _step(m0, var0)
    monkeypatch.setenv("MARF_STEP2_DZ", "1")
    m, var, inputs = _setup(case, tmp_path / "b")
    o = _compare_step(m, var, inputs, "bf16x3", nl)
    got = _step(m, var)
    print("DZ", case, "kernel grads %.2e dh %.2e cos %.6f / %.6f" % (o["grad_err"], o["dh_err"], o["grad_cos"], o["dh_cos"]))
    assert torch.equal(got["rgb"], ref["rgb"]) and torch.equal(got["loss"], ref["loss"])
    assert o["rgb"] <= 1e-5 and o["loss"] <= 1e-5, o
    assert o["grad_err"] <= 1e-2 and o["dh_err"] <= 1e-2 and o["grad_cos"] >= 0.9999 and o["dh_cos"] >= 0.9999, o
