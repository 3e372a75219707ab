"""The mask network's all-operands-split bf16 recipe (MARF_BF16X3A) and the mask_precision option
without a GPU: the torch emulation of the recipe (tests/mask_split_ref.py) against float64, the
library's planning for the new dtype code, the refusals, and Graph's host wiring."""
import pytest
import torch

import mask_split_ref as sr
from mask_common import fixture_opt


def _emulate(c, single=()):
    """m [B, Np, 1] and the gradients of the emulated recipe on a case (one matrix over all patches)."""
    B, Np, D = c["x32"].shape
    x = c["x32"].reshape(B * Np, D)
    m, saved = sr.forward(x, c["params"], single)
    grads = sr.backward(c["dm"].reshape(B * Np, 1), m, c["params"], saved, single)
    return m.view(B, Np, 1), grads


def _grad_errs(grads, c):
    return [float((g.double().reshape(r.shape) - r).abs().max() / r.abs().max()) for g, r in zip(grads, c["g64"])]


def test_emulated_recipe_against_float64():
    """All operands split: m <= 1e-5 abs and every gradient tensor <= 5e-4 of its max (the GPU test's bounds;
    the emulation itself sits near 1e-5).  With dz left as one bf16 -- the image net's bf16x3 -- the worst
    tensor is > 1e-3: the bound tells the two recipes apart."""
    c = sr.case("exact")
    assert c["excluded"] <= 0.25
    m, grads = _emulate(c)
    em = float((m.double() - c["m64"]).abs().max())
    errs = _grad_errs(grads, c)
    print(f"all split: m {em:.3e}, gradients {['%.2e' % e for e in errs]}")
    assert em <= 1e-5
    assert max(errs) <= 5e-4
    _, grads1 = _emulate(c, single=("dz",))
    errs1 = _grad_errs(grads1, c)
    print(f"dz single: gradients {['%.2e' % e for e in errs1]}")
    assert max(errs1) > 1e-3


def test_split_mask_net_planning_without_gpu():
    import marf_hip
    assert marf_hip.MARF_BF16X3A == 5
    n = marf_hip.MaskNet(1500, marf_hip.MARF_BF16X3A)
    assert n.param_count == 306945 and n.in_dim == 426
    # every matrix twice (hi and lo bf16 images), forward and transposed: more than one bf16 plane of each
    hi_only = 2 * (2 * 256 * 448 + 3 * 2 * 256 * 256 + 2 * 16 * 256)
    assert n.packed_bytes >= 2 * hi_only > hi_only
    g = marf_hip.grid_geometry(3, 100, 108, 50, 54, None)
    S = 3 * 2816
    # hi + lo bf16 planes of every layer input / dz: the fp32 recipe's bytes per pixel
    assert n.saved_bytes(g) >= S * (448 + 4 * 256) * 4
    assert n.workspace_bytes(g) >= S * 4 * 256 * 4
    f = marf_hip.MaskNet(1500, marf_hip.MARF_FP32)
    assert n.saved_bytes(g) == f.saved_bytes(g) and n.workspace_bytes(g) == f.workspace_bytes(g)
    bad = marf_hip.grid_geometry(3, 100, 108, 200, 54, None)
    assert n.saved_bytes(bad) == 0 and n.workspace_bytes(bad) == 0


def test_image_net_refuses_the_mask_recipe():
    import marf_hip
    with pytest.raises(RuntimeError, match="mask-network recipe"):
        marf_hip.Engine([34, 64, 64, 3], 8, marf_hip.MARF_BF16X3A, [0, 0.4], 100, 108, 50, 54)


def test_mask_precision_option(golden, tmp_path):
    from model import planar
    z = golden("mask_edges0")
    with pytest.raises(ValueError, match="fp32 or bf16x3a"):
        planar.Graph(fixture_opt(z, 0, "cpu", tmp_path, mask_precision="bf16"))
    # unset: the mask net takes `precision`, refused as before unless that is fp32
    with pytest.raises(NotImplementedError, match="fp32 only"):
        planar.Graph(fixture_opt(z, 0, "cpu", tmp_path, precision="bf16x3"))
    keys = [str(k) for k in z["state_keys"]]
    for prec, mp, code in (("bf16x3", "fp32", 0), ("fp32", "bf16x3a", 5), ("bf16x3", "bf16x3a", 5), ("fp16x2", "fp32", 0)):
        torch.manual_seed(3)
        g = planar.Graph(fixture_opt(z, 0, "cpu", tmp_path, precision=prec, mask_precision=mp))
        assert list(g.state_dict().keys()) == keys, (prec, mp)
        assert g.mask_engine("cpu").net.dtype == code
    # still refused with the option set
    with pytest.raises(NotImplementedError, match="cuda_graph.*use_implicit_mask"):
        planar.Graph(fixture_opt(z, 0, "cpu", tmp_path, precision="bf16x3", mask_precision="fp32", cuda_graph=True))
    with pytest.raises(NotImplementedError, match="build_single_masks.*CPU"):
        planar.Graph(fixture_opt(z, 0, "cpu", tmp_path, mask_precision="bf16x3a", build_single_masks=True))
