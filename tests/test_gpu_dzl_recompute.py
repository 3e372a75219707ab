"""dz_{n-1} recomputed by the weight gradient of layer n-2 instead of stored and read (DESIGN.md
§3.4, marf_abi.hip dzl_recompute): the mode changes where the bf16 words of dz_{n-1} come from, never
their bits, so every result of a step is bit-identical with the mode on (the default for 256-wide
split-recipe nets) and off (MARF_DZL_RECOMPUTE=0).  The golden bits of the default path are
test_gpu_parity.py's test_step2_bits_unchanged / test_c3_headline_step, which run with the mode on.
"""
import ctypes
import time

import numpy as np
import pytest
import torch

import step_bits

pytestmark = pytest.mark.gpu

DEV = step_bits.DEV
SWITCH = "MARF_DZL_RECOMPUTE"


def _build(B, ph, pw, L, hidden, out="/tmp/marf_dzl", **over):
    """A seeded bf16x3 model on B patches of ph x pw (512 x 512 canvas), as step_bits.build_case."""
    from model import planar
    from util import EasyDict as edict
    opt = step_bits._opt(out, H=512, W=512, patch_H=ph, patch_W=pw, batch_size=B, use_edges=False,
                         arch={"layers": [None] + list(hidden) + [3], "skip": [], "posenc": {"L_2D": L}}, **over)
    torch.manual_seed(3)
    m = planar.Model(opt)
    rng = np.random.default_rng(3)
    yy, xx = np.meshgrid(np.linspace(0, 1, ph), np.linspace(0, 1, pw), indexing="ij")
    rgb = np.stack([[0.5 + 0.4 * np.sin(2 * np.pi * (rng.uniform(1, 4) * xx + rng.uniform(1, 4) * yy) + rng.uniform(0, 6))
                     for _ in range(3)] for _ in range(B)]).astype(np.float32)
    mask = (rng.random((B, 1, ph, pw)) < 0.85).astype(np.float32)
    warp = (rng.standard_normal((B, 8)) * 0.01).astype(np.float32)
    mk = torch.from_numpy(mask).to(DEV)
    m.images = edict(rgb=torch.from_numpy(rgb).to(DEV), masks=mk, masks_eroded=mk, edges=None, gt_hom=None, gt=None)
    m.build_networks()
    m.graph.warp_param.weight.data.copy_(torch.from_numpy(warp).to(DEV))
    m.graph.neural_image.progress.data.fill_(0.2)
    m.setup_optimizer()
    m.timer = edict(start=time.time(), it_mean=None)
    return m, edict(idx=torch.arange(B), images=m.images)


def _step(m, var):
    """rgb, loss, every MLP gradient and d warp of one fused step (the state is left as it was)."""
    m.optim.zero_grad()
    v = m.graph.forward(var, mode="train")
    loss = m.summarize_loss(m.graph.compute_loss(v, mode="train"))
    loss.all.backward()
    out = {"rgb": v.rgb_prediction.detach().clone(), "loss": loss.rgb.detach().reshape(1).clone(),
           "dh": m.graph.warp_param.weight.grad.detach().clone()}
    for i, lay in enumerate(m.graph.neural_image.mlp):
        out[f"dW{i}"] = lay.weight.grad.detach().clone()
        out[f"db{i}"] = lay.bias.grad.detach().clone()
    return out


def _saved_bytes(m):
    """The step's saved-tensor bytes under the current switches (the mode shows in them: dz_{n-1}
    takes 512 B per pixel slot, what replaces it 48 B)."""
    import marf_hip
    eng = m.graph.neural_image.engine(torch.device(DEV))
    assert eng.net.step_kernel == "k_step2"
    Hm = torch.zeros(m.batch_size, 3, 3, device=DEV)
    geo = eng.grid_geo(m.batch_size, Hm)
    return marf_hip.lib().marf_step_saved_bytes(eng.net.handle, ctypes.byref(geo))


def _assert_equal(a, b, tag):
    bad = sorted(k for k in a if not torch.equal(a[k], b[k]))
    assert not bad, (tag, bad)
    assert all(torch.isfinite(v).all() for v in a.values()), tag


# 2 x 40x52: 2,080 pixels per patch, not a multiple of the 128-pixel tile (padded pixel slots, a
#   mostly empty last tile and weight-gradient chunk), one tile per block;
# 3 x 128^2, L = 16: 384 tiles on the persistent blocks -- half of them take one tile, so their dgrad
#   pass runs its second pixel set on zeros into the sink sets;
# 2 x 100^2, L = 16: 158 tiles, one per block, every block's second set a sink set
_SHAPES = {"pad": (2, 40, 52, 8), "odd": (3, 128, 128, 16), "1tile": (2, 100, 100, 16)}
_VARIANTS = {"default": None, "generic": ("MARF_STEP2_GENERIC", "1"), "perlayer": ("MARF_WGRAD_FUSED", "0")}
_off_ref = {}


def _off_reference(shape, monkeypatch):
    """The saved path's step of a shape (computed once, shared by the variants that run it)."""
    if shape not in _off_ref:
        m, var = _build(*_SHAPES[shape], [256] * 4)
        on_bytes = _saved_bytes(m)
        monkeypatch.setenv(SWITCH, "0")
        off_bytes = _saved_bytes(m)
        _off_ref[shape] = (m, var, _step(m, var), on_bytes, off_bytes)
        monkeypatch.delenv(SWITCH)
    return _off_ref[shape]


@pytest.mark.parametrize("shape,variant", [("pad", "default"), ("odd", "default"), ("1tile", "default"),
                                           ("odd", "generic"), ("odd", "perlayer")])
def test_on_equals_off(shape, variant, monkeypatch):
    """One step with dz_{n-1} recomputed (default) against the same step with it stored and read:
    torch.equal on rgb, loss, every MLP gradient and d warp; "generic" / "perlayer": the mode on
    under the generic step kernel / the per-layer weight-gradient launches.  The saved bytes show
    that the two runs did take different paths (dz_{n-1} is not allocated with the mode on)."""
    m, var, ref, on_bytes, off_bytes = _off_reference(shape, monkeypatch)
    B, ph, pw, _ = _SHAPES[shape]
    slots = B * (-(-ph * pw // 128) * 128)
    assert off_bytes - on_bytes >= slots * (512 - 48) - 65536, (on_bytes, off_bytes, slots)
    if _VARIANTS[variant]:
        monkeypatch.setenv(*_VARIANTS[variant])
    got = _step(m, var)
    _assert_equal(got, ref, (shape, variant))
    # a rerun from the same state is bit-identical
    _assert_equal(_step(m, var), got, (shape, variant, "rerun"))


def test_narrow_net_falls_back(monkeypatch):
    """Hidden widths [128, 96, 128] (the generic kernel on narrow layers) keep the saved path: the
    same saved bytes and the same bits with the switch on and off (its golden bits:
    test_switch_off_bits[narrow] and test_step2_bits_unchanged[narrow])."""
    m, var = _build(2, 64, 64, 8, [128, 96, 128])
    on_bytes, got = _saved_bytes(m), _step(m, var)
    monkeypatch.setenv(SWITCH, "0")
    assert _saved_bytes(m) == on_bytes
    _assert_equal(_step(m, var), got, "narrow")


@pytest.mark.parametrize("case", ["c1", "c3x2", "L16-1tile", "narrow"])
def test_switch_off_bits(case, monkeypatch):
    """MARF_DZL_RECOMPUTE=0 (dz_{n-1} stored and read) still computes the pinned bits of
    tests/golden/step2_bits.json."""
    import json
    monkeypatch.setenv(SWITCH, "0")
    ref = json.load(open(step_bits.BITS_JSON))["cases"][case]
    got = step_bits.case_bits(case)
    bad = sorted(k for k in ref["bits"] if got["bits"].get(k) != ref["bits"][k])
    assert not bad, (case, got["kernel"], bad)


def test_captured_step_matches_eager_mode_on(tmp_path, monkeypatch):
    """Model.captured_step (the whole iteration recorded as a HIP graph and replayed) against the
    eager iteration with the mode on, on the C1 batch (5 x 180x240, L = 8, use_edges off), as
    test_captured_step_matches_eager: after 5 iterations the losses, warps and every MLP weight are
    bit-identical.  (Nothing is decided inside the capture: the mode comes from the buffer plan.)"""
    from model import planar
    from util import EasyDict as edict
    imgs = np.load(step_bits.GOLDEN + "/cat_batch3_c1.npz", allow_pickle=False)
    res = {}
    for mode in ("eager", "graph"):
        opt = step_bits._opt(str(tmp_path / mode), use_edges=False, cuda_graph=(mode == "graph"))
        torch.manual_seed(3)
        m = planar.Model(opt)
        rgb = torch.from_numpy(imgs["rgb"].astype(np.float32) / np.float32(255)).to(DEV)
        mask = torch.from_numpy(imgs["mask"].astype(np.float32)).to(DEV)
        m.images = edict(rgb=rgb, masks=mask, masks_eroded=mask, edges=None, gt_hom=None, gt=None)
        m.build_networks()
        m.setup_optimizer()
        m.timer = edict(start=time.time(), it_mean=None)
        var = edict(idx=torch.arange(5), images=m.images)
        losses = []
        for _ in range(5):
            losses.append(float(m.train_iteration(var, step_bits._Loader()).rgb))
            m.graph.warp_param.weight.data[0] = 0
        assert (m._step_graph is not None) == (mode == "graph")
        res[mode] = (losses, m.graph.warp_param.weight.detach().cpu(),
                     [p.detach().cpu() for p in m.graph.neural_image.mlp.parameters()], _saved_bytes(m))
    (la, wa, pa, ba), (lb, wb, pb, bb) = res["eager"], res["graph"]
    monkeypatch.setenv(SWITCH, "0")
    assert ba == bb < _saved_bytes(m), (ba, bb)  # (both ran with dz_4 not allocated)
    assert la == lb, (la, lb)
    assert torch.equal(wa.view(torch.int32), wb.view(torch.int32))
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(pa, pb))
