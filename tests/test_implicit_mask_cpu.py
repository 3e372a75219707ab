"""The learned implicit mask without a GPU: the torch restatement (tests/mask_ref.py) against the
reference fixtures, the construction order (seeded init) and state-dict surface of Graph, the mask
net's planning in the library, the refused configurations, and the unchanged default path."""
import numpy as np
import pytest
import torch

import mask_ref
from mask_common import LOSS_KEYS, MASK_PARAM_NAMES, fixture_model, fixture_opt


@pytest.fixture(scope="module", params=[0, 1], ids=["edges_off", "edges_on"])
def fx(request, golden):
    return request.param, golden(f"mask_edges{request.param}")


@pytest.fixture(scope="module")
def graph0(golden, tmp_path_factory):
    """Graph of the fixture's options on the CPU under seed 3 (construction only: no kernel runs)."""
    z = golden("mask_edges0")
    return fixture_model(z, 0, "cpu", tmp_path_factory.mktemp("mask_cpu")).graph


def _grad_close(got, z, name, rel):
    key = "grad0_" + name
    if key in z.files:
        ref = z[key]
        assert np.abs(got - ref).max() <= rel * np.abs(ref).max(), name
    else:
        amax = float(z[key + "_absmax"])
        assert np.abs(got[::7, ::5] - z[key + "_sub"]).max() <= rel * amax, name
        assert np.abs(got.sum(1) - z[key + "_rowsum"]).max() <= rel * amax * got.shape[1], name
        assert np.abs(got.sum(0) - z[key + "_colsum"]).max() <= rel * amax * got.shape[0], name


def test_state_dict_and_seeded_init_match_the_reference(graph0, golden):
    """Keys, shapes and the seed-3 init checksums of implicit_mask.* and embedding_view.weight: the
    modules are built in the reference's order (model/planar.py:303-327), which is the RNG order."""
    z = golden("mask_edges0")
    sd = graph0.state_dict()
    assert list(sd.keys()) == [str(k) for k in z["state_keys"]]
    keys = [str(k) for k in z["init_keys"]]
    assert keys == ["implicit_mask." + n for n in MASK_PARAM_NAMES] + ["embedding_view.weight"]
    for k, shp, s, a in zip(keys, z["init_shapes"], z["init_sum"], z["init_abssum"]):
        assert ",".join(str(d) for d in sd[k].shape) == str(shp), k
        assert float(sd[k].double().sum()) == pytest.approx(float(s), rel=1e-12, abs=1e-12), k
        assert float(sd[k].double().abs().sum()) == pytest.approx(float(a), rel=1e-12), k
    assert np.array_equal(sd["embedding_view.weight"][:2].numpy(), z["embed_rows01"])
    assert sum(p.numel() for p in graph0.implicit_mask.parameters()) == 306945
    assert graph0.embedding_uv.freqs.tolist() == [2.0 ** k for k in range(10)]


def test_mask_ref_matches_the_reference(fx, graph0):
    """mask_ref in float32 on the reference's seed-3 state: m, the losses and the mask-net gradients
    of step 0 within 1e-6 (relative to each tensor's max)."""
    use_edges, z = fx
    H, W, PH, PW, B = (int(v) for v in z["cfg"][:5])
    params = [p.detach().clone().requires_grad_() for p in graph0.implicit_mask.parameters()]
    embed = graph0.embedding_view.weight.detach()
    rgb = torch.from_numpy(z["rgb"])
    index = rgb.long().reshape(B, 3, -1)
    assert set(index.unique().tolist()) == {0, 1}  # both vocabulary rows occur
    m = mask_ref.predict(index, embed, mask_ref.crop_grid(H, W, PH, PW), params)
    assert np.abs(m.detach().numpy() - z["m0"]).max() <= 1e-6
    m_map = m.view(B, PH, PW, 1).permute(0, 3, 1, 2)
    pred = torch.from_numpy(z["rgb_pred0"]).view(B, PH, PW, 3).permute(0, 3, 1, 2)
    edges = torch.from_numpy(z["edges"])
    ls = mask_ref.losses(pred, rgb, m_map, float(z["cfg"][7]) if use_edges else 0,
                         torch.zeros_like(edges) if use_edges else None, edges if use_edges else None)
    for k in LOSS_KEYS:
        if ls[k] is not None:
            assert float(ls[k].detach()) == pytest.approx(float(z["loss0_" + k]), rel=1e-6), k
    ls["all"].backward()
    for name, p in zip(MASK_PARAM_NAMES, params):
        _grad_close(p.grad.numpy(), z, name, 1e-6)


def test_mask_net_planning_without_gpu():
    import marf_hip
    n = marf_hip.MaskNet(1500, marf_hip.MARF_FP32)
    assert n.param_count == 426 * 256 + 256 + 3 * (256 * 256 + 256) + 256 + 1 == 306945
    assert n.in_dim == 426 and n.packed_bytes > 0
    # plain bf16 missed the 1e-2 gradient bound: every other recipe is refused by message
    for dt in (marf_hip.MARF_BF16, marf_hip.MARF_BF16X3, marf_hip.MARF_FP16, marf_hip.MARF_FP16X2):
        with pytest.raises(RuntimeError, match="fp32 only"):
            marf_hip.MaskNet(1500, dt)
    g = marf_hip.grid_geometry(3, 100, 108, 50, 54, None)
    S = 3 * 2816  # 2700 pixels per patch padded to 128
    assert n.saved_bytes(g) >= S * (448 + 4 * 256) * 4
    assert n.workspace_bytes(g) >= S * 4 * 256 * 4
    with pytest.raises(RuntimeError, match="N_vocab"):
        marf_hip.MaskNet(0, marf_hip.MARF_FP32)
    with pytest.raises(RuntimeError, match="dtype"):
        marf_hip.MaskNet(8, 9)
    with pytest.raises(RuntimeError, match="embedding width"):
        marf_hip.MaskNet(8, marf_hip.MARF_FP32, embed_dim=130)
    with pytest.raises(RuntimeError, match="hidden width"):
        marf_hip.MaskNet(8, marf_hip.MARF_FP32, width=250)
    with pytest.raises(RuntimeError, match="512"):
        marf_hip.MaskNet(8, marf_hip.MARF_FP32, embed_dim=256)
    with pytest.raises(RuntimeError, match="n_layers"):
        marf_hip.MaskNet(8, marf_hip.MARF_FP32, n_layers=1)
    bad = marf_hip.grid_geometry(3, 100, 108, 200, 54, None)  # a crop larger than the canvas
    assert n.saved_bytes(bad) == 0 and n.workspace_bytes(bad) == 0


def test_refused_configurations(golden, tmp_path, monkeypatch):
    from model import planar
    z = golden("mask_edges0")
    with pytest.raises(NotImplementedError, match="build_single_masks.*CPU"):
        planar.Graph(fixture_opt(z, 0, "cpu", tmp_path, build_single_masks=True))
    with pytest.raises(NotImplementedError, match="cuda_graph.*use_implicit_mask"):
        planar.Graph(fixture_opt(z, 0, "cpu", tmp_path, cuda_graph=True))
    for prec in ("bf16", "bf16x3", "fp16", "fp16x2"):
        with pytest.raises(NotImplementedError, match="fp32 only"):
            planar.Graph(fixture_opt(z, 0, "cpu", tmp_path, precision=prec))
    monkeypatch.setattr(planar, "_dist", lambda: True)
    monkeypatch.setattr(torch.distributed, "get_world_size", lambda *a, **k: 2)
    monkeypatch.setattr(torch.distributed, "get_rank", lambda *a, **k: 0)
    with pytest.raises(NotImplementedError, match="more than one rank.*all-reduce"):
        planar.Graph(fixture_opt(z, 0, "cpu", tmp_path))


def test_graph_capable_is_false_with_implicit_masks(golden, tmp_path):
    m = fixture_model(golden("mask_edges0"), 0, "cpu", tmp_path)
    m.setup_optimizer()
    assert [len(g["params"]) for g in m.optim.param_groups] == [len(list(m.graph.neural_image.parameters())), 1, 10]
    assert m.optim.param_groups[2]["lr"] == m.opt.optim.lr_mask
    mask_ids = {id(p) for p in m.graph.implicit_mask.parameters()}
    assert {id(p) for p in m.optim.param_groups[2]["params"]} == mask_ids
    assert all(id(m.graph.embedding_view.weight) != id(p) for g in m.optim.param_groups for p in g["params"])
    m.opt.device = "cuda:0"  # (graph_capable looks at the option only)
    assert not m.graph_capable()


def test_default_path_has_no_mask_attributes(golden, tmp_path):
    m = fixture_model(golden("mask_edges0"), 0, "cpu", tmp_path, use_implicit_mask=False)
    for name in ("implicit_mask", "embedding_view", "embedding_uv"):
        assert not hasattr(m.graph, name)
    assert not any(k.startswith(("implicit_mask", "embedding_view")) for k in m.graph.state_dict())
    m.setup_optimizer()
    assert len(m.optim.param_groups) == 2
