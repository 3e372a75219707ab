"""The warp-only fused step (a frozen image registers further patches) without a GPU: the three C-ABI
entries in the header, the library and the ctypes table; the buffer plan's size against the full step's
on the C3 geometry; the refused recipes; freeze_image on CPU graphs (construction only: no kernel runs)
and the checkpoint round trip."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT
from mask_common import fixture_model

ENTRIES = ("marf_warp_step_saved_bytes", "marf_warp_step_forward", "marf_warp_step_backward")
C3_NET = [66, 256, 256, 256, 256, 3]
C5_NET = [66] + [512] * 8 + [3]  # (bench.py's C5, as tests/test_bf16x3_tile_cpu.py names it)


@pytest.fixture(scope="module")
def lib():
    import build_lib
    return ctypes.CDLL(build_lib.build(verbose=False))


def _c3_geo():
    """64 patches of 256 x 256 on the 512 x 512 canvas (planning reads no device memory)."""
    import marf_hip
    g = marf_hip.grid_geometry(64, 512, 512, 256, 256, None)
    g.d_H = 1
    return g


def test_header_library_and_bindings_agree(lib):
    import marf_hip
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "marf.h")).read(), flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert hasattr(lib, name), name
        assert name in marf_hip._SIGS, name
    # argument counts of the declarations and of the ctypes table
    for name in ENTRIES:
        decl = re.search(r"\b%s\s*\(([^;]*)\);" % name, src).group(1)
        assert len(decl.split(",")) == len(marf_hip._SIGS[name][1]), name
    assert marf_hip._SIGS[ENTRIES[0]][0] is ctypes.c_size_t
    # the forward's contract is marf_step_forward's; the backward is marf_step_backward less d_dparams
    assert marf_hip._SIGS["marf_warp_step_forward"] == marf_hip._SIGS["marf_step_forward"]
    full = list(marf_hip._SIGS["marf_step_backward"][1])
    assert len(marf_hip._SIGS["marf_warp_step_backward"][1]) == len(full) - 1


def test_bf16x3_plan_is_a_few_bytes_per_slot(lib, monkeypatch):
    """k_step2w at C3: the dH partials (36 B per 32 slots) and per-block buffers -- at most 8 B per
    pixel slot in total, where the full step saves kilobytes."""
    import marf_hip
    monkeypatch.delenv("MARF_STEP2_GRID", raising=False)
    n = marf_hip.Net(C3_NET, 16, marf_hip.MARF_BF16X3)
    assert n.step_kernel == "k_step2"
    g = _c3_geo()
    slots = 64 * 256 * 256
    warp = n.warp_step_saved_bytes(g)
    full = marf_hip.lib().marf_step_saved_bytes(n.handle, ctypes.byref(g))
    print("bf16x3 C3: warp-only", warp, "B =", warp / slots, "B per slot; full step", full)
    assert 0 < warp <= 8 * slots
    assert warp >= slots // 32 * 36  # the dH partials are all there
    assert warp * 8 <= full


@pytest.mark.parametrize("prec", ["bf16", "fp32"])
def test_tile_plan_is_an_eighth_of_the_full_steps(lib, prec):
    """The tile kernels keep their ReLU records (about 1 / 29 of the bf16 bytes at C3) beside the
    partials: at most 1 / 8 of marf_step_saved_bytes."""
    import marf_hip
    n = marf_hip.Net(C3_NET, 16, {"bf16": marf_hip.MARF_BF16, "fp32": marf_hip.MARF_FP32}[prec])
    assert n.step_kernel == "k_mlp_step"
    g = _c3_geo()
    warp = n.warp_step_saved_bytes(g)
    full = marf_hip.lib().marf_step_saved_bytes(n.handle, ctypes.byref(g))
    print(prec, "C3: warp-only", warp, "full step", full, "ratio", full / warp)
    assert 0 < warp and warp * 8 <= full


def test_c5_split_tile_plan(lib):
    """The C5 net (eight hidden layers of 512, nine layers: eight ReLU-record regions) in bf16x3, on the
    split-bf16 tile kernel: at most 1 / 8 of marf_step_saved_bytes."""
    import marf_hip
    assert len(C5_NET) == 10
    n = marf_hip.Net(C5_NET, 16, marf_hip.MARF_BF16X3)
    assert n.step_kernel == "k_mlp_step_split"
    g = _c3_geo()
    warp = n.warp_step_saved_bytes(g)
    full = marf_hip.lib().marf_step_saved_bytes(n.handle, ctypes.byref(g))
    print("C5 bf16x3: warp-only", warp, "full step", full, "ratio", full / warp)
    assert 0 < warp and warp * 8 <= full


def test_pipeline_and_grid_switches(lib, monkeypatch):
    """The pipelined mode does not change the warp-only plan; MARF_STEP2_GRID does (per-block buffers)."""
    import marf_hip
    monkeypatch.delenv("MARF_STEP2_GRID", raising=False)
    n = marf_hip.Net(C3_NET, 16, marf_hip.MARF_BF16X3)
    g = _c3_geo()
    base = n.warp_step_saved_bytes(g)
    n.set_pipeline(1)
    assert n.warp_step_saved_bytes(g) == base
    n.set_pipeline(0)
    monkeypatch.setenv("MARF_STEP2_GRID", "3")
    assert n.warp_step_saved_bytes(g) < base


def test_refused_recipes_say_why(lib, monkeypatch):
    import marf_hip
    g = _c3_geo()
    n = marf_hip.Net(C3_NET, 16, marf_hip.MARF_FP16X2)
    with pytest.raises(RuntimeError, match="fp16x2"):
        n.warp_step_saved_bytes(g)
    rc = marf_hip.lib().marf_warp_step_forward(n.handle, ctypes.byref(g), None, 1, 1, None, None, None, 1, 1, None)
    assert rc == -3 and b"fp16x2" in marf_hip.lib().marf_last_error()
    monkeypatch.setenv("MARF_STEP2_DZ", "1")
    ndz = marf_hip.Net(C3_NET, 16, marf_hip.MARF_BF16X3)
    monkeypatch.delenv("MARF_STEP2_DZ")
    with pytest.raises(RuntimeError, match="MARF_STEP2_DZ"):
        ndz.warp_step_saved_bytes(g)
    rc = marf_hip.lib().marf_warp_step_backward(ndz.handle, ctypes.byref(g), 1, 1, 0, 1, 1, 1, None)
    assert rc == -3 and b"MARF_STEP2_DZ" in marf_hip.lib().marf_last_error()
    assert marf_hip.Net(C3_NET, 16, marf_hip.MARF_BF16X3).warp_step_saved_bytes(g) > 0  # (the switch is per net)


# ---------------------------------------------------------------- freeze_image on CPU graphs

@pytest.fixture(scope="module")
def z(golden):
    return golden("mask_edges0")


def _model(z, tmp, **extra):
    return fixture_model(z, 0, "cpu", tmp, **extra)


def test_freeze_image_parameters_and_optimizer(z, tmp_path):
    m = _model(z, tmp_path, freeze_image=True)
    image = list(m.graph.neural_image.parameters())
    assert image and not any(p.requires_grad for p in image)
    assert m.graph.warp_param.weight.requires_grad
    assert all(p.requires_grad for p in m.graph.implicit_mask.parameters())  # the mask still learns
    m.setup_optimizer()
    ids = {id(p) for g in m.optim.param_groups for p in g["params"]}
    assert not ids & {id(p) for p in image}
    assert id(m.graph.warp_param.weight) in ids
    assert {id(p) for p in m.graph.implicit_mask.parameters()} <= ids
    assert len(m.optim.param_groups) == 2
    assert not m.graph_capable()
    # the default stays as it was
    d = _model(z, tmp_path)
    assert all(p.requires_grad for p in d.graph.neural_image.parameters())
    d.setup_optimizer()
    assert len(d.optim.param_groups) == 3


def test_freeze_image_refusals(z, tmp_path, monkeypatch):
    monkeypatch.delenv("MARF_STEP2_DZ", raising=False)
    with pytest.raises(NotImplementedError, match="cuda_graph"):
        _model(z, tmp_path, freeze_image=True, use_implicit_mask=False, cuda_graph=True)
    with pytest.raises(NotImplementedError, match="fp16x2"):
        _model(z, tmp_path, freeze_image=True, use_implicit_mask=False, precision="fp16x2")
    monkeypatch.setenv("MARF_STEP2_DZ", "1")
    with pytest.raises(NotImplementedError, match="MARF_STEP2_DZ"):
        _model(z, tmp_path, freeze_image=True, use_implicit_mask=False, precision="bf16x3")
    monkeypatch.delenv("MARF_STEP2_DZ")
    import model.planar as planar
    monkeypatch.setattr(planar, "_dist", lambda: True)
    monkeypatch.setattr(torch.distributed, "get_world_size", lambda *a, **k: 2)
    monkeypatch.setattr(torch.distributed, "get_rank", lambda *a, **k: 0)
    with pytest.raises(NotImplementedError, match="more than one rank"):
        planar.Graph(_opt_of(z, tmp_path, freeze_image=True, use_implicit_mask=False))


def _opt_of(z, tmp, **extra):
    from mask_common import fixture_opt
    return fixture_opt(z, 0, "cpu", tmp, **extra)


def test_checkpoint_round_trip_into_another_batch_size(z, tmp_path):
    """save_checkpoint / load_checkpoint: the whole graph and `it` into an equal model; neural_image.*
    alone, bit for bit, into a model with another patch count (opt.load with freeze_image)."""
    src = _model(z, tmp_path / "a")
    with torch.no_grad():
        for p in src.graph.parameters():
            p.add_(torch.randn_like(p) * 0.01)
    src.it = 7
    path = str(tmp_path / "model.ckpt")
    src.save_checkpoint(path)
    want = {k: v.clone() for k, v in src.graph.state_dict().items()}

    same = _model(z, tmp_path / "b")
    same.load_checkpoint(path, image_only=False)
    assert same.it == 7
    got = same.graph.state_dict()
    assert list(got) == list(want) and all(torch.equal(got[k], want[k]) for k in want)

    B = src.batch_size
    from model import planar
    opt = _opt_of(z, tmp_path / "c", freeze_image=True, batch_size=B - 1, load=path)
    torch.manual_seed(11)
    other = planar.Model(opt)
    other.images = None
    other.build_networks()  # honours opt.load: the image alone
    got = other.graph.state_dict()
    image_keys = [k for k in want if k.startswith("neural_image.")]
    assert image_keys and all(torch.equal(got[k], want[k]) for k in image_keys)
    assert got["warp_param.weight"].shape[0] == B - 1 and not got["warp_param.weight"].any()
    assert other.it == 0
    assert not torch.equal(got["implicit_mask.mask_mapping.0.weight"], want["implicit_mask.mask_mapping.0.weight"])
    assert not any(p.requires_grad for p in other.graph.neural_image.parameters())
