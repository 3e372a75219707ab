"""Gauss-Newton registration on a frozen image without a GPU: the four C-ABI entries in the header, the
library and the ctypes table; the byte counts of the packed buffer and the scratch plan for the nets the
kernel takes, and the refusals with their reasons; the Graph refusals of warp_solver: lm; and the float64
reference itself (tests/gn_ref.py): its LM loop on the realisable problem of the solver tests decreases
every patch's sse monotonically and reaches below the floors those tests rely on."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import gn_ref
from conftest import ROOT

ENTRIES = ("marf_gn_packed_bytes", "marf_gn_pack", "marf_gn_scratch_bytes", "marf_gn_normal")
NETS = {  # name -> (dims, L, precision name)
    "fp32": ([34, 128, 128, 3], 8, "MARF_FP32"),
    "small_bf16x3": ([34, 64, 64, 3], 8, "MARF_BF16X3"),          # k_step2-shaped
    "ragged_bf16x3": ([34] + [128] * 6 + [3], 8, "MARF_BF16X3"),  # split tile, TP = 128
    "odd_bf16x3": ([34, 288, 512, 288, 3], 8, "MARF_BF16X3"),     # split tile, TP = 64
}


@pytest.fixture(scope="module")
def lib():
    import build_lib
    return ctypes.CDLL(build_lib.build(verbose=False))


def _geo(B=2, ph=50, pw=54, coords=False):
    import marf_hip
    if coords:
        g = marf_hip.Geometry()
        g.mode, g.B, g.Np, g.d_coords = marf_hip.GEO_COORDS, 1, 100, 1
        return g
    g = marf_hip.grid_geometry(B, 512, 512, ph, pw, None)
    g.d_H = 1  # (planning reads no device memory)
    return g


def test_header_library_and_bindings_agree(lib):
    import marf_hip
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "marf.h")).read(), flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert hasattr(lib, name), name
        decl = re.search(r"\b%s\s*\(([^;]*)\);" % name, src).group(1)
        assert len(decl.split(",")) == len(marf_hip._SIGS[name][1]), name
    assert marf_hip._SIGS["marf_gn_packed_bytes"][0] is ctypes.c_size_t
    assert marf_hip._SIGS["marf_gn_scratch_bytes"][0] is ctypes.c_size_t


@pytest.mark.parametrize("name", list(NETS))
def test_byte_counts_of_the_nets_the_kernel_takes(lib, name):
    """Packed: every Wf / Wt image at 4 B per weight (fp32, or bf16 hi + lo) and the fp32 biases.  Scratch:
    one 4 KB ReLU record per tile and hidden layer, 56 doubles per tile, the band weights; tiles of 128
    slots for bf16x3 up to 256 wide, of 64 above and for fp32."""
    import marf_hip
    dims, L, prec = NETS[name]
    n = marf_hip.Net(dims, L, getattr(marf_hip, prec))
    if name == "small_bf16x3":
        assert n.step_kernel == "k_step2"
    packed = marf_hip.lib().marf_gn_packed_bytes(n.handle)
    pad = lambda x: (x + 31) // 32 * 32  # noqa: E731
    widths = [pad(d) for d in dims[:-1]]
    weights = sum(a * b for a, b in zip(widths[:-1], widths[1:])) * 2 + widths[-1] * 16
    assert packed >= weights * 4, (packed, weights)
    if prec == "MARF_BF16X3" and n.step_kernel == "k_mlp_step_split":
        assert packed <= n.packed_bytes  # (the training buffer's tile images are these)
    g = _geo()
    scratch = marf_hip.lib().marf_gn_scratch_bytes(n.handle, ctypes.byref(g))
    TP = 128 if prec == "MARF_BF16X3" and max(widths) <= 256 else 64
    tiles = 2 * ((50 * 54 + 127) // 128 * 128) // TP
    hidden = len(dims) - 2
    want = tiles * (hidden * 4096 + 56 * 8)
    print(name, "packed", packed, "scratch", scratch, "tiles", tiles)
    assert want <= scratch <= want + 256 * (hidden + 3)


def test_refusals_say_why(lib):
    import marf_hip
    L = marf_hip.lib()
    g = _geo()
    for prec, dims, Lb in (("MARF_BF16", [34, 128, 128, 3], 8), ("MARF_FP16", [34, 128, 128, 3], 8),
                           ("MARF_FP16X2", [66, 256, 256, 256, 256, 3], 16)):
        n = marf_hip.Net(dims, Lb, getattr(marf_hip, prec))
        assert L.marf_gn_packed_bytes(n.handle) == 0 and b"16-bit Jacobian" in L.marf_last_error(), prec
        assert L.marf_gn_scratch_bytes(n.handle, ctypes.byref(g)) == 0 and b"16-bit Jacobian" in L.marf_last_error(), prec
        assert L.marf_gn_pack(n.handle, 1, 1, None) == -3
        rc = L.marf_gn_normal(n.handle, ctypes.byref(g), None, 1, 1, None, 0, None, 1, 1, None)
        assert rc == -3 and b"16-bit Jacobian" in L.marf_last_error(), prec
    sk = marf_hip.Net([34, 128, 128, 128, 3], 8, marf_hip.MARF_FP32, skip=(2,))
    assert L.marf_gn_packed_bytes(sk.handle) == 0 and b"skip" in L.marf_last_error()
    assert L.marf_gn_scratch_bytes(sk.handle, ctypes.byref(g)) == 0 and b"skip" in L.marf_last_error()
    ok = marf_hip.Net([34, 128, 128, 3], 8, marf_hip.MARF_FP32)
    gc = _geo(coords=True)
    assert L.marf_gn_scratch_bytes(ok.handle, ctypes.byref(gc)) == 0 and b"COORDS" in L.marf_last_error()
    rc = L.marf_gn_normal(ok.handle, ctypes.byref(gc), None, 1, 1, None, 0, None, 1, 1, None)
    assert rc == -3 and b"COORDS" in L.marf_last_error()
    assert L.marf_gn_scratch_bytes(ok.handle, ctypes.byref(g)) > 0


def test_plan_bytes_of_the_existing_buffers_did_not_move(lib):
    """(tests/test_plan_bytes_cpu.py pins them; here: the training packed buffer of a k_step2 net is not
    the Gauss-Newton one, which is why the feature has its own.)"""
    import marf_hip
    n = marf_hip.Net([34, 64, 64, 3], 8, marf_hip.MARF_BF16X3)
    assert marf_hip.lib().marf_gn_packed_bytes(n.handle) != n.packed_bytes


def _opt(tmp, **over):
    from test_gpu_parity import make_opt
    opt = make_opt(tmp, H=64, W=64, patch_H=48, patch_W=48, batch_size=3, use_edges=False, barf_c2f=None,
                   arch={"layers": [None, 64, 64, 3], "skip": [], "posenc": {"L_2D": 2}}, **over)
    opt.device = "cpu"
    return opt


def test_graph_refusals_and_optimizer(tmp_path):
    from model import planar
    with pytest.raises(NotImplementedError, match="freeze_image"):
        planar.Graph(_opt(tmp_path, warp_solver="lm"))
    with pytest.raises(NotImplementedError, match="use_implicit_mask"):
        planar.Graph(_opt(tmp_path, warp_solver="lm", freeze_image=True, use_implicit_mask=True))
    for prec in ("bf16", "fp16"):
        with pytest.raises(NotImplementedError, match="16-bit Jacobian"):
            planar.Graph(_opt(tmp_path, warp_solver="lm", freeze_image=True, precision=prec))
    with pytest.raises(NotImplementedError):
        planar.Graph(_opt(tmp_path, warp_solver="lm", freeze_image=True, precision="fp16x2"))
    with pytest.raises(ValueError, match="warp_solver"):
        planar.Graph(_opt(tmp_path, warp_solver="newton", freeze_image=True))
    m = planar.Model(_opt(tmp_path, warp_solver="lm", freeze_image=True, precision="bf16x3"))
    m.build_networks()
    assert m.graph.warp_solver == "lm" and m.graph.lm.lambda0 == 1e-3 and m.graph.lm.up == 10
    m.setup_optimizer()
    assert m.optim is None  # no warp group: the warps move by Graph.lm_step
    assert "lm_lambda" not in m.graph.state_dict()
    d = planar.Model(_opt(tmp_path, freeze_image=True))  # the default stays adam
    d.build_networks()
    d.setup_optimizer()
    assert d.graph.warp_solver == "adam" and len(d.optim.param_groups) == 1


def test_reference_lm_on_the_realisable_problem():
    """The float64 LM of gn_ref on the solver tests' problem (seed 3, h* + 0.01 noise): every patch's sse
    is non-increasing at every iteration, patch 0 stays, and after 10 iterations |h - h*|_inf is below
    1e-4, the smaller of the two floors tests/test_gpu_gn_solver.py relies on."""
    inputs, hstar, h0 = gn_ref.realisable(seed=3)
    inputs = gn_ref.with_targets(inputs, gn_ref.normal(inputs, warp=hstar)["rgb"])
    # (the targets are float32, as the product's: 6,912 values off by half an ulp of 0.5 at the most)
    assert gn_ref.normal(inputs, warp=hstar)["sse"].max() < 6912 * (2.0 ** -25) ** 2
    h, hist = gn_ref.lm(inputs, h0, 10)
    print("sse per iteration:", hist.sum(1), "final |h - h*|_inf", np.abs(h - hstar).max())
    assert (np.diff(hist, axis=0) <= 0).all()
    assert hist[-1].sum() < 1e-3 * hist[0].sum()
    assert np.array_equal(h[0], h0[0])
    assert np.abs(h - hstar).max() < 1e-4


@pytest.mark.parametrize("case", ["small"])
def test_kink_share_of_the_new_case(case):
    """The ReLU-kink pixels of the new k_step2-shaped case (bf16x3_tile_ref.kink_pixels, factor 4) stay
    within the 8 % the GPU test allows."""
    import bf16x3_tile_ref as R
    inputs = gn_ref.synthetic_inputs(case)
    near, thr = R.kink_pixels(inputs)
    print(case, "kink share %.2f %%" % (100 * near.mean()), "threshold", thr)
    assert near.mean() <= 0.08


def test_reference_pieces_agree():
    """gn_ref against itself: 2 E^T g9 / (3 sum m) is cpu_ref.CpuRefStep's warp gradient of loss.rgb (its
    step differentiates 2 loss.rgb), sum sse / (3 sum m) its loss -- the identities test 3 uses on the GPU."""
    import bf16x3_tile_ref as R
    inputs = gn_ref.synthetic_inputs("small")
    nm = gn_ref.normal(inputs)
    t64 = R.truth(inputs, torch.float64)
    E = gn_ref.tangent(inputs[2])
    dh = 2 * np.einsum("bki,bk->bi", E, nm["g9"]) / (3 * nm["msum"].sum())
    assert np.abs(2 * dh - t64["dh"]).max() <= 1e-9 * np.abs(t64["dh"]).max()
    assert abs(nm["sse"].sum() / (3 * nm["msum"].sum()) - t64["loss_rgb"]) <= 1e-12
    assert np.abs(nm["N"] - nm["N"].transpose(0, 2, 1)).max() == 0
