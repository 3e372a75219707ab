"""The split-bf16 tile recipe without a GPU: which nets the library routes to k_mlp_step_split, that
their buffers are plain bf16's, and that the recipe itself (tests/bf16x3_tile_ref.py, float64
accumulation) meets the parity contract on the inputs the GPU tests use -- so the bounds of
test_gpu_bf16x3_tile.py are conditions on the recipe that hold before any kernel runs."""
import ctypes

import pytest

import bf16x3_tile_ref as R

C5 = [66] + [512] * 8 + [3]
DEEP = [34] + [128] * 6 + [3]


@pytest.fixture(scope="module")
def lib():
    import build_lib
    return ctypes.CDLL(build_lib.build(verbose=False))


def test_routing(lib):
    """More than 5 layers, or a hidden width above 256: the split tile kernel.  What k_step2 holds stays
    on k_step2; skip nets stay refused ("skip"); plain bf16 keeps the plain tile kernel."""
    import marf_hip
    X3, BF = marf_hip.MARF_BF16X3, marf_hip.MARF_BF16
    assert marf_hip.Net(C5, 16, X3).step_kernel == "k_mlp_step_split"
    assert marf_hip.Net(DEEP, 8, X3).step_kernel == "k_mlp_step_split"
    assert marf_hip.Net([66, 512, 512, 3], 16, X3).step_kernel == "k_mlp_step_split"
    assert marf_hip.Net([34, 288, 512, 288, 3], 8, X3).step_kernel == "k_mlp_step_split"
    assert marf_hip.Net([66, 256, 256, 256, 256, 3], 16, X3).step_kernel == "k_step2"
    assert marf_hip.Net([34, 256, 256, 256, 256, 3], 8, X3).step_kernel == "k_step2"
    assert marf_hip.Net([34, 128, 128, 128, 128, 3], 8, X3).step_kernel == "k_step2"
    assert marf_hip.Net(C5, 16, BF).step_kernel == "k_mlp_step"
    with pytest.raises(RuntimeError, match="skip"):
        marf_hip.Net([66, 384, 384, 384, 3], 16, X3, skip=[2])  # 384 + 96 inputs: bf16 takes it
    with pytest.raises(RuntimeError, match="skip"):
        marf_hip.Net([34] + [128] * 6 + [3], 8, X3, skip=[3])
    with pytest.raises(RuntimeError, match="512"):
        marf_hip.Net([34, 1024, 3], 8, X3)
    with pytest.raises(RuntimeError, match="fp16x2"):
        marf_hip.Net(C5, 16, marf_hip.MARF_FP16X2)
    with pytest.raises(RuntimeError, match="mask-network recipe"):
        marf_hip.Net(C5, 16, marf_hip.MARF_BF16X3A)


@pytest.mark.parametrize("dims,L", [(C5, 16), (DEEP, 8), ([34, 288, 512, 288, 3], 8)])
def test_buffers_are_plain_bf16s(lib, dims, L):
    """Same parameter layout, the same saved / workspace / step-buffer bytes as the bf16 net of the same
    dims (hi planes and ReLU records only); the packed weights are larger (hi + lo images)."""
    import marf_hip
    a, b = marf_hip.Net(dims, L, marf_hip.MARF_BF16X3), marf_hip.Net(dims, L, marf_hip.MARF_BF16)
    assert a.layer_spans == b.layer_spans and a.param_count == b.param_count
    assert a.packed_bytes > b.packed_bytes
    for geo in (marf_hip.grid_geometry(2, 512, 512, 64, 64, None), marf_hip.grid_geometry(3, 512, 512, 50, 54, None),
                marf_hip.grid_geometry(64, 512, 512, 256, 256, None)):
        geo.d_H = 1  # planning reads no device memory
        assert a.saved_bytes(geo) == b.saved_bytes(geo) > 0
        assert a.workspace_bytes(geo) == b.workspace_bytes(geo) > 0
        # the fused step's buffer: the same per-pixel tensors; above 256 wide the tile is 64 slots
        # against plain bf16's 128, so the per-tile partials (dW_last 3 x Kp floats, db_last, dH, loss)
        # are twice as many: 48 B more per pixel slot beside ~17 KB of saved tensors at C5
        f = marf_hip.lib().marf_step_saved_bytes
        sa, sb = f(a.handle, ctypes.byref(geo)), f(b.handle, ctypes.byref(geo))
        if max(dims[1:-1]) <= 256:
            assert sa == sb > 0
        else:
            S = geo.B * -(-(2 * (geo.patch_H // 2) * 2 * (geo.patch_W // 2)) // 128) * 128
            rows = -(-dims[-2] // 32) * 32
            assert sb < sa <= sb + S // 128 * (3 * rows * 4 + 12 + 36 + 16) + 4 * 256, (sa, sb)
        assert marf_hip.lib().marf_render_workspace_bytes(a.handle, ctypes.byref(geo)) == 0


_CACHE = {}


def _case(case):
    if case not in _CACHE:
        inp = R.synthetic_inputs(case)
        _CACHE[case] = (inp, R.truth(inp))
    return _CACHE[case]


@pytest.mark.parametrize("case", list(R.SHAPES))
def test_recipe_meets_the_contract(case):
    """The emulated recipe against float64 truth (cpu_ref.CpuRefStep): rgb <= 1e-5 abs, every MLP
    gradient tensor and d warp <= 1e-2 of its max.  Measured (rgb / worst MLP gradient / d warp):
    c5 8.9e-8 / 6.2e-3 / 8.6e-3, deep 1.4e-7 / 1.1e-3 / 5.4e-4, wide 2.4e-6 / 1.5e-3 / 3.7e-3,
    odd 6.3e-7 / 3.5e-3 / 1.9e-3, ragged 1.3e-7 / 2.7e-3 / 8.3e-4."""
    (cfg, params, warp, rgb, mask, progress), t64 = _case(case)
    e = R.errors(R.step(cfg, params, warp, rgb, mask, progress), t64)
    print(case, e["rgb"], max(e["grads"]), e["dh"])
    assert e["rgb"] <= 1e-5, e
    assert max(e["grads"]) <= 1e-2 and e["dh"] <= 1e-2, e


@pytest.mark.parametrize("term", ["fwd_hl", "fwd_lh"])
@pytest.mark.parametrize("case", list(R.SHAPES))
def test_both_forward_lo_terms_are_needed(case, term):
    """Without W_h a_l or without W_l a_h the recipe misses the contract (rgb 1.3e-5 .. 8.8e-4)."""
    (cfg, params, warp, rgb, mask, progress), t64 = _case(case)
    e = R.errors(R.step(cfg, params, warp, rgb, mask, progress, drop=(term,)), t64)
    print(case, term, e["rgb"], max(e["grads"]), e["dh"])
    assert e["rgb"] > 1e-5 or max(e["grads"]) > 1e-2 or e["dh"] > 1e-2, e
