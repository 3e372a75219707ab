"""Robust Gauss-Newton registration without a GPU: the float64 reference (tests/gn_robust_ref.py) against
autograd, against gn_ref and on the occluded problem it exists for; then the product side -- the entry in
the header, the library and the ctypes table, unchanged byte counts, the refusals with their reasons, the
lm.robust options and the Graph they build."""
import ctypes
import os
import re

import numpy as np
import pytest

import gn_ref
import gn_robust_ref as G
from conftest import PKG, ROOT
from test_gn_cpu import NETS, _geo, _opt, lib  # noqa: F401 (lib: fixture)

_OCC = {}


def occluded():
    """The occluded problem and the float64 Cauchy solve on it (delta = 0.01, 25 iterations): computed once."""
    if not _OCC:
        inputs, hstar, h0, inside = G.occluded()
        h, hist, w = G.lm(inputs, h0, 25, "cauchy", 0.01)
        _OCC.update(inputs=inputs, hstar=hstar, h0=h0, inside=inside, h=h, hist=hist, w=w)
    return _OCC


@pytest.mark.parametrize("kind,delta", [("huber", 0.5), ("cauchy", 0.5), ("cauchy", 0.05)])
def test_twice_g9_is_the_gradient_of_the_cost(kind, delta):
    """d cost_b / d vec(H_b) = 2 g9_b (the IRLS weight is rho'), so 2 E^T g9 is the gradient in the tangent:
    against float64 autograd through the reference's render, 1e-9 of its max.  Huber at delta = 0.5 has
    both branches on this input (47 % of the pixels beyond delta)."""
    inputs = gn_ref.synthetic_inputs("small")
    nm = G.normal(inputs, kind, delta)
    if kind == "huber":
        assert 0.2 <= (nm["e"] > delta * delta).mean() <= 0.8
    want = G.cost_gradient(inputs, kind, delta)
    assert np.abs(2 * nm["g9"] - want).max() <= 1e-9 * np.abs(want).max()
    E = gn_ref.tangent(inputs[2])
    got_t, want_t = 2 * np.einsum("bki,bk->bi", E, nm["g9"]), np.einsum("bki,bk->bi", E, want)
    assert np.abs(got_t - want_t).max() <= 1e-9 * np.abs(want_t).max()
    assert np.abs(nm["N"] - nm["N"].transpose(0, 2, 1)).max() <= 1e-12 * np.abs(nm["N"]).max()


def test_huber_with_a_huge_delta_is_gn_ref():
    inputs = gn_ref.synthetic_inputs("small")
    nm, ref = G.normal(inputs, "huber", 1e3), gn_ref.normal(inputs)
    assert np.array_equal(G.pack56(nm), gn_ref.pack56(ref)) and np.array_equal(nm["rgb"], ref["rgb"])
    assert (nm["weight"] == 1).all()


def test_cauchy_recovers_the_occluded_warps():
    """The issue's table: from h* + 0.01 noise (0 / 0.028 / 0.014 from h*), 25 Cauchy iterations at delta =
    0.01 end within 1e-3 of h* (2.8e-4 / 2.5e-4), every patch's accepted cost non-increasing, the weight at
    most 4.6e-4 inside the rectangles and at least 0.99998 outside."""
    o = occluded()
    d = np.abs(o["h"] - o["hstar"]).max(1)
    w, inside = o["w"], o["inside"]
    print("Cauchy |h - h*|_inf per patch", d, "weight inside <=", w[inside].max(), "outside >=", w[~inside].min())
    assert (d <= 1e-3).all() and np.array_equal(o["h"][0], o["h0"][0])
    assert (np.diff(o["hist"], axis=0) <= 0).all()
    assert inside.mean() == pytest.approx(320 / 2304) and w[inside].max() <= 1e-3 and w[~inside].min() >= 0.9999


def test_plain_lm_is_dragged_away_by_the_occluder():
    """Least squares under the all-ones mask, 12 iterations: both moving patches end farther from h* than
    they started (0.92 / 0.91 against 0.028 / 0.014) -- the behaviour lm.robust answers."""
    o = occluded()
    h, _, _ = G.lm(o["inputs"], o["h0"], 12)
    d0, d = np.abs(o["h0"] - o["hstar"]).max(1), np.abs(h - o["hstar"]).max(1)
    print("plain LM |h - h*|_inf per patch", d, "start", d0)
    assert (d[1:] > d0[1:]).all()


def test_huber_and_a_wider_cauchy_on_the_occluded_problem():
    """The table's other rows: Huber at 0.01 keeps both patches near the start's distance (0.017 / 0.017:
    its weight never falls below delta / s), Cauchy at 0.05 reaches 7.5e-3 / 6.3e-3."""
    o = occluded()
    for kind, delta, bound in (("huber", 0.01, 0.03), ("cauchy", 0.05, 0.01)):
        h, hist, _ = G.lm(o["inputs"], o["h0"], 25, kind, delta)
        d = np.abs(h - o["hstar"]).max(1)
        print(kind, delta, d)
        assert (d <= bound).all() and (np.diff(hist, axis=0) <= 0).all()


# ---- the product, without a GPU

def test_header_library_and_bindings_agree(lib):
    import marf_hip
    name = "marf_gn_normal_robust"
    text = open(os.path.join(ROOT, "include", "marf.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert hasattr(lib, name)
    decl = re.search(r"\b%s\s*\(([^;]*)\);" % name, src).group(1)
    assert len(decl.split(",")) == len(marf_hip._SIGS[name][1]) == 14
    assert re.search(r"#define\s+MARF_GN_HUBER\s+1\b", src) and re.search(r"#define\s+MARF_GN_CAUCHY\s+2\b", src)
    assert marf_hip.GN_ROBUST == {"huber": 1, "cauchy": 2}
    assert marf_hip._SIGS[name][1][8] is ctypes.c_float


@pytest.mark.parametrize("name", list(NETS))
def test_byte_counts_are_marf_gn_normals(lib, name):
    """The robust entry has no plan of its own: the packed buffer and the scratch of every net the kernel
    takes are what they were (the figures tests/test_gn_cpu.py derives), and static LDS did not grow -- the
    160 KB refusal still passes the widest fp32 net it passed."""
    import marf_hip
    dims, L, prec = NETS[name]
    n = marf_hip.Net(dims, L, getattr(marf_hip, prec))
    g = _geo()
    pad = lambda x: (x + 31) // 32 * 32  # noqa: E731
    TP = 128 if prec == "MARF_BF16X3" and max(pad(d) for d in dims[:-1]) <= 256 else 64
    tiles = 2 * ((50 * 54 + 127) // 128 * 128) // TP
    hidden = len(dims) - 2
    want = tiles * (hidden * 4096 + 56 * 8)
    scratch = marf_hip.lib().marf_gn_scratch_bytes(n.handle, ctypes.byref(g))
    assert want <= scratch <= want + 256 * (hidden + 3)
    assert marf_hip.lib().marf_gn_packed_bytes(n.handle) > 0


def test_refusals_say_why(lib):
    import marf_hip
    L = marf_hip.lib()
    g = _geo()

    def call(net, geo, kind, delta):
        return L.marf_gn_normal_robust(net.handle, ctypes.byref(geo), None, 1, 1, None, 0, kind, delta, None, None, 1, 1, None)
    ok = marf_hip.Net([34, 128, 128, 3], 8, marf_hip.MARF_FP32)
    for kind in (0, 3, -1):
        assert call(ok, g, kind, 0.1) == -1 and b"unknown kind" in L.marf_last_error(), kind
    for delta in (0.0, -0.1, float("nan"), float("inf")):
        assert call(ok, g, 1, delta) == -1 and b"delta must be finite and > 0" in L.marf_last_error(), delta
    # marf_gn_normal's refusals with its reasons
    for prec in ("MARF_BF16", "MARF_FP16"):
        n = marf_hip.Net([34, 128, 128, 3], 8, getattr(marf_hip, prec))
        assert call(n, g, 2, 0.1) == -3 and b"16-bit Jacobian" in L.marf_last_error(), prec
    sk = marf_hip.Net([34, 128, 128, 128, 3], 8, marf_hip.MARF_FP32, skip=(2,))
    assert call(sk, g, 1, 0.1) == -3 and b"skip" in L.marf_last_error()
    assert call(ok, _geo(coords=True), 1, 0.1) == -3 and b"COORDS" in L.marf_last_error()
    assert L.marf_gn_normal_robust(ok.handle, ctypes.byref(g), None, None, 1, None, 0, 1, 0.1, None, None, 1, 1, None) == -1
    assert b"NULL" in L.marf_last_error()
    with pytest.raises(ValueError, match="kind"):
        marf_hip.gn_normal_robust(None, None, None, None, None, None, 1.5, 0.1)


def test_options_and_graph_state(tmp_path):
    """lm.robust: none (the yaml's default) builds the Graph of before -- the same lm record, no robust
    state; huber / cauchy are parsed with lm.robust_delta (default 0.1); the refusals are ValueErrors."""
    import yaml
    from model import planar
    y = yaml.safe_load(open(os.path.join(PKG, "options", "planar.yaml")))
    assert y["lm"]["robust"] == "none" and y["lm"]["robust_delta"] == 0.1
    base = dict(warp_solver="lm", freeze_image=True, precision="bf16x3")
    plain = planar.Graph(_opt(tmp_path, **base))
    none = planar.Graph(_opt(tmp_path, lm={"robust": "none", "robust_delta": -1}, **base))  # (delta unread)
    assert plain.lm_robust is None and none.lm_robust is None
    assert dict(plain.lm) == dict(none.lm) == dict(lambda0=1e-3, up=10.0, down=10.0, lambda_min=1e-9, lambda_max=1e9)
    assert list(plain.state_dict()) == list(none.state_dict()) and none.lm_lambda is None
    assert planar.Graph(_opt(tmp_path, freeze_image=True)).lm_robust is None  # adam: nothing to refuse
    g = planar.Graph(_opt(tmp_path, lm={"robust": "Huber"}, **base))
    assert g.lm_robust == ("huber", 0.1) and g.lm.lambda0 == 1e-3
    g = planar.Graph(_opt(tmp_path, lm={"robust": "cauchy", "robust_delta": 0.01, "lambda0": 1e-2}, **base))
    assert g.lm_robust == ("cauchy", 0.01) and g.lm.lambda0 == 1e-2
    with pytest.raises(ValueError, match="lm.robust must be none, huber or cauchy"):
        planar.Graph(_opt(tmp_path, lm={"robust": "tukey"}, **base))
    for delta in (0, -0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="robust_delta"):
            planar.Graph(_opt(tmp_path, lm={"robust": "huber", "robust_delta": delta}, **base))
    with pytest.raises(ValueError, match="needs warp_solver: lm"):
        planar.Graph(_opt(tmp_path, lm={"robust": "cauchy"}, freeze_image=True))
    with pytest.raises(NotImplementedError, match="use_implicit_mask"):  # (the LM refusals stay)
        planar.Graph(_opt(tmp_path, lm={"robust": "cauchy"}, use_implicit_mask=True, **base))


def test_render_gn_keeps_its_default_call():
    """NeuralImageFunction.render_gn: `robust` is a keyword whose default leaves the two-tuple call."""
    import inspect
    from model import planar
    sig = inspect.signature(planar.NeuralImageFunction.render_gn)
    assert list(sig.parameters)[:6] == ["self", "warp_weight", "gt", "masks", "loss_only", "want_rgb"]
    assert sig.parameters["robust"].default is None
