"""The mosaic of the registered patches without a GPU: the entry in the header, the library
and the ctypes table; marf_compose's argument refusals (made before any HIP call); the mosaic options and the
Graph / Model they build; and the float64 reference of tests/compose_ref.py held to what it must mean --
the inverse warp inverts, interior pixels are torch's grid_sample, a smooth analytic image comes back within
the bilinear bound, and the seam score falls when the warps are right."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import compose_ref as C
import gn_ref
from conftest import PKG, ROOT
from test_gn_cpu import _opt, lib  # noqa: F401 (lib: fixture)

NAME = "marf_compose"


# ---- the product, without a GPU

def test_header_library_and_bindings_agree(lib):
    import marf_hip
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "marf.h")).read(), flags=re.S)
    assert hasattr(lib, NAME)
    decl = re.search(r"\b%s\s*\(([^;]*)\);" % NAME, src).group(1)
    assert len(decl.split(",")) == len(marf_hip._SIGS[NAME][1]) == 15
    assert marf_hip._SIGS[NAME][0] is ctypes.c_int
    assert callable(marf_hip.compose)


def test_argument_refusals_say_why(lib):
    """MARF_ERR_INVALID with the reason, before any HIP call: these run on a machine without a GPU (the
    pointers are never read)."""
    import marf_hip
    L = marf_hip.lib()
    P = ctypes.c_void_p(64)

    def call(H=36, W=48, ph=18, pw=24, crop=1, B=2, Hinv=P, img=P, weight=None, feather=0, image=P, wsum=P,
             count=None, var=None):
        return L.marf_compose(H, W, ph, pw, crop, B, Hinv, img, weight, feather, image, wsum, count, var, None)
    for kw in (dict(Hinv=None), dict(img=None), dict(image=None), dict(wsum=None)):
        assert call(**kw) == -1 and b"NULL" in L.marf_last_error(), kw
    for B in (0, -3):
        assert call(B=B) == -1 and b"at least one patch" in L.marf_last_error(), B
    for kw in (dict(H=0), dict(W=-1), dict(ph=0), dict(pw=-2)):
        assert call(**kw) == -1 and b"positive" in L.marf_last_error(), kw
    for kw in (dict(H=16385, crop=0), dict(W=16385, crop=0)):
        assert call(**kw) == -1 and b"at most 16384" in L.marf_last_error(), kw
    for kw in (dict(ph=37), dict(pw=49)):
        assert call(**kw) == -1 and b"larger than the canvas" in L.marf_last_error(), kw
    for kw in (dict(ph=1), dict(pw=1)):  # the integer crop window H/2 -+ 1/2 is empty
        assert call(**kw) == -1 and b"empty crop window" in L.marf_last_error(), kw
    for kw in (dict(H=1, W=5, crop=0), dict(H=5, W=1, crop=0)):
        assert call(feather=1, **kw) == -1 and b"feather needs" in L.marf_last_error(), kw
    # (without crop the patch sizes are not read)
    assert call(crop=0, ph=0, pw=0, B=0) == -1 and b"at least one patch" in L.marf_last_error()
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        marf_hip.compose(36, 48, 18, 24, True, torch.zeros(2, 3, 3), torch.zeros(2, 3, 18, 24))


def test_options_and_the_graph_they_build(tmp_path, monkeypatch):
    """mosaic: {eval: false, weights: mask, feather: false} is the yaml's default and builds a Graph with that
    record; the refusals are ValueErrors with the reason."""
    import yaml
    from model import planar
    y = yaml.safe_load(open(os.path.join(PKG, "options", "planar.yaml")))
    assert y["mosaic"] == {"eval": False, "weights": "mask", "feather": False}
    g = planar.Graph(_opt(tmp_path))
    assert g.mosaic == {"eval": False, "weights": "mask", "feather": False}
    g = planar.Graph(_opt(tmp_path, mosaic={"eval": True, "weights": "Ones", "feather": True}))
    assert g.mosaic == {"eval": True, "weights": "ones", "feather": True}
    lm = dict(warp_solver="lm", freeze_image=True)
    assert planar.Graph(_opt(tmp_path, mosaic={"weights": "robust"}, lm={"robust": "cauchy"}, **lm)).mosaic.weights == "robust"
    assert planar.Graph(_opt(tmp_path, mosaic={"weights": "learned"}, use_implicit_mask=True)).mosaic.weights == "learned"
    with pytest.raises(ValueError, match="mosaic.weights must be one of"):
        planar.Graph(_opt(tmp_path, mosaic={"weights": "median"}))
    with pytest.raises(ValueError, match="learned needs use_implicit_mask"):
        planar.Graph(_opt(tmp_path, mosaic={"weights": "learned"}))
    with pytest.raises(ValueError, match="robust needs lm.robust"):
        planar.Graph(_opt(tmp_path, mosaic={"weights": "robust"}, **lm))
    monkeypatch.setattr(planar, "_dist", lambda: True)
    monkeypatch.setattr(torch.distributed, "get_world_size", lambda *a, **k: 2)
    with pytest.raises(ValueError, match="more than one process"):
        planar.Graph(_opt(tmp_path, mosaic={"eval": True}))
    assert planar.Graph(_opt(tmp_path)).mosaic.eval is False  # eval off: nothing to refuse


def test_model_methods_refuse_what_the_graph_cannot_supply(tmp_path):
    from model import planar
    m = planar.Model(_opt(tmp_path))
    m.graph = planar.Graph(m.opt)
    for w, why in (("median", "must be one of"), ("learned", "use_implicit_mask"), ("robust", "lm.robust")):
        with pytest.raises(ValueError, match=why):
            m.compose_mosaic(weights=w)
    m.world = 2
    with pytest.raises(ValueError, match="more than one process"):
        m.compose_mosaic()


def test_dataset_npz_may_carry_gt(tmp_path, monkeypatch):
    """An optional uint8 gt [3, H, W] becomes images.gt in [0, 1]; a file without it loads as before.  (The
    mask erosion is a GPU kernel and not what is looked at: it is stubbed out.)"""
    import inputs
    from model import planar
    monkeypatch.setattr(inputs, "erode_images", lambda mask, device: mask)
    rng = np.random.default_rng(0)
    rgb = rng.integers(0, 256, (3, 3, 48, 48), dtype=np.uint8)
    mask = np.ones((3, 1, 48, 48), np.uint8)
    gt = rng.integers(0, 256, (3, 64, 64), dtype=np.uint8)
    np.savez(tmp_path / "a.npz", rgb=rgb, mask=mask)
    np.savez(tmp_path / "b.npz", rgb=rgb, mask=mask, gt=gt)
    got = []
    for f in ("a.npz", "b.npz"):
        m = planar.Model(_opt(tmp_path, dataset_npz=str(tmp_path / f)))
        m.load_dataset()
        got.append(m.images)
    assert got[0].gt is None
    assert got[1].gt.shape == (3, 64, 64) and torch.equal(got[1].gt, torch.from_numpy(gt.astype(np.float32)) / 255)
    assert torch.equal(got[0].rgb, got[1].rgb)


# ---- the reference statement

def test_inverse_warp_inverts():
    """Hinv from -h times H from h is the identity to 1e-12 in float64 (sl(3) and embedded se(2))."""
    rng = np.random.default_rng(1)
    for h in (0.1 * rng.standard_normal((6, 8)), C.se2_embed(0.2 * rng.standard_normal((4, 3)))):
        P = (C.hinv(h) @ C.hmat(h)).numpy()
        assert np.abs(P - np.eye(3)).max() <= 1e-12


def test_interior_pixels_are_grid_sample():
    """One patch at a time, interior pixels only (at least 1 px inside the patch): the reference's sample is
    torch.nn.functional.grid_sample(align_corners=False) at the same point, and the blend composed by hand
    from those samples is the reference's image and wsum, to 1e-12."""
    cs = C.case(37, 50, 20, 24, 3, 0.05, seed=2)
    H, W, h, w = cs["H"], cs["W"], 20, 24
    Hinv = C.hinv(cs["h"])
    ref = C.compose(H, W, 20, 24, True, Hinv, cs["img"], cs["weight"])
    r, c, X2 = C.patch_coords(H, W, 20, 24, True, Hinv)
    img = torch.as_tensor(cs["img"]).double()
    wgt = torch.as_tensor(cs["weight"]).double()
    # grid_sample's normalised coordinates of pixel centre k of n: (2 k + 1) / n - 1
    grid = torch.stack([(2 * c + 1) / w - 1, (2 * r + 1) / h - 1], -1)  # [B, H, W, 2]
    v = torch.nn.functional.grid_sample(img, grid, mode="bilinear", padding_mode="border", align_corners=False)
    m = torch.nn.functional.grid_sample(wgt, grid, mode="bilinear", padding_mode="border", align_corners=False)[:, 0]
    inside = (X2 > 0) & (c >= 1) & (c <= w - 2) & (r >= 1) & (r <= h - 2)
    edge = torch.as_tensor(ref["valid"]) & ~inside
    om = torch.where(inside, m, torch.zeros_like(m))
    wsum = om.sum(0)
    image = (om[:, None] * v).sum(0) / torch.where(wsum > 0, wsum, torch.ones_like(wsum))
    ok = ~edge.any(0) & (wsum > 0)  # pixels whose every contribution is an interior one
    assert ok.float().mean() > 0.1  # (17 % of the canvas here)
    assert np.abs(ref["wsum"] - wsum.numpy())[ok.numpy()].max() <= 1e-12
    assert np.abs(ref["image"] - image.numpy())[:, ok.numpy()].max() <= 1e-12


@pytest.mark.parametrize("shape", [(37, 50, 20, 24, 3, 0.05), (64, 80, 32, 40, 4, 0.1)])
def test_smooth_image_comes_back_within_the_bilinear_bound(shape):
    """Patches sampled from the smooth analytic image at true warps: on covered pixels the reference mosaic is
    the image within the bilinear bound, and var within its square.  The bound: bilinear interpolation on a grid
    of spacing s errs by at most (1/8) s^2 (|f_xx| + |f_yy|) <= (1/4) s^2 K with K the Hessian's operator norm
    (compose_ref.smooth_curvature, per canvas pixel squared); the patch grid's spacing on the canvas is one
    pixel stretched by the warp, by far less than sqrt(2) at this noise, so (1/8) K (2 px)^2 = K / 2 holds.
    Every v_b then lies within the bound of the image, so their weighted variance is at most its square."""
    H, W, ph, pw, B, noise = shape
    cs = C.case(H, W, ph, pw, B, noise, seed=5)
    assert C.smooth_slope(H, W) <= 0.1
    ref = C.compose(H, W, ph, pw, True, C.hinv(cs["h"]), cs["img"].astype(np.float64), None)
    bound = C.smooth_curvature(H, W) / 8 * 2.0 ** 2
    norm_h, norm_w = H / max(H, W), W / max(H, W)
    gx = ((np.arange(W) + 0.5) / W * 2 - 1) * norm_w
    gy = ((np.arange(H) + 0.5) / H * 2 - 1) * norm_h
    truth = C.smooth_image(*np.meshgrid(gx, gy), H, W)
    cov = ref["wsum"] > 0
    err = np.abs(ref["image"] - truth)[:, cov].max()
    print("covered %.2f, overlap %.2f, image error %.2e, var max %.2e, bound %.2e" % (
        cov.mean(), (ref["count"] >= 2).mean(), err, ref["var"].max(), bound))
    assert cov.mean() > 0.2 and (ref["count"] >= 2).mean() > 0.1
    assert err <= bound + 1e-7  # (the patches are float32 values: 6e-8)
    assert 0 <= ref["var"].min() and ref["var"].max() <= bound ** 2
    assert (ref["image"][:, ~cov] == 0).all() and (ref["var"][ref["count"] < 2] == 0).all()


def test_feather_keeps_coverage_and_one_patch_is_a_copy():
    """Feathering changes weights, never membership (the 2^-10 floor); one identity patch without crop is the
    patch itself, every border pixel included (they sit on the validity line: E decides for them)."""
    cs = C.case(37, 50, 20, 24, 3, 0.05, seed=2)
    a = C.compose(37, 50, 20, 24, True, C.hinv(cs["h"]), cs["img"], cs["weight"])
    b = C.compose(37, 50, 20, 24, True, C.hinv(cs["h"]), cs["img"], cs["weight"], feather=True)
    assert np.array_equal(a["count"], b["count"]) and not np.array_equal(a["wsum"], b["wsum"])
    one = C.case(36, 48, 36, 48, 1, 0.0, crop=False)
    r = C.compose(36, 48, 36, 48, False, C.hinv(one["h"]), one["img"], None)
    assert (r["count"] == 1).all() and (r["var"] == 0).all()
    # the definition's +1e-8 in the divide moves a point by up to 1e-8 of its distance to the centre, W / 2 =
    # 24 px, and neighbouring pixels of the smooth image differ by at most 0.1
    assert np.abs(r["image"] - one["img"][0]).max() <= 1e-8 * 24 * 0.1


def test_seam_score_falls_at_the_true_warps():
    """gn_ref.realisable()'s problem (3 patches of 48 x 48 on 64 x 64, the frozen random image's own float64
    render at h* as the patches): the reference's seam_rmse at h* is below half its value at the start h* +
    0.01 noise (the noise realisable() uses; not raised)."""
    inputs, hstar, h0 = gn_ref.realisable(seed=3, noise=0.01)
    rgb = gn_ref.normal(inputs)["rgb"]  # [B, Np, 3] at h*
    img = rgb.reshape(3, 48, 48, 3).transpose(0, 3, 1, 2)
    s = {}
    for k, h in (("start", h0), ("true", hstar)):
        s[k] = C.scores(C.compose(64, 64, 48, 48, True, C.hinv(h), img, None))
    print("seam_rmse start %.3e, at h* %.3e; overlap %.2f" % (s["start"]["seam_rmse"], s["true"]["seam_rmse"], s["true"]["overlap"]))
    assert s["true"]["overlap"] > 0.3
    assert s["true"]["seam_rmse"] < 0.5 * s["start"]["seam_rmse"]
