"""marf_compose on the GPU against the float64 statement of tests/compose_ref.py, for its bits
(determinism, NULL arguments, the early-out's patches), its buffer bounds, and end to end: Model.evaluate's
seam score on the Levenberg-Marquardt registration of tests/test_gpu_gn_solver.py, and train.py's mosaic.eval.

Cases (canvas / patch / B / warp noise; h_0 = 0 throughout; compose_ref.case, seed 1): the smallest shapes at
which tile edges, the integer crop window, uncovered pixels and overlaps all occur, and "b66", 66 patches: more
than the 64 whose matrices one LDS chunk holds, so the kernel's chunk loop runs twice.  The patches are the smooth
image (slope <= 0.1 per pixel) sampled 0.2 off their warps, so overlapping patches disagree by some percent:
patches that agree to 3e-4 leave var at 1e-7, where torch's own float32 evaluation of the statement is 1e-4 of
var's max off.  Weights are random in [0, 1] with a zero rectangle in the patches b >= 1 (compose_ref.case says
why not in patch 0).  The kernel is given its inverse homographies by marf_sl3_to_SL3(-h); the reference takes
those very matrices.  A canvas pixel is left out only if the reference puts some patch's (r, c) within 1e-4 px of
a validity line."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import compose_ref as C
from test_gpu_parity import DEV, gpu, t  # noqa: F401 (gpu: fixture)

pytestmark = pytest.mark.gpu

SMALL = dict(H=37, W=50, ph=20, pw=24)
CASES = {
    "b3": dict(B=3, noise=0.05, **SMALL),
    "b5": dict(B=5, noise=0.1, **SMALL),
    "identity": dict(H=36, W=48, ph=36, pw=48, B=1, noise=0.0, crop=False),  # every border pixel on the validity line
    "b4": dict(H=64, W=80, ph=32, pw=40, B=4, noise=0.1),
    "off": dict(B=3, noise=0.05, special="off", **SMALL),    # the last patch wholly off the canvas
    "zero": dict(B=3, noise=0.05, special="zero", **SMALL),  # the last patch's weight map all zero
    "se2": dict(B=3, noise=0.1, special="se2", **SMALL),
    "b66": dict(B=66, noise=0.1, **SMALL),  # more patches than one LDS chunk of matrices (64) holds
}
# coverage and overlap of the float64 reference (weights on), as the test found them with the project's basis
# (26 to 100 % coverage, 23 to 30 % overlap on the multi-patch cases; no pixel of any case is left out)
FIGURES = {"b3": (0.264, 0.248), "b5": (0.504, 0.304), "identity": (1.0, 0.0), "b4": (0.387, 0.270), "off": (0.262, 0.232),
           "zero": (0.262, 0.232), "se2": (0.309, 0.227), "b66": (0.714, 0.562)}
_CASE, _REF = {}, {}


def case(name):
    if name not in _CASE:
        _CASE[name] = C.case(seed=1, misreg=0.2, **CASES[name])
    return _CASE[name]


def hinv_gpu(cs):
    """The inverse homographies as the product forms them, on the GPU: [B, 3, 3] float32."""
    import marf_hip
    if cs["p"] is not None:
        h = marf_hip.se2_to_sl3(t(cs["p"]))
        assert np.array_equal(h.cpu().numpy(), cs["h"])
    else:
        h = t(cs["h"])
    return marf_hip.sl3_to_SL3(-h)


def launch(cs, weight=True, feather=False, want_var=True, sub=None):
    import marf_hip
    Hi, img, wgt = hinv_gpu(cs), t(cs["img"]), t(cs["weight"]) if weight is True else weight
    if sub is not None:  # the first `sub` patches only
        Hi, img, wgt = Hi[:sub].contiguous(), img[:sub].contiguous(), None if wgt is None else wgt[:sub].contiguous()
    out = marf_hip.compose(cs["H"], cs["W"], cs["ph"], cs["pw"], cs["crop"], Hi, img, wgt, feather=feather, want_var=want_var)
    torch.cuda.synchronize()
    return out


def reference(name, feather=False):
    """(float64 reference, torch's float32 evaluation, excluded pixels) on the kernel's own Hinv: computed once."""
    key = (name, feather)
    if key not in _REF:
        cs = case(name)
        Hi = hinv_gpu(cs).cpu()
        assert np.abs(Hi.double().numpy() - C.hinv(cs["h"]).numpy()).max() <= 1e-6
        args = (cs["H"], cs["W"], cs["ph"], cs["pw"], cs["crop"])
        ref = C.compose(*args, Hi.double(), cs["img"], cs["weight"], feather)
        f32 = C.compose(*args, Hi, cs["img"], cs["weight"], feather, dtype=torch.float32)
        near = (ref["dist"].min(-1) < 1e-4).any(0)
        _REF[key] = (ref, f32, near)
    return _REF[key]


def _bits(x):
    return x.contiguous().view(torch.int32)


def _same(a, b):
    return all((x is None and y is None) or torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))


@pytest.mark.parametrize("feather", [False, True])
@pytest.mark.parametrize("name", list(CASES))
def test_against_float64(name, feather):
    """image, wsum and var within 1e-5 of each tensor's max (the project's fp32 rule, §11 / §13), count exact,
    on every pixel but those within 1e-4 px of a validity line (at most 1 %); coverage and overlap are the
    recorded ones.  feather = 1 is held to the same bound and its count is feather = 0's."""
    cs = case(name)
    ref, f32, near = reference(name, feather)
    image, wsum, count, var = [x.cpu().numpy().astype(np.float64) for x in launch(cs, feather=feather)]
    got = dict(image=image, wsum=wsum[0], count=count[0], var=var[0])
    s = C.scores(ref)
    line = [f"{name} feather={int(feather)}: excluded {near.mean():.4f} coverage {s['coverage']:.3f} overlap {s['overlap']:.3f}"]
    errs = {}
    for k in ("image", "wsum", "var"):
        mx = np.abs(ref[k]).max()
        errs[k] = np.abs(got[k] - ref[k])[..., ~near].max() / mx if mx > 0 else np.abs(got[k]).max()
        e32 = np.abs(f32[k] - ref[k])[..., ~near].max() / mx if mx > 0 else np.abs(f32[k]).max()
        line.append(f"{k} {errs[k]:.2e} (torch float32 {e32:.2e})")
    print(" | ".join(line))
    assert near.mean() <= 0.01
    cov, over = FIGURES[name]
    assert abs(s["coverage"] - cov) <= 0.01 and abs(s["overlap"] - over) <= 0.01, s
    assert np.array_equal(got["count"][~near], ref["count"][~near])
    for k, e in errs.items():
        assert e <= 1e-5, (k, e)
    assert got["var"].min() >= 0 and (got["var"][got["count"] < 2] == 0).all()
    assert (got["image"][:, got["wsum"] == 0] == 0).all()
    if feather:
        assert torch.equal(launch(cs)[2], launch(cs, feather=True)[2])


def test_special_cases_are_what_they_claim():
    """ "off": no canvas pixel accepts the last patch, and the result is, bit for bit, that of the other patches
    alone (the early-out drops it per block; the pixel test would per pixel).  "zero": the same for a patch
    whose weights are all zero.  "identity": one patch, no crop -- the mosaic is the patch, borders included."""
    for name in ("off", "zero"):
        cs = case(name)
        ref, _, _ = reference(name)
        assert ref["valid"][-1].any() == (name == "zero")
        assert _same(launch(cs), launch(cs, sub=cs["B"] - 1)), name
    cs = case("identity")
    image, wsum, count, var = launch(cs, weight=None)
    assert bool((count == 1).all()) and bool((wsum == 1).all()) and bool((var == 0).all())
    assert float((image - t(cs["img"][0])).abs().max()) <= 1e-6


def test_bits():
    """Two launches are identical; d_weight = NULL gives the bits of an explicit map of ones; d_var = NULL and
    d_count = NULL leave image and wsum bits unchanged."""
    import marf_hip
    cs = case("b5")
    a = launch(cs)
    assert _same(a, launch(cs))
    ones = torch.ones_like(t(cs["weight"]))
    for feather in (False, True):
        assert _same(launch(cs, weight=None, feather=feather), launch(cs, weight=ones, feather=feather)), feather
    b = launch(cs, want_var=False)
    assert b[3] is None and _same(a[:3], b[:3])
    Hi, img, wgt = hinv_gpu(cs), t(cs["img"]), t(cs["weight"])
    image, wsum = torch.zeros_like(a[0]), torch.zeros_like(a[1])
    p = lambda x: ctypes.c_void_p(x.data_ptr())  # noqa: E731
    rc = marf_hip.lib().marf_compose(cs["H"], cs["W"], cs["ph"], cs["pw"], 1, cs["B"], p(Hi), p(img), p(wgt), 0, p(image),
                                     p(wsum), None, None, None)
    torch.cuda.synchronize()
    assert rc == 0 and _same(a[:2], (image, wsum))


@pytest.mark.parametrize("name", ["b5", "b4"])
def test_guard_bytes(name):
    """1 MiB of guard bytes behind each of the four outputs is untouched, and the outputs are the binding's."""
    import marf_hip
    cs = case(name)
    want = launch(cs)
    n = cs["H"] * cs["W"] * 4
    guard = 1 << 20
    bufs = [torch.full((k * n + guard,), 0xA5, dtype=torch.uint8, device=DEV) for k in (3, 1, 1, 1)]
    Hi, img, wgt = hinv_gpu(cs), t(cs["img"]), t(cs["weight"])
    p = lambda x: ctypes.c_void_p(x.data_ptr())  # noqa: E731
    rc = marf_hip.lib().marf_compose(cs["H"], cs["W"], cs["ph"], cs["pw"], 1, cs["B"], p(Hi), p(img), p(wgt), 0,
                                     *[p(b) for b in bufs], None)
    torch.cuda.synchronize()
    assert rc == 0
    for k, b, w in zip((3, 1, 1, 1), bufs, want):
        assert bool((b[k * n:] == 0xA5).all())
        assert torch.equal(b[:k * n].view(torch.int32), _bits(w).reshape(-1))


@pytest.mark.parametrize("prec", ["fp32", "bf16x3"])
def test_seam_score_falls_with_the_registration(prec, tmp_path):
    """The realisable problem registered with warp_solver: lm (tests/test_gpu_gn_solver.py): Model.evaluate's
    seam_rmse after 10 iterations is within 1e-5 (absolute, pixel-value units) of the float64 reference at the
    same warps, and below half the product's own value at the start."""
    from test_gpu_gn_solver import _problem
    m, var, inputs, hstar, h0 = _problem(prec, tmp_path)
    start = m.evaluate()
    for _ in range(10):
        m.graph.lm_step(var)
        m.graph.warp_param.weight.data[0] = 0  # (Model.train's loop: fix_first)
    end = m.evaluate()
    h = m.graph.warp_param.weight.detach().cpu().numpy().astype(np.float64)
    ref = C.scores(C.compose(64, 64, 48, 48, True, C.hinv(h), m.images.rgb.cpu().numpy().astype(np.float64), None))
    print(prec, "seam_rmse start %.3e end %.3e float64 reference %.3e" % (start["seam_rmse"], end["seam_rmse"], ref["seam_rmse"]),
          "| coverage %.3f overlap %.3f" % (end["coverage"], end["overlap"]))
    assert set(end) == {"coverage", "overlap", "seam_rmse"}  # no gt: no PSNR keys
    assert abs(end["seam_rmse"] - ref["seam_rmse"]) <= 1e-5
    assert abs(end["coverage"] - ref["coverage"]) <= 1e-3 and abs(end["overlap"] - ref["overlap"]) <= 1e-3
    assert end["seam_rmse"] < 0.5 * start["seam_rmse"]
    if prec == "fp32":  # with a gt image the two PSNRs are the masked-MSE kernel's on the mosaic and the render
        m.images.gt = t(np.random.default_rng(0).random((3, 64, 64)).astype(np.float32))
        mo = m.compose_mosaic()
        ev = m.evaluate(mo)
        cov = (mo.wsum > 0).expand(3, -1, -1)
        want = -10 * np.log10(float(((mo.image - m.images.gt)[cov].double() ** 2).mean()))
        assert abs(ev["psnr_mosaic_gt"] - want) <= 1e-3
        frame = m.predict_entire_image().to(DEV)
        want = -10 * np.log10(float(((frame - m.images.gt).double() ** 2).mean()))
        assert abs(ev["psnr_render_gt"] - want) <= 1e-3


def _model_reference(m, weight):
    """The float64 reference of the model's mosaic at its current warps with `weight` [B, h*w] values."""
    import marf_hip
    o = m.opt
    Hi = marf_hip.sl3_to_SL3(-m.graph.warp_h().detach()).cpu().double()  # the inverse warps as the model forms them
    img = m.images.rgb.cpu().numpy().astype(np.float64)
    ph, pw = (o.patch_H, o.patch_W) if o.use_cropped_images else (o.H, o.W)
    w = weight.detach().cpu().numpy().astype(np.float64).reshape(img.shape[0], 1, img.shape[2], img.shape[3])
    return C.compose(o.H, o.W, ph, pw, bool(o.use_cropped_images), Hi, img, w)


def _check_model_mosaic(mo, ref):
    near = (ref["dist"].min(-1) < 1e-4).any(0)
    wsum = mo.wsum[0].cpu().numpy().astype(np.float64)
    assert near.mean() <= 0.01 and ref["wsum"].max() > 0
    assert all(bool(torch.isfinite(x).all()) for x in (mo.image, mo.wsum, mo.count, mo.var))
    assert np.abs(wsum - ref["wsum"])[~near].max() <= 1e-5 * ref["wsum"].max()
    assert np.array_equal(mo.count[0].cpu().numpy()[~near], ref["count"][~near])


def test_learned_weights(tmp_path):
    """compose_mosaic(weights='learned'): the implicit mask network's prediction [B, h*w, 1] is the weight map
    -- a finite mosaic whose wsum and count are the reference's on the same weights."""
    from test_gpu_parity import small_setup
    z, m, var, nl = small_setup("a", "fp32", tmp_path, use_implicit_mask=True, mosaic={"weights": "learned"})
    mo = m.compose_mosaic()
    with torch.no_grad():
        wgt = m.graph.predict_mask(m.images.rgb)
    assert wgt.shape == (m.batch_size, int(m.graph.h) * int(m.graph.w), 1)
    _check_model_mosaic(mo, _model_reference(m, wgt))
    assert _same(tuple(mo.values()), tuple(m.compose_mosaic(weights="learned").values()))


def test_robust_weights(tmp_path):
    """compose_mosaic(weights='robust'): refused with the reason before any lm iteration; after one, the IRLS
    weights lm_last.weight [B, h*w] are the weight map."""
    from test_gpu_gn_solver import _problem
    m, var, inputs, hstar, h0 = _problem("fp32", tmp_path, lm={"robust": "cauchy", "robust_delta": 0.01},
                                         mosaic={"weights": "robust"})
    with pytest.raises(RuntimeError, match="run an lm iteration first"):
        m.compose_mosaic()
    m.graph.lm_step(var)
    wgt = m.graph.lm_last.weight
    assert wgt.shape == (3, 48 * 48) and 0 < float(wgt.min()) and float(wgt.max()) <= 1
    _check_model_mosaic(m.compose_mosaic(), _model_reference(m, wgt))


def test_evaluate_without_coverage(tmp_path):
    """Every weight zero: coverage 0, seam_rmse and psnr_mosaic_gt NaN (not an error), psnr_render_gt finite."""
    from test_gpu_gn_solver import _problem
    m, var, inputs, hstar, h0 = _problem("fp32", tmp_path)
    m.images.masks = torch.zeros_like(m.images.masks)
    m.images.gt = t(np.random.default_rng(0).random((3, 64, 64)).astype(np.float32))
    ev = m.evaluate()
    assert ev["coverage"] == 0 and ev["overlap"] == 0
    assert np.isnan(ev["seam_rmse"]) and np.isnan(ev["psnr_mosaic_gt"]) and np.isfinite(ev["psnr_render_gt"])


def test_train_py_writes_the_mosaic(tmp_path):
    """train.py --mosaic.eval=true on the golden C1 patches, 3 iterations of a small net: mosaic.npy is float32
    [3, 360, 480], eval.json holds finite coverage and overlap and no gt keys; with a gt array in a copy of the
    npz both PSNR keys are there, finite."""
    from conftest import GOLDEN, PKG
    z = np.load(os.path.join(GOLDEN, "cat_batch3_c1.npz"))
    gt = np.random.default_rng(0).integers(0, 256, (3, 360, 480), dtype=np.uint8)
    np.savez(tmp_path / "gt.npz", rgb=z["rgb"], mask=z["mask"], gt=gt)
    for name, npz in (("plain", os.path.join(GOLDEN, "cat_batch3_c1.npz")), ("gt", str(tmp_path / "gt.npz"))):
        cmd = [sys.executable, "train.py", "--group=mosaic", "--model=planar", "--yaml=planar", "--seed=3",
               "--barf_c2f=[0,0.4]", f"--dataset_npz={npz}", "--arch.layers=[null,64,64,3]", "--max_iter=3",
               "--use_edges=false", "--freq.scalar=1", "--freq.vis=1000", f"--output_root={tmp_path}", f"--name={name}",
               "--mosaic.eval=true"]
        r = subprocess.run(cmd, cwd=PKG, capture_output=True, text=True, timeout=240)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        out = tmp_path / "mosaic" / f"{name}_seed3"
        mosaic = np.load(out / "mosaic.npy")
        assert mosaic.dtype == np.float32 and mosaic.shape == (3, 360, 480) and np.isfinite(mosaic).all()
        ev = json.loads((out / "eval.json").read_text())
        assert np.isfinite(ev["coverage"]) and np.isfinite(ev["overlap"]) and 0 < ev["coverage"] <= 1
        keys = {"psnr_mosaic_gt", "psnr_render_gt"}
        if name == "gt":
            assert keys <= set(ev) and all(np.isfinite(ev[k]) for k in keys), ev
        else:
            assert not (keys & set(ev)), ev
