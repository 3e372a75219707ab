"""The plain 16-bit tile recipe without a GPU: that its torch statement (tests/plain16_ref.py) is the
reference's network when nothing is rounded, that each case (tests/plain16_cases.py) reaches the kernels its
table names, and that the inputs and bounds of tests/test_gpu_plain16.py are conditions on the statement
that hold before any kernel runs.  Measured values: profiles/plain16/README.md."""
import ctypes

import numpy as np
import pytest

import bf16x3_tile_ref as R
import plain16_cases as C
import plain16_ref as P

NUMERIC = [k for k in C.ALL if not C.CASES[k]["env"]]  # (a row with a switch has another row's inputs)


@pytest.fixture(scope="module")
def lib():
    import build_lib
    return ctypes.CDLL(build_lib.build(verbose=False))


@pytest.mark.parametrize("case", C.ALL)
def test_table_and_plan(lib, case, monkeypatch):
    """The case table against the restated rules (plain16_cases.plan), and those against what the ABI gives
    out: both 16-bit types run k_mlp_step, and marf_step_saved_bytes is plan()'s total -- its ReLU records are
    S / TP x NW KB a layer and its per-tile partials S / TP, so the figure moves with (TP, NW): 4 waves at
    TP 128, 8 waves at TP 128 and 4 waves at TP 64 all differ.  BL, SK and the weight-gradient picks show in
    no figure the ABI gives out; wg_pick's own rows are pinned by the static_asserts beside it."""
    import marf_hip
    for v in C.SWITCHES:
        monkeypatch.delenv(v, raising=False)
    c = C.CASES[case]
    for k, v in c["env"].items():
        monkeypatch.setenv(k, v)
    p = C.plan(case)
    (tp, nw, bl, sk), picks = C.REACHES[case]
    assert (p["TP"], p["NW"], p["BL"], p["SK"]) == (tp, nw, bl, sk), (case, p)
    assert p["picks"] == picks, (case, p["picks"])
    geo = marf_hip.grid_geometry(c["B"], C.CANVAS, C.CANVAS, c["ph"], c["pw"], None)
    geo.d_H = 1  # planning reads no device memory
    for dt in (marf_hip.MARF_BF16, marf_hip.MARF_FP16):
        net = marf_hip.Net(C.dims(case), c["L"], dt, skip=c["skip"])
        assert net.step_kernel == "k_mlp_step"
        assert net.step_saved_bytes(geo) == p["step_saved_bytes"], (case, net.step_saved_bytes(geo), p["step_saved_bytes"])
    if c["env"].get("MARF_STEP_NW") == "4":  # the switch moved the plan
        monkeypatch.delenv("MARF_STEP_NW")
        assert marf_hip.Net(C.dims(case), c["L"], marf_hip.MARF_BF16).step_saved_bytes(geo) != p["step_saved_bytes"]


@pytest.mark.parametrize("case", NUMERIC)
def test_unrounded_statement_is_the_reference(case):
    """T = None (nothing rounded, float64 throughout) equals cpu_ref.CpuRefStep in float64, skip nets
    included: rgb, loss, every gradient tensor and d warp to 1e-10 of the tensor's max (measured <= 3e-14)."""
    inp = C.inputs(case, "bf16")
    got, ref = P.step(*inp, T=None), R.truth(inp)
    e = P.errs(got, ref)
    rgb = float(np.abs(got["rgb"] - ref["rgb"]).max())
    print(case, "unrounded vs cpu_ref: rgb %.1e loss %.1e worst tensor %.1e" % (rgb, abs(got["loss_rgb"] / ref["loss_rgb"] - 1), max(e)))
    assert rgb <= 1e-10 and abs(got["loss_rgb"] / ref["loss_rgb"] - 1) <= 1e-10
    assert max(e) <= 1e-10, (case, e)


@pytest.mark.parametrize("case", [k for k in NUMERIC if not C.CASES[k]["skip"]])
def test_bf16_is_the_split_recipe_without_its_lo_terms(case):
    """bf16, no skip: the statement equals bf16x3_tile_ref.step with its four lo terms dropped, bit for bit
    under float64 accumulation -- rgb, every weight gradient, every hidden bias gradient, d warp.  db_last is
    summed in float32 by torch there and in `acc` here (so that it has an accumulation error at all): equal
    to 1e-6 of its max, float32's rounding of 960 terms."""
    inp = C.inputs(case, "bf16")
    got = P.step(*inp, T="bf16")
    ref = R.step(*inp, drop=("fwd_hl", "fwd_lh", "dgrad_wl", "dgrad_dzl"))
    n = len(inp[1])
    assert np.array_equal(got["rgb"], ref["rgb"])
    for i, (a, b) in enumerate(zip(P.flat(got), P.flat(ref))):
        if i == 2 * n - 1:
            assert P.err(a, b) <= 1e-6, (case, P.err(a, b))
        else:
            assert np.array_equal(a, b), (case, i, P.err(a, b))


@pytest.mark.parametrize("T", C.TYPES)
@pytest.mark.parametrize("case", NUMERIC)
def test_bound_conditions(case, T):
    """What tests/test_gpu_plain16.py rests on, from the statement alone (plain16_ref.held):
      * the pixels left out (the per-layer kink rule and the rounding-flip rule together) are at most 6 %: the
        project's 8 % cap less the 2 % the GPU test allows the prologue's differing pixels; at least 256
        unmasked pixels remain; none of eight float32 summation orders takes a ReLU decision the float64 one
        does not;
      * every gradient tensor, d warp included, is touched by a defect;
      * for every tensor a defect touches, the defect moves it by >= 10 x the tensor's accumulation error in
        the first float32 order (E_mut_i >= 10 E_sum_i) -- at the row's seed (plain16_cases: Seeds);
      * every defect is >= 3 x above every bound the GPU test asserts on a tensor it touches: sqrt(max(E_sum_i,
        one flip's worth) min E_mut_i) on the MLP tensors, max(1e-5, 3 E32, 3 x the larger of d warp's own order noise and one flip's worth)
        on d warp.
    plain16_cases.NOT_HELD names the three tensors of two fp16 rows where no seed of 150 meets the last two
    (separation 2 to just under 3 x there); this test holds the list to the statement, no more and no fewer.
    The GPU test asserts the bound on them all the same."""
    h = P.held(case, T)
    nl = len(h["inputs"][1])
    names = [f"{k}{l}" for l in range(nl) for k in ("dW", "db")] + ["dh"]
    print("HELD", case, T, "seed %d kink %.4f (per-layer rule %.4f, |z| < %.1e) left %d | rgb bound %.1e (first order %.1e, one flip %.1e) loss32 %.1e "
          "E32 %.1e dh order noise %.1e" % (C.seed_of(case, T), h["out"], h["out_layer"], h["thr"], h["left"], h["rgb_bound"], h["rgb32"],
                                            h["rgb_flip"], h["loss32"], h["e32"], h["dh_noise"]))
    for i, nm in enumerate(names):
        print("HELD", case, T, nm, "E_sum %.1e one flip %.1e min E_mut %.1e bound %.1e (defect / bound %.1f) |" %
              (h["e_sum"][i], h["e_flip"][i] if i < 2 * nl else h["dh_flip"], h["e_min"][i], h["bound"][i], h["e_min"][i] / h["bound"][i]),
              " ".join("%s %.1e" % (mu, h["e_mut"][mu][i]) for mu in h["e_mut"] if i in P.touched(mu, nl)))
    assert h["out"] <= 0.06 and h["left"] >= 256, (case, T, h["out"], h["left"])
    assert h["relu_flips"] == 0, (case, T, h["relu_flips"])  # no order of the eight takes another ReLU decision
    assert sorted(set(i for mu in h["e_mut"] for i in P.touched(mu, nl))) == list(range(2 * nl + 1)), (case, T)
    not_held = C.NOT_HELD.get((case, T), ())
    assert [nm for nm, ok in zip(names, h["held"]) if not ok] == list(not_held), (case, T, h["held"])
    for mu, e in h["e_mut"].items():
        for i in P.touched(mu, nl):
            if names[i] not in not_held:
                assert e[i] >= 10 * h["e_sum"][i], (case, T, mu, names[i], e[i], h["e_sum"][i])
                assert e[i] >= 3 * h["bound"][i], (case, T, mu, names[i], e[i], h["bound"][i])


@pytest.mark.parametrize("T", C.TYPES)
@pytest.mark.parametrize("case", ["p-tp128", "p-wide8", "p-skip"])
def test_the_bounds_see_what_the_contract_cannot(case, T):
    """The mutation check: each defect, compared with the statement as the kernel is, misses the bound of a
    tensor it touches; (a), (b), (d) and (f) stay inside max(1e-2, 2 E_emu) of float64 on every tensor, where
    the contract bound cannot see them."""
    h = P.held(case, T)
    nl = len(h["inputs"][1])
    t64 = R.truth(h["inputs"])
    e_emu = P.errs(h["emu"], t64)
    for mu in P.mutations_for(T):
        mut = P.step(*h["inputs"], T=T, features=h["features"], mutate=mu)
        e = P.errs(mut, h["emu"])
        assert any(e[i] > h["bound"][i] for i in P.touched(mu, nl)), (case, T, mu)
        if mu in ("wlast_no_gl", "dgrad_full_g", "dz_trunc", "blast_rounded"):
            e64 = P.errs(mut, t64)
            assert all(a <= max(1e-2, 2 * b) for a, b in zip(e64, e_emu)), (case, T, mu, e64, e_emu)


def test_warp_grad_from_the_statements_own_dz():
    """warp_grad_from_dz fed the statement's own dz gives the statement's d warp bits (p-skip: the skip
    layer's posenc share included)."""
    for case in ("p-tp128", "p-skip"):
        h = P.held(case, "bf16")
        skip = C.CASES[case]["skip"]
        dz = {l: h["emu"]["dzs"][l].numpy() for l in (0,) + tuple(skip)}
        got = P.warp_grad_from_dz(h["inputs"], "bf16", dz, features=h["features"])
        assert np.array_equal(got, h["emu"]["dh"]), case
