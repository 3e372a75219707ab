"""Case table of the host buffer plans (helper module, not a test file; used by
test_plan_bytes_cpu.py and tools/make_plan_bytes.py).

Every kernel reads its buffers at byte offsets planned on the host (csrc/marf_abi.hip), and planning
needs no device: a geometry with d_H = 1 is never dereferenced.  record() returns, for every entry,
what the library's planning entry points give; tests/golden/plan_bytes.json holds the same from the
library of the commit named in it, so a change of the planning code that moves a byte shows.

The totals pin every region's size, not the regions' order: the forward and the backward take their
offsets from the same plan, so the order is checked by reading.

Entries that take different plan paths record different step totals on the 3-patch geometry (dzl
on / off, pipelined, fp16x2, plain bf16 on k_step2): test_plan_bytes_cpu.py checks that on the
fixture, so an entry that moved no byte would show as a duplicate.
"""
import contextlib
import ctypes
import os

FULL16 = [66, 256, 256, 256, 256, 3]   # the benchmark nets (C1 at L = 8, C3 at L = 16) are this wide
WIDE = [66] + [512] * 8 + [3]
GRID3 = {"MARF_STEP2_GRID": "3"}       # caps the persistent grid: the figure does not rest on the CU count

# every switch the planning code reads (csrc/marf_abi.hip); an entry runs with exactly its own set
# (MARF_WGRAD_FUSED is read once per process: the fixture holds its default, unset)
SWITCHES = ("MARF_STEP2", "MARF_STEP2_DZ", "MARF_STEP2_NW4", "MARF_STEP_NW", "MARF_PIPE", "MARF_PIPE_WG",
            "MARF_PIPE_PIECE", "MARF_DIAG_PREC", "MARF_STEP2_GRID", "MARF_F0_RECOMPUTE", "MARF_DZL_RECOMPUTE",
            "MARF_STEP2_GENERIC", "MARF_DH_SIDE", "MARF_WGRAD_FUSED")

# name: (patches, patch_H, patch_W), all on a 64 x 64 canvas
GEOMETRIES = {
    "3x16x20": (3, 16, 20),   # 320 pixels per patch: 9 tiles of 128, three padded patches
    "1x16x24": (1, 16, 24),   # 384 pixels: an odd tile count per block
    "2x8x8": (2, 8, 8),       # (the two-layer net's)
}

# name: (dims, L, precision, environment, options); options: "skip" layers, "pipeline" (mode, wg, piece)
NETS = {
    # ---- k_step2 and its siblings
    "s2-dzl-on": (FULL16, 16, "bf16x3", GRID3, {}),
    "s2-dzl-off": (FULL16, 16, "bf16x3", dict(GRID3, MARF_DZL_RECOMPUTE="0"), {}),
    "s2-dz": (FULL16, 16, "bf16x3", dict(GRID3, MARF_STEP2_DZ="1"), {}),
    "s2-fp16x2": (FULL16, 16, "fp16x2", GRID3, {}),
    "s2-bf16": (FULL16, 16, "bf16", dict(GRID3, MARF_STEP2="1"), {}),
    "s2-narrow": ([34, 128, 96, 128, 3], 8, "bf16x3", GRID3, {}),
    "s2-two-layer": ([2, 64, 3], 0, "bf16x3", GRID3, {}),
    # pipelined weight gradients, no grid override: G = CUs - R rests on 256 CUs, which both the
    # no-device fallback of the library's CU query and an MI355X give
    "s2-pipe": (FULL16, 16, "bf16x3", {}, {"pipeline": (1, 2, 2)}),
    # ---- the tile kernels
    "tile-c3-fp32": (FULL16, 16, "fp32", {}, {}),
    "tile-c3-bf16": (FULL16, 16, "bf16", {}, {}),
    "tile-c3-fp16": (FULL16, 16, "fp16", {}, {}),
    "tile-512-fp32": (WIDE, 16, "fp32", {}, {}),
    "tile-512-bf16": (WIDE, 16, "bf16", {}, {}),           # one 8-wave block at TP = 128
    "tile-512-fp16": (WIDE, 16, "fp16", {}, {}),
    "tile-512-bf16-nw4": (WIDE, 16, "bf16", {"MARF_STEP_NW": "4"}, {}),
    "split-512": (WIDE, 16, "bf16x3", {}, {}),             # k_mlp_step_split, TP = 64
    "split-256x6": ([66] + [256] * 6 + [3], 16, "bf16x3", {}, {}),   # k_mlp_step_split, TP = 128
    "tile-skip-fp32": ([34, 64, 64, 64, 3], 8, "fp32", {}, {"skip": [2]}),
}

# name: (precision, MaskNet shape); {}: the defaults of marf_hip.MaskNet
MASK_NETS = {
    "mask-default-fp32": ("fp32", {}),
    "mask-default-bf16x3a": ("bf16x3a", {}),
    "mask-small-fp32": ("fp32", dict(embed_dim=8, n_freqs=4, width=64, n_layers=3)),
    "mask-small-bf16x3a": ("bf16x3a", dict(embed_dim=8, n_freqs=4, width=64, n_layers=3)),
}

# entries that take different plan paths: their step totals on "3x16x20" differ.  (s2-dz is not
# among them: k_step2dz has no dz_{n-1} recompute, so it plans the bytes of s2-dzl-off; it differs
# from it in its packed program and in having no warp-only plan.)
DISTINCT = ("s2-dzl-on", "s2-dzl-off", "s2-pipe", "s2-fp16x2", "s2-bf16")


@contextlib.contextmanager
def _switches(env):
    old = {k: os.environ.get(k) for k in SWITCHES}
    try:
        for k in SWITCHES:
            os.environ.pop(k, None)
        os.environ.update(env)
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _geometry(name):
    import marf_hip
    B, ph, pw = GEOMETRIES[name]
    g = marf_hip.grid_geometry(B, 64, 64, ph, pw, None)
    g.d_H = 1  # planning reads no device memory
    return g


def _dtype(name):
    import marf_hip
    return getattr(marf_hip, "MARF_" + name.upper())


def record_net(name):
    import marf_hip
    dims, L, prec, env, opts = NETS[name]
    lib = marf_hip.lib()
    with _switches(env):
        n = marf_hip.Net(dims, L, _dtype(prec), skip=opts.get("skip", ()))
        if "pipeline" in opts:
            n.set_pipeline(*opts["pipeline"])
        res = {"step_kernel": n.step_kernel, "param_count": n.param_count, "packed_bytes": n.packed_bytes,
               "layer_spans": [list(s) for s in n.layer_spans], "geometries": {}}
        for gname in GEOMETRIES:
            g = ctypes.byref(_geometry(gname))
            res["geometries"][gname] = {
                "saved_bytes": lib.marf_saved_bytes(n.handle, g),
                "workspace_bytes": lib.marf_workspace_bytes(n.handle, g),
                "step_saved_bytes": lib.marf_step_saved_bytes(n.handle, g),
                "warp_step_saved_bytes": lib.marf_warp_step_saved_bytes(n.handle, g),  # 0: recipe refused
                "render_workspace_bytes": lib.marf_render_workspace_bytes(n.handle, g),
            }
    return res


def record_mask_net(name):
    import marf_hip
    prec, shape = MASK_NETS[name]
    with _switches({}):
        n = marf_hip.MaskNet(5, _dtype(prec), **shape)
        res = {"param_count": n.param_count, "packed_bytes": n.packed_bytes, "geometries": {}}
        for gname in GEOMETRIES:
            g = _geometry(gname)
            res["geometries"][gname] = {"saved_bytes": n.saved_bytes(g), "workspace_bytes": n.workspace_bytes(g)}
    return res


def record():
    return {"nets": {k: record_net(k) for k in NETS}, "mask_nets": {k: record_mask_net(k) for k in MASK_NETS}}
