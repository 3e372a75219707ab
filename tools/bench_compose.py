"""Time marf_compose with the library's profile scope: the median of 20 launches after warm-up.

    python tools/bench_compose.py [--label NAME] [--launches 20] [--warmup 5]

Two geometries: C1 (360 x 480 canvas, 5 patches of 180 x 240) and C3 (512 x 512 canvas, 64 patches of 256 x 256,
BASELINE.md's patch count and size), seeded warps of noise 0.1 with patch 0 at the identity, random images and
weights (the time does not depend on the values), weights on, var and count on.  One JSON line per geometry:
the times, the bytes the kernel must move at least (outputs written once, every patch image and weight map read
once), the time those bytes take at 6.3 TB/s (the achievable HBM rate) and a sha1 of the four outputs, so two
builds (MARF_LIB=..., the early-out A/B) can be compared for time and for bits.
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "masking-bundle-adjusting-neural-radiance-fields_amd"))

import marf_hip  # noqa: E402

GEOMETRIES = {"C1": (360, 480, 180, 240, 5), "C3": (512, 512, 256, 256, 64)}
HBM_BYTES_PER_S = 6.3e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--label", default="default")
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    marf_hip.lib()
    for name, (H, W, ph, pw, B) in GEOMETRIES.items():
        rng = np.random.default_rng(7)
        h = (0.1 * rng.standard_normal((B, 8))).astype(np.float32)
        h[0] = 0
        img = torch.from_numpy(rng.random((B, 3, ph, pw)).astype(np.float32)).to(dev)
        wgt = torch.from_numpy(rng.random((B, 1, ph, pw)).astype(np.float32)).to(dev)
        Hinv = marf_hip.sl3_to_SL3(-torch.from_numpy(h).to(dev))
        for _ in range(a.warmup):
            out = marf_hip.compose(H, W, ph, pw, True, Hinv, img, wgt)
        torch.cuda.synchronize()
        marf_hip.profile_enable(True)
        marf_hip.profile_filter(["compose"])
        ms = []
        for _ in range(a.launches):
            marf_hip.profile_reset()
            out = marf_hip.compose(H, W, ph, pw, True, Hinv, img, wgt)
            torch.cuda.synchronize()
            tot, n = marf_hip.profile_read()["compose"]
            assert n == 1
            ms.append(tot)
        marf_hip.profile_enable(False)
        marf_hip.profile_filter(None)
        sha = hashlib.sha1()
        for x in out:
            sha.update(x.cpu().numpy().tobytes())
        count = out[2]
        min_bytes = 6 * 4 * H * W + B * 4 * 4 * ph * pw
        print(json.dumps(dict(label=a.label, lib=os.path.basename(marf_hip.LIB_PATH), geometry=name, canvas=[H, W],
                              patch=[ph, pw], B=B, launches=a.launches, ms_median=float(np.median(ms)), ms_min=min(ms),
                              ms_max=max(ms), min_bytes=min_bytes, ms_at_hbm_rate=min_bytes / HBM_BYTES_PER_S * 1e3,
                              ratio=float(np.median(ms)) / (min_bytes / HBM_BYTES_PER_S * 1e3),
                              coverage=float((out[1] > 0).float().mean()), mean_count=float(count.mean()),
                              sha1=sha.hexdigest())), flush=True)


if __name__ == "__main__":
    main()
