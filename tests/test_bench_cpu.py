"""bench.py --dump-outputs (bench.dump_outputs) on a CPU stand-in for the model: the files it writes,
their dtypes, the 64 MB bound and the fixed row sample of a large prediction; no kernels run."""
import os

import numpy as np
import torch

from util import EasyDict as edict


def _model(B):
    torch.manual_seed(0)
    mlp = torch.nn.ModuleList([torch.nn.Linear(6, 8), torch.nn.Linear(8, 3)])
    warp = torch.nn.Embedding(B, 8)
    for p in list(mlp.parameters()) + [warp.weight]:
        p.grad = torch.full_like(p, 0.5)
    return edict(graph=edict(neural_image=edict(mlp=mlp), warp_param=warp))


def _dump(tmp_path, name, rows, B=3):
    import bench
    m = _model(B)
    v = edict(rgb_prediction=torch.arange(rows * 3, dtype=torch.float32).view(1, rows, 3))
    out = str(tmp_path / name)
    bench.dump_outputs(out, m, v, edict(rgb=torch.tensor(0.25)))
    files = {f[:-4]: np.load(os.path.join(out, f)) for f in os.listdir(out)}
    assert all(a.dtype in (np.float32, np.float64) for a in files.values())
    return m, v, files


def test_dump_outputs_small(tmp_path):
    m, v, d = _dump(tmp_path, "a", 50)
    assert set(d) == {"rgb_prediction", "loss_rgb", "mlp_params", "warp_params", "mlp_grads", "warp_grads"}
    np.testing.assert_array_equal(d["rgb_prediction"], v.rgb_prediction.numpy().reshape(-1, 3))
    assert d["loss_rgb"].tolist() == [0.25]
    l0, l1 = m.graph.neural_image.mlp
    want = np.concatenate([t.detach().numpy().ravel() for t in (l0.weight, l0.bias, l1.weight, l1.bias)])
    np.testing.assert_array_equal(d["mlp_params"], want)
    np.testing.assert_array_equal(d["mlp_grads"], np.full(want.size, 0.5, np.float32))
    np.testing.assert_array_equal(d["warp_params"], m.graph.warp_param.weight.detach().numpy().ravel())
    assert d["warp_grads"].shape == (24,)


def test_dump_outputs_samples_large_predictions(tmp_path, monkeypatch):
    import bench
    assert bench.DUMP_BUDGET + 1024 * 8 <= 64 * 10 ** 6  # eight files and their headers within 64 MB
    monkeypatch.setattr(bench, "DUMP_BUDGET", 3000)
    _, v, d = _dump(tmp_path, "a", 1000)
    _, _, d2 = _dump(tmp_path, "b", 1000)
    rows = d["rgb_prediction_rows"].astype(np.int64)
    other = sum(a.nbytes for k, a in d.items() if not k.startswith("rgb_prediction"))
    assert rows.size == (3000 - other) // 20 > 50 and np.all(np.diff(rows) > 0) and rows[0] >= 0 and rows[-1] < 1000
    np.testing.assert_array_equal(d["rgb_prediction"], v.rgb_prediction.numpy().reshape(-1, 3)[rows])
    np.testing.assert_array_equal(d["rgb_prediction_rows"], d2["rgb_prediction_rows"])  # the same sample every run
    assert sum(a.nbytes for a in d.values()) <= 3000
