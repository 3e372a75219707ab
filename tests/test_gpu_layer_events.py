"""A layer's event marks its gradient final, on every path of the step backward.

marf_step_backward_ev records event l on the step's stream once layer l's weight and bias gradient are
written (last layer first), so that a layer's all-reduce may start while the other layers' weight
gradients still run.  One driver records them for the per-layer, the pipelined and the tile paths, the
fused path after its one reduction launch.  Here a side stream waits for event l and copies layer l's
span of the flat gradient at once; after the device has drained, every copy must equal the final
gradient, and the step's digests are the fixture's, since events change no bit.  A correct build always
passes; a wrong order is not caught in every run.
"""
import json

import pytest
import torch

import step2_sched_cases as sc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", ["acc", "wg-perlayer", "wg-ranged", "tile-bf16"])
def test_layer_events_mark_final_gradients(case, monkeypatch):
    import marf_hip
    dev = torch.device(sc.DEV)
    m, var = sc.build(case, monkeypatch.setenv)
    engine = m.graph.neural_image.engine(dev)
    n_layers = len(engine.net.layer_spans)
    ev = marf_hip.GradEvents(n_layers, dev)
    engine.grad_events = ev
    out = sc.step(m, var)
    flat = engine.last_flat_grad
    side = torch.cuda.Stream(dev)
    snaps = []
    with torch.cuda.stream(side):
        for l, (off, n) in enumerate(engine.net.layer_spans):
            side.wait_event(ev.events[l])
            snaps.append(flat[off:off + n].clone())
    torch.cuda.synchronize(dev)
    assert engine.events_for == flat.data_ptr(), case
    bad = [l for l, (off, n) in enumerate(engine.net.layer_spans) if not torch.equal(snaps[l], flat[off:off + n])]
    assert not bad, (case, bad)
    ref = json.load(open(sc.BITS_JSON))["cases"][case]["bits"]
    assert {k: sc.digest(v) for k, v in out.items()} == ref, case
