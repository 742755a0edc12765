"""GPU parity of a chain network with stride-2 grouped conv layers (NitiModel.from_chain(level=6)) against the step
reference of tests/grouped_stride2_cases.py: three steps at batch 4, every layer's weights after each step and the
logits, bit for bit (the level record and the default routing's refusal: tests/test_grouped_stride2_cpu.py)."""
import numpy as np
import pytest

import grouped_stride2_cases as G2
from test_gpu_grouped_ops import T  # noqa: F401 -- the GPU fixture

pytestmark = pytest.mark.gpu


def _model(batch=G2.BATCH, level=6):
    from niti_amd.model import NitiModel
    m = NitiModel.from_chain(G2.NET_S[2], G2.NET_S[0], G2.NET_S[1], batch, level=level)
    m.init_weights(3)
    return m


@pytest.mark.parametrize("graph,keep", [(False, True), (True, True), (False, False)])
def test_three_steps(T, graph, keep):
    """Eagerly, as a captured graph (replayed twice), and without the gradient taps."""
    layers, W, S, data, ref = G2.reference()
    m = _model()
    assert [(l["stride"], l.get("groups", 1), l["h"], l["oh"]) for l in m.layers] == \
           [(l["stride"], l["groups"], l["h"], 1 if l["gpool"] else (l["h"] + 2 * l["pad"] - l["k"]) // l["stride"] + 1)
            for l in layers][:5] + [(2, 2, 8, 4), (1, 1, 1, 1)]
    assert all(np.array_equal(m.get_weight(i), w) for i, w in enumerate(W))
    m.set_graph(graph)
    m.keep_grads(keep)
    xd, ld = T.from_numpy(data[0][0].copy()).cuda(), T.from_numpy(data[0][1].copy()).cuda()
    for step, ((x, labels), (newW, rec)) in enumerate(zip(data, ref)):
        xd.copy_(T.from_numpy(x.copy()))  # (the same device buffers: a captured graph replays)
        ld.copy_(T.from_numpy(labels.copy()))
        m.train_step(xd, -3, ld)
        logits, e = m.logits()
        assert e == rec["exp"][-1] and np.array_equal(logits, rec["logits"]), step
        for i, w in enumerate(newW):
            assert np.array_equal(m.get_weight(i), w), ("w", step, i)
    assert m.rowconv_error() == 0
    assert not any(layers[i]["groups"] > 1 for i, _ in m.plans())  # no GEMM plan on such a layer

