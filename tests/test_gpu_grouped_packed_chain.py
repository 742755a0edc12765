"""GPU parity of a chain network with grouped layers of group width 24 (stride 1, 72 channels) and 48 (stride 2)
(NitiModel.from_chain(level=8)) against the step reference of tests/grouped_cases.py: two steps at batch 4, every
layer's weights after each step and the logits, bit for bit, and one save / load round trip."""
import numpy as np
import pytest

import grouped_cases as GC
from grouped_cases import DC
from test_gpu_grouped_ops import T  # noqa: F401 -- the GPU fixture
from test_grouped_packed_cpu import NET  # a RegNetX-1.6GF stage-1 block at cg 24, a strided grouped layer at cg 48

pytestmark = pytest.mark.gpu


BATCH = 4


def test_two_steps_and_a_snapshot(T, tmp_path):
    from niti_amd.model import NitiModel
    layers = GC.derive(NET)
    W, S = GC.init_weights(layers, 3)
    m = NitiModel.from_chain(NET[2], NET[0], NET[1], BATCH, level=8)
    m.init_weights(3)
    assert [(l.get("groups", 1), l["h"]) for l in m.layers] == [(1, 8), (1, 8), (3, 8), (1, 8), (1, 8), (2, 8), (1, 4), (1, 1)]
    assert all(np.array_equal(m.get_weight(i), w) for i, w in enumerate(W))
    cur = W
    for step, (x, labels) in enumerate(DC.batches(layers, BATCH, 2, 1)):
        cur, rec = GC.chain_step_ref(layers, cur, S, x, -3, labels)
        m.train_step(T.from_numpy(x.copy()).cuda(), -3, T.from_numpy(labels.copy()).cuda())
        logits, e = m.logits()
        assert e == rec["exp"][-1] and np.array_equal(logits, rec["logits"]), step
        for i, w in enumerate(cur):
            assert np.array_equal(m.get_weight(i), w), ("w", step, i)
    assert not np.array_equal(cur[2], W[2]) and not np.array_equal(cur[5], W[5])  # (the grouped layers learned)
    path = str(tmp_path / "a.safetensors")
    m.save(path)
    same = NitiModel.from_chain(NET[2], NET[0], NET[1], BATCH, level=8)
    same.load(path)
    assert same.chain_level == 8 and all(np.array_equal(same.get_weight(i), w) for i, w in enumerate(cur))
