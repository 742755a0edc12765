"""The plain two-launch forms of the step drivers at model level: range launch, [MAX], requantise
launch, neither fused nor speculative.

NITI_RC_SPEC2=0 (the row kernels) and NITI_RES_SPEC=0 (ResNet's residual sums) are read once per
process, so the checks run in one fresh child.  A captured step and a data-parallel step cannot take
the fused launches, so with both pairs off they take the plain forms: the row kernels at 16 / 8 / 4 /
2 px (the K-split form and the W = 1 head among them), the residual sums, and the GEMM phases of
ResNet's strided convs.  Every tap, the logits and every updated weight against the oracle
(niti_model_ref.py, niti_resnet_ref.py), bit for bit.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def T():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import niti_amd  # noqa: F401
    return torch


def _vgg11_graph(T):
    """VGG-11 at 32 px, batch 4, two steps: the first captures the step, the second replays it."""
    import niti_amd
    import niti_model_ref as R
    import test_gpu_model as TM
    TM._run(T, niti_amd.ARCH_VGG11, R.vgg11_layers(), batch=4, steps=2, seed=71, graph=True)


def _resnet18_graph(T):
    """ResNet-18 at 32 px, batch 2, 10 classes, two steps on one pair of device buffers under
    set_graph(True): capture, then replay."""
    import niti_resnet_ref as RR
    import test_gpu_resnet_cpp as TR
    hw, batch, classes = 32, 2, 10
    convs = RR.resnet18_convs(hw, classes)
    W, S = RR.init_weights(convs, seed=72)
    rng = np.random.default_rng(72)
    m = TR._model(batch, hw, classes, W, S)
    m.set_graph(True)
    xd = T.zeros((batch, 3, hw, hw), dtype=T.int8, device="cuda")
    ld = T.zeros(batch, dtype=T.int32, device="cuda")
    for step in range(2):
        x = rng.integers(-127, 128, (batch, 3, hw, hw)).astype(np.int8)
        labels = rng.integers(0, classes, batch).astype(np.int32)
        newW, rec = RR.train_step(convs, W, S, x, -2, labels, classes=classes)
        xd.copy_(T.from_numpy(x))
        ld.copy_(T.from_numpy(labels))
        m.train_step(xd, -2, ld)
        TR._check_step(m, convs, rec, newW, step)
        W = newW
    assert m.rowconv_error() == 0


def _vgg11_dp(T):
    """VGG-11 at 32 px as 2 in-process ranks of batch 2 (exact mode: the MAX exchange sits between the
    two launches) against one batch-4 device and the oracle, one step."""
    import ctypes as C

    import niti_amd
    import niti_model_ref as R
    import test_dp_local as TD
    from niti_amd.model import LocalGroup, NitiModel
    layers = R.vgg11_layers()
    W, S = R.init_weights(layers, seed=73)
    world, b = 2, 2
    full = NitiModel(niti_amd.ARCH_VGG11, b * world)
    ranks = [NitiModel(niti_amd.ARCH_VGG11, b) for _ in range(world)]
    group = LocalGroup(world)
    for r, m in enumerate(ranks):
        m.attach_local(group, r, exact=True)
    for m in [full] + ranks:
        for i, (w, s) in enumerate(zip(W, S)):
            m.set_weight(i, w, s)
    rng = np.random.default_rng(73)
    x = rng.integers(-127, 128, (b * world, 3, 32, 32)).astype(np.int8)
    labels = rng.integers(0, 10, b * world).astype(np.int32)
    newW, rec = R.train_step(layers, W, S, x, -3, labels)
    xd, ld = T.from_numpy(x).cuda(), T.from_numpy(labels).cuda()
    full.train_step(xd, -3, ld)
    T.cuda.synchronize()
    streams = [T.cuda.Stream() for _ in range(world)]
    parts = [(xd[r * b:(r + 1) * b].contiguous(), ld[r * b:(r + 1) * b].contiguous()) for r in range(world)]

    def rank_step(r):
        ranks[r].train_step(parts[r][0], -3, parts[r][1], stream=C.c_void_p(streams[r].cuda_stream))
        streams[r].synchronize()

    TD._in_threads([lambda r=r: rank_step(r) for r in range(world)])
    fl, fe = full.logits()
    assert fe == rec["exp"][-1] and np.array_equal(fl, rec["logits"])
    for r, m in enumerate(ranks):
        sl = slice(r * b, (r + 1) * b)
        lg, e = m.logits()
        assert e == fe and np.array_equal(lg, fl[sl]), r
        for i in range(len(layers)):
            assert np.array_equal(full.tap(i, 0), rec["r"][i]), ("full fwd", i)
            assert np.array_equal(m.tap(i, 0), rec["r"][i][sl]), ("fwd", r, i)
            assert np.array_equal(m.tap(i, 2), rec["dy"][i][sl]), ("dy", r, i)
            assert np.array_equal(m.tap(i, 1), rec["dw"][i]), ("dw", r, i)
            assert np.array_equal(m.get_weight(i), newW[i]), ("w", r, i)
            assert np.array_equal(full.get_weight(i), newW[i]), ("full w", i)
        assert m.rowconv_error() == 0


CHECKS = (_vgg11_graph, _resnet18_graph, _vgg11_dp)


def child_main():
    """Every check in this process (the two variables are in its environment): prints each mismatch and
    the count."""
    import torch
    assert os.environ.get("NITI_RC_SPEC2") == "0" and os.environ.get("NITI_RES_SPEC") == "0"
    bad = []
    for check in CHECKS:
        try:
            check(torch)
        except AssertionError as e:
            bad.append((check.__name__, e.args))
        torch.cuda.synchronize()
    for b in bad:
        print("MISMATCH", b)
    print("checked", len(CHECKS), "mismatches", len(bad))
    return 1 if bad else 0


_CHILD = """
import sys
sys.path[:0] = {paths!r}
import test_gpu_plain_pair as P
sys.exit(P.child_main())
"""


def test_plain_range_requantise_forms(T):
    """NITI_RC_SPEC2=0 and NITI_RES_SPEC=0 in a fresh child: the captured VGG-11 and ResNet-18 steps
    and the data-parallel VGG-11 step, each against the oracle."""
    paths = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"),
             os.path.join(ROOT, "mandheling-dsp-training_amd")]
    env = dict(os.environ, NITI_RC_SPEC2="0", NITI_RES_SPEC="0")
    r = subprocess.run([sys.executable, "-c", _CHILD.format(paths=paths)], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert f"checked {len(CHECKS)} mismatches 0" in r.stdout
