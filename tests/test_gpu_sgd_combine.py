"""GPU parity of the update launch's split-K combine alone (sgd_combine_kernel through niti_sgd_combine).

The combine sums a job's K-split slabs into its accumulator and takes the range.  A job with a few
1024-element chunks per split gives one thread all splits of its four elements; a small gradient over
many splits (n < 4096 * splits) gives G lanes one 16-byte group, each summing every G-th split, and
finishes with a shuffle tree.  Int32 sums are exact, so both forms must equal the numpy sum bit for
bit, alone and mixed in one launch.

Jobs (n, splits): (2048, 256) is VGG-11 conv0's weight gradient at batch 256 (G = 16, 32 chunks);
(36, 7) has G = 4, a ragged last pass and a partly filled chunk; (2048, 1) is a single slab;
(18432, 2) has n >= 4096 * splits, the one-thread form.

Model level: VGG-11 at batch 16 with a split-K slab plan forced on layer 0's weight gradient
(64 x 144 = 9216 elements, fewer than 4096 per split), so its sum runs in the combine's lane form
inside the step, against the same steps under that layer's unsplit plan.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def T():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import niti_amd  # noqa: F401
    return torch


JOBS = [(2048, 256), (36, 7), (2048, 1), (18432, 2)]  # (n, splits)


@pytest.fixture(scope="module")
def slabs(T):
    """Per job: the slabs on the device ([splits][stride], stride > n so a read past n would show)
    and the numpy sum, computed once."""
    rng = np.random.default_rng(411)
    out = []
    for n, splits in JOBS:
        stride = n + 64
        s = rng.integers(-(2 ** 20) + 1, 2 ** 20, (splits, stride)).astype(np.int32)  # |sum| < 2^28
        ref = s[:, :n].astype(np.int64).sum(axis=0)
        assert np.abs(ref).max() < 2 ** 31
        out.append((T.from_numpy(s).to("cuda"), n, ref.astype(np.int32)))
    return out


def _run(T, slabs, which):
    from niti_amd import ops
    for rep in range(2):  # fresh outputs each time: the second launch inherits nothing
        jobs = []
        for k in which:
            slab, n, _ = slabs[k]
            # a sentinel behind and past the n elements the combine writes
            acc = T.full((n + 16,), -77, dtype=T.int32, device="cuda")
            jobs.append((slab, n, acc, ops.new_range()))
        ops.sgd_combine(jobs)
        for k, (_, n, acc, amax) in zip(which, jobs):
            got = acc.cpu().numpy()
            ref = slabs[k][2]
            assert np.array_equal(got[:n], ref), (JOBS[k], rep)
            assert np.all(got[n:] == -77), (JOBS[k], rep)
            assert ops.range_max(amax) == int(np.abs(ref.astype(np.int64)).max()), (JOBS[k], rep)


@pytest.mark.parametrize("k", range(len(JOBS)))
def test_sgd_combine_one_job(T, slabs, k):
    _run(T, slabs, [k])


def test_sgd_combine_all_jobs_one_launch(T, slabs):
    _run(T, slabs, list(range(len(JOBS))))


BATCH, STEPS = 16, 3


def _train(T, split):
    """3 VGG-11 steps at batch 16 with layer 0's weight gradient under its tile shape's split-K slab
    plan (16 ways asked) or its unsplit plan: every layer's weights, the last logits and exponent."""
    import niti_amd
    import niti_model_ref as R
    from niti_amd.model import NitiModel
    layers = R.vgg11_layers()
    rng = np.random.default_rng(78)
    W, S = R.init_weights(layers, seed=10)
    NitiModel.reset_plans()
    try:
        m = NitiModel(niti_amd.ARCH_VGG11, BATCH)
        m.set_graph(False)
        for i, (w, s) in enumerate(zip(W, S)):
            m.set_weight(i, w, s)
        bm, bn, _, _ = m.plan(0, 2)
        m.set_plan(0, 2, (bm, bn, 16, 2) if split else (bm, bn, 1, 0))
        _, _, splits, strat = m.plan(0, 2)
        if split:  # the case the combine's lane form exists for: fewer than 4096 elements per split
            assert strat == 2 and 64 * 9 * 16 < splits * 4096, (splits, strat)
        else:
            assert strat == 0 and splits == 1, (splits, strat)
        x = T.empty((BATCH, 3, 32, 32), dtype=T.int8, device="cuda")
        lab = T.empty(BATCH, dtype=T.int32, device="cuda")
        for _ in range(STEPS):
            x.copy_(T.from_numpy(rng.integers(-127, 128, (BATCH, 3, 32, 32)).astype(np.int8)))
            lab.copy_(T.from_numpy(rng.integers(0, 10, BATCH).astype(np.int32)))
            m.train_step(x, -3, lab)
        return {"w": [m.get_weight(i) for i in range(len(layers))], "logits": m.logits()}
    finally:
        NitiModel.reset_plans()


def test_vgg11_layer0_split_plan_combines_in_step(T):
    ref = _train(T, False)
    got = _train(T, True)
    for i, (a, b) in enumerate(zip(got["w"], ref["w"])):
        assert np.array_equal(a, b), ("w", i)
    assert got["logits"][1] == ref["logits"][1]
    assert np.array_equal(got["logits"][0], ref["logits"][0])
