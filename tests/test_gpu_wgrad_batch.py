"""GPU parity of the batched P16 weight gradient (wgrad_p16_many_kernel, niti_wgrad.hip).

One persistent launch runs every 3x3 layer's weight gradient of a step: each workgroup walks a list
of (layer, tile, K range) items.  Int32 sums are exact, so whatever the schedule the result must be
bit-equal to the oracle (op level) and to the per-layer launches (model level).

Op level: the jobs below mix the four block forms (2x2, 4x4, 8x8, 16x16 images) and a ragged c_out,
forced into 2 and into 3 workgroups so each runs several items of different forms, split and unsplit,
back to back.  K groups (32 pixels) per job: 2, 4, 8, 16, 4, 6.  A K range is whole images (2 K groups
per 8x8 image, 8 per 16x16 image) and no range is empty, so the first five jobs can only be cut 1, 2
or 4 ways; the sixth (twelve 4x4 images) is there for the 3-way cut.  Item size 2 cuts the list
1, 2, 4, 2, 2, 3 ways, item size 3 cuts it 1, 1, 2, 2, 1, 2 ways.

Model level: VGG-11 at batch 16 (K groups per tile: 128 at 16x16, 32 at 8x8, 8 at 4x4, 2 at 2x2), item
sizes 8 (conv1 8 ways, conv2-3 4 ways) and 64 (conv1 2 ways), against the per-layer sequence.
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


def _dev(T, a):
    return T.from_numpy(np.ascontiguousarray(a)).to("cuda")


# (n, ci, h, co)
JOBS = [(16, 32, 2, 32), (8, 32, 4, 64), (4, 64, 8, 32), (2, 32, 16, 64), (2, 64, 8, 60), (12, 32, 4, 32)]
SPLITS = {2: [1, 2, 4, 2, 2, 3], 3: [1, 1, 2, 2, 1, 2]}


@pytest.fixture(scope="module")
def op_case(T):
    """The job list's operands on the device and the oracle's accumulators, computed once."""
    import niti_oracle as O
    from niti_amd import ops
    rng = np.random.default_rng(2024)
    case = []
    for n, ci, h, co in JOBS:
        g = O.geom(n, ci, h, h, co, 3, stride=1, pad=1)
        x = O.synth_x(rng, (n, ci, h, h))
        dy = O.synth_dy(rng, (n, co, g.oh, g.ow))
        ref, _ = O.conv_wgrad_acc(g, x, dy)  # [co][ci][kh][kw]
        gg = ops.geom(n, ci, h, h, co, 3, stride=1, pad=1)
        xP = ops.nhwc16_to_p16(ops.nchw_to_nhwc16(_dev(T, x)))
        dP = ops.nhwc16_to_p16(ops.nchw_to_nhwc16(_dev(T, dy)))
        case.append((gg, xP, dP, ref, co, ci))
    return case


@pytest.mark.parametrize("blocks", [2, 3])
@pytest.mark.parametrize("t", [2, 3])
def test_wgrad_p16_many_vs_oracle(T, op_case, blocks, t):
    from niti_amd import ops
    for rep in range(2):  # fresh outputs each time: the second launch inherits nothing
        amax = [ops.new_range() for _ in op_case]
        accs, splits = ops.conv_wgrad_p16_many([(gg, xP, dP, a) for (gg, xP, dP, _, _, _), a in zip(op_case, amax)],
                                               blocks, t)
        assert splits == SPLITS[t]  # (1: the range word comes from the kernel itself, else from the reduce)
        for (gg, _, _, ref, co, ci), acc, a, s in zip(op_case, accs, amax, splits):
            got = acc.cpu().numpy()[:co, :, :, :ci].transpose(0, 3, 1, 2)
            assert np.array_equal(got, ref), (blocks, t, rep, co, ci, s)
            assert ops.range_max(a) == int(np.abs(ref).max()), (blocks, t, rep, co, ci, s)


BATCH, STEPS = 16, 3


def _train(T, mode, graph=False, keep=False, probe=False, local=False):
    """3 VGG-11 steps at batch 16 under niti_diag_wgrad_batch(mode): every layer's weights, the last
    logits and exponent, the int8 gradient taps (keep), the probe's launch count, and the number of
    batched launches the steps made."""
    import niti_amd
    import niti_amd._lib as L
    import niti_model_ref as R
    from niti_amd.model import LocalGroup, NitiModel
    layers = R.vgg11_layers()
    rng = np.random.default_rng(77)
    W, S = R.init_weights(layers, seed=9)
    lib = L.lib()
    lib.niti_diag_wgrad_batch(mode)
    try:
        m = NitiModel(niti_amd.ARCH_VGG11, BATCH)
        m.set_graph(graph)
        m.set_overlap(False)
        m.keep_grads(keep)
        if local:
            m.attach_local(LocalGroup(1), 0, exact=True)
        for i, (w, s) in enumerate(zip(W, S)):
            m.set_weight(i, w, s)
        if probe:
            m.set_probe(3, 2, 16)
        n0 = lib.niti_diag_wgrad_batch_launches()
        x = T.empty((BATCH, 3, 32, 32), dtype=T.int8, device="cuda")
        lab = T.empty(BATCH, dtype=T.int32, device="cuda")
        for _ in range(STEPS):
            x.copy_(T.from_numpy(rng.integers(-127, 128, (BATCH, 3, 32, 32)).astype(np.int8)))
            lab.copy_(T.from_numpy(rng.integers(0, 10, BATCH).astype(np.int32)))
            m.train_step(x, -3, lab)
        out = {"w": [m.get_weight(i) for i in range(len(layers))], "logits": m.logits()}
        if keep:
            out["dw"] = [m.tap(i, 1) for i in range(len(layers))]
        if probe:
            out["probe"] = m.probe_read()
        out["batched"] = lib.niti_diag_wgrad_batch_launches() - n0
        return out
    finally:
        lib.niti_diag_wgrad_batch(1)


@pytest.fixture(scope="module")
def per_layer(T):
    """The per-layer sequence (batching off), with the int8 gradient taps kept: the reference of
    every model-level test, computed once."""
    ref = _train(T, 0, keep=True)
    assert ref["batched"] == 0
    return ref


def _same(got, ref):
    for i, (a, b) in enumerate(zip(got["w"], ref["w"])):
        assert np.array_equal(a, b), ("w", i)
    assert got["logits"][1] == ref["logits"][1]
    assert np.array_equal(got["logits"][0], ref["logits"][0])
    if "dw" in got:
        for i, (a, b) in enumerate(zip(got["dw"], ref["dw"])):
            assert np.array_equal(a, b), ("dw", i)


@pytest.mark.parametrize("t", [8, 64])
def test_vgg11_batched_wgrad_matches_per_layer(T, per_layer, t):
    got = _train(T, t)
    assert got["batched"] == STEPS
    _same(got, per_layer)


@pytest.mark.parametrize("t", [8, 64])
def test_vgg11_batched_wgrad_graph(T, per_layer, t):
    got = _train(T, t, graph=True)
    assert got["batched"] >= 1  # (captured once, replayed after)
    _same(got, per_layer)


@pytest.mark.parametrize("t", [8, 64])
def test_vgg11_batched_wgrad_keep_grads(T, per_layer, t):
    got = _train(T, t, keep=True)
    assert got["batched"] == STEPS
    _same(got, per_layer)


@pytest.mark.parametrize("t", [8, 64])
def test_vgg11_batched_wgrad_probe_keeps_its_launch(T, per_layer, t):
    """A probe armed on layer 3's weight gradient: that layer runs as its own launch (timed), the
    others in the batch."""
    got = _train(T, t, probe=True)
    assert got["batched"] == STEPS
    assert got["probe"][1] > 0
    _same(got, per_layer)


@pytest.mark.parametrize("t", [8, 64])
def test_vgg11_batched_wgrad_off_under_data_parallel(T, per_layer, t):
    """The one-rank group takes the data-parallel step: per-layer weight gradients, same results."""
    got = _train(T, t, local=True)
    assert got["batched"] == 0
    _same(got, per_layer)
