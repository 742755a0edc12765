"""GPU parity of the quad items of the batched P16 weight gradient (wgrad_p16_many_kernel, niti_wgrad.hip).

A quad item runs up to four consecutive tiles of one unsplit short-K job, one tile per wave, each wave
its tile's whole K range; the wave turns its own tile through its quarter of the LDS merge buffer and
stores it, with no cross-wave sum.  Int32 sums are exact, so results are bit-equal to the oracle, to
the merged form (threshold 0) and, in a model, to the per-layer launches.

Op level, jobs (n, ci, h, co) and what each is there for:
  (8, 32, 2, 32)    one tile, one K group: three idle waves, a K range shorter than the ring depth
  (16, 64, 2, 96)   six tiles: a full quad and a two-tile quad
  (64, 32, 2, 160)  five tiles, 8 K groups: two ring rounds
  (8, 64, 4, 60)    4x4 maps, ragged c_out
  (6, 32, 4, 32)    3 K groups, not a multiple of the ring depth
  (4, 64, 8, 32)    8x8 maps: always the merged form, so a block alternates forms
  (2, 32, 16, 64)   16x16 maps: always the merged form
K groups per job: 1, 2, 8, 4, 3, 8, 16; tiles: 1, 6, 5, 4, 1, 2, 2.  Cases (item size t, threshold k),
each in 1, 2 and 3 workgroups, with the cuts and the form counts worked out by hand:
  t 16, k 8: nothing is cut; jobs 0-4 go quad (1 + 2 + 2 + 1 + 1 = 7 items), 2 + 2 merged items
  t 4, k 4:  cuts 1, 1, 2, 1, 1, 2, 2; jobs 0, 1, 3, 4 go quad (5 items), 2*5 + 2*2 + 2*2 = 18 merged
  t 2, k 8:  cuts 1, 1, 4, 2, 2, 4, 2; jobs 0, 1 go quad (3 items) -- jobs 3 and 4 are under the
             threshold but cut, so they stay merged; 4*5 + 2*4 + 2*1 + 4*2 + 2*2 = 42 merged
In every run some workgroup runs a merged item right after a quad item and some a quad item right
after a merged one (asserted from the read-out schedule), so each form meets the other's LDS leavings.

Model level: VGG-11 at batch 16 (K groups per tile: L4 / L5 8 at 4x4, L6 / L7 2 at 2x2), item size
64, threshold 8 (L4-L7 as quads) against threshold 0 and the per-layer sequence.
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


JOBS = [(8, 32, 2, 32), (16, 64, 2, 96), (64, 32, 2, 160), (8, 64, 4, 60), (6, 32, 4, 32), (4, 64, 8, 32),
        (2, 32, 16, 64)]
# (t, k): (cuts per job, quad items, merged items)
CASES = {(16, 8): ([1, 1, 1, 1, 1, 1, 1], 7, 4),
         (4, 4): ([1, 1, 2, 1, 1, 2, 2], 5, 18),
         (2, 8): ([1, 1, 4, 2, 2, 4, 2], 3, 42)}


@pytest.fixture(scope="module")
def op_case(T):
    """The job list's operands on the device and the oracle's accumulators, computed once."""
    import niti_oracle as O
    from niti_amd import ops
    rng = np.random.default_rng(411)
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


def _forms(op_case, blocks, t):
    """Per workgroup, the forms (0 merged, 1 quad) of its items in order, from the read-out schedule."""
    from niti_amd import ops
    lists = ops.conv_wgrad_p16_many_schedule([(gg, xP, dP, None) for gg, xP, dP, _, _, _ in op_case], blocks, t)
    return [[it[7] for it in lst] for lst in lists]


@pytest.mark.parametrize("blocks", [1, 2, 3])
@pytest.mark.parametrize("t,k", sorted(CASES))
def test_wgrad_quad_vs_oracle(T, op_case, blocks, t, k):
    import niti_amd._lib as L
    from niti_amd import ops
    lib = L.lib()
    cuts, n_quad, n_merged = CASES[(t, k)]
    out = {}
    try:
        for quad in (k, 0):
            lib.niti_diag_wgrad_quad(quad)
            forms = _forms(op_case, blocks, t)
            flat = [f for lst in forms for f in lst]
            if quad:
                assert (sum(flat), len(flat) - sum(flat)) == (n_quad, n_merged)  # (no quad run: a failure)
                pairs = {p for lst in forms for p in zip(lst, lst[1:])}
                assert (0, 1) in pairs and (1, 0) in pairs, forms
            else:
                assert sum(flat) == 0
            for rep in range(2):  # fresh outputs each time: the second launch inherits nothing
                amax = [ops.new_range() for _ in op_case]
                accs, splits = ops.conv_wgrad_p16_many(
                    [(gg, xP, dP, a) for (gg, xP, dP, _, _, _), a in zip(op_case, amax)], blocks, t)
                assert splits == cuts
                for (gg, _, _, ref, co, ci), acc, a, s in zip(op_case, accs, amax, splits):
                    got = acc.cpu().numpy()[:co, :, :, :ci].transpose(0, 3, 1, 2)
                    assert np.array_equal(got, ref), (blocks, t, quad, rep, co, ci, s)
                    assert ops.range_max(a) == int(np.abs(ref).max()), (blocks, t, quad, rep, co, ci, s)
            out[quad] = accs
    finally:
        lib.niti_diag_wgrad_quad(-1)
    for a, b in zip(out[k], out[0]):  # whole buffers, padding included
        assert T.equal(a, b)


BATCH, STEPS = 16, 3


def _train(T, mode, quad):
    """3 VGG-11 steps at batch 16 under niti_diag_wgrad_batch(mode) and niti_diag_wgrad_quad(quad)."""
    import niti_amd
    import niti_amd._lib as L
    import niti_model_ref as R
    from niti_amd.model import NitiModel
    layers = R.vgg11_layers()
    rng = np.random.default_rng(77)
    W, S = R.init_weights(layers, seed=9)
    lib = L.lib()
    lib.niti_diag_wgrad_batch(mode)
    lib.niti_diag_wgrad_quad(quad)
    try:
        m = NitiModel(niti_amd.ARCH_VGG11, BATCH)
        m.set_graph(False)
        m.set_overlap(False)
        for i, (w, s) in enumerate(zip(W, S)):
            m.set_weight(i, w, s)
        n0 = lib.niti_diag_wgrad_batch_launches()
        x = T.empty((BATCH, 3, 32, 32), dtype=T.int8, device="cuda")
        lab = T.empty(BATCH, dtype=T.int32, device="cuda")
        for _ in range(STEPS):
            x.copy_(T.from_numpy(rng.integers(-127, 128, (BATCH, 3, 32, 32)).astype(np.int8)))
            lab.copy_(T.from_numpy(rng.integers(0, 10, BATCH).astype(np.int32)))
            m.train_step(x, -3, lab)
        return {"w": [m.get_weight(i) for i in range(len(layers))], "logits": m.logits(),
                "batched": lib.niti_diag_wgrad_batch_launches() - n0}
    finally:
        lib.niti_diag_wgrad_batch(1)
        lib.niti_diag_wgrad_quad(-1)


def test_vgg11_quad_matches_merged_and_per_layer(T):
    per_layer = _train(T, 0, 0)
    merged = _train(T, 64, 0)
    quad = _train(T, 64, 8)
    assert (per_layer["batched"], merged["batched"], quad["batched"]) == (0, STEPS, STEPS)
    for got in (merged, quad):
        for i, (a, b) in enumerate(zip(got["w"], per_layer["w"])):
            assert a.tobytes() == b.tobytes(), ("w", i)
        assert got["logits"][1] == per_layer["logits"][1]
        assert got["logits"][0].tobytes() == per_layer["logits"][0].tobytes()
