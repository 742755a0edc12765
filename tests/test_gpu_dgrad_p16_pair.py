"""The input gradient's P16 copy on a 4x4 map behind a relu (no pool): two waves share a tile.

At 4x4 and two rows per band a wave of the register-fed input gradient holds half of each of its 8
images, so no wave has a whole 16-pixel block.  The two bands of an image group are waves 2k and
2k + 1 of one workgroup: they stage one tile, meet at a workgroup barrier and store it in the weight
gradient's P16 layout.  Checked here: the NHWC16 dx against the oracle's input gradient with the relu
mask, the P16 copy bit-equal to nhwc16_to_p16 of that dx with nothing written past n * 16 pixels,
and the kernel's error word, in every mode that writes outputs (fused; range + requantise; the
speculative pair with no hint, a hit and a forced miss).

Batches: 8 is one image group (two waves of the workgroup without a unit), 16 one full workgroup,
20 a group with four images past n, 24 a second, half-filled workgroup.  Channels: the gradient of
a 64 -> 32 layer (dx has 64 channels: two output blocks) and of a 32 -> 64 layer.

Model level: VGG-11 at batch 16 (layer 5's input gradient writes layer 4's dy at 4x4 through this
path), three steps against the same steps with that copy switched off: layer 4's weight gradient on a
GEMM plan, which reads the NHWC16 dy.
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


SENTINEL = 0x55
TAIL = 8  # P16 blocks behind the n the launch may write: a whole image group's worth


@pytest.fixture(scope="module")
def refs():
    """(n, ci, co) -> operands and the oracle's dx, computed once and left unchanged."""
    import niti_oracle as O
    out = {}
    for k, (ci, co) in enumerate([(64, 32), (32, 64)]):
        for n in (8, 16, 20, 24):
            rng = np.random.default_rng(1300 + 10 * k + n)
            g = O.geom(n, ci, 4, 4, co, 3, pad=1)
            dy = rng.integers(-127, 128, (n, co, 4, 4)).astype(np.int8)
            w = rng.integers(-127, 128, (co, ci, 3, 3)).astype(np.int8)
            mk = rng.integers(-2, 3, (n, ci, 4, 4)).astype(np.int8)
            dq, _, _, _ = O.conv_dgrad(g, dy, w)
            out[(n, ci, co)] = (dy, w, mk, O.relu_grad(mk, dq))
    return out


@pytest.mark.parametrize("mode", [0, 2, 4])
@pytest.mark.parametrize("n", [8, 16, 20, 24])
@pytest.mark.parametrize("ci,co", [(64, 32), (32, 64)])
def test_dgrad_rows_p16_pair(T, refs, ci, co, n, mode):
    from test_gpu_rowconv import _spec_pairs
    from niti_amd import ops
    dy, w, mk, want = refs[(n, ci, co)]
    dev = lambda a: T.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    nhwc = lambda a: ops.nchw_to_nhwc16(dev(a))  # noqa: E731
    gg = ops.geom(n, ci, 4, 4, co, 3, pad=1)
    dyc = ops.nhwc16_to_c32(nhwc(dy), co)
    wft = ops.weights_to_wf(ops.oihw_to_ohwi16(dev(w)), ci, transpose=True)
    amax = ops.new_range()
    st = ops.RowConvState()
    kw = dict(relu_mask=nhwc(mk))

    def fresh():  # outputs filled with a sentinel, the P16 copy with room behind its n blocks
        dx = T.full((n, 4, 4, gg.cip), SENTINEL, dtype=T.int8, device="cuda")
        nxt = T.full((n, gg.cip // 32, 4, 4, 32), SENTINEL, dtype=T.int8, device="cuda")
        p16 = T.full((n + TAIL, gg.cip, 16), SENTINEL, dtype=T.int8, device="cuda")
        return dx, nxt, p16

    def check(dx, nxt, p16):
        T.cuda.synchronize()
        assert int(st.err.item()) == 0
        assert np.array_equal(dx.cpu().numpy()[..., :ci].transpose(0, 3, 1, 2), want)
        got = p16.cpu().numpy()
        assert np.array_equal(got[:n], ops.nhwc16_to_p16(dx).cpu().numpy())
        assert np.all(got[n:] == SENTINEL)

    if mode == 0:
        check(*ops.conv_dgrad_rows(gg, dyc, wft, amax, mode=0, state=st, outs=fresh(), **kw))
    elif mode == 2:
        ops.conv_dgrad_rows(gg, dyc, wft, amax, mode=1, **kw)
        check(*ops.conv_dgrad_rows(gg, dyc, wft, amax, mode=2, outs=fresh(), **kw))
    else:
        _spec_pairs(T, st, True, amax, None,
                    lambda m, outs: ops.conv_dgrad_rows(gg, dyc, wft, amax, mode=m, state=st,
                                                        outs=fresh() if outs is None else outs, **kw), check)


def _train(T, fused):
    """3 VGG-11 steps at batch 16.  fused: layer 4's weight gradient on its P16 plan, its dy's P16
    copy written by layer 5's input gradient; else layer 4 on a GEMM plan, which reads the NHWC16 dy
    and switches that copy off (the model writes it only for a P16 weight gradient)."""
    import niti_amd
    import niti_model_ref as R
    from niti_amd.model import NitiModel
    layers = R.vgg11_layers()
    rng = np.random.default_rng(79)
    W, S = R.init_weights(layers, seed=11)
    NitiModel.reset_plans()
    try:
        m = NitiModel(niti_amd.ARCH_VGG11, 16)
        m.set_graph(False)
        for i, (w, s) in enumerate(zip(W, S)):
            m.set_weight(i, w, s)
        assert m.plan(4, 2)[0] == 16  # the P16 weight gradient
        if not fused:
            m.set_plan(4, 2, (128, 128, 1, 0))
            assert m.plan(4, 2)[0] != 16
        x = T.empty((16, 3, 32, 32), dtype=T.int8, device="cuda")
        lab = T.empty(16, dtype=T.int32, device="cuda")
        for _ in range(3):
            x.copy_(T.from_numpy(rng.integers(-127, 128, (16, 3, 32, 32)).astype(np.int8)))
            lab.copy_(T.from_numpy(rng.integers(0, 10, 16).astype(np.int32)))
            m.train_step(x, -3, lab)
        return [m.get_weight(i) for i in range(len(layers))], m.logits()
    finally:
        NitiModel.reset_plans()


def test_vgg11_b16_steps_match_unfused(T):
    """(The CPU reference model takes over a minute for these steps; the plan switch gives the same
    comparison on the device: int32 weight gradients are exact on either kernel.)"""
    w_ref, l_ref = _train(T, False)
    w_got, l_got = _train(T, True)
    for i, (a, b) in enumerate(zip(w_got, w_ref)):
        assert np.array_equal(a, b), i
    assert l_got[1] == l_ref[1] and np.array_equal(l_got[0], l_ref[0])
