"""The grid barrier's slot form (csrc/niti_gridbar.hpp) through the fused row kernels
(niti_conv_fwd_rows / niti_conv_dgrad_rows, mode 0): every case against the oracle bit for bit, with
the barrier's error word 0.  Grid sizes at the edges of the slot layout (one lane's first slot, one
64-slot load, one 256-slot round), a state reused by launches of other grids and other bit widths
(a slot left by an earlier launch must not be believed), epochs set far apart (the tag is the full
32-bit epoch: nothing truncated may alias), and a single workgroup holding the whole tensor's max.

The strategy-4 GEMM takes its state and epoch from the step driver (no op entry carries them), so
the second slot region (slots 256-511, past the hint lines) is driven through a chain model whose
middle layer is forced onto plan (64, 64, 1, 4): 288 tiles, and 512 -- the slot capacity, which is
what bounds the fused GEMM where the device holds more 64x64 tiles than that -- over three steps on
the layer's one state, every tap against the oracle, the fused-launch counter advancing and the
layer's hint lines (which lie between the two slot regions) still zero.  The fused residual launch
(NITI_RES_FUSED=1, read once per process, with no counter that shows it ran) has no test here."""
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

COUNTS = [1, 2, 7, 8, 9, 63, 64, 65, 255, 256]


@pytest.fixture(scope="module")
def T():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import niti_amd  # noqa: F401
    return torch


def _shape_for(count, dgrad=False, hs=(2, 4)):
    """(n, h, c_out) of the cheapest 32-channel-input layer on 2x2 / 4x4 maps whose fused launch is
    exactly `count` workgroups, by the library's own plan (host arithmetic)."""
    from niti_amd import ops
    best = None
    for h in hs:
        for cob in (1, 2, 3, 4, 5, 8):
            for n in range(1, 4097):
                cost = n * h * h * cob
                if best is not None and cost >= best[0]:
                    break
                plan = ops.conv_rows_plan(ops.geom(n, 32, h, h, 32 * cob, 3, pad=1), dgrad=dgrad)
                if plan is not None and plan[3] == count:
                    best = (cost, n, h, 32 * cob)
                    break
                if plan is not None and plan[3] > count:
                    break
    assert best is not None, count
    return best[1:]


class _Fwd:
    """One forward layer's device operands and oracle result; launch(st) runs it fused on state st."""

    def __init__(self, T, n, h, co, seed, xmax=127, x=None, w=None):
        import niti_oracle as O
        from niti_amd import ops
        rng = np.random.default_rng(seed)
        ci = 32
        self.T, self.n, self.co = T, n, co
        g = O.geom(n, ci, h, h, co, 3, pad=1)
        x = rng.integers(-xmax, xmax + 1, (n, ci, h, h)).astype(np.int8) if x is None else x
        w = rng.integers(-127, 128, (co, ci, 3, 3)).astype(np.int8) if w is None else w
        self.y_ref, self.e_ref, acc, _ = O.conv_fwd(g, x, w, -3, -5)
        self.bw = int(np.abs(acc).max()).bit_length()
        dev = lambda a: T.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
        self.gg = ops.geom(n, ci, h, h, co, 3, pad=1)
        self.wgs = ops.conv_rows_plan(self.gg)[3]
        self.xc = ops.nhwc16_to_c32(ops.nchw_to_nhwc16(dev(x)), ci)
        self.wf = ops.weights_to_wf(ops.oihw_to_ohwi16(dev(w)), ci)
        self.ein, self.ws = dev(np.array([-3], np.int8)), dev(np.array([-5], np.int8))
        self.amax = ops.new_range()

    def launch(self, st):
        from niti_amd import ops
        T = self.T
        eo = T.full((1,), 99, dtype=T.int8, device="cuda")
        out, _, _ = ops.conv_fwd_rows(self.gg, self.xc, self.wf, self.amax, mode=0, state=st, exp_in=self.ein,
                                      wscale=self.ws, exp_out=eo)
        T.cuda.synchronize()
        assert int(st.err.item()) == 0
        assert int(eo.item()) == self.e_ref
        assert np.array_equal(out.cpu().numpy()[..., :self.co].transpose(0, 3, 1, 2), self.y_ref)


@pytest.mark.parametrize("count", COUNTS)
def test_forward_grid_sizes(T, count):
    from niti_amd import ops
    n, h, co = _shape_for(count)
    c = _Fwd(T, n, h, co, seed=1500 + count)
    assert c.wgs == count
    st = ops.RowConvState()
    c.launch(st)
    c.launch(st)  # and again over its own slots of the launch before


@pytest.mark.parametrize("count", [9, 65])
def test_forward_4x4_maps(T, count):
    from niti_amd import ops
    n, h, co = _shape_for(count, hs=(4,))
    c = _Fwd(T, n, h, co, seed=1550 + count)
    assert c.wgs == count and h == 4
    c.launch(ops.RowConvState())


@pytest.mark.parametrize("count", [7, 65, 256])
def test_dgrad_grid_sizes(T, count):
    import niti_oracle as O
    from niti_amd import ops
    n, h, co = _shape_for(count, dgrad=True)
    ci = 32
    rng = np.random.default_rng(1600 + count)
    g = O.geom(n, ci, h, h, co, 3, pad=1)
    dy = rng.integers(-127, 128, (n, co, h, h)).astype(np.int8)
    w = rng.integers(-127, 128, (co, ci, 3, 3)).astype(np.int8)
    mk = rng.integers(-2, 3, (n, ci, h, h)).astype(np.int8)
    dq, _, _, _ = O.conv_dgrad(g, dy, w)
    want = O.relu_grad(mk, dq)
    dev = lambda a: T.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    gg = ops.geom(n, ci, h, h, co, 3, pad=1)
    assert ops.conv_rows_plan(gg, dgrad=True)[3] == count
    dyc = ops.nhwc16_to_c32(ops.nchw_to_nhwc16(dev(dy)), co)
    wft = ops.weights_to_wf(ops.oihw_to_ohwi16(dev(w)), ci, transpose=True)
    st = ops.RowConvState()
    dx, _, _ = ops.conv_dgrad_rows(gg, dyc, wft, ops.new_range(), mode=0, state=st,
                                   relu_mask=ops.nchw_to_nhwc16(dev(mk)), dx_c32=True)
    T.cuda.synchronize()
    assert int(st.err.item()) == 0
    assert np.array_equal(dx.cpu().numpy()[..., :ci].transpose(0, 3, 1, 2), want)


def test_stale_slot_is_not_believed(T):
    """Five launches on one state, the tensor's bit width alternating high / low: a slot of launch
    e - 1 or e - 2 taken for this launch's would give the other tensor's shift."""
    from niti_amd import ops
    n, h, co = _shape_for(64)
    hi, lo = _Fwd(T, n, h, co, seed=1701), _Fwd(T, n, h, co, seed=1702, xmax=1)
    assert hi.bw >= lo.bw + 4, (hi.bw, lo.bw)
    st = ops.RowConvState()
    for c in (hi, lo, hi, lo, lo):
        c.launch(st)
    assert st.epoch == 5


def test_grid_shrinks_then_grows(T):
    """256 workgroups, then 64, then 256 on one state, other data each time: the second launch leaves
    192 slots of the first behind it, and the third must wait for all 256 again."""
    from niti_amd import ops
    big, small = _shape_for(256), _shape_for(64)
    a, b = _Fwd(T, *big, seed=1801), _Fwd(T, *small, seed=1802, xmax=3)
    c = _Fwd(T, *big, seed=1803, xmax=1)
    assert (a.wgs, b.wgs, c.wgs) == (256, 64, 256) and len({a.bw, b.bw, c.bw}) == 3
    st = ops.RowConvState()
    for k in (a, b, c):
        k.launch(st)


def test_epochs_far_apart(T):
    """The tag is the full epoch: launches whose epochs differ by 2^8, 2^16, 2^24, 2^26 and 2^31 --
    the period of any truncated tag -- on one state, bit widths alternating, up to the last epoch."""
    from niti_amd import ops
    n, h, co = _shape_for(9)
    hi, lo = _Fwd(T, n, h, co, seed=1901), _Fwd(T, n, h, co, seed=1902, xmax=1)
    assert hi.bw != lo.bw
    st = ops.RowConvState()
    e = 5
    for k, step in enumerate([0, 1 << 8, 1 << 16, 1 << 24, 1 << 26, 1 << 31, 0xFFFFFFFF - 5 - (1 << 31) - (1 << 26)
                              - (1 << 24) - (1 << 16) - (1 << 8)]):
        e += step
        st.epoch = e - 1  # the op entry launches with state.epoch + 1
        (hi if k % 2 == 0 else lo).launch(st)
    assert st.epoch == 0xFFFFFFFF


@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_one_maximum_in_one_workgroup(T, where):
    """All zeros but one image's outputs in one 32-channel block (a +-127 product chain): one
    workgroup's slot carries the whole tensor's bit width, every other slot 0, at either end and in
    the middle of the (image, channel block) order.  A lost slot shows as a wrong exponent."""
    from niti_amd import ops
    n, h, co = _shape_for(65)
    i, ch = {"first": (0, 0), "middle": (n // 2, (co // 64) * 32 + 7), "last": (n - 1, co - 1)}[where]
    x = np.zeros((n, 32, h, h), np.int8)
    w = np.zeros((co, 32, 3, 3), np.int8)
    x[i] = 127
    w[ch] = np.where(np.arange(32 * 9).reshape(32, 3, 3) % 2 == 0, 127, -127)
    w[ch, :, 1, 1] = -127
    c = _Fwd(T, n, h, co, seed=0, x=x, w=w)
    assert c.wgs == 65 and c.bw > 14 and np.count_nonzero(c.y_ref.reshape(n, co, -1).any(axis=2)) == 1
    c.launch(ops.RowConvState())


# a 6x6 net (no row kernel takes 6-px maps): layer 1 is 16 -> 72 channels, so its forward GEMM is
# M = 36 batch rows by N = 80 padded columns, two 64-column tiles per 64-row tile
GEMM_NET = (4, 6, [(16, 3, 1, 1, 0, 0), (72, 3, 1, 1, 0, 0), (16, 3, 1, 1, 1, 1), (10, 1, 0, 0, 0, 0)])
GEMM_STEPS = 3


@functools.lru_cache(maxsize=None)
def _gemm_ref(batch, tail):
    """(layers, W, S, data, oracle steps) of GEMM_NET at `batch`: computed once, shared, never written.
    tail: only the last 20 images are non-zero and layer 1's first 64 output channels start with zero
    weights, so in the first step every non-zero accumulator of layer 1's forward lies in the last
    M tiles of the second column tile -- tiles past 256 in either tile order: a poll that left the
    second slot region out would take bit width 0."""
    import chain_cases as CC
    import niti_model_ref as R
    layers = CC.derive(GEMM_NET)
    W, S = R.init_weights(layers, seed=2100 + batch)
    data = CC.batches(layers, batch, GEMM_STEPS, 2200 + batch)
    if tail:
        W = [w.copy() for w in W]
        W[1][:64] = 0
        for x, _ in data:
            x[:-20] = 0
    threads = max(1, min(16, len(os.sched_getaffinity(0))))
    step = lambda layers, W, S, x, e, lab: R.train_step(layers, W, S, x, e, lab, impl="mnn", threads=threads)  # noqa: E731
    return layers, W, S, data, CC.ref_steps(layers, W, S, data, step_fn=step)


@pytest.mark.parametrize("tail", [False, True])
@pytest.mark.parametrize("batch,tiles", [(256, 288), (454, 512)])
def test_fused_gemm_second_slot_region(T, batch, tiles, tail):
    from niti_amd import _lib as L
    from niti_amd.model import NitiModel
    assert -(-36 * batch // 64) * -(-80 // 64) == tiles  # the forward launch's grid under the forced plan
    layers, W, S, data, ref = _gemm_ref(batch, tail)
    if tail:
        assert np.any(ref[0][1]["r"][1][-20:, 64:]) and not np.any(ref[0][1]["r"][1][:-20]) \
            and not np.any(ref[0][1]["r"][1][:, :64])
    in_c, in_hw, spec = GEMM_NET
    m = NitiModel.from_chain(spec, in_c, in_hw, batch)
    try:
        m.train_step(T.from_numpy(data[0][0]).cuda(), -3, T.from_numpy(data[0][1]).cuda())  # fills the buffers
        for ph in (0, 1):
            m.set_plan(1, ph, (64, 64, 1, 4))
            assert m.plan(1, ph)[:2] == (64, 64) and m.plan(1, ph)[3] == 4, ph
        for i, (w, s) in enumerate(zip(W, S)):
            m.set_weight(i, w, s)
        n0 = L.lib().niti_diag_gemm_fused_launches()
        for step, ((x, labels), (newW, rec, _, _)) in enumerate(zip(data, ref)):
            m.train_step(T.from_numpy(x).cuda(), -3, T.from_numpy(labels).cuda())
            logits, e = m.logits()
            assert e == rec["exp"][-1] and np.array_equal(logits, rec["logits"]), step
            for i in range(len(layers)):
                assert np.array_equal(m.tap(i, 0), rec["r"][i]), ("fwd", step, i)
                assert np.array_equal(m.tap(i, 2), rec["dy"][i]), ("dy", step, i)
                assert np.array_equal(m.get_weight(i), newW[i]), ("w", step, i)
            # the forward launch of layer 1 ran fused in every step so far (its input gradient too where
            # the driver admits it)
            assert L.lib().niti_diag_gemm_fused_launches() - n0 >= step + 1, step
        assert m.rowconv_error() == 0
        # the two hint lines between the slot regions: the GEMM path never writes them
        assert not any(m.spec_slot(1, 0)) and not any(m.spec_slot(1, 1))
    finally:
        NitiModel.reset_plans()
