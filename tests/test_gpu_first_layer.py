"""GPU parity of the first layer's two launches alone -- the fused input pass (niti_input_im2col)
and the K = 32 conv on its im2col copy (niti_conv0_fwd) -- and of one whole chain step through
them, against the CPU oracle, bit for bit (tests/first_layer_cases.py holds inputs and references).
"""
import functools

import numpy as np
import pytest

import chain_cases as CC
import first_layer_cases as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def T():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import niti_amd  # noqa: F401
    return torch


def _i8(T, v):
    return T.tensor([v], dtype=T.int8, device="cuda")


@pytest.mark.parametrize("pool", [False, True])
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("cls", F.CONV0_CLASSES)
@pytest.mark.parametrize("c_out", F.CONV0_COUT)
def test_conv0(T, c_out, cls, relu, pool):
    """Range pass and requantise / relu / pool pass at batch 3, 3 x 32 x 32, 3x3 pad 1: 48 units, run
    on the default grid and on 2 and 5 workgroups (6 units per wave; 48 = 2 x 20 + 8, a ragged
    tail).  The weights pin the rule: raw cast, shift 1 (run as PSTO 2, exponent + 2), PSTO."""
    from niti_amd import _lib as L
    from niti_amd import ops
    x, w, ws = F.conv0_inputs(c_out, cls)
    ref = F.conv0_reference(c_out, cls, relu)
    assert {"raw": ref["shift"] <= 0, "one": ref["shift"] == 1, "psto": ref["shift"] >= 2}[cls], ref["shift"]
    cop = F.r32(c_out)
    g = ops.geom(F.BATCH, 32, 32, 32, c_out, 1)
    assert g.cop == cop
    xcol = T.from_numpy(F.xcol_of(x, 3, 1)).cuda()
    wd = T.from_numpy(F.wcol_of(w, c_out)).cuda()
    P = F.BATCH * 32 * 32
    want = dict(out=F.nhwc_of(ref["out"], cop), out_c32=F.c32_of(ref["out"], cop))
    if pool:
        want.update(pool_out=F.nhwc_of(ref["pool"], cop), pool_code=F.nhwc_of(ref["code"], cop),
                    pool_c32=F.c32_of(ref["pool"], cop))
        # (a pad channel's window is four zeros: its first element takes the route, unless relu drops it)
        want["pool_code"][:, c_out:] = 0 if relu else 1
    try:
        for blocks in (0, 2, 5):
            L.lib().niti_diag_conv0_blocks(blocks)
            amax = ops.new_range()
            ops.conv0_fwd(g, xcol, wd, amax, 0)
            assert ops.range_max(amax) == ref["range"], blocks
            got = {k: T.full(v.shape, 77, dtype=T.int8, device="cuda") for k, v in want.items()}
            e = T.zeros(1, dtype=T.int8, device="cuda")
            ops.conv0_fwd(g, xcol, wd, amax, 1, exp_in=_i8(T, F.CONV0_EXP[0]), wscale=_i8(T, ws), exp_out=e,
                          relu=relu, **got)
            assert int(e.item()) == ref["exp"], blocks
            for k, v in want.items():
                assert np.array_equal(got[k].cpu().numpy(), v), (k, blocks)
            if pool:  # without the pre-pool output: the pooled map and its codes carry everything
                got = {k: T.full(want[k].shape, 77, dtype=T.int8, device="cuda") for k in ("pool_out", "pool_code")}
                ops.conv0_fwd(g, xcol, wd, amax, 1, relu=relu, **got)
                for k in got:
                    assert np.array_equal(got[k].cpu().numpy(), want[k]), (k, blocks, "no out")
    finally:
        L.lib().niti_diag_conv0_blocks(0)
    assert P * cop == want["out"].size


@pytest.mark.parametrize("quant", [True, False])
@pytest.mark.parametrize("shape", F.IM2COL_SHAPES)
def test_input_im2col(T, shape, quant):
    """The input tap, its exponent, the im2col copy and the fused first-conv range, from uint8 images
    (the oracle's quantiser) and from int8 pixels; where conv0 takes the geometry, its output too."""
    from niti_amd import ops
    c, hw, k, pad, co = shape
    ref = F.im2col_reference(c, hw, k, pad, co, quant)
    inp = T.from_numpy(np.array(ref["inp"])).cuda()
    stats = ops.image_stats(inp) if quant else None
    cop = F.r32(co)
    wd = T.from_numpy(F.wcol_of(ref["w"], cop)).cuda()
    amax = ops.new_range()
    xcol, x8, ascale = ops.input_im2col(inp, k, pad, stats=stats, w0=wd, co0=co, amax0=amax)
    assert np.array_equal(x8.cpu().numpy(), ref["x"])
    if quant:
        assert int(ascale.item()) == ref["ascale"]
    assert np.array_equal(xcol.cpu().numpy(), ref["xcol"])
    assert ops.range_max(amax) == ref["range"]
    # without the range and the tap
    xcol2, _, _ = ops.input_im2col(inp, k, pad, stats=stats)
    assert np.array_equal(xcol2.cpu().numpy(), ref["xcol"])
    oh = hw + 2 * pad - k + 1
    if oh % 32 == 0:
        import niti_oracle as O
        y, _, _, _ = O.conv_fwd(O.geom(F.BATCH, c, hw, hw, co, k, pad=pad), ref["x"], ref["w"])
        out = T.full((F.BATCH * oh * oh, cop), 77, dtype=T.int8, device="cuda")
        ops.conv0_fwd(ops.geom(F.BATCH, 32, oh, oh, co, 1), xcol, wd, amax, 1, out=out)
        assert np.array_equal(out.cpu().numpy(), F.nhwc_of(y, cop))


@functools.lru_cache(maxsize=None)
def _first_net_ref(batch, steps, seed, images):
    import niti_model_ref as R
    layers = CC.derive(F.FIRST_NET)
    W, S = R.init_weights(layers, seed=seed)
    data = CC.batches(layers, batch, steps, seed + 1, images=images)
    return layers, W, S, data, CC.ref_steps(layers, W, S, data)


@pytest.mark.parametrize("images", [False, True])
def test_chain_step_through_the_first_layer(T, images):
    """Two from_chain steps of a net whose 20-channel 3 x 32 x 32 first layer takes the fused input
    pass and conv0: logits, exponents, every layer's forward / gradient taps and weights."""
    from niti_amd.model import NitiModel
    layers, W, S, data, ref = _first_net_ref(6, 2, 11, images)
    in_c, in_hw, spec = F.FIRST_NET
    m = NitiModel.from_chain(spec, in_c, in_hw, 6)
    for i, (w, s) in enumerate(zip(W, S)):
        m.set_weight(i, w, s)
    m.keep_grads(True)
    for step, ((x, labels), (newW, rec, xq, e_in)) in enumerate(zip(data, ref)):
        xd, ld = T.from_numpy(x).cuda(), T.from_numpy(labels).cuda()
        if images:
            m.train_step_images(xd, ld)
            xin, a = m.input()
            assert a == e_in and np.array_equal(xin, xq), step
        else:
            m.train_step(xd, -3, ld)
        logits, e = m.logits()
        assert e == rec["exp"][-1] and np.array_equal(logits, rec["logits"]), step
        for i in range(len(layers)):
            assert np.array_equal(m.tap(i, 0), rec["r"][i]), ("fwd", step, i)
            assert np.array_equal(m.tap(i, 2), rec["dy"][i]), ("dy", step, i)
            assert np.array_equal(m.tap(i, 1), rec["dw"][i]), ("dw", step, i)
            assert np.array_equal(m.get_weight(i), newW[i]), ("w", step, i)
    assert m.rowconv_error() == 0
