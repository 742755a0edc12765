"""GPU parity of the grouped conv launches (niti_gconv_*, niti_gconv2_*, niti_gconv_narrow_*) past one column
segment and one unit a workgroup: the cases of tests/grouped_map_cases.py, bit for bit against the direct sums of
the definition.  tests/test_grouped_map_cpu.py proves that each case reaches its hazard."""
import numpy as np
import pytest

import grouped_map_cases as GM
from grouped_cases import DC, O
from test_gpu_grouped_ops import POISON, POISON32, T, _dev, _nchw, _nhwc  # noqa: F401 -- T: the module's GPU fixture

pytestmark = pytest.mark.gpu


def _family(shape):
    """(the ops prefix of the launches that take the shape, its ops geometry)"""
    from niti_amd import ops
    n, c, groups, h, w, pad, stride = shape
    g = ops.geom(n, c, h, w, c, 3, stride=stride, pad=pad)
    pre = "gconv_narrow" if GM.narrow(shape) else "gconv2" if stride == 2 else "gconv"
    assert getattr(ops, pre + "_ok")(g, groups) and (g.oh, g.ow) == GM.out_hw(shape) and g.cip == g.cop == c
    return pre, g


def _act(T, shape, dgrad, a, w, mask, acc):
    """Pass 0's range, then pass 1 into a poisoned output without and with the relu / relu_mask: the whole output
    (C is a multiple of 16: it has no other bytes) and the exponent."""
    from niti_amd import ops
    pre, g = _family(shape)
    groups = shape[2]
    q, inc = DC.requant_under(acc)
    a16, w16, m16 = _nhwc(T, a), ops.gconv_weight(_dev(T, w)), _nhwc(T, mask)
    ei, ws = _dev(T, np.array([-5], np.int8)), _dev(T, np.array([-6], np.int8))
    fn = getattr(ops, pre + ("_dgrad" if dgrad else "_fwd"))
    for on in (False, True):
        kw = dict(relu_mask=m16 if on else None) if dgrad else dict(relu=on, exp_in=ei, wscale=ws)
        want = q if not on else O.relu_grad(mask, q) if dgrad else O.relu(q)
        amax = ops.new_range()
        fn(g, groups, a16, w16, amax, 0, **kw)
        assert ops.range_max(amax) == GM.GC.absmax(acc)
        out = T.full((g.n, g.h, g.w, g.cip) if dgrad else (g.n, g.oh, g.ow, g.cop), POISON, dtype=T.int8, device="cuda")
        e = T.full((1,), POISON, dtype=T.int8, device="cuda")
        fn(g, groups, a16, w16, amax, 1, out=out, exp_out=e, **kw)
        assert int(e.item()) == (inc if dgrad else DC._e8(-5 - 6 + inc)), (on, inc)
        got = _nchw(out)
        assert got.shape == want.shape
        assert np.array_equal(got, want), (on, np.argwhere(got != want)[:4].tolist())
    return inc


@pytest.mark.parametrize("dgrad", (False, True), ids=("fwd", "dgrad"))
@pytest.mark.parametrize("shape", GM.ACT_CASES, ids=GM.case_id)
def test_forward_and_input_gradient(T, shape, dgrad):
    _act(T, shape, dgrad, *GM.act_case(shape, dgrad))


@pytest.mark.parametrize("dgrad", (False, True), ids=("fwd", "dgrad"))
@pytest.mark.parametrize("shape", GM.EQ1_CASES, ids=GM.case_id)
def test_narrow_shift_class_eq1(T, shape, dgrad):
    """Bit width 8: shift 1, the exponent up by 2."""
    assert _act(T, shape, dgrad, *GM.eq1_case(shape, dgrad)) == 2


@pytest.mark.parametrize("shape", GM.WGRAD_CASES, ids=GM.case_id)
def test_weight_gradient(T, shape):
    from niti_amd import ops
    pre, g = _family(shape)
    n, c, groups, h, w, pad, stride = shape
    cg, cgp = c // groups, max(c // groups, 16)
    x, dy, acc = GM.wgrad_case(shape)
    slabs = getattr(ops, pre + "_wgrad_slabs")(g, groups)
    assert slabs == GM.slabs_of(shape)
    slab = getattr(ops, pre + "_wgrad")(g, groups, _nhwc(T, x), _nhwc(T, dy))
    assert slab.shape == (slabs, c * 9 * cgp)
    s = slab.cpu().numpy().reshape(slabs, c, 3, 3, cgp)
    assert not s[..., cg:].any()  # the padding of every slab (cg 4 / 8): written, as zeros
    assert np.array_equal(s.astype(np.int64).sum(axis=0)[..., :cg].transpose(0, 3, 1, 2), acc)
    amax = ops.new_range()
    got = _nchw(getattr(ops, pre + "_wgrad_reduce")(g, groups, slab, amax))
    assert got.shape == (c, cgp, 3, 3) and np.array_equal(got[:, :cg], acc) and not got[:, cg:].any()
    assert ops.range_max(amax) == GM.GC.absmax(acc)
