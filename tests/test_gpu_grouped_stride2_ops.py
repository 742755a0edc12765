"""GPU parity of the stride-2 grouped conv launches (niti_gconv2_*, csrc/niti_grouped.hip) against the oracle over
the block-diagonal dense weight, bit for bit, at the shapes of tests/grouped_stride2_cases.py."""
import ctypes as C

import numpy as np
import pytest

import grouped_cases as GC
import grouped_stride2_cases as G2
from grouped_cases import O
from test_gpu_grouped_ops import POISON, POISON32, T, _dev, _nchw, _nhwc  # noqa: F401 -- T: the module's GPU fixture

pytestmark = pytest.mark.gpu


def _geom(shape, stride=2):
    from niti_amd import ops
    n, c, _, h, pad = shape
    return ops.geom(n, c, h, h, c, 3, stride=stride, pad=pad)


def _act_case(T, shape, cls, dgrad, bump=0):
    """Both passes into poisoned outputs, without and with the relu / relu_mask; bump: that multiple of the own
    max (+ 1) is written into one range word between the passes, as a MAX all-reduce would leave it."""
    from niti_amd import ops
    g, go, groups = _geom(shape), G2.geom_of(shape), shape[2]
    assert ops.gconv2_ok(g, groups) and not ops.gconv_ok(g, groups)
    a, w, mask = G2.act_inputs(shape, cls, dgrad)
    own = GC.absmax(GC.act_ref(go, groups, a, w, dgrad)[2])
    q, inc, _ = GC.act_ref(go, groups, a, w, dgrad, amax=bump * own + 1 if bump else None)
    assert not bump or inc != GC.act_ref(go, groups, a, w, dgrad)[1]
    a16, w16, m16 = _nhwc(T, a), ops.gconv_weight(_dev(T, w)), _nhwc(T, mask)
    ei, ws = _dev(T, np.array([-5], np.int8)), _dev(T, np.array([-6], np.int8))
    fn = ops.gconv2_dgrad if dgrad else ops.gconv2_fwd
    for on in (False, True):
        kw = dict(relu_mask=m16 if on else None) if dgrad else dict(relu=on, exp_in=ei, wscale=ws)
        want = q if not on else O.relu_grad(mask, q) if dgrad else O.relu(q)
        amax = ops.new_range()
        fn(g, groups, a16, w16, amax, 0, **kw)
        assert ops.range_max(amax) == own
        if bump:
            amax[5 * 32] = bump * own + 1
        out = T.full((g.n, g.h, g.w, g.cip) if dgrad else (g.n, g.oh, g.ow, g.cop), POISON, dtype=T.int8, device="cuda")
        e = T.full((1,), POISON, dtype=T.int8, device="cuda")
        fn(g, groups, a16, w16, amax, 1, out=out, exp_out=e, **kw)
        assert int(e.item()) == (inc if dgrad else GC.DC._e8(-5 - 6 + inc)), (on, inc)
        assert np.array_equal(_nchw(out), want), on


@pytest.mark.parametrize("dgrad", (False, True))
@pytest.mark.parametrize("cls", GC.SHIFT_CLASSES)
@pytest.mark.parametrize("shape", G2.OP_SHAPES)
def test_forward_and_input_gradient(T, shape, cls, dgrad):
    _act_case(T, shape, cls, dgrad)


@pytest.mark.parametrize("dgrad,cls,bump", [(False, "gt1", 8), (True, "eq1", 4)])
def test_larger_range_between_the_passes(T, dgrad, cls, bump):
    _act_case(T, G2.OP_SHAPES[1], cls, dgrad, bump)


@pytest.mark.parametrize("shape", G2.OP_SHAPES)
def test_weight_gradient_and_update(T, shape):
    from niti_amd import ops
    n, c, groups, h, pad = shape
    cg = c // groups
    g = _geom(shape)
    x, dy, w = G2.wgrad_inputs(shape)
    acc = GC.wgrad_ref(G2.geom_of(shape), groups, x, dy)
    slabs = ops.gconv2_wgrad_slabs(g, groups)
    assert slabs >= 1 and (shape != G2.MULTI_SLAB or slabs > 1)
    slab = ops.gconv2_wgrad(g, groups, _nhwc(T, x), _nhwc(T, dy))
    assert slab.shape == (slabs, c * 9 * cg)
    assert np.array_equal(slab.cpu().numpy().astype(np.int64).sum(axis=0).reshape(c, 3, 3, cg).transpose(0, 3, 1, 2), acc)
    # summed by the reduce launch and by the update launch's combine: the same tensor, the same range
    a1, a2 = ops.new_range(), ops.new_range()
    got1 = ops.gconv2_wgrad_reduce(g, groups, slab, a1)
    got2 = T.full((c, 3, 3, cg), POISON32, dtype=T.int32, device="cuda")
    ops.sgd_combine([(slab, c * 9 * cg, got2, a2)])
    for got, a in ((got1, a1), (got2, a2)):
        assert np.array_equal(_nchw(got), acc) and ops.range_max(a) == GC.absmax(acc)
    # the update launch at 0 / 2 / 4 bits, the slabs combined inside it
    bits = (0, 2, 4)
    jobs = [dict(acc=T.full((c, 3, 3, cg), POISON32, dtype=T.int32, device="cuda"), amax=ops.new_range(),
                 w16=ops.gconv_weight(_dev(T, w)), ci=cg, g=T.full((c, 3, 3, cg), POISON, dtype=T.int8, device="cuda"), slab=slab)
            for _ in bits]
    ops.sgd_update_many_bits(jobs, _dev(T, np.array(bits, np.int32)))
    for job, b in zip(jobs, bits):
        nw, kept = GC.UB.apply_update(w, acc, b)
        assert np.array_equal(_nchw(job["w16"]), nw) and np.array_equal(_nchw(job["acc"]), acc), b
        assert b == 0 or np.array_equal(_nchw(job["g"]), kept), b


def test_stride_1_through_the_new_calls_is_the_old_launch(T):
    from niti_amd import ops
    shape = GC.OP_SHAPES[1]
    n, c, groups, h, pad = shape
    g = _geom(shape, stride=1)
    for dgrad in (False, True):
        a, w, _ = GC.act_inputs(shape, "gt1", dgrad)
        a16, w16 = _nhwc(T, a), ops.gconv_weight(_dev(T, w))
        outs = []
        for fn in ((ops.gconv_dgrad, ops.gconv2_dgrad) if dgrad else (ops.gconv_fwd, ops.gconv2_fwd)):
            amax = ops.new_range()
            fn(g, groups, a16, w16, amax, 0)
            outs.append((ops.range_max(amax), fn(g, groups, a16, w16, amax, 1)))
        assert outs[0][0] == outs[1][0] and T.equal(outs[0][1], outs[1][1]), dgrad
    x, dy, _ = GC.wgrad_inputs(shape)
    assert ops.gconv2_wgrad_slabs(g, groups) == ops.gconv_wgrad_slabs(g, groups)
    assert T.equal(ops.gconv2_wgrad(g, groups, _nhwc(T, x), _nhwc(T, dy)), ops.gconv_wgrad(g, groups, _nhwc(T, x), _nhwc(T, dy)))


def test_argument_errors_launch_nothing(T):
    from niti_amd import _lib as L, ops
    lib = L.lib()
    n, c, groups, h, pad = shape = G2.OP_SHAPES[3]
    g = _geom(shape)
    x, w, _ = G2.act_inputs(shape, "gt1")
    x16, w16, amax = _nhwc(T, x), ops.gconv_weight(_dev(T, w)), ops.new_range()
    out = T.full((n, h, h, c), POISON, dtype=T.int8, device="cuda")
    ns = ops.gconv2_wgrad_slabs(g, groups)
    slab = T.full((ns, c * 9 * (c // groups)), POISON32, dtype=T.int32, device="cuda")
    st, nb = C.c_void_p(T.cuda.current_stream().cuda_stream), slab.numel() * 4
    o = L.DwconvOut()
    o.out = out.data_ptr()
    P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    act = [C.byref(g), groups, P(x16), P(w16), P(amax), C.byref(o), 1, st]
    wg = [C.byref(g), groups, P(x16), P(x16), P(slab), nb, None, st]
    good = {"fwd": (lib.niti_gconv2_fwd, act), "dgrad": (lib.niti_gconv2_dgrad, act), "wgrad": (lib.niti_gconv2_wgrad, wg),
            "reduce": (lib.niti_gconv2_wgrad_reduce, [C.byref(g), groups, P(slab), ns, P(slab), None, st])}
    # a stride-2 geometry through the old calls
    old = {"fwd": (lib.niti_gconv_fwd, act), "dgrad": (lib.niti_gconv_dgrad, act), "wgrad": (lib.niti_gconv_wgrad, wg)}
    assert not ops.gconv_ok(g, groups) and ops.gconv_wgrad_slabs(g, groups) == 0
    for k, (fn, args) in old.items():
        assert fn(*args) == L.INVALID_VALUE, k
    uneq = ops.geom(n, c, 8, 8, c, 3, stride=2, pad=1)
    uneq.stride_w = 1  # (the output size is derived from the fields on the way in)
    geoms = [ops.geom(n, c, 8, 8, c, 3, stride=3, pad=1), ops.geom(n, c, 8, 8, c, 3, stride=2, pad=1, dilate=2),
             ops.geom(n, c, 8, 8, c, 3, stride=2, pads=(1, 1, 0, 0)), uneq]
    assert not any(ops.gconv2_ok(bg, groups) or ops.gconv2_wgrad_slabs(bg, groups) for bg in geoms)
    bad = [(k, {0: C.byref(bg)}) for bg in geoms for k in ("fwd", "dgrad", "wgrad")]
    bad += [(k, {i: None}) for k in ("fwd", "dgrad") for i in (0, 2, 3, 4, 5)] + [(k, {i: None}) for k, i in
            (("wgrad", 2), ("wgrad", 3), ("wgrad", 4), ("reduce", 2))]
    bad += [("fwd", {6: 2}), ("wgrad", {5: nb - 4}), ("reduce", {3: ns + 1})]
    for k, sub in bad:
        fn, args = good[k]
        assert fn(*[sub.get(i, a) for i, a in enumerate(args)]) == L.INVALID_VALUE, (k, sub)
    T.cuda.synchronize()
    assert bool((out == POISON).all()) and bool((slab == POISON32).all()) and ops.range_max(amax) == 0
