"""GPU parity of the grouped conv launches (niti_gconv_*, csrc/niti_grouped.hip) against the oracle over the
block-diagonal dense weight, bit for bit, at the shapes of tests/grouped_cases.py."""
import ctypes as C

import numpy as np
import pytest

import grouped_cases as GC
from grouped_cases import O

pytestmark = pytest.mark.gpu

POISON, POISON32 = 0x5A, 0x5A5A5A5A


@pytest.fixture(scope="module")
def T():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import niti_amd  # noqa: F401
    return torch


def _geom(shape):
    from niti_amd import ops
    n, c, _, h, pad = shape
    return ops.geom(n, c, h, h, c, 3, pad=pad)


def _dev(T, a):
    return T.from_numpy(np.array(a)).cuda()  # (a copy: the shared inputs are read-only)


def _nhwc(T, a):
    from niti_amd import ops
    return ops.nchw_to_nhwc16(_dev(T, a))


def _nchw(t):
    """NHWC16 (or a weight's [c_out][3][3][cg]) -> the host order."""
    return np.ascontiguousarray(np.transpose(t.cpu().numpy(), (0, 3, 1, 2)))


def _act_case(T, shape, cls, dgrad, bump=0):
    """Both passes into poisoned outputs, without and with the relu / relu_mask; bump: that multiple of the own
    max (+ 1) is written into one range word between the passes, as a MAX all-reduce would leave it."""
    from niti_amd import ops
    g, go, groups = _geom(shape), GC.geom_of(shape), shape[2]
    assert ops.gconv_ok(g, groups)
    a, w, mask = GC.act_inputs(shape, cls, dgrad)
    own = GC.absmax(GC.act_ref(go, groups, a, w, dgrad)[2])
    q, inc, _ = GC.act_ref(go, groups, a, w, dgrad, amax=bump * own + 1 if bump else None)
    assert not bump or inc != GC.act_ref(go, groups, a, w, dgrad)[1]
    a16, w16, m16 = _nhwc(T, a), ops.gconv_weight(_dev(T, w)), _nhwc(T, mask)
    ei, ws = _dev(T, np.array([-5], np.int8)), _dev(T, np.array([-6], np.int8))
    fn = ops.gconv_dgrad if dgrad else ops.gconv_fwd
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
@pytest.mark.parametrize("shape", GC.OP_SHAPES)
def test_forward_and_input_gradient(T, shape, cls, dgrad):
    _act_case(T, shape, cls, dgrad)


@pytest.mark.parametrize("dgrad,cls,bump", [(False, "gt1", 8), (True, "eq1", 4)])
def test_larger_range_between_the_passes(T, dgrad, cls, bump):
    _act_case(T, GC.OP_SHAPES[1], cls, dgrad, bump)


@pytest.mark.parametrize("shape", GC.OP_SHAPES)
def test_weight_gradient_and_update(T, shape):
    from niti_amd import ops
    n, c, groups, h, pad = shape
    cg = c // groups
    g = _geom(shape)
    x, dy, w = GC.wgrad_inputs(shape)
    acc = GC.wgrad_ref(GC.geom_of(shape), groups, x, dy)
    slabs = ops.gconv_wgrad_slabs(g, groups)
    assert slabs >= 1 and (shape != GC.MULTI_SLAB or slabs > 1)
    slab = ops.gconv_wgrad(g, groups, _nhwc(T, x), _nhwc(T, dy))
    assert slab.shape == (slabs, c * 9 * cg)
    assert np.array_equal(slab.cpu().numpy().astype(np.int64).sum(axis=0).reshape(c, 3, 3, cg).transpose(0, 3, 1, 2), acc)
    # summed by the reduce launch and by the update launch's combine: the same tensor, the same range
    a1, a2 = ops.new_range(), ops.new_range()
    got1 = ops.gconv_wgrad_reduce(g, groups, slab, a1)
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


def test_argument_errors_launch_nothing(T):
    from niti_amd import _lib as L, ops
    lib = L.lib()
    n, c, groups, h, pad = shape = GC.OP_SHAPES[3]
    g = _geom(shape)
    x, w, _ = GC.act_inputs(shape, "gt1")
    x16, w16, amax = _nhwc(T, x), ops.gconv_weight(_dev(T, w)), ops.new_range()
    out = T.full((n, h, h, c), POISON, dtype=T.int8, device="cuda")
    ns = ops.gconv_wgrad_slabs(g, groups)
    slab = T.full((ns, c * 9 * (c // groups)), POISON32, dtype=T.int32, device="cuda")
    st, nb = C.c_void_p(T.cuda.current_stream().cuda_stream), slab.numel() * 4
    o, o_none, o_relu, o_mask = (L.DwconvOut() for _ in range(4))
    o.out = o_relu.out = o_mask.out = o_mask.relu_mask = out.data_ptr()
    o_relu.relu = 1
    P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    act = [C.byref(g), groups, P(x16), P(w16), P(amax), C.byref(o), 1, st]
    good = {"fwd": (lib.niti_gconv_fwd, act), "dgrad": (lib.niti_gconv_dgrad, act),
            "wgrad": (lib.niti_gconv_wgrad, [C.byref(g), groups, P(x16), P(x16), P(slab), nb, None, st]),
            "reduce": (lib.niti_gconv_wgrad_reduce, [C.byref(g), groups, P(slab), ns, P(slab), None, st])}
    geoms = [(g, 1), (g, 0), (g, -3), (g, 5), (g, 6),                         # dense, c % groups, cg 8
             (ops.geom(n, c, h, h, c + 48, 3, pad=pad), groups),                 # c_in != c_out
             (ops.geom(n, c, 8, 8, c, 5, pad=2), groups), (ops.geom(n, c, 8, 8, c, 1), groups),
             (ops.geom(n, c, 8, 8, c, 3, stride=2, pad=1), groups), (ops.geom(n, c, 8, 8, c, 3, pads=(1, 1, 0, 0)), groups),
             (ops.geom(2 ** 31 // (64 * 64 * 64) + 1, 64, 64, 64, 64, 3, pad=1), 2)]  # an operand of 2^31 bytes
    assert not any(ops.gconv_ok(bg, gr) or ops.gconv_wgrad_slabs(bg, gr) for bg, gr in geoms)
    # (launch, {argument index: the bad value}) -- every other argument is the good call's
    bad = [(k, {0: C.byref(bg), 1: gr}) for bg, gr in geoms for k in ("fwd", "dgrad", "wgrad")]
    bad += [(k, {i: None}) for k in ("fwd", "dgrad") for i in (0, 2, 3, 4, 5)] + [(k, {i: None}) for k, i in
            (("wgrad", 2), ("wgrad", 3), ("wgrad", 4), ("reduce", 2))]
    bad += [("fwd", {6: 2}), ("dgrad", {6: 2}), ("fwd", {5: C.byref(o_none)}), ("dgrad", {5: C.byref(o_none)}),  # pass, no out
            ("dgrad", {5: C.byref(o_relu)}), ("fwd", {5: C.byref(o_mask)}), ("wgrad", {5: nb - 4}), ("reduce", {3: ns + 1})]
    for k, sub in bad:
        fn, args = good[k]
        assert fn(*[sub.get(i, a) for i, a in enumerate(args)]) == L.INVALID_VALUE, (k, sub)
    T.cuda.synchronize()
    assert bool((out == POISON).all()) and bool((slab == POISON32).all()) and ops.range_max(amax) == 0
