"""GPU parity of the depthwise launches at stride 2 (niti_dwconv2_*, csrc/niti_depthwise.hip) against the
oracle, bit for bit, at the shapes of tests/strided_cases.py: forward and input gradient in every shift
class with relu / relu_mask, the exponent, the published max|acc| and zero pad channels into poisoned
outputs, a larger range written between the passes, the weight gradient's slabs through both sums and the
update at 0 / 2 / 4 bits, the stride-1 results of the new calls against the old ones, and the argument errors."""
import ctypes as C

import numpy as np
import pytest

import depthwise_cases as DC
import strided_cases as SC

pytestmark = pytest.mark.gpu

POISON = 0x5A


@pytest.fixture(scope="module")
def T():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import niti_amd  # noqa: F401
    return torch


def _geom(shape, stride=2):
    from niti_amd import ops
    n, c, h, k, pad = shape
    return ops.geom(n, c, h, h, c, k, stride=stride, pad=pad)


def _dev(T, a):
    return T.from_numpy(np.array(a)).cuda()  # (a copy: the shared inputs are read-only)


def _nhwc16(T, a):
    from niti_amd import ops
    return ops.nchw_to_nhwc16(_dev(T, a))


def _check_out(T, out16, want, what):
    """out16 NHWC16 against want NCHW: the real channels equal, the pad channels zero."""
    got = out16.cpu().numpy()
    c = want.shape[1]
    assert got.shape[:3] == (want.shape[0], want.shape[2], want.shape[3]), what
    assert np.array_equal(np.transpose(got[..., :c], (0, 3, 1, 2)), want), what
    assert not np.any(got[..., c:]), (what, "pad channels")


def _two_passes(T, fn, dgrad, g, a16, w16, bump=None, **kw):
    """Both passes of fn into a poisoned output; bump: a larger max written into one range word between
    them (what a MAX all-reduce over ranks leaves there)."""
    from niti_amd import ops
    amax = ops.new_range()
    fn(g, a16, w16, amax, 0, **kw)
    own = ops.range_max(amax)
    if bump is not None:
        amax[5 * 32] = bump
    shape = (g.n, g.h, g.w, g.cip) if dgrad else (g.n, g.oh, g.ow, g.cip)
    out = T.full(shape, POISON, dtype=T.int8, device="cuda")
    e = T.full((1,), POISON, dtype=T.int8, device="cuda")
    fn(g, a16, w16, amax, 1, out=out, exp_out=e, **kw)
    return out, int(e.item()), own


@pytest.mark.parametrize("cls", SC.SHIFT_CLASSES)
@pytest.mark.parametrize("sid", SC.SHAPE_IDS)
def test_forward(T, sid, cls):
    from niti_amd import ops
    shape = SC.OP_SHAPES[sid]
    g, go = _geom(shape), SC.geom_of(shape)
    assert ops.dwconv2_ok(g) and not ops.dwconv_ok(g) and (g.oh, g.ow) == (go.oh, go.ow)
    x, w, _ = SC.act_inputs(sid, cls)
    x16, w16 = _nhwc16(T, x), ops.dwconv_weight(_dev(T, w))
    ei, ws = _dev(T, np.array([-5], np.int8)), _dev(T, np.array([-6], np.int8))
    for relu in (False, True):
        y, e, acc = SC.dw_fwd_ref(go, x, w, -5, -6, relu=relu)
        out, ge, own = _two_passes(T, ops.dwconv2_fwd, False, g, x16, w16, relu=relu, exp_in=ei, wscale=ws)
        assert own == int(np.abs(acc.astype(np.int64)).max())
        assert ge == e, (relu, ge, e)
        _check_out(T, out, y, ("fwd", relu))
    out, ge, _ = _two_passes(T, ops.dwconv2_fwd, False, g, x16, w16)  # no exponent operands: exp_out = inc alone
    assert ge == SC.dw_fwd_ref(go, x, w, 0, 0)[1]


@pytest.mark.parametrize("cls", SC.SHIFT_CLASSES)
@pytest.mark.parametrize("sid", SC.SHAPE_IDS)
def test_input_gradient(T, sid, cls):
    from niti_amd import ops
    shape = SC.OP_SHAPES[sid]
    g, go = _geom(shape), SC.geom_of(shape)
    dy, w, mask = SC.act_inputs(sid, cls, True)
    dy16, w16, m16 = _nhwc16(T, dy), ops.dwconv_weight(_dev(T, w)), _nhwc16(T, mask)
    for use_mask in (False, True):
        dx, inc, acc = SC.dw_dgrad_ref(go, dy, w, relu_mask=mask if use_mask else None)
        out, ge, own = _two_passes(T, ops.dwconv2_dgrad, True, g, dy16, w16, relu_mask=m16 if use_mask else None)
        assert own == int(np.abs(acc.astype(np.int64)).max()) and ge == inc
        _check_out(T, out, dx, ("dgrad", use_mask))  # (rows and columns no output reads: written, as zeros)


@pytest.mark.parametrize("sid", SC.BUMP_SHAPES)
def test_larger_range_between_the_passes(T, sid):
    """The range words after a MAX all-reduce: the second pass requantises under them, not its own max."""
    from niti_amd import ops
    shape = SC.OP_SHAPES[sid]
    g, go = _geom(shape), SC.geom_of(shape)
    x, w, _ = SC.act_inputs(sid, "gt1")
    acc = SC.dw_fwd_ref(go, x, w)[2]
    big = 8 * int(np.abs(acc.astype(np.int64)).max()) + 3
    y, e, _ = SC.dw_fwd_ref(go, x, w, -7, -7, relu=True, amax=big)
    ei = _dev(T, np.array([-7], np.int8))
    out, ge, _ = _two_passes(T, ops.dwconv2_fwd, False, g, _nhwc16(T, x), ops.dwconv_weight(_dev(T, w)), bump=big,
                             relu=True, exp_in=ei, wscale=ei)
    assert ge == e and e != SC.dw_fwd_ref(go, x, w, -7, -7)[1]
    _check_out(T, out, y, "fwd under a larger range")
    dy, w, mask = SC.act_inputs(sid, "eq1", True)
    acc = SC.dw_dgrad_ref(go, dy, w)[2]
    big = 4 * int(np.abs(acc.astype(np.int64)).max()) + 1
    dx, inc, _ = SC.dw_dgrad_ref(go, dy, w, relu_mask=mask, amax=big)
    out, ge, _ = _two_passes(T, ops.dwconv2_dgrad, True, g, _nhwc16(T, dy), ops.dwconv_weight(_dev(T, w)), bump=big,
                             relu_mask=_nhwc16(T, mask))
    assert ge == inc
    _check_out(T, out, dx, "dgrad under a larger range")


def _w_from16(acc16, c):
    """[1][k][k][cp] -> [C, 1, k, k]."""
    a = acc16.cpu().numpy()
    assert not np.any(a[..., c:]), "pad channels"
    return np.ascontiguousarray(np.transpose(a[0, :, :, :c], (2, 0, 1))[:, None])


@pytest.mark.parametrize("cls", SC.WGRAD_CLASSES)
@pytest.mark.parametrize("sid", SC.SHAPE_IDS)
def test_weight_gradient_and_update(T, sid, cls):
    from niti_amd import ops
    shape = SC.OP_SHAPES[sid]
    n, c, h, k, pad = shape
    g, go = _geom(shape), SC.geom_of(shape)
    x, dy, w = SC.wgrad_inputs(sid, cls)
    acc, bw, _ = SC.dw_wgrad_ref(go, x, dy)
    x16, dy16 = _nhwc16(T, x), _nhwc16(T, dy)
    slabs = ops.dwconv2_wgrad_slabs(g)
    assert slabs >= 1 and (sid != SC.MULTI_SLAB or slabs > 1) and ops.dwconv_wgrad_slabs(g) == 0
    slab = ops.dwconv2_wgrad(g, x16, dy16)
    assert slab.shape == (slabs, k * k * g.cip)
    assert np.array_equal(slab.cpu().numpy().astype(np.int64).sum(axis=0).reshape(k, k, g.cip)[:, :, :c],
                          np.transpose(acc[:, 0], (1, 2, 0)))
    # summed by the reduce launch and by the update launch's combine: the same tensor, the same range
    a1 = ops.new_range()
    got1 = ops.dwconv2_wgrad_reduce(g, slab, a1)
    got2 = T.full((1, k, k, g.cip), 0x5A5A5A5A, dtype=T.int32, device="cuda")
    a2 = ops.new_range()
    ops.sgd_combine([(slab, k * k * g.cip, got2, a2)])
    amax = int(np.abs(acc.astype(np.int64)).max())
    for got, a in ((got1, a1), (got2, a2)):
        assert np.array_equal(_w_from16(got, c), acc)
        assert ops.range_max(a) == amax
    # the update launch at 0 / 2 / 4 bits, the slabs combined inside it
    w16 = [ops.dwconv_weight(_dev(T, w)) for _ in range(3)]
    g16 = [T.full((1, k, k, g.cip), POISON, dtype=T.int8, device="cuda") for _ in range(3)]
    jobs = [dict(acc=T.full((1, k, k, g.cip), 0x5A5A5A5A, dtype=T.int32, device="cuda"), amax=ops.new_range(), w16=w16[j],
                 ci=c, g=g16[j], slab=slab) for j in range(3)]
    bits = (0, 2, 4)
    ops.sgd_update_many_bits(jobs, _dev(T, np.array(bits, np.int32)))
    for j, b in enumerate(bits):
        nw, kept = SC.dw_update_ref(w, acc, b)
        assert np.array_equal(_w_from16(w16[j], c), nw), (cls, b)
        assert np.array_equal(_w_from16(jobs[j]["acc"], c), acc)
        if b != 0:
            assert np.array_equal(_w_from16(g16[j], c), kept), (cls, b)


@pytest.mark.parametrize("shape", [DC.OP_SHAPES[2], DC.OP_SHAPES[4]])
def test_stride_1_through_the_new_calls_is_the_old_launch(T, shape):
    from niti_amd import ops
    n, c, h, k, pad = shape
    g = _geom(shape, stride=1)
    assert ops.dwconv2_ok(g) and ops.dwconv_ok(g) and ops.dwconv2_wgrad_slabs(g) == ops.dwconv_wgrad_slabs(g)
    x, w, mask = DC.act_inputs(shape, "gt1")
    x16, w16, m16 = _nhwc16(T, x), ops.dwconv_weight(_dev(T, w)), None
    old = _two_passes(T, ops.dwconv_fwd, False, g, x16, w16, relu=True)
    new = _two_passes(T, ops.dwconv2_fwd, False, g, x16, w16, relu=True)
    assert T.equal(old[0], new[0]) and old[1:] == new[1:]
    dy, w, mask = DC.act_inputs(shape, "gt1", True)
    dy16, w16, m16 = _nhwc16(T, dy), ops.dwconv_weight(_dev(T, w)), _nhwc16(T, mask)
    old = _two_passes(T, ops.dwconv_dgrad, True, g, dy16, w16, relu_mask=m16)
    new = _two_passes(T, ops.dwconv2_dgrad, True, g, dy16, w16, relu_mask=m16)
    assert T.equal(old[0], new[0]) and old[1:] == new[1:]
    x, dy, _ = DC.wgrad_inputs(shape, "large")
    x16, dy16 = _nhwc16(T, x), _nhwc16(T, dy)
    s_old, s_new = ops.dwconv_wgrad(g, x16, dy16), ops.dwconv2_wgrad(g, x16, dy16)
    assert T.equal(s_old, s_new)
    a_old, a_new = ops.new_range(), ops.new_range()
    assert T.equal(ops.dwconv_wgrad_reduce(g, s_old, a_old), ops.dwconv2_wgrad_reduce(g, s_new, a_new))
    assert ops.range_max(a_old) == ops.range_max(a_new)


def test_argument_errors_launch_nothing(T):
    from niti_amd import _lib as L, ops
    lib = L.lib()
    shape = SC.OP_SHAPES["B"]
    n, c, h, k, pad = shape
    g = _geom(shape)
    x, w, _ = SC.act_inputs("B", "gt1")
    x16, w16 = _nhwc16(T, x), ops.dwconv_weight(_dev(T, w))
    amax = ops.new_range()
    out = T.full((n, h, h, g.cip), POISON, dtype=T.int8, device="cuda")  # (the larger of the two outputs)
    slab = T.full((ops.dwconv2_wgrad_slabs(g), k * k * g.cip), 0x5A5A5A5A, dtype=T.int32, device="cuda")
    st = C.c_void_p(T.cuda.current_stream().cuda_stream)
    o = L.DwconvOut()
    o.out = out.data_ptr()
    P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    uneven = ops.geom(n, c, 8, 8, c, 3, stride=2, pad=1)
    uneven.stride_w = 1
    assert lib.niti_geom_finalize(C.byref(uneven)) == 0
    bad_geoms = [ops.geom(n, c, 9, 9, c, 3, stride=3, pad=1),                   # stride 3
                 uneven,                                                        # unequal strides
                 ops.geom(n, c, h, h, c + 16, k, stride=2, pad=pad),            # c_in != c_out
                 ops.geom(n, c, 8, 8, c, 7, stride=2, pad=3),                   # k not 3 or 5
                 ops.geom(n, c, 8, 8, c, 1, stride=2, pad=0),
                 ops.geom(n, c, 8, 8, c, 3, stride=2, pads=(1, 1, 0, 0)),       # uneven pads
                 ops.geom(n, c, 8, 8, c, 3, stride=2, pad=1, dilate=2),         # dilation
                 ops.geom(2 ** 31 // (64 * 64 * 64) + 1, 64, 64, 64, 64, 3, stride=2, pad=1)]  # an operand of 2^31 bytes
    for bg in bad_geoms:
        assert not ops.dwconv2_ok(bg) and ops.dwconv2_wgrad_slabs(bg) == 0
    calls = []
    for bg in bad_geoms:
        calls.append(lambda bg=bg: lib.niti_dwconv2_fwd(C.byref(bg), P(x16), P(w16), P(amax), C.byref(o), 1, st))
        calls.append(lambda bg=bg: lib.niti_dwconv2_dgrad(C.byref(bg), P(x16), P(w16), P(amax), C.byref(o), 1, st))
        calls.append(lambda bg=bg: lib.niti_dwconv2_wgrad(C.byref(bg), P(x16), P(x16), P(slab), slab.numel() * 4, None, st))
    # the stride-2 geometry through the calls that take stride 1 alone
    calls += [lambda: lib.niti_dwconv_fwd(C.byref(g), P(x16), P(w16), P(amax), C.byref(o), 1, st),
              lambda: lib.niti_dwconv_dgrad(C.byref(g), P(x16), P(w16), P(amax), C.byref(o), 1, st),
              lambda: lib.niti_dwconv_wgrad(C.byref(g), P(x16), P(x16), P(slab), slab.numel() * 4, None, st),
              lambda: lib.niti_dwconv_wgrad_reduce(C.byref(g), P(slab), slab.shape[0], P(slab), None, st)]
    for fn in (lib.niti_dwconv2_fwd, lib.niti_dwconv2_dgrad):
        calls += [lambda fn=fn: fn(None, P(x16), P(w16), P(amax), C.byref(o), 1, st),
                  lambda fn=fn: fn(C.byref(g), None, P(w16), P(amax), C.byref(o), 1, st),
                  lambda fn=fn: fn(C.byref(g), P(x16), None, P(amax), C.byref(o), 1, st),
                  lambda fn=fn: fn(C.byref(g), P(x16), P(w16), None, C.byref(o), 1, st),
                  lambda fn=fn: fn(C.byref(g), P(x16), P(w16), P(amax), None, 1, st),
                  lambda fn=fn: fn(C.byref(g), P(x16), P(w16), P(amax), C.byref(o), 2, st),
                  lambda fn=fn: fn(C.byref(g), P(x16), P(w16), P(amax), C.byref(L.DwconvOut()), 1, st)]  # no out
    o_relu, o_mask = L.DwconvOut(), L.DwconvOut()
    o_relu.out = o_mask.out = out.data_ptr()
    o_relu.relu = 1
    o_mask.relu_mask = out.data_ptr()
    calls += [lambda: lib.niti_dwconv2_dgrad(C.byref(g), P(x16), P(w16), P(amax), C.byref(o_relu), 1, st),
              lambda: lib.niti_dwconv2_fwd(C.byref(g), P(x16), P(w16), P(amax), C.byref(o_mask), 1, st),
              lambda: lib.niti_dwconv2_wgrad(C.byref(g), None, P(x16), P(slab), slab.numel() * 4, None, st),
              lambda: lib.niti_dwconv2_wgrad(C.byref(g), P(x16), None, P(slab), slab.numel() * 4, None, st),
              lambda: lib.niti_dwconv2_wgrad(C.byref(g), P(x16), P(x16), None, slab.numel() * 4, None, st),
              lambda: lib.niti_dwconv2_wgrad(C.byref(g), P(x16), P(x16), P(slab), slab.numel() * 4 - 4, None, st),
              lambda: lib.niti_dwconv2_wgrad_reduce(C.byref(g), P(slab), slab.shape[0] + 1, P(slab), None, st),
              lambda: lib.niti_dwconv2_wgrad_reduce(C.byref(g), None, slab.shape[0], P(slab), None, st)]
    for i, call in enumerate(calls):
        assert call() == L.INVALID_VALUE, i
    T.cuda.synchronize()
    assert bool((out == POISON).all()) and bool((slab == 0x5A5A5A5A).all()) and ops.range_max(amax) == 0
