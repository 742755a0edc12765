"""GPU parity of the grouped conv launches at group widths 4 and 8 (niti_gconv_narrow_*, csrc/niti_grouped_narrow.hip)
against the oracle over the block-diagonal dense weight, bit for bit."""
import ctypes as C
import functools

import numpy as np
import pytest

import grouped_cases as GC
from grouped_cases import DC, O
from test_gpu_grouped_ops import POISON, POISON32, T, _dev, _nchw, _nhwc  # noqa: F401 -- T: the module's GPU fixture

pytestmark = pytest.mark.gpu

SHAPES = (  # (n, C, G, h, pad, stride)
    (1, 64, 16, 1, 1, 1),    # cg 4, one full instruction; only the centre tap is real
    (3, 80, 20, 5, 1, 1),    # cg 4, a partial 64-channel chunk, a partial quad, odd batch
    (2, 32, 4, 7, 0, 1),     # cg 8, half the blocks idle, output smaller than input
    (2, 128, 16, 6, 2, 1),   # cg 8, two chunks, the input gradient's pad 0
    (2, 64, 16, 9, 1, 2),    # cg 4 at stride 2, odd map to 5x5
    (3, 48, 6, 8, 1, 2),     # cg 8 at stride 2, even map; the last dx row and column read by one tap
    (1, 64, 8, 4, 0, 2),     # a dx row and column that no output reads must be zeros
    (4, 64, 16, 16, 1, 1),   # more than one weight-gradient slab
)
AMPS = {"raw": 1, "shifted": 127}  # |a|, |w| <= 1: |acc| <= 72, no shift; <= 127: a shift above 1


def _geoms(shape):
    from niti_amd import ops
    n, c, _, h, pad, stride = shape
    return ops.geom(n, c, h, h, c, 3, stride=stride, pad=pad), O.geom(n, c, h, h, c, 3, stride=stride, pad=pad)


@functools.lru_cache(maxsize=None)
def _inputs(shape):
    """(x, dy, w, mask_y, mask_x) as uniform draws in [-1, 1], to be scaled: every channel's weights differ."""
    n, c, groups, h, _, _ = shape
    oh = _geoms(shape)[1].oh
    rng = np.random.default_rng(7000 + SHAPES.index(shape))
    return DC._ro(rng.uniform(-1, 1, (n, c, h, h)), rng.uniform(-1, 1, (n, c, oh, oh)), rng.uniform(-1, 1, (c, c // groups, 3, 3)),
                  rng.integers(-3, 4, (n, c, oh, oh)).astype(np.int8), rng.integers(-3, 4, (n, c, h, h)).astype(np.int8))


@pytest.mark.parametrize("dgrad", (False, True))
@pytest.mark.parametrize("cls", AMPS)
@pytest.mark.parametrize("shape", SHAPES)
def test_forward_and_input_gradient(T, shape, cls, dgrad):
    """Both passes into poisoned outputs, without and with the relu / relu_mask."""
    from niti_amd import ops
    (g, go), groups = _geoms(shape), shape[2]
    assert ops.gconv_narrow_ok(g, groups) and not ops.gconv2_ok(g, groups)
    ux, udy, uw, my, mx = _inputs(shape)
    a, w, mask = np.rint((udy if dgrad else ux) * AMPS[cls]).astype(np.int8), np.rint(uw * AMPS[cls]).astype(np.int8), mx if dgrad else my
    q, inc, acc = GC.act_ref(go, groups, a, w, dgrad)
    assert DC._in_class(DC._bw(acc), "le0" if cls == "raw" else "gt1")
    a16, w16, m16 = _nhwc(T, a), ops.gconv_weight(_dev(T, w)), _nhwc(T, mask)
    assert tuple(w16.shape) == (shape[1], 3, 3, 16)
    ei, ws = _dev(T, np.array([-5], np.int8)), _dev(T, np.array([-6], np.int8))
    fn = ops.gconv_narrow_dgrad if dgrad else ops.gconv_narrow_fwd
    for on in (False, True):
        kw = dict(relu_mask=m16 if on else None) if dgrad else dict(relu=on, exp_in=ei, wscale=ws)
        want = q if not on else O.relu_grad(mask, q) if dgrad else O.relu(q)
        amax = ops.new_range()
        fn(g, groups, a16, w16, amax, 0, **kw)
        assert ops.range_max(amax) == GC.absmax(acc)
        out = T.full((g.n, g.h, g.w, g.cip) if dgrad else (g.n, g.oh, g.ow, g.cop), POISON, dtype=T.int8, device="cuda")
        e = T.full((1,), POISON, dtype=T.int8, device="cuda")
        fn(g, groups, a16, w16, amax, 1, out=out, exp_out=e, **kw)
        assert int(e.item()) == (inc if dgrad else DC._e8(-5 - 6 + inc)), (on, inc)
        assert np.array_equal(_nchw(out), want), on


@pytest.mark.parametrize("shape", SHAPES)
def test_weight_gradient(T, shape):
    from niti_amd import ops
    n, c, groups, h, pad, stride = shape
    cg = c // groups
    g, go = _geoms(shape)
    ux, udy, _, _, _ = _inputs(shape)
    x, dy = np.rint(ux * 127).astype(np.int8), np.rint(udy * 127).astype(np.int8)
    acc = GC.wgrad_ref(go, groups, x, dy)
    slabs = ops.gconv_narrow_wgrad_slabs(g, groups)
    assert slabs >= 1 and (shape != SHAPES[-1] or slabs > 1)
    slab = ops.gconv_narrow_wgrad(g, groups, _nhwc(T, x), _nhwc(T, dy))
    assert slab.shape == (slabs, c * 9 * 16)
    s = slab.cpu().numpy().reshape(slabs, c, 3, 3, 16)
    assert not s[..., cg:].any()  # the padding of every slab: written, as zeros
    assert np.array_equal(s.astype(np.int64).sum(axis=0)[..., :cg].transpose(0, 3, 1, 2), acc)
    amax = ops.new_range()
    got = _nchw(ops.gconv_narrow_wgrad_reduce(g, groups, slab, amax))
    assert np.array_equal(got[:, :cg], acc) and not got[:, cg:].any() and ops.range_max(amax) == GC.absmax(acc)


def test_argument_errors_launch_nothing(T):
    from niti_amd import _lib as L, ops
    lib = L.lib()
    n, c, h = 2, 64, 8
    g = ops.geom(n, c, h, h, c, 3, pad=1)
    x16 = T.zeros((n, h, h, c), dtype=T.int8, device="cuda")
    w16 = T.zeros((c, 3, 3, 16), dtype=T.int8, device="cuda")
    amax = ops.new_range()
    out = T.full((n, h, h, c), POISON, dtype=T.int8, device="cuda")
    ns = ops.gconv_narrow_wgrad_slabs(g, 16)
    slab = T.full((ns, c * 9 * 16), POISON32, dtype=T.int32, device="cuda")
    st, nb = C.c_void_p(T.cuda.current_stream().cuda_stream), slab.numel() * 4
    o = L.DwconvOut()
    o.out = out.data_ptr()
    P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    act = [C.byref(g), 16, P(x16), P(w16), P(amax), C.byref(o), 1, st]
    good = {"fwd": (lib.niti_gconv_narrow_fwd, act), "dgrad": (lib.niti_gconv_narrow_dgrad, act),
            "wgrad": (lib.niti_gconv_narrow_wgrad, [C.byref(g), 16, P(x16), P(x16), P(slab), nb, None, st]),
            "reduce": (lib.niti_gconv_narrow_wgrad_reduce, [C.byref(g), 16, P(slab), ns, P(slab), None, st])}
    geoms = [(g, 32), (ops.geom(n, 48, h, h, 48, 3, pad=1), 4), (g, 4),  # cg 2, 12, 16
             (ops.geom(n, 8, h, h, 8, 3, pad=1), 2),                      # cg 4, C = 8
             (ops.geom(n, c, h, h, c, 3, stride=3, pad=1), 16), (ops.geom(n, c, h, h, c, 5, pad=2), 16)]
    assert ns >= 1 and not any(ops.gconv_narrow_ok(bg, gr) or ops.gconv_narrow_wgrad_slabs(bg, gr) for bg, gr in geoms)
    bad = [(k, {0: C.byref(bg), 1: gr}) for bg, gr in geoms for k in ("fwd", "dgrad", "wgrad")]
    bad += [(k, {i: None}) for k in ("fwd", "dgrad") for i in (0, 2, 3, 4, 5)] + [(k, {i: None}) for k, i in
            (("wgrad", 2), ("wgrad", 3), ("wgrad", 4), ("reduce", 2))]
    for k, sub in bad:
        fn, args = good[k]
        assert fn(*[sub.get(i, a) for i, a in enumerate(args)]) == L.INVALID_VALUE, (k, sub)
    # the wider launches keep refusing these widths
    assert lib.niti_gconv2_fwd(*act) == L.INVALID_VALUE and lib.niti_gconv_fwd(*act) == L.INVALID_VALUE
    T.cuda.synchronize()
    assert bool((out == POISON).all()) and bool((slab == POISON32).all()) and ops.range_max(amax) == 0
