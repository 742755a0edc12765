"""GPU parity of the grouped conv launches at the group widths 24, 40, 48, 56, 72, ..., 128 (niti_gconv_packed_*,
csrc/niti_grouped_packed.hip) against the oracle over the block-diagonal dense weight, bit for bit."""
import ctypes as C
import functools

import numpy as np
import pytest

import grouped_cases as GC
from grouped_cases import DC, O
from test_gpu_grouped_ops import POISON, POISON32, T, _dev, _nchw, _nhwc  # noqa: F401 -- T: the module's GPU fixture

pytestmark = pytest.mark.gpu

SHAPES = (  # (n, C, G, h, pad, stride)
    (2, 48, 2, 5, 1, 1),     # cg 24: 216 K bytes, slots that straddle taps, a 24-byte tail chunk, 1.5 output tiles
    (3, 72, 3, 7, 0, 1),     # cg 24, C no multiple of 16 (8 padding channels), odd batch
    (1, 80, 2, 6, 2, 1),     # cg 40, the input gradient at pad 0
    (2, 96, 2, 9, 1, 2),     # cg 48 at stride 2, odd map
    (1, 112, 2, 8, 1, 2),    # cg 56 at stride 2, even map, C a multiple of 16 but not of 32
    (1, 48, 2, 4, 0, 2),     # dx rows and columns that no output reads must be zeros
    (1, 240, 2, 4, 1, 1),    # cg 120, 16.875 chunks
    (1, 256, 2, 4, 1, 1),    # cg 128, the weight-tile loop at its LDS maximum
    (1, 144, 2, 34, 1, 1),   # cg 72: a map wider than one column segment (32 columns from cg 72 up), 5 output tiles
    (4, 48, 2, 8, 1, 1),     # more than one weight-gradient slab
)
AMPS = {"raw": 1, "shifted": 127}  # |a|, |w| <= 1: the sums stay below 2^7, no shift; <= 127: a shift above 1


def _geoms(shape):
    from niti_amd import ops
    n, c, _, h, pad, stride = shape
    return ops.geom(n, c, h, h, c, 3, stride=stride, pad=pad), O.geom(n, c, h, h, c, 3, stride=stride, pad=pad)


@functools.lru_cache(maxsize=None)
def _inputs(shape):
    """(x, dy, w, mask_y, mask_x) as uniform draws in [-1, 1], to be scaled: every channel's weights differ."""
    n, c, groups, h, _, _ = shape
    oh = _geoms(shape)[1].oh
    rng = np.random.default_rng(8000 + SHAPES.index(shape))
    return DC._ro(rng.uniform(-1, 1, (n, c, h, h)), rng.uniform(-1, 1, (n, c, oh, oh)), rng.uniform(-1, 1, (c, c // groups, 3, 3)),
                  rng.integers(-3, 4, (n, c, oh, oh)).astype(np.int8), rng.integers(-3, 4, (n, c, h, h)).astype(np.int8))


@pytest.mark.parametrize("dgrad", (False, True))
@pytest.mark.parametrize("cls", AMPS)
@pytest.mark.parametrize("shape", SHAPES)
def test_forward_and_input_gradient(T, shape, cls, dgrad):
    """Both passes into poisoned outputs, without and with the relu / relu_mask; the padding channels come out zero."""
    from niti_amd import ops
    (g, go), (_, c, groups) = _geoms(shape), shape[:3]
    assert ops.gconv_packed_ok(g, groups) and not ops.gconv2_ok(g, groups)
    ux, udy, uw, my, mx = _inputs(shape)
    a, w, mask = np.rint((udy if dgrad else ux) * AMPS[cls]).astype(np.int8), np.rint(uw * AMPS[cls]).astype(np.int8), mx if dgrad else my
    q, inc, acc = GC.act_ref(go, groups, a, w, dgrad)
    assert DC._in_class(DC._bw(acc), "le0" if cls == "raw" else "gt1")
    a16, w16, m16 = _nhwc(T, a), ops.gconv_weight(_dev(T, w)), _nhwc(T, mask)
    assert tuple(w16.shape) == (c, 3, 3, c // groups)
    ei, ws = _dev(T, np.array([-5], np.int8)), _dev(T, np.array([-6], np.int8))
    fn = ops.gconv_packed_dgrad if dgrad else ops.gconv_packed_fwd
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
        got = _nchw(out)
        assert np.array_equal(got[:, :c], want) and not got[:, c:].any(), on


@pytest.mark.parametrize("shape", SHAPES)
def test_weight_gradient(T, shape):
    from niti_amd import ops
    n, c, groups, h, pad, stride = shape
    cg = c // groups
    g, go = _geoms(shape)
    ux, udy, _, _, _ = _inputs(shape)
    x, dy = np.rint(ux * 127).astype(np.int8), np.rint(udy * 127).astype(np.int8)
    acc = GC.wgrad_ref(go, groups, x, dy)
    slabs = ops.gconv_packed_wgrad_slabs(g, groups)
    assert slabs >= 1 and (shape != SHAPES[-1] or slabs > 1)
    slab = ops.gconv_packed_wgrad(g, groups, _nhwc(T, x), _nhwc(T, dy))
    assert slab.shape == (slabs, c * 9 * cg)  # unpadded, every element written
    s = slab.cpu().numpy().reshape(slabs, c, 3, 3, cg)
    assert np.array_equal(s.astype(np.int64).sum(axis=0).transpose(0, 3, 1, 2), acc)
    amax = ops.new_range()
    got = _nchw(ops.gconv_packed_wgrad_reduce(g, groups, slab, amax))
    assert np.array_equal(got, acc) and ops.range_max(amax) == GC.absmax(acc)
    w = np.rint(_inputs(shape)[2] * 127).astype(np.int8)  # gconv_weight and its inverse at this width
    assert np.array_equal(ops.ohwi16_to_oihw(ops.gconv_weight(_dev(T, w)), cg).cpu().numpy(), w)


def test_argument_errors_launch_nothing(T):
    from niti_amd import _lib as L, ops
    lib = L.lib()
    n, c, h, gr = 2, 48, 8, 2
    g = ops.geom(n, c, h, h, c, 3, pad=1)
    x16 = T.zeros((n, h, h, c), dtype=T.int8, device="cuda")
    w16 = T.zeros((c, 3, 3, c // gr), dtype=T.int8, device="cuda")
    amax = ops.new_range()
    out = T.full((n, h, h, c), POISON, dtype=T.int8, device="cuda")
    ns = ops.gconv_packed_wgrad_slabs(g, gr)
    slab = T.full((ns, c * 9 * (c // gr)), POISON32, dtype=T.int32, device="cuda")
    st, nb = C.c_void_p(T.cuda.current_stream().cuda_stream), slab.numel() * 4
    o = L.DwconvOut()
    o.out = out.data_ptr()
    P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    act = [C.byref(g), gr, P(x16), P(w16), P(amax), C.byref(o), 1, st]
    good = {"fwd": (lib.niti_gconv_packed_fwd, act), "dgrad": (lib.niti_gconv_packed_dgrad, act),
            "wgrad": (lib.niti_gconv_packed_wgrad, [C.byref(g), gr, P(x16), P(x16), P(slab), nb, None, st]),
            "reduce": (lib.niti_gconv_packed_wgrad_reduce, [C.byref(g), gr, P(slab), ns, P(slab), None, st])}
    geoms = [(g, 4), (g, 3), (ops.geom(n, 64, h, h, 64, 3, pad=1), 2), (ops.geom(n, 272, h, h, 272, 3, pad=1), 2),  # cg 12, 16, 32, 136
             (g, 1), (ops.geom(n, c, h, h, c, 3, stride=3, pad=1), gr), (ops.geom(n, c, h, h, c, 5, pad=2), gr)]
    assert ns >= 1 and not any(ops.gconv_packed_ok(bg, k) or ops.gconv_packed_wgrad_slabs(bg, k) for bg, k in geoms)
    bad = [(k, {0: C.byref(bg), 1: grp}) for bg, grp in geoms for k in ("fwd", "dgrad", "wgrad")]
    bad += [(k, {i: None}) for k in ("fwd", "dgrad") for i in (0, 2, 3, 4, 5)] + [(k, {i: None}) for k, i in
            (("wgrad", 2), ("wgrad", 3), ("wgrad", 4), ("reduce", 2))]
    for k, sub in bad:
        fn, args = good[k]
        assert fn(*[sub.get(i, a) for i, a in enumerate(args)]) == L.INVALID_VALUE, (k, sub)
    # the other two families keep refusing this width
    assert lib.niti_gconv2_fwd(*act) == L.INVALID_VALUE and lib.niti_gconv_narrow_fwd(*act) == L.INVALID_VALUE
    T.cuda.synchronize()
    assert bool((out == POISON).all()) and bool((slab == POISON32).all()) and ops.range_max(amax) == 0
