"""Shapes and runners for tests/test_gpu_rowconv_bands.py and tests/test_rowconv_plan_cpu.py: the
smallest layers that reach each form of the row kernels' K loop the small-batch tests in
test_gpu_rowconv.py never run -- 4 and 8 rows per band (bands that are the image's top, its bottom,
both, or neither), the UNC loop (input channels a multiple of 128) and the K-split form at 2 and 4
chunks per wave.  R follows rowconv_rows: halved while groups * (W / R) * co-blocks < 768.

Every oracle result is computed once per shape (functools caches) and shared, read-only, by the
modes that check against it."""
import functools

import numpy as np

# name: (n, c_in, H, c_out, pool, (W, R, ks, workgroups)) -- forward layers
FWD_LARGE = {
    "16x16_r8": (64, 32, 16, 384, True, (16, 8, 0, 192)),    # top + bottom bands
    "16x16_r4": (32, 32, 16, 384, False, (16, 4, 0, 192)),   # top, two middle, bottom
    "8x8_r4_unc": (128, 128, 8, 384, True, (8, 4, 0, 192)),  # UNC, top + bottom
    "4x4_r4": (384, 128, 4, 512, False, (4, 4, 0, 192)),     # one band that is both
}
# the same geometries with the layer's channel counts swapped: the input gradient's kernel then
# reduces over 32 / 128 channels into 384 / 512 (R starts at 4 there)
DGRAD_LARGE = {
    "16x16_r4_n64": (64, 384, 16, 32, (16, 4, 0, 384)),
    "16x16_r4_n32": (32, 384, 16, 32, (16, 4, 0, 192)),
    "8x8_r4_unc": (128, 384, 8, 128, (8, 4, 0, 192)),
    "4x4_r4": (384, 512, 4, 128, (4, 4, 0, 192)),
}
# ragged image groups on the UNC loop at R = 2 (at 2x2 a 128-channel input is the K-split form, one
# chunk per wave)
SMALL_N = (3, 5)
SMALL_H = (2, 4, 8, 16)
# K-split: (n, reduced channels, ks); n = 19 leaves a ragged second unit
KS_CASES = [(16, 512, 4), (19, 512, 4), (16, 256, 2), (19, 256, 2)]
# VGG-11's 3x3 layers 1..7 at batch 256: (c_in, c_out, H) and the forward form
VGG11_B256 = [((64, 128, 16), (16, 8, 0)), ((128, 256, 8), (8, 4, 0)), ((256, 256, 8), (8, 4, 0)),
              ((256, 512, 4), (4, 2, 0)), ((512, 512, 4), (4, 2, 0)), ((512, 512, 2), (2, 2, 4)),
              ((512, 512, 2), (2, 2, 4))]


def small_plan(n, h):
    """(W, R, ks, workgroups) of the ragged 128 -> 32 (kernel channels) cases."""
    g = 32 // h
    groups = (n + g - 1) // g
    if h == 2:
        return (2, 2, 1, groups)
    return (h, 2, 0, (groups * (h // 2) + 3) // 4)


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def fwd_ref(n, ci, h, co, seed):
    """(x, w, y, exponent) of the oracle's NITI_Conv_Int8 with exp_in -3, wscale -5."""
    import niti_oracle as O
    rng = np.random.default_rng(seed)
    x = rng.integers(-127, 128, (n, ci, h, h)).astype(np.int8)
    w = rng.integers(-127, 128, (co, ci, 3, 3)).astype(np.int8)
    y, e, _, _ = O.conv_fwd(O.geom(n, ci, h, h, co, 3, pad=1), x, w, -3, -5)
    return _ro(x, w, y) + (e,)


@functools.lru_cache(maxsize=None)
def dgrad_q(n, ci, h, co, seed):
    """(dy, w, requantised dx) of the oracle's input gradient of the layer ci -> co."""
    import niti_oracle as O
    rng = np.random.default_rng(seed)
    dy = rng.integers(-127, 128, (n, co, h, h)).astype(np.int8)
    w = rng.integers(-127, 128, (co, ci, 3, 3)).astype(np.int8)
    dq, _, _, _ = O.conv_dgrad(O.geom(n, ci, h, h, co, 3, pad=1), dy, w)
    return _ro(dy, w, dq)


@functools.lru_cache(maxsize=None)
def dgrad_ref(n, ci, h, co, pool, seed):
    """(dy, w, mask or pool input, pool output or None, wanted dx): dx through the previous layer's relu
    mask, or routed through its 2x2 max pool + relu (ties and non-positive inputs included)."""
    import niti_oracle as O
    dy, w, dq = dgrad_q(n, ci, h, co, seed)
    rng = np.random.default_rng(seed + 1)
    if pool:
        px = np.maximum(rng.integers(-2, 6, (n, ci, 2 * h, 2 * h)), 0).astype(np.int8)
        py = O.maxpool(px)
        want = O.relu_grad(px, O.maxpool_grad(px, py, dq))
        return (dy, w) + _ro(px, py, want)
    mk = rng.integers(-2, 3, (n, ci, h, h)).astype(np.int8)
    return (dy, w) + _ro(mk) + (None,) + _ro(O.relu_grad(mk, dq))


def _dev(T, a):
    return T.from_numpy(np.array(a)).cuda()  # (a copy: the cached references are read-only)


def _c32_to_nchw(t, c):
    a = t.cpu().numpy()  # [n][cb][h][w][32]
    return a.transpose(0, 1, 4, 2, 3).reshape(a.shape[0], -1, a.shape[2], a.shape[3])[:, :c]


def spec_pairs(st, dgrad, amax, eo, launch, check):
    """The speculative pair (modes 3 + 4) three times on one state: no hint yet (launch 4 redoes), the
    first pair's hint (a hit), and every predictor's guess forced one bit wide (launch 4 redoes); each
    pair's outputs are the rule's and the slot counts the two misses."""
    off = st.spec_offset(dgrad)
    for rep in range(3):
        if rep == 2:
            for j in (0, 24, 25):
                hint = int(st.state[off + j].item())
                if hint != 0:
                    st.state[off + j] = hint + 1
        amax.zero_()
        if eo is not None:
            eo.zero_()
        check(*launch(4, launch(3, None)))
        assert st.spec_slot(dgrad)[2] == (1 if rep < 2 else 2), (rep, st.spec_slot(dgrad))


def run_fwd(T, n, ci, h, co, pool, mode, form, seed):
    """The forward of one layer (relu where it pools) in `mode` (0 fused, 2 range + requantise, 4 the
    speculative pair) against fwd_ref, bit for bit: output, exponent, pooled output, C32 copy."""
    import niti_oracle as O
    from niti_amd import ops
    relu = pool
    x, w, y_ref, e_ref = fwd_ref(n, ci, h, co, seed)
    r_ref = O.relu(y_ref) if relu else y_ref
    p_ref = O.maxpool(r_ref) if pool else None
    gg = ops.geom(n, ci, h, h, co, 3, pad=1)
    assert ops.conv_rows_plan(gg) == form
    xc = ops.nhwc16_to_c32(ops.nchw_to_nhwc16(_dev(T, x)), ci)
    wf = ops.weights_to_wf(ops.oihw_to_ohwi16(_dev(T, w)), ci)
    eo = T.zeros(1, dtype=T.int8, device="cuda")
    amax = ops.new_range()
    st = ops.RowConvState()
    kw = dict(exp_in=_dev(T, np.array([-3], np.int8)), wscale=_dev(T, np.array([-5], np.int8)), exp_out=eo,
              relu=relu, pool=pool, next_c32=True)

    def check(out, pout, nxt):
        T.cuda.synchronize()
        assert int(st.err.item()) == 0
        assert np.array_equal(out.cpu().numpy()[..., :co].transpose(0, 3, 1, 2), r_ref)
        assert int(eo.item()) == e_ref
        if pool:
            assert np.array_equal(pout.cpu().numpy()[..., :co].transpose(0, 3, 1, 2), p_ref)
        assert np.array_equal(_c32_to_nchw(nxt, co), p_ref if pool else r_ref)

    if mode == 0:
        check(*ops.conv_fwd_rows(gg, xc, wf, amax, mode=0, state=st, **kw))
    elif mode == 4:
        spec_pairs(st, False, amax, eo,
                   lambda m, outs: ops.conv_fwd_rows(gg, xc, wf, amax, mode=m, state=st, outs=outs, **kw), check)
    else:
        ops.conv_fwd_rows(gg, xc, wf, amax, mode=1, **kw)
        check(*ops.conv_fwd_rows(gg, xc, wf, amax, mode=2, **kw))


def run_dgrad(T, n, ci, h, co, pool, mode, form, seed):
    """The input gradient of the layer ci -> co in `mode` against dgrad_ref, bit for bit: the NHWC16
    gradient, its C32 copy and (where a launch's pixels make whole 16-pixel blocks) its P16 copy.
    Returns False if the fused launch was refused because its grid is not resident at once."""
    from niti_amd import ops
    from niti_amd._lib import NitiError
    dy, w, px, py, want = dgrad_ref(n, ci, h, co, pool, seed)
    gg = ops.geom(n, ci, h, h, co, 3, pad=1)
    assert ops.conv_rows_plan(gg, dgrad=True) == form
    nhwc = lambda a: ops.nchw_to_nhwc16(_dev(T, a))  # noqa: E731
    dyc = ops.nhwc16_to_c32(nhwc(dy), co)
    wft = ops.weights_to_wf(ops.oihw_to_ohwi16(_dev(T, w)), ci, transpose=True)
    amax = ops.new_range()
    st = ops.RowConvState()
    kw = dict(dx_c32=True, dx_p16=True)
    if pool:
        kw.update(pool_x=nhwc(px), pool_y=nhwc(py), pool_relu=True)
    else:
        kw.update(relu_mask=nhwc(px))

    def launch(m, outs=None):
        return ops.conv_dgrad_rows(gg, dyc, wft, amax, mode=m, state=st if m != 1 and m != 2 else None, outs=outs, **kw)

    def check(dx, dxc, p16):
        T.cuda.synchronize()
        assert int(st.err.item()) == 0
        assert np.array_equal(dx.cpu().numpy()[..., :ci].transpose(0, 3, 1, 2), want)
        assert np.array_equal(_c32_to_nchw(dxc, ci), want)
        if p16 is not None and p16.numel() > 0:  # (fewer than 16 pixels: an empty copy, nothing asked for)
            assert np.array_equal(p16.cpu().numpy(), ops.nhwc16_to_p16(dx).cpu().numpy())

    def once():  # the mode's launches, or None where the library answers NITI_NOT_SUPPORT
        try:
            if mode == 0:
                return launch(0)
            if mode == 2:
                amax.zero_()
                launch(1)
                return launch(2)
            return launch(4, launch(3))
        except NitiError as e:
            assert e.code == 2, e
            return None

    res = once()
    if res is None and not pool and (h == 4 or n * h * h % 16 != 0):
        kw["dx_p16"] = False  # no whole 16-pixel blocks per wave (4x4, small batch) or tensor
        res = once()
    if res is None:  # a fused launch needs every tile resident at once: more tiles than compute units
        assert mode == 0 and form[3] > T.cuda.get_device_properties(0).multi_processor_count, form
        return False
    if mode == 4:
        st.state.zero_()  # a fresh slot for the three pairs
        spec_pairs(st, True, amax, None, launch, check)
    else:
        check(*res)
    return True
