"""Shapes, references and runners for tests/test_gpu_rowconv_mirror.py: the row kernels' forms with
two bands per image (W == 2 R: <4,2>, <8,4>, <16,8>), whose bottom band runs mirrored top to bottom,
and the one-row-per-band form <4,1> of a pooled 4x4 input gradient.

Forward inputs are small (x in {-1, 0, 1, 2}, weights in {-1, 0, 1}) so that after the requantisation
most 2x2 pool windows hold ties: a band whose rows came out in the wrong order then changes which
element the pool takes, not only where values land.  The one-row inputs (one image row of 127s in an
otherwise zero tensor) break the vertical symmetry a mirrored band could hide behind.

Every oracle result is computed once (functools caches) and shared, read-only, by the modes."""
import functools

import numpy as np

import rowconv_band_cases as B

# name: (n, c_in, H, c_out, (W, R, ks, workgroups)) -- forward layers, each with relu + 2x2 pool
FWD = {
    "4x4_r2_unc": (5, 128, 4, 32, (4, 2, 0, 1)),      # UNC loop; a ragged image group (5 of 8)
    "4x4_r2_2chunks": (5, 64, 4, 32, (4, 2, 0, 1)),   # the non-UNC loop, two chunks
    "8x8_r4_unc": (128, 128, 8, 384, (8, 4, 0, 192)),
    "16x16_r8": (64, 32, 16, 384, (16, 8, 0, 192)),
}
# which image the one-row inputs fill: not the first of its image group, and of the second group
# where there is one
ROW_IMG = {"4x4_r2_unc": 1, "4x4_r2_2chunks": 3, "8x8_r4_unc": 5, "16x16_r8": 3}
ROWS = ("above_boundary", "below_boundary", "last")
# the input gradients of the channel-swapped layers (n, layer c_in, H, layer c_out, form), relu mask
DGRAD = {
    "4x4_r2_unc": (5, 32, 4, 128, (4, 2, 0, 1)),      # P16 through p16_pair_store (80 pixels)
    "4x4_r2_2chunks": (5, 32, 4, 64, (4, 2, 0, 1)),
    "8x8_r4_unc": (128, 384, 8, 128, (8, 4, 0, 192)),
}
# one row per band: (n, layer c_in, layer c_out, units at R = 2, workgroups at R = 1) at 4x4, pooled
ROWS1 = {
    "n48_unc": (48, 1024, 128, 384, 192),
    "n45_ragged": (45, 1024, 128, 384, 192),
    "n64_1chunk": (64, 1024, 32, 512, 256),
}


def row_of(case, which):
    h = FWD[case][2]
    return {"above_boundary": h // 2 - 1, "below_boundary": h // 2, "last": h - 1}[which]


@functools.lru_cache(maxsize=None)
def fwd_ref(case, which=None):
    """(x, w, relu'd y, exponent, pooled y) of the oracle's NITI_Conv_Int8 + relu + 2x2 max pool with
    exp_in -3, wscale -5.  which: a one-row input instead of the tie-rich one.  The oracle then runs
    on the one non-zero image alone: the conv works image by image, the rule's max over the tensor
    is that image's, and a zero accumulator requantises to zero -- so the other images' outputs
    are zero and the exponent is the one-image oracle's."""
    import niti_oracle as O
    n, ci, h, co, _ = FWD[case]
    rng = np.random.default_rng(1800 + h + ci)
    w = rng.integers(-1, 2, (co, ci, 3, 3)).astype(np.int8)
    if which is None:
        x = rng.integers(-1, 3, (n, ci, h, h)).astype(np.int8)
        y, e, _, _ = O.conv_fwd(O.geom(n, ci, h, h, co, 3, pad=1), x, w, -3, -5)
    else:
        k = ROW_IMG[case]
        x = np.zeros((n, ci, h, h), np.int8)
        x[k, :, row_of(case, which), :] = 127
        y = np.zeros((n, co, h, h), np.int8)
        y[k:k + 1], e, _, _ = O.conv_fwd(O.geom(1, ci, h, h, co, 3, pad=1), x[k:k + 1], w, -3, -5)
    r = O.relu(y)
    return B._ro(x, w, r) + (e,) + B._ro(O.maxpool(r))


def run_fwd(T, case, mode, which=None):
    """The forward (relu, pool, C32 copy of the pooled output) in `mode` (0 fused, 2 range +
    requantise, 4 the speculative pair) against fwd_ref, bit for bit.  (The C entry records no pool
    codes; the pooled output and its C32 copy carry the pool's choice of element.)"""
    from niti_amd import ops
    n, ci, h, co, form = FWD[case]
    x, w, r_ref, e_ref, p_ref = fwd_ref(case, which)
    gg = ops.geom(n, ci, h, h, co, 3, pad=1)
    assert ops.conv_rows_plan(gg) == form and form[0] == 2 * form[1]
    xc = ops.nhwc16_to_c32(ops.nchw_to_nhwc16(B._dev(T, x)), ci)
    wf = ops.weights_to_wf(ops.oihw_to_ohwi16(B._dev(T, w)), ci)
    eo = T.zeros(1, dtype=T.int8, device="cuda")
    amax = ops.new_range()
    st = ops.RowConvState()
    kw = dict(exp_in=B._dev(T, np.array([-3], np.int8)), wscale=B._dev(T, np.array([-5], np.int8)), exp_out=eo,
              relu=True, pool=True, next_c32=True)

    def check(out, pout, nxt):
        T.cuda.synchronize()
        assert int(st.err.item()) == 0
        assert np.array_equal(out.cpu().numpy()[..., :co].transpose(0, 3, 1, 2), r_ref)
        assert int(eo.item()) == e_ref
        assert np.array_equal(pout.cpu().numpy()[..., :co].transpose(0, 3, 1, 2), p_ref)
        assert np.array_equal(B._c32_to_nchw(nxt, co), p_ref)

    if mode == 0:
        check(*ops.conv_fwd_rows(gg, xc, wf, amax, mode=0, state=st, **kw))
    elif mode == 4:
        B.spec_pairs(st, False, amax, eo,
                     lambda m, outs: ops.conv_fwd_rows(gg, xc, wf, amax, mode=m, state=st, outs=outs, **kw), check)
    else:
        ops.conv_fwd_rows(gg, xc, wf, amax, mode=1, **kw)
        check(*ops.conv_fwd_rows(gg, xc, wf, amax, mode=2, **kw))


def run_dgrad(T, n, ci, h, co, pool, mode, form, seed, pooled_plan=False):
    """The input gradient of the layer ci -> co in `mode` against rowconv_band_cases.dgrad_ref, bit
    for bit: the NHWC16 gradient, its C32 copy and its P16 copy (always asked for and checked).
    Returns False if the fused launch was refused because its grid is not resident at once."""
    from niti_amd import ops
    from niti_amd._lib import NitiError
    dy, w, px, py, want = B.dgrad_ref(n, ci, h, co, pool, seed)
    gg = ops.geom(n, ci, h, h, co, 3, pad=1)
    assert ops.conv_rows_plan(gg, dgrad=True, pooled=pooled_plan) == form
    nhwc = lambda a: ops.nchw_to_nhwc16(B._dev(T, a))  # noqa: E731
    dyc = ops.nhwc16_to_c32(nhwc(dy), co)
    wft = ops.weights_to_wf(ops.oihw_to_ohwi16(B._dev(T, w)), ci, transpose=True)
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
        assert np.array_equal(B._c32_to_nchw(dxc, ci), want)
        assert p16 is not None and p16.numel() == dx.numel()
        assert np.array_equal(p16.cpu().numpy(), ops.nhwc16_to_p16(dx).cpu().numpy())

    if mode == 0:
        try:
            res = launch(0)
        except NitiError as e:  # a grid barrier needs the grid resident: more tiles than compute units
            assert e.code == 2 and form[3] > T.cuda.get_device_properties(0).multi_processor_count, (e, form)
            return False
        check(*res)
    elif mode == 2:
        amax.zero_()
        launch(1)
        check(*launch(2))
    else:
        B.spec_pairs(st, True, amax, None, launch, check)
    return True
