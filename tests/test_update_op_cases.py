"""The case tables of tests/update_op_cases.py reach the branches the GPU tests
(tests/test_gpu_update_ops.py) rely on -- checked on the CPU references alone."""
import numpy as np
import pytest

import update_op_cases as U


def test_residual_table_reaches_every_branch():
    """Each case takes the branch, exponent step and low-operand shift its table row states, and the
    table as a whole covers raw / shift 1 / PSTO, r >= 8 (min(r, 7)) and r >= 31 (residual_z)."""
    seen, rs = set(), set()
    for n, cases in ((U.RES_N, U.RES_CASES), (U.RES_N_BIG, U.RES_BIG_CASES)):
        for amp, gap, e_hi, branch, inc, r in cases:
            for swap in (False, True):
                ref = U.res_reference(amp, gap, e_hi, swap, n)
                assert ref["branch"] == branch, (amp, gap, swap, ref["branch"], ref["bw"])
                assert ref["ez"] == e_hi - min(gap, 23)
                assert ref["exp_out"] == ref["ez"] + inc
                assert r == gap - min(gap, 23)
                a, _, b, _, mask = U.res_inputs(amp, gap, e_hi, swap, n)
                assert a.size == n and a[0] == b[0] == amp and a[1] == b[1] == -amp
                assert set(np.unique(mask)) == {-128, 0, 1, 127}
                if amp == 127:
                    assert (a == -128).any() and (b == -128).any()
                if n == U.RES_N:
                    seen.add(branch)
                    rs.add(r)
    assert seen == {"raw", "one", "psto"}
    assert any(8 <= r < 31 for r in rs) and any(r >= 31 for r in rs) and max(rs) == 232
    # the rows the issue spells out
    by = {(c[0], c[1]): c for c in U.RES_CASES}
    assert U.res_reference(127, 0, -5, False)["range"] == 254 and U.res_reference(127, 0, -5, False)["exp_out"] == -3
    assert [U.res_reference(a, 0, -5, False)["bw"] for a in (1, 40, 64)] == [1, 7, 7]
    assert (U.res_reference(64, 0, -5, False)["out"] == -128).any()   # 128 wraps in the raw cast
    for gap in (127, 200, 255):
        ref = U.res_reference(127, gap, 127, True)
        assert by[(127, gap)][2] == 127 and ref["ez"] == 104 and ref["exp_out"] == 127
    assert U.RES_N_BIG // 16 == 2048 * 256 + 300 and len(U.RES_BIG_CASES) == 2


def test_residual_table_tells_a_wrapped_shift():
    """A low-operand shift taken mod 32 (a 32-bit shift without residual_z's r >= 31 arm) changes z at
    exactly the two gaps added for it; at the other r >= 31 gaps it would go unnoticed."""
    differs = []
    for amp, gap, e_hi, _, _, r in U.RES_CASES:
        a, ea, b, eb, _ = U.res_inputs(amp, gap, e_hi, False)
        z = U.res_reference(amp, gap, e_hi, False)["z"]
        wrapped = a.astype(np.int32) * (1 << min(gap, 23)) + (b.astype(np.int32) >> (r & 31))
        if r >= 31 and not np.array_equal(wrapped, z):
            differs.append(gap)
    assert differs == [55, 87]


def test_requant_cases_reach_every_branch():
    for rows, ldc in U.RQ_SHAPES:
        seen = set()
        for name, pin in U.RQ_PINS:
            ref = U.rq_reference(rows, ldc, pin)
            assert ref["branch"] == name, (rows, ldc, pin)
            seen.add(ref["branch"])
        assert seen == {"raw", "one", "psto"}
    w = U.RQ_WRAP
    inc = U.rq_reference(*w["shape"], w["pin"])["inc"]
    assert inc == 9 and w["exp_in"] + w["wscale"] + inc == 134   # the int8 exponent wraps to -122
    assert (U.rq_reference(1, 16, 128)["out"] == -128).any()   # 128 wraps in the raw cast
    assert U.RQ_SHAPES[-1][0] * U.RQ_SHAPES[-1][1] // 4 == 4 * 2048 * 256 + 2048


@pytest.mark.parametrize("rule", U.SGD_RULES)
@pytest.mark.parametrize("layer", U.SGD_LAYERS, ids=lambda l: "x".join(map(str, l[:3])))
def test_sgd_random_cases_clip(layer, rule):
    """Every random-acc case has at least one cell with |w - g| > 127, -128 weights, zero pads."""
    co, ci, kk, with_wf = layer
    acc, w16 = U.sgd_inputs(co, ci, kk)
    assert not acc[..., ci:].any() and not w16[..., ci:].any()
    assert int(np.abs(acc.astype(np.int64)).max()) == U.SGD_RANDOM_TOP
    assert (w16 == -128).any()
    ref = U.sgd_reference(co, ci, kk, rule, with_wf)
    assert ref["clipped"] >= 1, (layer, rule)
    assert np.abs(ref["w"].astype(np.int32)).max() <= 127


def test_sgd_small_range_shifts():
    """The pinned ranges give bw 0 (twice), 1, 2, 3 and 31: shifts -2 .. 1 and the top shift."""
    bws = [U.O.range_estimate(U.sgd_inputs(12, 500, 1, pin)[0]) for pin in U.SGD_SMALL_MAX]
    assert bws == [0, 0, 1, 2, 3, 31]
    for co, ci, kk, _ in U.SGD_SMALL_LAYERS:
        for pin in U.SGD_SMALL_MAX:
            acc = U.sgd_inputs(co, ci, kk, pin)[0]
            assert int(np.abs(acc.astype(np.int64)).max()) == pin
    assert not U.sgd_reference(12, 500, 1, 2, False, 1)["g"].any()   # bw == 0: no gradient


@pytest.mark.parametrize("co,ci", [(l[0], l[1]) for l in U.SGD_LAYERS if l[3]])
def test_wf_index_maps_are_bijections(co, ci):
    size = U.wf_bytes(co, ci)
    assert size == (co // 32) * (ci // 32) * 9 * 1024 == co * ci * 9
    for idx in (U.wf_index(co, ci), U.wft_index(co, ci)):
        assert idx.shape == (co, 9, ci)
        assert np.array_equal(np.sort(idx.ravel()), np.arange(size))
    ref = U.sgd_reference(co, ci, 9, 2, True)
    # spot values of the stated layouts: w[o][k][i] at its WF byte, and at tap 8 - k transposed
    o, k, i = co - 1, 4, ci - 17
    w = ref["w"]
    assert ref["wf"][(((((o >> 5) * (ci // 32) + (i >> 5)) * 9 + k) * 2 + ((i >> 4) & 1)) * 32 + (o & 31)) * 16 +
                     (i & 15)] == w[o, 1, 1, i]
    assert ref["wft"][(((((i >> 5) * (co // 32) + (o >> 5)) * 9 + 4) * 2 + ((o >> 4) & 1)) * 32 + (i & 31)) * 16 +
                      (o & 15)] == w[o, 1, 1, i]
