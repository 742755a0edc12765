"""The case tables of tests/fused_requant_cases.py reach what the GPU tests
(tests/test_gpu_fused_requant.py) rely on -- conditions on the inputs, checked against the CPU
references alone."""
import numpy as np
import pytest

import fused_requant_cases as F
from update_op_cases import O


def _group_accs():
    """(group, pin, clean accumulators) of every small requantise case."""
    for _, pin in F.PINS:
        for shape in F.PF_SHAPES:
            yield "A", pin, F.pf_case(shape, pin, False)["acc"]
        for n, h, w, ldc, _ in F.PB_SHAPES:
            yield "B", pin, F.pb_case(n, h, w, ldc, pin, False)["acc"]
        for rows, ldc in F.P16_SHAPES:
            yield "C", pin, F.p16_case(rows, ldc, pin)["acc"]
        for n, w, ldc in F.P16B_SHAPES:
            yield "D", pin, F.pb_case(n, w, w, ldc, pin, True)["acc"]
        for shape in F.ZC_SHAPES:
            yield "E", pin, F.zc_case(shape, 0, pin)["acc"]
        for shape in F.P3_SHAPES:
            yield "F", pin, F.p3_case(shape, pin, True)["acc"]


def test_every_group_sees_the_three_shift_branches():
    """raw at bw 7, shift 1 at bw 8, PSTO at bw 9 / 16 / 31; the accumulators fill the pinned range
    exactly, so the oracle's own range estimate picks the same rule, and outside the raw branch
    they hold both exact half-way values of PSTO's rounding."""
    assert [F.rule(pin)[0] for _, pin in F.PINS] == [name for name, _ in F.PINS]
    assert [O.range_estimate(np.array([pin], np.int32)) for _, pin in F.PINS] == [7, 8, 9, 16, 31]
    seen = {}
    for group, pin, acc in _group_accs():
        assert int(np.abs(acc.astype(np.int64)).max()) == pin, (group, pin)
        q, inc = O.requant_fwd(acc)
        assert inc == F.rule(pin)[2] and np.array_equal(q, F.requant_ref(acc, pin)), (group, pin)
        branch, s, _ = F.rule(pin)
        if branch != "raw" and acc.size >= 64:
            low = acc.astype(np.int64) & ((1 << s) - 1)
            assert ((low == 1 << (s - 1)) & (acc > 0)).any() and ((low == 1 << (s - 1)) & (acc < 0)).any(), (group, pin)
        seen.setdefault(group, set()).add(branch)
    assert seen == {g: {"raw", "one", "psto"} for g in "ABCDEF"}
    assert (F.requant_ref(np.array([128], np.int32), 128) == -128).all()   # 128 wraps in the raw cast
    inc = F.rule(F.WRAP["pin"])[2]
    assert inc == 9 and F.WRAP["exp_in"] + F.WRAP["wscale"] + inc == 134
    assert F.exp_ref(F.WRAP["pin"], F.WRAP["exp_in"], F.WRAP["wscale"]) == -122


def test_big_cases_take_a_second_ragged_pass():
    n, h, w, ldc = F.PF_BIG
    assert 0 < n * (h // 2) * (w // 2) * (ldc // 4) - 2048 * 256 * 4 < 2048 * 256
    n, h, w, ldc, _ = F.PB_BIG
    assert 0 < n * (h // 2) * (w // 2) * (ldc // 4) - 2048 * 256 * 4 < 2048 * 256
    rows, ldc = F.P16_BIG
    assert rows % 16 == 0 and 0 < rows // 16 * (ldc // 4) * 4 - 2048 * 256 < 2048 * 256
    assert F.rule(F.BIG_PIN)[0] == "psto"


def test_pool_backward_inputs_hold_ties_equal_and_nonpositive_windows():
    geos = [(n, h, w, ldc) for n, h, w, ldc, _ in F.PB_SHAPES] + [(n, w, w, ldc) for n, w, ldc in F.P16B_SHAPES]
    for n, h, w, ldc in geos:
        for relu in (False, True):
            x, y = F.pool_x(n, h, w, ldc, relu)
            assert x.min() == (0 if relu else -2) and x.max() == 5
            kinds = F.window_kinds(x, y)
            assert kinds["tie"] >= ldc and kinds["equal"] >= ldc and kinds["nonpos"] >= ldc, (n, h, w, ldc, relu, kinds)
    # the requantised dy spans the int8 range where the pinned range allows, and some of it is dropped
    c = F.pb_case(2, 6, 10, 96, 128, True)
    assert c["q"].min() == -128 and c["q"].max() == 127
    assert ((c["dx"] == 0) & (np.repeat(np.repeat(c["q"].reshape(c["y"].shape), 2, 1), 2, 2) != 0)).any()
    # the 2x2 pool reference against plain numpy
    x, y = F.pool_x(2, 6, 10, 96, False)
    assert np.array_equal(y, x.reshape(2, 3, 2, 5, 2, 96).max(axis=(2, 4)))


def test_layout_restatements():
    x = np.arange(48 * 32, dtype=np.int64).reshape(48, 32)
    p = F.p16_of(x)
    assert p.shape == (3, 32, 16) and p[2, 7, 5] == x[2 * 16 + 5, 7]
    d = np.arange(2 * 4 * 6 * 96, dtype=np.int64).reshape(2, 4, 6, 96)
    c = F.c32_of(d)
    assert c.shape == (2, 3, 4, 6, 32) and c[1, 2, 3, 5, 9] == d[1, 3, 5, 2 * 32 + 9]


def test_zero_cls_poison_covers_every_parity_class():
    for shape in F.ZC_SHAPES:
        n, h, w, ldc = shape
        cls_of = F.zc_classes(n, h, w).reshape(-1)
        assert set(np.unique(cls_of)) == {0, 1, 2, 3}
        poisoned = {k: set() for k in range(4)}
        for cls in F.ZC_MASKS:
            assert 0 < cls < 15
            c = F.zc_case(shape, cls, 200)
            assert np.array_equal(c["skip"], ((cls >> cls_of) & 1).astype(bool))
            assert c["skip"].any() and not c["skip"].all()
            assert not c["out"][c["skip"]].any() and c["out"][~c["skip"]].any()
            for k in range(4):
                if (cls >> k) & 1:
                    poisoned[k] |= set(np.unique(c["acc"][cls_of == k]).tolist())
            # a kernel that read the poison would not write 0: both values requantise to non-zero
            for _, pin in F.PINS:
                assert F.requant_ref(np.array(F.POISON, np.int32), pin)[0] != 0
        assert all(v == {0x7fffffff, -2**31} for v in poisoned.values()), poisoned
        assert abs(int(F.POISON[0])) > max(pin for _, pin in F.PINS[:-1])


def test_pool3_cases_reach_every_position_and_zero_windows():
    positions, zero_at = set(), set()
    for shape in F.P3_SHAPES:
        n, h, w, ldc = shape
        oh, ow = F.p3_out(h), F.p3_out(w)
        for _, pin in F.PINS:
            c = F.p3_case(shape, pin, True)
            assert c["pre"].min() == 0 and c["arg"].min() >= 0 and c["out"].shape == (n, oh, ow, ldc)
            positions |= set(np.unique(c["arg"]).tolist())
            for b, oy, ox, _ in np.argwhere(c["out"] == 0):
                zero_at.add(F.window_place(oy, ox, oh, ow))
            # an all-zero window keeps its first in-image position
            z = c["out"] == 0
            oy_i, ox_i = np.nonzero(z)[1], np.nonzero(z)[2]
            first = np.where(oy_i > 0, 0, 3) + np.where(ox_i > 0, 0, 1)
            assert np.array_equal(c["arg"][z], first)
            if min(h, w) >= 3:   # the oracle's pool has the same windows there
                assert np.array_equal(c["out"], F.nhwc(O.maxpool(F.nchw(c["pre"]), 3, 2, 1)))
            assert not np.array_equal(F.p3_case(shape, pin, False)["pre"], c["pre"])
    assert positions == set(range(9))
    assert zero_at == {"corner", "edge", "interior"}
    # odd sides: the last window's right column / bottom row lies outside the image
    assert any(s[1] % 2 and s[1] > 1 for s in F.P3_SHAPES) and any(s[2] % 2 and s[2] > 1 for s in F.P3_SHAPES)
    assert F.p3_out(17) == 9   # three strips of RQ3_ROWS = 4 pooled rows, one row in the last
    assert set(F.P3_CHILD_SHAPES) <= set(F.P3_SHAPES)


def test_first_max_reference_on_a_hand_case():
    x = np.array([[1, 5, 5], [5, 0, 2], [7, 7, -3]], np.int8).reshape(1, 3, 3, 1)
    y, arg = F.pool_first_max(x, 3, 2, 1, 2, 2)
    # windows: rows -1..1 x cols -1..1 | cols 1..3; rows 1..3 x cols -1..1 | cols 1..3
    assert y.reshape(-1).tolist() == [5, 5, 7, 7]
    assert arg.reshape(-1).tolist() == [5, 3, 4, 3]


def test_stem_pool_pair_references():
    wrapped = degenerate = 0
    for n, h, w in F.PP_MAPS:
        for cp in F.PP_CPS:
            for k, s, p in F.PP_POOLS + [F.PP_GENERIC_POOL]:
                for relu in (False, True):
                    c = F.pp_case(n, h, w, cp, k, s, p, relu)
                    assert c["dy"].min() == -128 and c["dy"].max() == 127
                    assert {0, 1, 127} <= set(np.unique(c["pooled"]).tolist()) and c["pooled"].min() < 0
                    # the oracle's pool gradient routes where arg says, on every map
                    assert np.array_equal(F.oracle_pool_grad(c["x"], c["y"], c["dy"], k, s, p), c["sums"].astype(np.int8))
                    if min(h, w) >= k:   # whole windows: arg is the first element equal to the window max
                        y, arg = F.pool_first_max(c["x"], k, s, p, *c["y"].shape[1:3])
                        assert np.array_equal(y, c["y"]) and np.array_equal(arg, c["arg"])
                        if (k, s, p) != (3, 2, 1) or (h % 2 and w % 2):
                            assert np.array_equal(F.nhwc(O.maxpool(F.nchw(c["x"]), k, s, p)), c["y"])
                    else:   # a map smaller than the kernel: the forward's window is clipped, the gradient's is not
                        degenerate += int((c["arg"] != F.pool_first_max(c["x"], k, s, p, *c["y"].shape[1:3])[1]).sum())
                    if (k, s, p) == (3, 2, 1):
                        wrapped += int((c["sums"] != c["sums"].astype(np.int8)).sum())
                        wrapped_pooled = int((c["sums_pooled"] != c["sums_pooled"].astype(np.int8)).sum())
                        if (n, h, w) in F.PP_WRAP_MAPS:
                            assert (c["sums"][0, 3, 3] == 508).all() and wrapped_pooled >= 1
    assert wrapped >= 1 and degenerate >= 1
    # F's relu cases that G's arg is compared with exist, and G's maps include them
    for n, h, w, ldc in F.PP_SHARED_WITH_F:
        assert (n, h, w, ldc) in F.P3_SHAPES and (n, h, w) in F.PP_MAPS and ldc in F.PP_CPS


@pytest.mark.parametrize("w,n", [(2, 4), (2, 12), (4, 1), (4, 3), (8, 1), (8, 3), (16, 1), (16, 2)])
def test_p16_pool_backward_shapes_fit_the_run(w, n):
    """rows are a multiple of the kernel's group (4 pooled pixels, 8 at W = 16) and dx pixels of 16."""
    assert any((n, w) == s[:2] for s in F.P16B_SHAPES)
    rows = n * (w // 2) ** 2
    assert rows % (8 if w == 16 else 4) == 0 and (n * w * w) % 16 == 0
