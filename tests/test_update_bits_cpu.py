"""The update-bits rule as the tests restate it (tests/update_bits_cases.py), without a GPU: the
bits == 2 form against the oracle's own weight-gradient rule, the schedule helper, and that the
op-level GPU cases' inputs are not degenerate (checked on the reference alone)."""
import numpy as np
import pytest

import update_bits_cases as UB

import niti_oracle as O


@pytest.mark.parametrize("bw", sorted(UB.BW_CONVS))
def test_bits_2_is_the_reference_rule(bw):
    g, x, dy, w = UB.bw_conv(bw)
    dw, ref_bw, acc, st = O.conv_wgrad(g, x, dy)
    assert st.overflow == 0 and ref_bw == bw == O.range_estimate(acc)
    want = O.sgd_update(w, dw).reshape(w.shape)
    got, kept = UB.apply_update(w, acc, 2)
    assert np.array_equal(kept, dw) and np.array_equal(got, want)
    if bw == 0:
        assert not dw.any() and np.array_equal(got, w)
    else:
        assert dw.any()
    if bw == 1:
        # the shift -1 through the reference's PSTO: every nonzero element becomes +-1, which is
        # not the gradient applied as it is (the extension's form for a negative shift)
        assert np.abs(acc).max() == 2
        assert np.array_equal(dw, np.sign(acc).astype(np.int8))
        assert not np.array_equal(dw, UB.clip127(acc))
        assert not np.array_equal(UB.apply_update(w, acc, 3)[1], dw)


def test_extension_classes():
    """bits != 2: PSTO for a shift >= 0, the clipped gradient below, zero at bw == 0, frozen at 0."""
    g, x, dy, w = UB.bw_conv(7)
    acc, _ = O.conv_wgrad_acc(g, x, dy)
    for bits in (1, 3, 4, 5, 6, 7):
        assert np.array_equal(UB.rule_gradient(acc, bits)[0], O.psto(acc, 7 - bits).astype(np.int8))
    g, x, dy, w = UB.bw_conv(2)
    acc, _ = O.conv_wgrad_acc(g, x, dy)
    for bits in (3, 5, 7):
        assert np.array_equal(UB.rule_gradient(acc, bits)[0], acc.astype(np.int8))
    g, x, dy, w = UB.bw_conv(0)
    acc, _ = O.conv_wgrad_acc(g, x, dy)
    assert acc.any()
    for bits in range(1, 8):
        assert not UB.rule_gradient(acc, bits)[0].any()
    g, x, dy, w = UB.bw_conv(20)
    got, kept = UB.apply_update(w, O.conv_wgrad_acc(g, x, dy)[0], 0)
    assert np.array_equal(got, w) and not kept.any()


def test_bits_schedule():
    from niti_amd import bits_schedule
    ms = (10, 20, 20, 35)
    assert [bits_schedule(e, 5, ms) for e in (0, 9, 10, 19, 20, 34, 35, 99)] == [5, 5, 4, 4, 2, 2, 1, 1]
    assert bits_schedule(0, 5, ()) == 5 and bits_schedule(3, 2, (1, 2, 3)) == 1
    assert bits_schedule(7, 7, [7]) == 6
    assert isinstance(bits_schedule(1, 5, [1]), int)


@pytest.mark.parametrize("name", list(UB.SHAPES))
def test_op_inputs_are_not_degenerate(name):
    for bits in UB.BITS:
        for shift, bw in UB.classes_of(bits):
            acc, w = UB.inputs(name, bw)
            assert O.range_estimate(acc) == bw
            if bw == 0:
                assert acc.any()  # a nonzero gradient whose range gives the zero class
                continue
            w_b, g_b = UB.apply_update(w, acc, bits)
            if bits > 0:
                assert g_b.any(), (bits, shift)
            if bits == 7:
                moved = w_b.astype(np.int32)
                assert (np.abs(moved) == 127).any() and (np.abs(moved) < 127).any()
                raw = w.astype(np.int32) - g_b.astype(np.int32)
                assert (np.abs(raw) > 127).any(), "no element clips"
            if bits != 2:
                assert not np.array_equal(w_b, UB.apply_update(w, acc, 2)[0]), (bits, shift)
            if bits > 2 and shift == -1:
                assert bw < bits and np.array_equal(g_b, UB.clip127(acc))  # the raw class


def test_three_job_case_reaches_three_classes():
    kinds = []
    for name, bits, shift in UB.THREE_JOBS:
        bw = UB.bw_of(bits, shift)
        g, _ = UB.rule_gradient(UB.inputs(name, bw)[0], bits)
        kinds.append("frozen" if g is None else "raw" if bw - bits < 0 else "psto")
    assert kinds == ["psto", "frozen", "raw"]


def test_slabs_sum_to_the_gradient():
    acc, _ = UB.inputs("slab", 9)
    a16 = UB.ohwi16(acc)
    s = UB.slabs_of(a16, 4, 1)
    assert s.shape == (4, a16.size) and s.dtype == np.int32
    assert not np.array_equal(s[0], a16.ravel())


def test_subw_layout_holds_every_tap_once():
    w = np.arange(1, 1 + 24 * 16 * 9, dtype=np.int64).reshape(24, 16, 3, 3)
    w8 = (w % 251 - 125).astype(np.int8)
    sub = UB.subw_of(w8, 1)
    assert sub.size == 16 * 9 * 32
    # class (0, 0) of a pad-1 3x3 kernel is the centre tap alone, first in the buffer
    first = sub[:16 * 32].reshape(16, 32)
    assert np.array_equal(first[:, :24], w8[:, :, 1, 1].T) and not first[:, 24:].any()
