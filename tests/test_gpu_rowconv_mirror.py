"""The row kernels' two-band forms (csrc/niti_rowconv.hip, MIRROR: W == 2 R -- the bottom band's rows
loaded and accumulated bottom-up with the ky = 0 / ky = 2 weight fragments swapped, so the padding
row is left out of every band alike) and the one-row-per-band form of a pooled 4x4 input gradient
(<4,1>): each against the oracle bit for bit in the fused, two-launch and speculative modes, each
asserting through conv_rows_plan that the shape runs the form it is here for.

On a device with fewer compute units than a launch has workgroups the library refuses the fused
mode; only that mode of a case is then skipped (no case here has more than 256 workgroups)."""
import pytest

import rowconv_mirror_cases as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def T():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import niti_amd  # noqa: F401
    return torch


def _ran(ran, mode):
    if not ran:
        assert mode == 0
        pytest.skip("fused launch not resident on this device")


@pytest.mark.parametrize("mode", [0, 2, 4])
@pytest.mark.parametrize("case", sorted(M.FWD))
def test_mirror_fwd_ties(T, case, mode):
    M.run_fwd(T, case, mode)


@pytest.mark.parametrize("which", M.ROWS)
@pytest.mark.parametrize("case", sorted(M.FWD))
def test_mirror_fwd_one_row(T, case, which):
    """One image row of 127s -- the last row of the top band, the first of the bottom band, the
    image's last -- in a zero tensor, in the three modes."""
    for mode in (0, 2, 4):
        M.run_fwd(T, case, mode, which)


@pytest.mark.parametrize("mode", [0, 2, 4])
@pytest.mark.parametrize("case", sorted(M.DGRAD))
def test_mirror_dgrad(T, case, mode):
    """The channel-swapped layers' input gradients with the relu mask: <4,2,true> (its P16 copy by
    p16_pair_store) and <8,4,true>."""
    n, ci, h, co, form = M.DGRAD[case]
    _ran(M.run_dgrad(T, n, ci, h, co, False, mode, form, seed=1400), mode)


@pytest.mark.parametrize("mode", [0, 2, 4])
@pytest.mark.parametrize("case", sorted(M.ROWS1))
def test_rows1_dgrad_pooled(T, case, mode):
    """A 4x4 input gradient through the pool at one row per band: gradient, C32 and P16 copies."""
    n, ci, co, u2, wgs = M.ROWS1[case]
    assert (n + 7) // 8 * 2 * (ci // 32) == u2
    _ran(M.run_dgrad(T, n, ci, 4, co, True, mode, (4, 1, 0, wgs), seed=1900, pooled_plan=True), mode)


@pytest.mark.parametrize("mode", [0, 2, 4])
def test_rows1_switch_off(T, mode):
    """niti_diag_rowconv_rows1(0): the same launch at two rows per band, the same results."""
    from niti_amd import ops
    n, ci, co, u2, _ = M.ROWS1["n48_unc"]
    try:
        ops.L.lib().niti_diag_rowconv_rows1(0)
        _ran(M.run_dgrad(T, n, ci, 4, co, True, mode, (4, 2, 0, u2 // 4), seed=1900, pooled_plan=True), mode)
    finally:
        ops.L.lib().niti_diag_rowconv_rows1(-1)
