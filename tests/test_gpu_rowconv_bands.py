"""The row kernels' K loop (csrc/niti_rowconv.hip: rowconv_compute, rowconv_compute_ks) on the forms
the small-batch tests of test_gpu_rowconv.py never reach: 4 and 8 rows per band with bands that are
the image's top, its bottom, both or neither (the loop skips the zero padding row's shifts and MFMAs
per band), the UNC loop, and the K-split form at 2 and 4 chunks per wave -- each against the oracle
bit for bit (output, exponent, pooled output and C32 copy; for input gradients the NHWC16, C32 and
P16 copies), each asserting through conv_rows_plan that the shape runs the form it is here for.

The input gradient's pool route is given as the pool's input and output (the operands
niti_conv_dgrad_rows takes); the recorded route is an operand of the model step only."""
import pytest

import rowconv_band_cases as B

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def T():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import niti_amd  # noqa: F401
    return torch


@pytest.mark.parametrize("mode", [0, 2, 4])
@pytest.mark.parametrize("case", sorted(B.FWD_LARGE))
def test_bands_fwd(T, case, mode):
    n, ci, h, co, pool, form = B.FWD_LARGE[case]
    B.run_fwd(T, n, ci, h, co, pool, mode, form, seed=1200)


@pytest.mark.parametrize("mode", [0, 2, 4])
@pytest.mark.parametrize("h", B.SMALL_H)
def test_bands_fwd_ragged_unc(T, h, mode):
    """128 -> 32 channels at 3 and 5 images: ragged image groups on the UNC loop at R = 2."""
    for n in B.SMALL_N:
        B.run_fwd(T, n, 128, h, 32, False, mode, B.small_plan(n, h), seed=1300 + n)


@pytest.mark.parametrize("mode", [0, 2])
@pytest.mark.parametrize("pool", [False, True], ids=["relu_mask", "pool"])
@pytest.mark.parametrize("case", sorted(B.DGRAD_LARGE))
def test_bands_dgrad(T, case, pool, mode):
    n, ci, h, co, form = B.DGRAD_LARGE[case]
    ran = B.run_dgrad(T, n, ci, h, co, pool, mode, form, seed=1400)
    # only the 384-tile launch may be refused the fused mode (a grid barrier needs the grid resident)
    assert ran or case == "16x16_r4_n64"


@pytest.mark.parametrize("mode", [0, 2, 4])
@pytest.mark.parametrize("h", B.SMALL_H)
def test_bands_dgrad_ragged_unc(T, h, mode):
    """The layer 32 -> 128 (the kernel reduces over 128 channels) at 3 images with the relu mask and
    at 5 through the pool."""
    for n in B.SMALL_N:
        assert B.run_dgrad(T, n, 32, h, 128, n == 5, mode, B.small_plan(n, h), seed=1500 + n)


@pytest.mark.parametrize("mode", [0, 2])
@pytest.mark.parametrize("n,k,ks", B.KS_CASES)
def test_bands_ks(T, n, k, ks, mode):
    """The K-split form, k -> 32 channels at 2x2, forward and input gradient."""
    form = (2, 2, ks, (n + 15) // 16)
    B.run_fwd(T, n, k, 2, 32, True, mode, form, seed=1600 + k)
    assert B.run_dgrad(T, n, 32, 2, k, False, mode, form, seed=1700 + k)
