"""niti_sum_pool_wide bit for bit against numpy's int32 sums and their max, and against niti_sum_pool.

Shapes (n, hw, cp): one chunk of one pixel; a chunk count that is no power of two with fewer pixels than
pixel lanes; more pixels than lanes of a two-chunk group; one chunk over many pixels (every lane, four
passes); five chunks (80 channels); a pixel count that is no multiple of the lanes at extents the oracle's
conv checks do not reach (numpy only)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 16), (3, 4, 48), (2, 49, 32), (2, 1024, 16), (4, 256, 80), (2, 3000, 16)]
CLASSES = ["random", "max", "min", "zero", "one_pixel"]


@pytest.fixture(scope="module")
def T():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import niti_amd  # noqa: F401
    return torch


def _input(shape, cls):
    n, hw, cp = shape
    rng = np.random.default_rng(100 + 7 * SHAPES.index(shape) + CLASSES.index(cls))
    if cls == "random":
        return rng.integers(-128, 128, (n, hw, 1, cp)).astype(np.int8)
    if cls == "max":
        return np.full((n, hw, 1, cp), 127, np.int8)
    if cls == "min":  # the largest |sum|
        return np.full((n, hw, 1, cp), -128, np.int8)
    x = np.zeros((n, hw, 1, cp), np.int8)
    if cls == "one_pixel":  # the last image's last pixel, last chunk
        x[n - 1, hw - 1, 0, cp - 16:] = rng.integers(1, 128, 16).astype(np.int8) * np.where(np.arange(16) % 2, 1, -1).astype(np.int8)
    return x


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_sums_and_range(T, shape, cls):
    from niti_amd import ops
    x = _input(shape, cls)
    want = x.astype(np.int32).sum(axis=(1, 2))
    wmax = int(np.abs(want.astype(np.int64)).max())
    xd = T.from_numpy(x).cuda()
    amax = ops.new_range()
    acc = ops.sum_pool_wide(xd, amax)
    T.cuda.synchronize()
    assert np.array_equal(acc.cpu().numpy(), want)
    assert int(amax.max().item()) == wmax
    # amax is MAXed into, not stored over: a larger value stays, a smaller one is raised
    for pre in (wmax + 5, max(wmax - 1, 0)):
        amax = ops.new_range()
        amax.view(-1)[0] = pre
        ops.sum_pool_wide(xd, amax)
        T.cuda.synchronize()
        assert int(amax.max().item()) == max(pre, wmax), pre
    if shape != (2, 3000, 16):  # (nothing pins niti_sum_pool at such extents: numpy alone there)
        amax2 = ops.new_range()
        acc2 = ops.sum_pool(xd, amax2)
        T.cuda.synchronize()
        assert T.equal(acc, acc2) and int(amax2.max().item()) == wmax


def test_argument_errors_launch_nothing(T):
    import ctypes as C

    from niti_amd import _lib as L
    x = T.zeros((2, 4, 1, 16), dtype=T.int8, device="cuda")
    acc = T.full((2, 16), 77, dtype=T.int32, device="cuda")
    lib = L.lib()
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    too_many = (2 ** 31 + 253) // 254  # the smallest hw with hw * 254 >= 2^31 (never a launch: x holds 4 pixels)
    assert too_many * 254 >= 2 ** 31 > (too_many - 1) * 254
    bad = [(None, 2, 4, 16, p(acc)), (p(x), 2, 4, 16, None), (p(x), 0, 4, 16, p(acc)), (p(x), 2, 0, 16, p(acc)),
           (p(x), 2, 4, 0, p(acc)), (p(x), 2, 4, 24, p(acc)), (p(x), 2, too_many, 16, p(acc)), (p(x), -1, 4, 16, p(acc))]
    for xx, n, hw, cp, aa in bad:
        assert lib.niti_sum_pool_wide(xx, n, hw, cp, aa, None, None) == L.INVALID_VALUE, (n, hw, cp)
    T.cuda.synchronize()
    assert int((acc != 77).sum().item()) == 0
    assert lib.niti_sum_pool_wide(p(x), 2, 4, 16, p(acc), None, None) == 0  # (no range asked for)
    T.cuda.synchronize()
    assert int(acc.abs().sum().item()) == 0
