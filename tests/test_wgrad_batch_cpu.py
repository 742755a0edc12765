"""Host side of the batched P16 weight gradient: the schedule and its workspace need no device."""
import ctypes as C

import pytest


@pytest.fixture(scope="module")
def L():
    import niti_amd._lib as L
    return L


def _jobs(L, shapes):
    lib = L.lib()
    # the structure classes the loaded library binds (a test that reloads the module leaves new ones)
    job_t = lib.niti_conv_wgrad_p16_many_workspace.argtypes[0]._type_
    geom_t = lib.niti_geom_finalize.argtypes[0]._type_
    arr = (job_t * len(shapes))()
    for j, (n, ci, h, co) in enumerate(shapes):
        g = geom_t(n, ci, h, h, co, 3, 3, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0)
        assert lib.niti_geom_finalize(C.byref(g)) == 0
        arr[j].g = g
        arr[j].x_p16 = arr[j].dy_p16 = arr[j].acc = 4096  # (never dereferenced: sizes only)
    return arr


def test_wgrad_p16_many_workspace(L):
    lib = L.lib()
    shapes = [(16, 32, 2, 32), (4, 64, 8, 32)]
    nb = C.c_size_t()
    assert lib.niti_conv_wgrad_p16_many_workspace(_jobs(L, shapes), 2, 2, 2, C.byref(nb)) == 0
    # the table's 4 KiB and each job's room for 8 slabs (a slab: the int32 tile rows rounded up to an
    # odd number of 4 KiB pages)
    slab = lambda co, ci: (-(-co * 9 * ci * 4 // 4096) | 1) * 4096  # noqa: E731
    assert nb.value == 4096 + 8 * slab(32, 32) + 8 * slab(32, 64)
    # more items than one page of table: the slabs move behind it
    big = C.c_size_t()
    assert lib.niti_conv_wgrad_p16_many_workspace(_jobs(L, [(256, 256, 8, 256)] * 2), 2, 256, 8, C.byref(big)) == 0
    assert big.value > 16 * slab(256, 256) + 4096


def test_wgrad_p16_many_rejects(L):
    lib = L.lib()
    nb = C.c_size_t()
    ok = _jobs(L, [(16, 32, 2, 32)])
    assert lib.niti_conv_wgrad_p16_many_workspace(ok, 0, 2, 2, C.byref(nb)) == 5   # no job
    assert lib.niti_conv_wgrad_p16_many_workspace(ok, 1, 0, 2, C.byref(nb)) == 5   # no workgroup
    assert lib.niti_conv_wgrad_p16_many_workspace(ok, 1, 2, 0, C.byref(nb)) == 5   # no item size
    assert lib.niti_conv_wgrad_p16_many_workspace(ok, 17, 2, 2, C.byref(nb)) == 5  # more than 16 jobs
    bad = _jobs(L, [(4, 16, 8, 32)])  # Cip 16: not a whole 32-channel tile
    assert lib.niti_conv_wgrad_p16_many_workspace(bad, 1, 2, 2, C.byref(nb)) != 0
    lib.niti_diag_wgrad_batch(1)  # host-side setter: no device call
