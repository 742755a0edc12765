"""conv_rows_plan (niti_conv_rows_plan): which row-kernel instantiation a shape runs, by host
arithmetic alone -- the forms tests/test_gpu_rowconv_bands.py is built around, VGG-11's batch-256
layers, and the geometries conv_rows_ok refuses."""
import ctypes as C

import pytest

import rowconv_band_cases as B


class _Ops:
    """ops.conv_rows_plan / ops.conv_rows_ok over geometries of the class the loaded library binds
    (as the other CPU tests build them: tests/test_capi_cpu.py reloads niti_amd._lib, after which
    ops.geom's Geom is no longer the class the cached library's prototypes name)."""

    def __init__(self, ops):
        self.lib = ops.L.lib()
        self.geom_t = self.lib.niti_geom_finalize.argtypes[0]._type_
        self.conv_rows_plan = ops.conv_rows_plan
        self.conv_rows_ok = ops.conv_rows_ok

    def geom(self, n, c_in, h, w, c_out, k, stride=1, pad=0):
        g = self.geom_t(n, c_in, h, w, c_out, k, k, stride, stride, pad, pad, pad, pad, 1, 1, 0, 0, 0, 0, 0)
        assert self.lib.niti_geom_finalize(C.byref(g)) == 0
        return g


@pytest.fixture(scope="module")
def ops():
    pytest.importorskip("torch")
    from niti_amd import ops
    return _Ops(ops)


def test_plan_band_forms(ops):
    for n, ci, h, co, _, form in B.FWD_LARGE.values():
        assert ops.conv_rows_plan(ops.geom(n, ci, h, h, co, 3, pad=1)) == form
    for n, ci, h, co, form in B.DGRAD_LARGE.values():
        assert ops.conv_rows_plan(ops.geom(n, ci, h, h, co, 3, pad=1), dgrad=True) == form
    for n in B.SMALL_N:
        for h in B.SMALL_H:
            assert ops.conv_rows_plan(ops.geom(n, 128, h, h, 32, 3, pad=1)) == B.small_plan(n, h)
            assert ops.conv_rows_plan(ops.geom(n, 32, h, h, 128, 3, pad=1), dgrad=True) == B.small_plan(n, h)
    for n, k, ks in B.KS_CASES:
        form = (2, 2, ks, (n + 15) // 16)
        assert ops.conv_rows_plan(ops.geom(n, k, 2, 2, 32, 3, pad=1)) == form
        assert ops.conv_rows_plan(ops.geom(n, 32, 2, 2, k, 3, pad=1), dgrad=True) == form


def test_plan_rows_halve_below_768_units(ops):
    """R is halved while image groups x bands x co-blocks stay under 768: one image fewer than the
    <16,8> case's 64 still fills 32 groups; half of them does not."""
    assert ops.conv_rows_plan(ops.geom(63, 32, 16, 16, 384, 3, pad=1))[:2] == (16, 8)
    assert ops.conv_rows_plan(ops.geom(62, 32, 16, 16, 384, 3, pad=1))[:2] == (16, 4)
    assert ops.conv_rows_plan(ops.geom(16, 32, 16, 16, 384, 3, pad=1))[:2] == (16, 2)
    # the input gradient keeps at most 4 rows per band
    assert ops.conv_rows_plan(ops.geom(256, 384, 16, 16, 32, 3, pad=1), dgrad=True)[:2] == (16, 4)


def test_plan_vgg11_b256(ops):
    for (ci, co, h), form in B.VGG11_B256:
        assert ops.conv_rows_plan(ops.geom(256, ci, h, h, co, 3, pad=1))[:3] == form


def test_plan_row_segment_form(ops):
    w, r, ks, wgs = ops.conv_rows_plan(ops.geom(2, 64, 28, 28, 64, 3, pad=1))
    assert (w, ks) == (0, 0) and r in (2, 4) and wgs > 0


def test_plan_refuses_what_rows_ok_refuses(ops):
    for g in (ops.geom(4, 32, 6, 6, 32, 3, pad=1), ops.geom(4, 32, 8, 8, 32, 3, stride=2, pad=1),
              ops.geom(4, 32, 8, 8, 32, 5, pad=2), ops.geom(4, 32, 8, 8, 32, 3, pad=0)):
        assert not ops.conv_rows_ok(g)
        assert ops.conv_rows_plan(g) is None
        assert ops.conv_rows_plan(g, dgrad=True) is None
    g = ops.geom(4, 32, 8, 8, 32, 3, pad=1)
    assert ops.conv_rows_ok(g) and ops.conv_rows_plan(g) is not None
