"""conv_rows_plan(..., pooled=True) (niti_conv_rows_plan2): a 4x4 input gradient routed through the
previous layer's 2x2 pool runs one row per band where its grid at two rows per band would be 384 to
512 units (image groups x 2 bands x co blocks) -- host arithmetic alone.  Shapes are the LAYER's: its
input gradient reduces over c_out and has c_in / 32 co blocks."""
import ctypes as C

import pytest

import rowconv_band_cases as B


class _Ops:
    """ops.conv_rows_plan over geometries of the class the loaded library binds (see
    tests/test_rowconv_plan_cpu.py)."""

    def __init__(self, ops):
        self.lib = ops.L.lib()
        self.geom_t = self.lib.niti_geom_finalize.argtypes[0]._type_
        self.conv_rows_plan = ops.conv_rows_plan

    def geom(self, n, c_in, h, w, c_out, k, stride=1, pad=0):
        g = self.geom_t(n, c_in, h, w, c_out, k, k, stride, stride, pad, pad, pad, pad, 1, 1, 0, 0, 0, 0, 0)
        assert self.lib.niti_geom_finalize(C.byref(g)) == 0
        return g


@pytest.fixture(scope="module")
def ops():
    pytest.importorskip("torch")
    from niti_amd import ops
    o = _Ops(ops)
    o.lib.niti_diag_rowconv_rows1(-1)
    return o


def _plan(ops, n, ci, co, **kw):
    return ops.conv_rows_plan(ops.geom(n, ci, 4, 4, co, 3, pad=1), dgrad=True, **kw)


def test_rows1_vgg11_layer4(ops):
    """VGG-11's layer 4 (256 -> 512 at 4x4, behind a pool) at batch 256: 32 image groups x 8 co
    blocks, 512 units at R = 2 -> 1024 units, 256 workgroups at R = 1."""
    assert _plan(ops, 256, 256, 512, pooled=True) == (4, 1, 0, 256)
    assert _plan(ops, 256, 256, 512) == (4, 2, 0, 128)


# (n, layer c_in, units at R = 2): the rule's two edges, reached by the batch and by the co blocks
EDGES_IN = [(48, 1024, 384), (64, 1024, 512), (8, 32 * 192, 384), (8, 32 * 256, 512), (512, 96, 384)]
EDGES_OUT = [(40, 1024, 320), (65, 1024, 576), (8, 32 * 191, 382), (8, 32 * 257, 514), (504, 96, 378),
             (56, 32 * 27, 378), (72, 32 * 29, 522)]


def _units2(n, ci):
    return (n + 7) // 8 * 2 * (ci // 32)


def test_rows1_edges(ops):
    for n, ci, u2 in EDGES_IN:
        assert _units2(n, ci) == u2
        w, r, ks, wgs = _plan(ops, n, ci, 128, pooled=True)
        assert (w, r, ks) == (4, 1, 0) and wgs == 2 * u2 // 4
    for n, ci, u2 in EDGES_OUT:
        assert _units2(n, ci) == u2
        assert _plan(ops, n, ci, 128, pooled=True) == _plan(ops, n, ci, 128)
        assert _plan(ops, n, ci, 128, pooled=True)[:3] == (4, 2, 0)


def test_rows1_only_4x4_input_gradients(ops):
    """The same unit counts on other maps, and the forward of the same layer, keep their plan."""
    for h, n in ((2, 96), (8, 24), (16, 12)):  # 6 image groups x 2 bands (1 at 2x2) x 32 co blocks
        g = ops.geom(n, 1024, h, h, 128, 3, pad=1)
        assert ops.conv_rows_plan(g, dgrad=True, pooled=True) == ops.conv_rows_plan(g, dgrad=True)
    g = ops.geom(48, 128, 4, 4, 1024, 3, pad=1)
    assert ops.conv_rows_plan(g, pooled=True) == ops.conv_rows_plan(g) == (4, 2, 0, 96)


def test_rows1_switch(ops):
    try:
        ops.lib.niti_diag_rowconv_rows1(0)
        assert _plan(ops, 256, 256, 512, pooled=True) == (4, 2, 0, 128)
        ops.lib.niti_diag_rowconv_rows1(1)
        assert _plan(ops, 256, 256, 512, pooled=True) == (4, 1, 0, 256)
    finally:
        ops.lib.niti_diag_rowconv_rows1(-1)
    assert _plan(ops, 256, 256, 512, pooled=True) == (4, 1, 0, 256)


def test_unpooled_is_the_old_entry(ops):
    """pooled=False gives niti_conv_rows_plan's answer on every shape, and that entry's answers over
    the band cases are what they were."""
    shapes = [(n, ci, 4, 128) for n, ci, _ in EDGES_IN + EDGES_OUT]
    shapes += [(n, ci, h, co) for n, ci, h, co, _ in B.DGRAD_LARGE.values()]
    shapes += [(n, 32, h, 128) for n in B.SMALL_N for h in B.SMALL_H]
    shapes += [(256, ci, h, co) for (ci, co, h), _ in B.VGG11_B256]
    for n, ci, h, co in shapes:
        g = ops.geom(n, ci, h, h, co, 3, pad=1)
        assert ops.conv_rows_plan(g, dgrad=True, pooled=False) == ops.conv_rows_plan(g, dgrad=True)
        assert ops.conv_rows_plan(g, pooled=False) == ops.conv_rows_plan(g)
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
    for (ci, co, h), form in B.VGG11_B256:
        assert ops.conv_rows_plan(ops.geom(256, ci, h, h, co, 3, pad=1))[:3] == form
