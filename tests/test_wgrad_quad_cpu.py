"""Host side of the batched P16 weight gradient's quad items (conv_wgrad_p16_many_build, niti_wgrad.hip).

A quad item is up to four consecutive tiles of one unsplit 2x2 / 4x4-map job, one tile per wave, each
over the job's whole K range.  The schedule is read back through niti_conv_wgrad_p16_many_items (no
device call) and checked for coverage: every (job, tile, K group) exactly once, whatever the forms.
With the threshold at 0 the list must be the one the schedule had before quads existed, which
`_merged_schedule` below rebuilds from its rules: a job of kg K groups is cut max(1, (kg + t / 2) / t)
ways (whole images, at most 8 slabs at the op level), every (split, tile) is an item, and the items
go longest first (stable) into the list with the least K groups + 20 per item so far.
"""
import ctypes as C

import pytest

# (n, ci, h, co): tiles 1, 4, 5, 6, 4, 2 and K groups 1, 2, 8, 2, 4, 8 -- on both sides of a
# threshold of 4 and of 2; the last job is 8x8 maps, which never go quad
SHAPES = [(8, 32, 2, 32), (16, 64, 2, 64), (64, 32, 2, 160), (16, 64, 2, 96), (8, 64, 4, 60), (4, 64, 8, 32)]


@pytest.fixture(scope="module")
def L():
    import niti_amd._lib as L
    return L


def _jobs(L, shapes):
    lib = L.lib()
    job_t = lib.niti_conv_wgrad_p16_many_workspace.argtypes[0]._type_
    geom_t = lib.niti_geom_finalize.argtypes[0]._type_
    arr = (job_t * len(shapes))()
    for j, (n, ci, h, co) in enumerate(shapes):
        g = geom_t(n, ci, h, h, co, 3, 3, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0)
        assert lib.niti_geom_finalize(C.byref(g)) == 0
        arr[j].g = g
        arr[j].x_p16 = arr[j].dy_p16 = arr[j].acc = 4096  # (never dereferenced: the schedule only)
    return arr


def _schedule(L, shapes, blocks, t, quad):
    """[[(job, tile, tiles, slab, kb, ke, kpw, form), ...] per block] under threshold `quad`."""
    lib = L.lib()
    cap = 4096
    items = (C.c_int * (8 * cap))()
    starts = (C.c_int * (blocks + 1))()
    n = C.c_int()
    lib.niti_diag_wgrad_quad(quad)
    try:
        assert lib.niti_conv_wgrad_p16_many_items(_jobs(L, shapes), len(shapes), blocks, t, items, cap, starts,
                                                  blocks + 1, C.byref(n)) == 0
    finally:
        lib.niti_diag_wgrad_quad(-1)
    assert starts[0] == 0 and starts[blocks] == n.value
    rows = [tuple(items[8 * i:8 * i + 8]) for i in range(n.value)]
    return [rows[starts[b]:starts[b + 1]] for b in range(blocks)]


def _dims(shape):
    n, ci, h, co = shape
    pad = lambda c: -(-c // 32) * 32  # noqa: E731
    kpi = {8: 2, 16: 8}.get(h, 1)
    return n * h * h // 32, (pad(co) // 32) * (pad(ci) // 32), kpi


def _merged_schedule(shapes, blocks, t):
    items = []
    for j, shape in enumerate(shapes):
        kg, tiles, kpi = _dims(shape)
        rk = lambda v: -(-v // kpi) * kpi  # noqa: E731
        s = min(max(1, (kg + t // 2) // t), max(1, kg // kpi), 8)
        per = rk(-(-kg // s))
        s = -(-kg // per)
        for sp in range(s):
            kb, ke = sp * per, min(kg, sp * per + per)
            for tile in range(tiles):
                items.append((j, tile, 0, sp if s > 1 else -1, kb, ke, rk(-(-(ke - kb) // 4)), 0))
    order = sorted(range(len(items)), key=lambda i: -(items[i][5] - items[i][4]))  # (stable)
    load = [0] * blocks
    lists = [[] for _ in range(blocks)]
    for i in order:
        b = load.index(min(load))
        lists[b].append(items[i])
        load[b] += items[i][5] - items[i][4] + 20
    return lists


@pytest.mark.parametrize("blocks", [1, 2, 3])
@pytest.mark.parametrize("t", [2, 16])
def test_threshold_zero_is_the_merged_schedule(L, blocks, t):
    assert _schedule(L, SHAPES, blocks, t, 0) == _merged_schedule(SHAPES, blocks, t)


@pytest.mark.parametrize("blocks", [1, 2, 3])
@pytest.mark.parametrize("t,quad", [(16, 4), (16, 2), (16, 8), (2, 8), (4, 4)])
def test_quad_schedule_covers_every_k_group_once(L, blocks, t, quad):
    lists = _schedule(L, SHAPES, blocks, t, quad)
    merged = _merged_schedule(SHAPES, 1, t)[0]
    split = {j: any(it[0] == j and it[3] >= 0 for it in merged) for j in range(len(SHAPES))}
    seen = {}
    quads = {}
    for lst in lists:
        for job, tile, cnt, slab, kb, ke, kpw, form in lst:
            kg, tiles, _ = _dims(SHAPES[job])
            assert 0 <= kb < ke <= kg
            if form:
                # 1..4 consecutive tiles of one unsplit short-K job of small maps, its whole K range
                assert 1 <= cnt <= 4 and tile % 4 == 0 and tile + cnt <= tiles
                assert cnt == min(4, tiles - tile)
                assert slab == -1 and (kb, ke) == (0, kg) and kg <= quad
                assert not split[job] and SHAPES[job][2] <= 4
                quads[job] = quads.get(job, 0) + 1
            else:
                assert cnt == 0 and 4 * kpw >= ke - kb
            for tl in range(tile, tile + (cnt if form else 1)):
                for k in range(kb, ke):
                    seen[(job, tl, k)] = seen.get((job, tl, k), 0) + 1
    want = {(j, tl, k) for j, s in enumerate(SHAPES) for tl in range(_dims(s)[1]) for k in range(_dims(s)[0])}
    assert set(seen) == want and set(seen.values()) == {1}
    # exactly the unsplit 2x2 / 4x4 jobs at or under the threshold went quad, whole
    for j, s in enumerate(SHAPES):
        kg, tiles, _ = _dims(s)
        if not split[j] and s[2] <= 4 and kg <= quad:
            assert quads.get(j, 0) == -(-tiles // 4), j
        else:
            assert j not in quads, j
    # a quad replaces up to four items: the table cannot grow
    assert sum(len(lst) for lst in lists) <= len(merged)


def test_quad_forms_present(L):
    """The job list really has both sides: at threshold 4, item size 16, jobs 0, 1, 3 and 4 go quad
    (1 + 1 + 2 + 1 items; tiles 1, 4, 4 + 2, 4), job 2 (8 K groups) and the 8x8 job stay merged."""
    rows = [it for lst in _schedule(L, SHAPES, 2, 16, 4) for it in lst]
    assert sorted((it[0], it[1], it[2]) for it in rows if it[7]) == [(0, 0, 1), (1, 0, 4), (3, 0, 4), (3, 4, 2), (4, 0, 4)]
    assert sum(1 for it in rows if not it[7]) == 5 + 2


def test_quad_entries_reject(L):
    lib = L.lib()
    ok = _jobs(L, [(16, 32, 2, 32)])
    items = (C.c_int * 64)()
    starts = (C.c_int * 3)()
    n = C.c_int()
    f = lib.niti_conv_wgrad_p16_many_items
    assert f(ok, 1, 2, 2, items, 8, starts, 3, C.byref(n)) == 0 and n.value == 1
    assert f(ok, 1, 2, 2, None, 8, starts, 3, C.byref(n)) == 5    # no room for the items
    assert f(ok, 1, 2, 2, items, 8, None, 3, C.byref(n)) == 5     # ... for the starts
    assert f(ok, 1, 2, 2, items, 8, starts, 3, None) == 5         # ... for the count
    assert f(ok, 1, 2, 2, items, 0, starts, 3, C.byref(n)) == 5   # fewer items than the schedule has
    assert f(ok, 1, 2, 2, items, 8, starts, 2, C.byref(n)) == 5   # fewer than blocks + 1 starts
    assert f(ok, 1, 2, 2, items, -1, starts, 3, C.byref(n)) == 5
    assert f(ok, 0, 2, 2, items, 8, starts, 3, C.byref(n)) == 5   # no job
    assert f(ok, 1, 0, 2, items, 8, starts, 3, C.byref(n)) == 5   # no workgroup
    assert f(ok, 1, 2, 0, items, 8, starts, 3, C.byref(n)) == 5   # no item size
    assert f(None, 1, 2, 2, items, 8, starts, 3, C.byref(n)) == 5
    bad = _jobs(L, [(4, 16, 8, 32)])  # Cip 16: not a whole 32-channel tile
    assert f(bad, 1, 2, 2, items, 8, starts, 3, C.byref(n)) != 0
    # the setter: any negative value is the default again (host side, no device call)
    lib.niti_diag_wgrad_quad(-7)
    assert f(ok, 1, 2, 2, items, 8, starts, 3, C.byref(n)) == 0 and items[7] == 1  # (32: the one tile is a quad)
    lib.niti_diag_wgrad_quad(0)
    assert f(ok, 1, 2, 2, items, 8, starts, 3, C.byref(n)) == 0 and items[7] == 0
    lib.niti_diag_wgrad_quad(-1)
