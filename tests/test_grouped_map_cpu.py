"""The grouped map cases on the host (tests/grouped_map_cases.py): the direct reference against the oracle over the
block-diagonal weight at every shape of the older grouped op tests and two non-square ones, and each case of the
table against the hazard its comment names, by integer arithmetic over the kernels' tile sizes.  The ids of
test_a_case_reaches_its_hazard show segments, a full segment, units and slabs of every case."""
import numpy as np
import pytest

import grouped_cases as GC
import grouped_map_cases as GM
import grouped_stride2_cases as G2
from grouped_cases import DC, O
from test_gpu_grouped_narrow_ops import SHAPES as NARROW_SHAPES

# (n, C, G, h, w, pad, stride) of the older op shapes, and two small non-square maps
ORACLE_SHAPES = tuple((n, c, g, h, h, p, 1) for n, c, g, h, p in GC.OP_SHAPES) + \
    tuple((n, c, g, h, h, p, 2) for n, c, g, h, p in G2.OP_SHAPES) + \
    tuple((n, c, g, h, h, p, s) for n, c, g, h, p, s in NARROW_SHAPES) + \
    ((2, 32, 2, 3, 7, 1, 1), (3, 48, 6, 9, 4, 2, 2))


@pytest.mark.parametrize("shape", ORACLE_SHAPES, ids=GM.case_id)
def test_direct_reference_is_the_oracles(shape):
    n, c, groups, h, w, pad, stride = shape
    g = O.geom(n, c, h, w, c, 3, stride=stride, pad=pad)
    assert (g.oh, g.ow) == GM.out_hw(shape)
    rng = np.random.default_rng(8000 + ORACLE_SHAPES.index(shape))
    x = rng.integers(-128, 128, (n, c, h, w)).astype(np.int8)
    dy = rng.integers(-128, 128, (n, c, g.oh, g.ow)).astype(np.int8)
    wt = rng.integers(-127, 128, (c, c // groups, 3, 3)).astype(np.int8)
    assert np.array_equal(GM.g_fwd_direct(x, wt, groups, pad, stride), GC.act_ref(g, groups, x, wt)[2])
    assert np.array_equal(GM.g_dgrad_direct(dy, wt, groups, pad, stride, h, w), GC.act_ref(g, groups, dy, wt, dgrad=True)[2])
    assert np.array_equal(GM.g_wgrad_direct(x, dy, groups, pad, stride), GC.wgrad_ref(g, groups, x, dy))


def test_the_direct_reference_refuses_an_accumulator_past_int32():
    x = np.full((1, 16, 1, 1), 2 ** 20, np.int64)
    with pytest.raises(AssertionError):
        GM.g_fwd_direct(x, np.full((16, 8, 3, 3), 2 ** 9, np.int64), 2, 1, 1)


# ------------------------------------------------------------------------------------ the hazards
def _hazard_id(shape):
    t = {op: GM.tiling(shape, op) for op in ("fwd", "dgrad", "wgrad")}
    segs = "/".join(str(t[op]["segs"]) for op in ("fwd", "dgrad", "wgrad"))
    full = "".join("fF"[t[op]["full"]] for op in ("fwd", "dgrad", "wgrad"))
    return f"{GM.case_id(shape)}-segs{segs}-full{full}-units{t['wgrad']['units']}-slabs{GM.slabs_of(shape)}"


def _kind(shape):
    tables = dict(seg=GM.SEG_CASES, twin=GM.TWIN_CASES, full=GM.FULL_CASES, unit=GM.UNIT_CASES, eq1=GM.EQ1_CASES)
    return next(k for k, t in tables.items() if shape in t)


@pytest.mark.parametrize("shape", GM.ALL_CASES, ids=_hazard_id)
def test_a_case_reaches_its_hazard(shape):
    """Segments (forward / input gradient / weight gradient), a full segment, units and slabs are in the id."""
    n, c, groups, h, w, pad, stride = shape
    kind, cg = _kind(shape), GM.cg_of(shape)
    t = {op: GM.tiling(shape, op) for op in ("fwd", "dgrad", "wgrad")}
    slabs = GM.slabs_of(shape)
    print(_hazard_id(shape), {op: (v["bands"], v["segs"], v["last"]) for op, v in t.items()})
    assert c % groups == 0 and cg in (4, 8, 16, 32, 64) and c % 16 == 0 and groups >= 2 and 0 <= pad <= 2
    assert 1 <= slabs <= t["wgrad"]["units"] == n * t["wgrad"]["bands"] * t["wgrad"]["segs"]
    if kind == "seg":  # every launch: a second segment, partial; the first then is full; a partial last band
        for op in t:
            assert t[op]["segs"] >= 2 and t[op]["last"] < GM.seg_cols(shape) and t[op]["full"], op
            assert t[op]["part_band"] and h != w, op
        assert n >= 2  # (the image's pitch in the addresses)
    elif kind == "twin":  # the transpose of a segment case (two bands): one segment, many bands
        assert GM.transposed(shape) in GM.SEG_CASES
        for op in t:
            assert t[op]["segs"] == 1 and t[op]["bands"] > 2, op
    elif kind == "full":  # every strip or quad of some segment in use
        assert all(t[op]["full"] for op in t)
    elif kind == "unit":  # a second unit for some workgroups, not for all: the reuse path and the remainder
        u = t["wgrad"]["units"]
        assert slabs == GM.MIN_SLABS and slabs < u < 2 * slabs, (u, slabs)
        x, dy, _ = GM.wgrad_case(shape)
        assert (x == -128).any() and (dy == -128).any() and (dy == 0).any() and (x > 0).any() and (x < 0).any()
    else:  # the amplitude search lands in its class, both ways; the mask has non-positive entries where dx is not 0
        assert cg in (4, 8)
        for dgrad in (False, True):
            a, wt, mask, acc = GM.eq1_case(shape, dgrad)
            assert O.range_estimate(acc) == 8 and 128 <= GC.absmax(acc) <= 255
            q, inc = DC.requant_under(acc)
            assert inc == 2 and ((mask <= 0) & (q != 0)).any() and ((mask > 0) & (q != 0)).any()


def test_every_instantiation_meets_every_hazard():
    """cg in {4, 8, 16, 32, 64} x stride {1, 2}: a second segment, a full segment, a non-square map and its transpose
    for the three launches; more units than slabs for the weight gradient; eq1 for the narrow act kernels."""
    def have(cases):
        return {(GM.cg_of(s), s[6]) for s in cases}
    every = set(GM.INSTANTIATIONS)
    assert have(GM.SEG_CASES) == have(GM.TWIN_CASES) == have(GM.FULL_CASES) == have(GM.UNIT_CASES) == every
    assert have(GM.EQ1_CASES) == {i for i in every if i[0] < 16}
    assert len(set(GM.ALL_CASES)) == len(GM.ALL_CASES)


def test_slab_rule_on_the_older_shapes():
    """slabs_of is the plan rule the older tests ran under: few units, so one slab a unit."""
    for shape in ORACLE_SHAPES:
        assert GM.slabs_of(shape) == GM.tiling(shape, "wgrad")["units"] <= GM.MIN_SLABS, shape
