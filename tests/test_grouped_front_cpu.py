"""The grouped conv layers' one host front (csrc/niti_grouped_host.hip) on the host: every prefix's predicate and
slab count against values recorded before the three families' host code was merged, the width rule, and the
refusals of the 24 grouped and 12 depthwise C entries, all of which return before any launch.

The fixture tests/golden/grouped_front_plans.json was recorded by record() below from the library of the commit
before the merge:  NITI_HIP_LIB=<that library> python tests/test_grouped_front_cpu.py"""
import ctypes as C
import itertools
import json
import os

import pytest

from niti_amd import _lib as L

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "grouped_front_plans.json")
PREFIXES = ("gconv", "gconv2", "gconv_narrow", "gconv_packed")
# the width rule (gc_width, csrc/niti_grouped.hpp) over the grid's widths: the prefixes that take each
FAMILY = {4: ("gconv_narrow",), 8: ("gconv_narrow",), 12: (), 16: ("gconv", "gconv2"), 24: ("gconv_packed",),
          32: ("gconv", "gconv2"), 40: ("gconv_packed",), 64: ("gconv", "gconv2"), 72: ("gconv_packed",),
          128: ("gconv_packed",), 136: ()}
GRID = dict(cg=sorted(FAMILY), groups=(2, 3, 16), stride=(1, 2, 3), pad=(0, 1, 2, 3),
            nhw=((1, 1, 1), (1, 3, 3), (2, 8, 8), (4, 9, 70), (64, 56, 56), (256, 112, 112)), kernel=(3, 5),
            pitch16=(0, 1), wrong_oh=(0, 1))
# (cg, groups, n, hw): the slab buffer (slabs x c_out x 9 x cgp x 4 bytes) on either side of 2^31 bytes at 64 slabs,
# and the same channels at one slab
EXTRA = [(cg, groups, n, 3) for cg, pair in ((64, (227, 228)), (128, (56, 57)), (8, (7280, 7282)), (128, (8192,)))
         for groups in pair for n in (64, 1)]


def r16(c):
    return (c + 15) // 16 * 16


# the structure classes the loaded library binds (a test that reloads niti_amd._lib leaves new ones in the module)
def Geom(*fields):
    return L.lib().niti_gconv_ok.argtypes[0]._type_(*fields)


def DwconvOut():
    return L.lib().niti_gconv_fwd.argtypes[5]._type_()


def rows():
    """Every (cg, groups, stride, pad, (n, h, w), kernel, pitch16, wrong_oh) of the grid, then EXTRA at stride 1."""
    yield from itertools.product(*GRID.values())
    for cg, groups, n, hw in EXTRA:
        for stride in (1, 2):
            yield cg, groups, stride, 0, (n, hw, hw), 3, int(cg > 64), 0


def geom_of(cg, groups, stride, pad, nhw, kernel, pitch16, wrong_oh):
    n, h, w = nhw
    c = cg * groups
    oh, ow = (h + 2 * pad - kernel) // stride + 1, (w + 2 * pad - kernel) // stride + 1
    cp = r16(c) if pitch16 else c
    return Geom(n, c, h, w, c, kernel, kernel, stride, stride, pad, pad, pad, pad, 1, 1, oh + wrong_oh, ow, cp, cp, n)


def evaluate(lib):
    """{row index: [ok bits by prefix, slabs by prefix]} of the rows some prefix admits."""
    got = {}
    for i, row in enumerate(rows()):
        g, groups = geom_of(*row), row[1]
        ok = [int(getattr(lib, f"niti_{p}_ok")(C.byref(g), groups)) for p in PREFIXES]
        slabs = [int(getattr(lib, f"niti_{p}_wgrad_slabs")(C.byref(g), groups)) for p in PREFIXES]
        if any(ok) or any(slabs):
            got[str(i)] = [ok, slabs]
    return got


def record():
    admitted = evaluate(L.lib())
    with open(FIXTURE, "w") as f:
        json.dump({"rows": sum(1 for _ in rows()), "admitted": admitted}, f, separators=(",", ":"))
    print(f"{len(admitted)} admitted rows of {sum(1 for _ in rows())} -> {FIXTURE}")


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def current():
    return evaluate(L.lib())


def test_every_row_and_prefix_returns_the_recorded_value(recorded, current):
    assert recorded["rows"] == sum(1 for _ in rows()) and len(recorded["admitted"]) > 500
    assert current == recorded["admitted"]


def test_exactly_the_width_rules_families_accept_each_width(current):
    all_rows = list(rows())
    took = {cg: set() for cg in FAMILY}
    for i, (ok, slabs) in current.items():
        cg = all_rows[int(i)][0]
        assert [bool(s) for s in slabs] == [bool(o) for o in ok]
        for p, o in zip(PREFIXES, ok):
            if o:
                assert p in FAMILY[cg], (all_rows[int(i)], p)
                took[cg].add(p)
    assert {cg: tuple(p for p in PREFIXES if p in took[cg]) for cg in FAMILY} == FAMILY
    # the slab bound: each EXTRA pair's first count of groups is taken at 64 slabs, its second only at one slab;
    # at 8192 groups of 128 one slab is already too large
    extra = {r[:3] + (r[4][0],): current.get(str(i)) for i, r in enumerate(all_rows) if r[1] > 16}
    for (cg, groups, n, _), stride in itertools.product(EXTRA, (1, 2)):
        over = (groups in (228, 57, 7282) and n == 64) or groups == 8192
        assert (extra[(cg, groups, stride, n)] is None) == over, (cg, groups, stride, n)


# one admitted and one refused (a 4x4 kernel) geometry per grouped prefix, (cg, groups, stride); the same for the
# depthwise pair.  Each: the geometry, the arguments behind it, the int32 elements of one slab
ADMITTED = {"gconv": (32, 2, 1), "gconv2": (32, 2, 2), "gconv_narrow": (8, 4, 2), "gconv_packed": (24, 3, 1)}
FAKE = C.c_void_p(0x1000)  # a non-null operand no refusing path reads


def _grouped(prefix, kernel=3):
    cg, groups, stride = ADMITTED[prefix]
    g = geom_of(cg, groups, stride, 1, (2, 8, 8), kernel, int(prefix == "gconv_packed"), 0)
    return g, (groups,), cg * groups * 9 * (16 if prefix == "gconv_narrow" else cg)


def _depthwise(prefix, kernel=3):
    stride = 2 if prefix == "dwconv2" else 1
    g = Geom(2, 32, 8, 8, 32, kernel, kernel, stride, stride, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0)
    return g, (), 9 * 32


CASES = [(p, _grouped) for p in PREFIXES] + [(p, _depthwise) for p in ("dwconv", "dwconv2")]


@pytest.mark.parametrize("prefix,make", CASES)
def test_a_refused_geometry_is_invalid_value_at_every_entry(prefix, make):
    lib, (g, gr, _), out, n = L.lib(), make(prefix, kernel=4), DwconvOut(), C.c_int(0)
    fn = lambda kind: getattr(lib, f"niti_{prefix}_{kind}")  # noqa: E731
    assert fn("ok")(C.byref(g), *gr) == 0 and fn("wgrad_slabs")(C.byref(g), *gr) == 0
    for kind in ("fwd", "dgrad"):
        assert fn(kind)(C.byref(g), *gr, FAKE, FAKE, FAKE, C.byref(out), 0, None) == L.INVALID_VALUE
    assert fn("wgrad")(C.byref(g), *gr, FAKE, FAKE, FAKE, 1 << 40, C.byref(n), None) == L.INVALID_VALUE
    assert fn("wgrad_reduce")(C.byref(g), *gr, FAKE, 1, FAKE, FAKE, None) == L.INVALID_VALUE
    assert fn("ok")(None, *gr) == 0 and fn("fwd")(None, *gr, FAKE, FAKE, FAKE, C.byref(out), 0, None) == L.INVALID_VALUE


@pytest.mark.parametrize("prefix,make", CASES)
def test_an_admitted_geometry_with_a_bad_operand_is_invalid_value(prefix, make):
    lib, (g, gr, elems), out, n = L.lib(), make(prefix), DwconvOut(), C.c_int(0)
    fn = lambda kind: getattr(lib, f"niti_{prefix}_{kind}")  # noqa: E731
    slabs = fn("wgrad_slabs")(C.byref(g), *gr)
    assert fn("ok")(C.byref(g), *gr) == 1 and slabs >= 1
    out.out = FAKE.value
    for kind in ("fwd", "dgrad"):
        for args in ((None, FAKE, FAKE, C.byref(out), 0), (FAKE, None, FAKE, C.byref(out), 0),
                     (FAKE, FAKE, None, C.byref(out), 0), (FAKE, FAKE, FAKE, None, 0),
                     (FAKE, FAKE, FAKE, C.byref(out), 2), (FAKE, FAKE, FAKE, C.byref(out), -1),
                     (FAKE, FAKE, FAKE, C.byref(DwconvOut()), 1)):  # pass 1 without an output
            assert fn(kind)(C.byref(g), *gr, *args, None) == L.INVALID_VALUE, (kind, args)
    for args in ((None, FAKE, FAKE, 1 << 40), (FAKE, None, FAKE, 1 << 40), (FAKE, FAKE, None, 1 << 40),
                 (FAKE, FAKE, FAKE, 0), (FAKE, FAKE, FAKE, slabs * elems * 4 - 1)):  # slab_bytes one byte short
        assert fn("wgrad")(C.byref(g), *gr, *args, C.byref(n), None) == L.INVALID_VALUE, args
    for args in ((None, slabs, FAKE), (FAKE, slabs, None), (FAKE, slabs + 1, FAKE), (FAKE, 0, FAKE)):
        assert fn("wgrad_reduce")(C.byref(g), *gr, *args, FAKE, None) == L.INVALID_VALUE, args


if __name__ == "__main__":
    record()
