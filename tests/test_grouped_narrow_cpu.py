"""Grouped conv layers of group width 4 and 8 on the host: the opt-in `level=7` routing (niti_model_chain_check7), the
derived shapes against the oracle's geometry, and what stays refused."""
import pytest

import grouped_cases as GC
from grouped_cases import O
from test_grouped_cpu import REFUSED, _net

from niti_amd import _lib as L
from niti_amd.chain import chain_layers


def _l(co, k, pad=0, relu=0, stride=1, skip=0, gpool=0, groups=1):
    return (co, k, pad, relu, 0, 0, 0, stride, skip, gpool, groups)


# a ResNeXt block at cg 4, a strided grouped layer at cg 8
NET = (3, 8, [_l(64, 3, 1, 1), _l(64, 1, 0, 1), _l(64, 3, 1, 1, groups=16), _l(64, 1, 0, 1, skip=3), _l(64, 1, 0, 1),
              _l(64, 3, 1, 1, stride=2, groups=8), _l(64, 1, 0, 1, gpool=1), _l(10, 1)])


def test_level_7_derives_the_shapes():
    c, hw, spec = NET
    got, want = chain_layers(spec, c, hw, level=7), GC.derive(NET)
    assert [(g["ci"], g["co"], g["h"], g.get("stride", 1), g["groups"]) for g in got] == \
           [(w["ci"], w["co"], w["h"], w["stride"], w["groups"]) for w in want]
    for g, nxt in zip(got[:-2], got[1:]):  # the next layer's map is the oracle's output size
        assert nxt["h"] == O.geom(1, g["ci"], g["h"], g["h"], g["co"], g["k"], stride=g.get("stride", 1), pad=g["pad"]).oh
    assert [g["h"] for g in got] == [8, 8, 8, 8, 8, 8, 4, 1]


@pytest.mark.parametrize("level", (None, 6))
def test_only_the_7_entry_points_take_it(level):
    with pytest.raises(L.NitiError) as e:
        chain_layers(NET[2], NET[0], NET[1], level=level)
    assert e.value.code == L.NOT_SUPPORT


@pytest.mark.parametrize("case", [REFUSED[0], REFUSED[4], REFUSED[6], REFUSED[8], REFUSED[10], REFUSED[11],
                                  (dict(stride=3), 3, 8, False), (dict(groups=32), 3, 8, False),
                                  ([_l(24, 3, 1, 1), _l(24, 3, 1, 1, groups=6), _l(10, 1)], 3, 8, False)])
def test_level_7_keeps_the_other_refusals(case):
    """groups < 0, unequal group widths, cg 1 and 2, kernel 5, stride 3, a grouped first or last layer, and cg 4 on
    24 channels (no multiple of 16)."""
    spec, c, hw, malformed = case
    spec = _net(**spec) if isinstance(spec, dict) else spec
    with pytest.raises(ValueError if malformed else L.NitiError) as e:
        chain_layers(spec, c, hw, level=7)
    assert malformed or e.value.code == L.NOT_SUPPORT


@pytest.mark.parametrize("name", GC.NETS)
def test_a_list_without_a_narrow_layer_is_unchanged(name):
    net = GC.NETS[name]
    assert chain_layers(net[2], net[0], net[1], level=7) == chain_layers(net[2], net[0], net[1])
