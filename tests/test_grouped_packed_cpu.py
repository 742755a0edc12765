"""Grouped conv layers at the group widths of niti_gconv_packed_* on the host: the opt-in `level=8` routing
(niti_model_chain_check8), the derived shapes against the oracle's geometry, and what stays refused."""
import pytest

import grouped_cases as GC
import skip_cases as SK
from grouped_cases import O

from niti_amd import _lib as L
from niti_amd.chain import chain_layers, entry_points, level_of, normalize_spec
from niti_amd.checkpoint import chain_record


def _l(co, k, pad=0, relu=0, stride=1, skip=0, gpool=0, groups=1):
    return (co, k, pad, relu, 0, 0, 0, stride, skip, gpool, groups)


# a RegNetX-1.6GF stage-1 block (72 channels in 3 groups of 24: no multiple of 16), a strided grouped layer at cg 48
NET = (3, 8, [_l(72, 3, 1, 1), _l(72, 1, 0, 1), _l(72, 3, 1, 1, groups=3), _l(72, 1, 0, 1, skip=3), _l(96, 1, 0, 1),
              _l(96, 3, 1, 1, stride=2, groups=2), _l(96, 1, 0, 1, gpool=1), _l(10, 1)])


def test_level_8_derives_the_shapes():
    c, hw, spec = NET
    got, want = chain_layers(spec, c, hw, level=8), GC.derive(NET)
    assert [(g["ci"], g["co"], g["h"], g.get("stride", 1), g["groups"]) for g in got] == \
           [(w["ci"], w["co"], w["h"], w["stride"], w["groups"]) for w in want]
    for g, nxt in zip(got[:-2], got[1:]):  # the next layer's map is the oracle's output size
        assert nxt["h"] == O.geom(1, g["ci"], g["h"], g["h"], g["co"], g["k"], stride=g.get("stride", 1), pad=g["pad"]).oh
    assert [g["h"] for g in got] == [8, 8, 8, 8, 8, 8, 4, 1]


@pytest.mark.parametrize("level", (None, 6, 7))
def test_only_the_8_entry_points_take_it(level):
    with pytest.raises(L.NitiError) as e:
        chain_layers(NET[2], NET[0], NET[1], level=level)
    assert e.value.code == L.NOT_SUPPORT


@pytest.mark.parametrize("layer", [_l(36, 3, 1, 1, groups=3), _l(272, 3, 1, 1, groups=2), _l(72, 5, 2, 1, groups=3),
                                   _l(72, 3, 1, 1, stride=3, groups=3), _l(24, 3, 1, 1, groups=6)])
def test_level_8_keeps_the_other_refusals(layer):
    """cg 12 and 136, a 5x5 kernel, stride 3, and level 7's cg 4 on 24 channels."""
    with pytest.raises(L.NitiError) as e:
        chain_layers([_l(layer[0], 3, 1, 1), layer, _l(10, 1)], 3, 8, level=8)
    assert e.value.code == L.NOT_SUPPORT


def test_a_list_without_such_a_layer_is_unchanged():
    for net in GC.NETS.values():  # group widths 16 and 32: the same shapes
        assert chain_layers(net[2], net[0], net[1], level=8) == chain_layers(net[2], net[0], net[1])
    c, hw, layers = SK.NETS[sorted(SK.NETS)[0]]  # no grouped layer: the old entry points, the old record
    spec = normalize_spec(layers)
    assert level_of(spec, 8) is None and entry_points(spec, 8) == entry_points(spec)
    assert chain_record(spec, c, hw, level_of(spec, 8)) == chain_record(spec, c, hw)
    assert chain_record(normalize_spec(NET[2]), 3, 8, level_of(normalize_spec(NET[2]), 8))["level"] == 8
    with pytest.raises(ValueError):
        level_of(spec, 5)
