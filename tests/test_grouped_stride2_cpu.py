"""Grouped conv layers at stride 2 on the host: the opt-in `level=6` routing (niti_model_chain_check6), the derived
strided shapes against the oracle's geometry, what stays refused, and records that do not change."""
import ctypes as C

import pytest

import grouped_cases as GC
import grouped_stride2_cases as G2
from grouped_cases import O
from test_grouped_cpu import REFUSED, _net

from niti_amd import _lib as L
from niti_amd.chain import chain_layers, entry_points, normalize_spec, to_c
from niti_amd.checkpoint import chain_record


def test_level_6_derives_the_strided_shapes():
    c, hw, spec = G2.NET_S
    got, want = chain_layers(spec, c, hw, level=6), GC.derive(G2.NET_S)
    assert [(g["ci"], g["co"], g["h"], g.get("stride", 1), g["groups"]) for g in got] == \
           [(w["ci"], w["co"], w["h"], w["stride"], w["groups"]) for w in want]
    for g, nxt in zip(got[:-2], got[1:]):  # the next layer's map is the oracle's output size
        assert nxt["h"] == O.geom(1, g["ci"], g["h"], g["h"], g["co"], g["k"], stride=g.get("stride", 1), pad=g["pad"]).oh
    assert [g["h"] for g in got] == [16, 16, 16, 8, 8, 8, 1]


def test_only_the_6_entry_points_take_it():
    c, hw, spec = G2.NET_S
    with pytest.raises(L.NitiError) as e:
        chain_layers(spec, c, hw)
    assert e.value.code == L.NOT_SUPPORT
    with pytest.raises(ValueError):
        chain_layers(spec, c, hw, level=5)
    lib, norm = L.lib(), normalize_spec(spec)
    arr, n = to_c(norm)
    shapes = ((C.c_int * 8) * n)()
    assert lib.niti_model_chain_check5(arr, n, c, hw, shapes) == L.NOT_SUPPORT
    assert lib.niti_model_chain_check6(arr, n, c, hw, shapes) == 0
    assert entry_points(norm)[0] is lib.niti_model_chain_check5 and entry_points(norm, 6)[0] is lib.niti_model_chain_check6
    plain = normalize_spec([dict(c_out=16, kernel=3, pad=1), dict(c_out=10, kernel=1, flatten=1)])
    assert entry_points(plain, 6)[0] is lib.niti_model_chain_check2  # level 6 moves grouped lists only


def test_records_without_level_are_unchanged():
    net = GC.NETS["NET_R"]
    assert chain_record(net[2], net[0], net[1]) == {"spec": normalize_spec(net[2]), "in_c": 1, "in_hw": 8}
    assert chain_record(net[2], net[0], net[1], 6)["level"] == 6
    assert chain_layers(net[2], net[0], net[1], level=6) == chain_layers(net[2], net[0], net[1])


@pytest.mark.parametrize("case", [REFUSED[0], REFUSED[4], REFUSED[7], REFUSED[10], (dict(stride=3), 3, 8, False)])
def test_level_6_keeps_the_other_refusals(case):
    spec, c, hw, malformed = case
    spec = _net(**spec) if isinstance(spec, dict) else spec
    with pytest.raises(ValueError if malformed else L.NitiError) as e:
        chain_layers(spec, c, hw, level=6)
    assert malformed or e.value.code == L.NOT_SUPPORT
