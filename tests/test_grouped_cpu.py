"""Grouped conv layers on the host: the spec key, every refusal of niti_model_chain_check5 (malformed against
unsupported), unchanged records for lists without the key, and the step reference of tests/grouped_cases.py
against the direct sums of the definition."""
import numpy as np
import pytest

import grouped_cases as GC
from grouped_cases import O

from niti_amd import _lib as L
from niti_amd.chain import chain_layers, entry_points, normalize_spec


def _net(**kw):
    """stem 3x3 -> 64, the layer under test (a grouped 3x3 of 2 groups unless overridden), fc on a flatten"""
    mid = dict(dict(c_out=64, kernel=3, pad=1, relu=1, groups=2), **kw)
    return [dict(c_out=64, kernel=3, pad=1, relu=1), mid, dict(c_out=16, kernel=1, flatten=1), dict(c_out=10, kernel=1)]


def test_chain_layers_derives_a_grouped_list():
    for name, net in GC.NETS.items():
        got = chain_layers(net[2], net[0], net[1])
        want = GC.derive(net)
        assert [(g["ci"], g["co"], g["k"], g["h"], g["groups"]) for g in got] == \
               [(w["ci"], w["co"], w["k"], w["h"], w["groups"]) for w in want], name
    spec = normalize_spec(_net())
    assert entry_points(spec)[0] is L.lib().niti_model_chain_check5
    assert [d["groups"] for d in spec] == [1, 2, 1, 1]
    assert normalize_spec([(64, 3, 1, 1, 0, 0, 0, 1, 0, 0, 2)])[0]["groups"] == 2  # the eleventh tuple entry


def test_a_list_without_groups_is_unchanged():
    plain = [dict(c_out=16, kernel=3, pad=1, relu=1, pool=1), dict(c_out=10, kernel=1, flatten=0)]
    for spec in (plain, [dict(d, groups=g) for d, g in zip(plain, (1, 0))]):
        norm = normalize_spec(spec)
        assert all(set(d) == {"c_out", "kernel", "pad", "relu", "pool", "flatten"} for d in norm)
        assert entry_points(norm)[0] is L.lib().niti_model_chain_check2


_G = dict(c_out=32, kernel=3, pad=1, groups=2)
REFUSED = [  # (the mid layer's overrides or a whole list, in_c, in_hw, malformed)
    (dict(groups=-1), 3, 8, True), (dict(groups=2, depthwise=1, c_out=0), 3, 8, True),
    (dict(groups=3), 3, 8, True),            # c_in = 64 is not divisible
    (dict(groups=4, c_out=66), 3, 8, True),  # c_in is, c_out is not
    (dict(c_out=128), 3, 8, False),          # c_in / groups != c_out / groups
    (dict(groups=8), 3, 8, False), (dict(groups=64), 3, 8, False),  # cg 8, cg 1
    (dict(kernel=1, pad=0), 3, 8, False), (dict(kernel=5, pad=2), 3, 8, False), (dict(stride=2), 3, 8, False),
    ([_G, dict(c_out=10, kernel=1, flatten=1)], 32, 8, False),                              # layer 0
    ([dict(c_out=32, kernel=3, pad=1), dict(_G, pad=0)], 3, 3, False),                      # the last layer
    ([dict(c_out=32, kernel=3, pad=1, gpool=1), _G, dict(c_out=10, kernel=1)], 3, 8, False),  # on a 1x1 map
]


@pytest.mark.parametrize("case", REFUSED)
def test_refusals(case):
    spec, c, hw, malformed = case
    spec = _net(**spec) if isinstance(spec, dict) else spec
    if malformed:  # (the check's own refusal, not normalize_spec's of an unknown key)
        with pytest.raises(ValueError, match="malformed layer list"):
            chain_layers(spec, c, hw)
    else:
        with pytest.raises(L.NitiError) as e:  # (the class as it is now: another test module reloads niti_amd._lib)
            chain_layers(spec, c, hw)
        assert e.value.code == L.NOT_SUPPORT


def test_step_reference_on_a_tiny_net():
    """One step of stem -> grouped 3x3 (2 groups of 16) -> fc: the grouped layer's forward and update from the
    direct sums of the definition, acc[n][o] = sum over the group's cg channels i and the taps of
    x[n][cg (o / cg) + i] w[o][i], dw[o][i] = sum over images and pixels of dy[n][o] x[n][cg (o / cg) + i]."""
    import niti_model_ref as R
    net = (3, 4, [GC._l(32, 3, 1, 1), GC._l(32, 3, 1, 1, groups=2, flatten=1), GC._l(5, 1)])
    layers = GC.derive(net)
    W, S = GC.init_weights(layers, 5)
    (x, labels), = GC.DC.batches(layers, 2, 1, 2)
    newW, rec = GC.chain_step_ref(layers, W, S, x, -3, labels)
    # the gradient at the grouped layer's output: the head's input gradient through the flatten and the relu
    d = O.loss_grad(rec["logits"], rec["exp"][2], R.onehot(labels, 5)).reshape(2, 5, 1, 1)
    dflat, _, _, _ = O.conv_dgrad(rec["geom"][2], d, W[2])
    dy = O.relu_grad(rec["y"][1], dflat.reshape(rec["r"][1].shape)).astype(np.int64)
    xp = np.zeros((2, 32, 6, 6), np.int64)
    xp[:, :, 1:5, 1:5] = rec["inp"][1]
    acc, dw = np.zeros((2, 32, 4, 4), np.int64), np.zeros((32, 16, 3, 3), np.int64)
    for o in range(32):
        xs = xp[:, 16 * (o // 16):16 * (o // 16) + 16]
        for ky in range(3):
            for kx in range(3):
                win = xs[:, :, ky:ky + 4, kx:kx + 4]
                acc[:, o] += np.einsum("nihw,i->nhw", win, W[1][o, :, ky, kx].astype(np.int64))
                dw[o, :, ky, kx] = np.einsum("nhw,nihw->i", dy[:, o], win)
    y, inc = O.requant_fwd(acc.astype(np.int32))
    assert np.array_equal(rec["y"][1], y) and rec["exp"][1] == rec["exp"][0] + S[1] + inc
    want, _ = GC.UB.apply_update(W[1], dw.astype(np.int32), 2)
    assert np.array_equal(newW[1], want) and not np.array_equal(want, W[1])
