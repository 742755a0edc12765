"""Host-side checks of skip connections, the global pool and the 64-layer limit of chain networks
(niti_model_chain_check4, the Python spec keys) and of the reference the GPU tests trust
(tests/skip_cases.py).  No GPU."""
import ctypes as C
import functools
import json

import numpy as np
import pytest

import chain_cases as CC
import depthwise_cases as DC
import skip_cases as K
import strided_cases as SC
from niti_amd._lib import INVALID_VALUE as INVALID, NOT_SUPPORT

OLD_NETS = ["LENET", "VGG11", "VGG16_32", "NET_A", "NET_B", "NET_C", "NET_D", "NET_D2", "NET_E", "NET_F", "NET_G"]


@pytest.fixture(scope="module")
def L():
    from niti_amd import _lib
    return _lib


def _arr3(L, spec):
    arr = (L.ChainLayer3 * len(spec))()
    for a, l in zip(arr, spec):
        l = tuple(l) + (0,) * (10 - len(l))
        a.c_out, a.kernel, a.pad, a.relu, a.pool, a.flatten, a.depthwise = l[:7]
        a.stride, a.skip, a.gpool = l[7] or 1, l[8], l[9]
    return arr


def _check4(L, spec, in_c, in_hw):
    arr = _arr3(L, spec)
    shapes = ((C.c_int * 8) * len(spec))()
    code = L.lib().niti_model_chain_check4(arr, len(spec), in_c, in_hw, shapes)
    return code, [list(s) for s in shapes]


@functools.lru_cache(maxsize=None)
def _ref(name):
    layers = K.derive(K.NETS[name])
    W, S = K.init_weights(layers, seed=K.SEED_W)
    data = K.batches(layers, K.BATCH[name], 2, K.SEED_X)
    return layers, W, S, data, K.ref_steps(layers, W, S, data)


# ------------------------------------------------------------------------------------ the check
@pytest.mark.parametrize("name", sorted(K.NETS))
def test_chain_check4_shapes_equal_derive(L, name):
    in_c, in_hw, spec = K.NETS[name]
    code, shapes = _check4(L, spec, in_c, in_hw)
    assert code == 0
    assert shapes == K.shapes_of(K.derive(K.NETS[name]))


def test_the_nets_are_what_they_claim():
    assert [len(K.NETS[n][2]) for n in ("NET_V", "NET_W", "NET_X", "NET_D", "NET_E")] == [15, 6, 6, 27, 27]
    v = K.derive(K.NET_V)
    assert [i for i, l in enumerate(v) if l["skip"]] == [3, 6, 12] and v[0]["relu"] and not v[3]["relu"]
    assert v[9]["co"] == 24 and v[8]["stride"] == 2 and v[13]["gpool"] and v[14]["h"] == 1
    x = K.derive(K.NET_X)
    assert x[1]["dw"] and x[1]["skip"] == 1 and x[1]["co"] == 40 and x[1]["h"] == 9 and x[3]["pool"] and x[3]["skip"] == 1


_c = lambda co, k, pad=0, relu=0, **kw: K._l(co, k, pad, relu, **kw)  # noqa: E731
REFUSALS = {
    # malformed
    "skip_negative": ([_c(16, 3, 1, 1), _c(16, 3, 1, 1, skip=-1), _c(16, 3, 1, flatten=1), _c(10, 1)], 8, INVALID),
    "skip_before_the_first_layer": ([_c(16, 3, 1, 1), _c(16, 3, 1, 1, skip=2), _c(16, 3, 1, flatten=1), _c(10, 1)], 8, INVALID),
    "source_channels_differ": ([_c(16, 3, 1, 1), _c(32, 3, 1, 1, skip=1), _c(16, 3, 1, flatten=1), _c(10, 1)], 8, INVALID),
    "source_map_differs": ([_c(16, 3, 1, 1), _c(16, 3, 0, 1, skip=1), _c(16, 3, 1, flatten=1), _c(10, 1)], 8, INVALID),
    "source_pooled_map_differs": ([_c(16, 3, 1, 1, pool=1), _c(16, 3, 1, 1), _c(16, 3, 1, 1, stride=1, skip=2),
                                   _c(16, 3, 1, flatten=1), _c(10, 1)], 8, NOT_SUPPORT),  # (shapes agree: the source pools)
    "gpool_two": ([_c(16, 3, 1, 1, gpool=2), _c(10, 1)], 8, INVALID),
    "gpool_negative": ([_c(16, 3, 1, 1, gpool=-1), _c(10, 1)], 8, INVALID),
    # well formed, not run
    "last_layer_adds": ([_c(10, 1, 0, 1, flatten=0), _c(10, 1, 0, 0, skip=1)], 1, NOT_SUPPORT),
    "adding_layer_behind_a_flatten": ([_c(16, 3, 1, 1, flatten=1), _c(64, 1, 0, 1), _c(64, 1, 0, 1, skip=1), _c(10, 1)], 2, NOT_SUPPORT),
    "source_behind_a_gpool": ([_c(16, 3, 1, 1, gpool=1), _c(16, 1, 0, 1), _c(16, 1, 0, 1, skip=1), _c(10, 1)], 8, NOT_SUPPORT),
    "source_flattens": ([_c(16, 3, 1, 1, flatten=1), _c(16, 1, 0, 1, skip=1), _c(10, 1)], 1, NOT_SUPPORT),
    "source_gpools": ([_c(16, 3, 1, 1, gpool=1), _c(16, 1, 0, 1, skip=1), _c(10, 1)], 1, NOT_SUPPORT),
    "source_of_two": ([_c(16, 3, 1, 1), _c(16, 3, 1, 1, skip=1), _c(16, 3, 1, 1, skip=2), _c(16, 3, 1, flatten=1), _c(10, 1)], 4, NOT_SUPPORT),
    "spans_nest": ([_c(16, 3, 1, 1), _c(16, 3, 1, 1), _c(16, 3, 1, 1, skip=1), _c(16, 3, 1, 1, skip=3),
                    _c(16, 3, 1, flatten=1), _c(10, 1)], 4, NOT_SUPPORT),
    "spans_cross": ([_c(16, 3, 1, 1), _c(16, 3, 1, 1), _c(16, 3, 1, 1, skip=2), _c(16, 3, 1, 1, skip=2),
                     _c(16, 3, 1, flatten=1), _c(10, 1)], 4, NOT_SUPPORT),
    "spans_share_an_endpoint": ([_c(16, 3, 1, 1), _c(16, 3, 1, 1, skip=1), _c(16, 3, 1, 1, skip=1), _c(16, 3, 1, flatten=1),
                                 _c(10, 1)], 4, 0),  # (control: runs)
    "gpool_with_pool": ([_c(16, 3, 1, 1, pool=1, gpool=1), _c(10, 1)], 8, NOT_SUPPORT),
    "gpool_with_flatten": ([_c(16, 3, 1, 1, flatten=1, gpool=1), _c(10, 1)], 1, NOT_SUPPORT),
    "gpool_on_the_last_layer": ([_c(16, 3, 1, 1, flatten=1), _c(10, 1, gpool=1)], 1, NOT_SUPPORT),
    "gpool_sums_past_int32": ([_c(16, 1, 0, 1, gpool=1), _c(10, 1)], 2908, NOT_SUPPORT),  # 2908^2 * 254 >= 2^31
    "gpool_sums_within_int32": ([_c(16, 1, 0, 1, gpool=1), _c(10, 1)], 2907, 0),
    "kernel_3_after_a_gpool": ([_c(16, 3, 1, 1, gpool=1), _c(16, 3, 1, 1), _c(10, 1)], 8, NOT_SUPPORT),
    "depthwise_after_a_gpool": ([_c(16, 3, 1, 1, gpool=1), _c(0, 3, 1, 1, dw=1), _c(10, 1)], 8, NOT_SUPPORT),
    "sixty_five_layers": ([_c(16, 3, 1, 1)] * 63 + [_c(16, 3, 1, 1, gpool=1), _c(10, 1)], 4, NOT_SUPPORT),
    "sixty_four_layers": ([_c(16, 3, 1, 1)] * 62 + [_c(16, 3, 1, 1, gpool=1), _c(10, 1)], 4, 0),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_chain_check4_codes(L, name):
    spec, in_hw, want = REFUSALS[name]
    assert _check4(L, spec, 3, in_hw)[0] == want


def test_create_chain4_refuses_before_anything_is_allocated(L):
    spec, in_hw, want = REFUSALS["spans_cross"]
    arr = _arr3(L, spec)
    h = C.c_void_p()
    assert L.lib().niti_model_create_chain4(arr, len(spec), 3, in_hw, 2, C.byref(h)) == want and not h
    assert L.lib().niti_model_create_chain4(arr, len(spec), 3, in_hw, 0, C.byref(h)) == INVALID and not h
    assert L.lib().niti_model_layer_skip(None, 0, None, None) == INVALID


def test_the_older_entry_points_still_refuse_25_layers(L):
    spec = [(16, 3, 1, 1, 0, 0)] * 23 + [(16, 3, 1, 1, 0, 1), (10, 1, 0, 0, 0, 0)]
    assert len(spec) == 25
    a1 = (L.ChainLayer * 25)()
    a2 = (L.ChainLayer2 * 25)()
    for x, y, (co, k, pad, relu, pool, fl) in zip(a1, a2, spec):
        for s in (x, y):
            s.c_out, s.kernel, s.stride, s.pad, s.relu, s.pool, s.flatten = co, k, 1, pad, relu, pool, fl
    lib = L.lib()
    assert lib.niti_model_chain_check(a1, 25, 3, 2, None) == NOT_SUPPORT
    assert lib.niti_model_chain_check2(a2, 25, 3, 2, None) == NOT_SUPPORT
    assert lib.niti_model_chain_check3(a2, 25, 3, 2, None) == NOT_SUPPORT
    assert lib.niti_model_chain_check2(a2, 24, 3, 2, None) == NOT_SUPPORT  # (24 of them: the last layer flattens)
    h = C.c_void_p()
    for fn, arr in (("niti_model_create_chain", a1), ("niti_model_create_chain2", a2), ("niti_model_create_chain3", a2)):
        assert getattr(lib, fn)(arr, 25, 3, 2, 1, C.byref(h)) == NOT_SUPPORT and not h
    assert _check4(L, [tuple(l) for l in spec], 3, 2)[0] == 0
    # ... and from Python such a list goes through the `4` entry points
    from niti_amd import chain_layers
    assert len(chain_layers(spec, 3, 2)) == 25


# ------------------------------------------------------------------------------------ specs and records
@pytest.mark.parametrize("net", OLD_NETS)
def test_records_of_lists_without_the_new_keys_are_unchanged(net):
    from niti_amd import chain_layers, checkpoint, normalize_spec
    in_c, in_hw, spec = getattr(CC, net)
    want = [dict(c_out=l[0], kernel=l[1], pad=l[2], relu=l[3], pool=l[4], flatten=l[5]) for l in spec]
    assert normalize_spec(spec) == want
    assert normalize_spec([tuple(l) + (0, 1, 0, 0) for l in spec]) == want
    assert normalize_spec([{**d, "skip": 0, "gpool": 0} for d in want]) == want
    rec = checkpoint.chain_record(spec, in_c, in_hw)
    assert json.dumps(rec, sort_keys=True) == json.dumps({"spec": want, "in_c": in_c, "in_hw": in_hw}, sort_keys=True)
    assert all(set(l) == {"ci", "co", "k", "pad", "h", "relu", "pool", "flatten"} for l in chain_layers(spec, in_c, in_hw))


@pytest.mark.parametrize("name", sorted(SC.NETS) + sorted(DC.NETS))
def test_records_of_strided_and_depthwise_lists_are_unchanged(name):
    from niti_amd import normalize_spec
    from niti_amd.chain import wide
    spec = (SC.NETS[name] if name in SC.NETS else DC.NETS[name])[2]
    norm = normalize_spec(spec)
    assert all("skip" not in d and "gpool" not in d for d in norm) and not wide(norm)


def test_a_list_with_the_new_keys_round_trips():
    from niti_amd import chain_layers, checkpoint, normalize_spec
    from niti_amd.chain import wide
    in_c, in_hw, spec = K.NET_V
    norm = normalize_spec(spec)
    assert wide(norm) and normalize_spec(norm) == norm
    assert [d["skip"] for d in norm] == [0, 0, 0, 3, 0, 0, 3, 0, 0, 0, 0, 0, 3, 0, 0]
    assert [d["gpool"] for d in norm] == [0] * 13 + [1, 0]
    got = chain_layers(spec, in_c, in_hw)
    want = K.derive(K.NET_V)
    assert [(l["ci"], l["co"], l["h"], l["skip"], l["gpool"]) for l in got] == \
        [(l["ci"], l["co"], l["h"], l["skip"], l["gpool"]) for l in want]
    # a gpool-only list carries gpool and no skip; the records of lists that differ in one key differ
    g = normalize_spec(K.NET_G[2])
    assert all("gpool" in d and "skip" not in d for d in g)
    other = [tuple(l) for l in spec]
    other[6] = other[6][:8] + (0, 0)
    assert checkpoint.chain_record(spec, in_c, in_hw) != checkpoint.chain_record(other, in_c, in_hw)
    with pytest.raises(ValueError):
        chain_layers(REFUSALS["source_channels_differ"][0], 3, 8)


# ------------------------------------------------------------------------------------ the reference
def test_net_w_equals_the_residual_reference():
    """NET_W is the pool-less-stem ResNet dict(depths=(2,), width=16) at 8 px: chain_step_ref against
    resnet_family_cases.family_step_ref with the same weights, two steps."""
    import resnet_family_cases as F
    layers, W, S, data, ref = _ref("NET_W")
    spec = dict(depths=(2,), width=16, classes=10, stem="cifar")
    convs = F.family_convs(spec, 8)
    assert [(c["ci"], c["co"], c["k"], c["stride"], c["pad"], c["h"]) for c in convs] == \
        [(l["ci"], l["co"], l["k"], l["stride"], l["pad"], l["h"]) for l in layers]
    Wf = W
    for (x, labels), (newW, rec, _, e) in zip(data, ref):
        newF, recF = F.family_step_ref(convs, Wf, S, x, e, labels, 10, pool=False)
        assert np.array_equal(rec["logits"], recF["logits"]) and rec["exp"][-1] == recF["exp_logits"]
        for i in range(len(layers)):
            assert np.array_equal(rec["dy"][i], recF["dy"][i]), ("dy", i)
            assert np.array_equal(rec["dw"][i], recF["dw"][i]), ("dw", i)
            assert np.array_equal(newW[i], newF[i]), ("w", i)
        Wf = newF


def test_the_sums_are_not_degenerate():
    """Over the skip nets' steps the forward sums align both ways and tie, the gradient sums at least two of
    the three, and no sum is all zero (so the alignment shifts of both operands are exercised)."""
    fwd, bwd = set(), set()
    for name in K.SKIP_NETS:
        for _, rec, _, _ in _ref(name)[4]:
            assert rec["sums"]
            for kind, _, ea, eb, zmax in rec["sums"]:
                assert zmax > 0, (name, kind)
                (fwd if kind == "fwd" else bwd).add((ea > eb) - (ea < eb))
    assert fwd == {-1, 0, 1}
    assert len(bwd) >= 2


@pytest.mark.parametrize("name", sorted(K.NETS))
def test_step_ref_trains_every_layer(name):
    layers, W, S, data, ref = _ref(name)
    for newW, rec, _, _ in ref:
        assert np.any(rec["logits"])
        assert all(np.any(d) for d in rec["dw"]) and all(np.any(d) for d in rec["dy"])
    assert all(not np.array_equal(a, b) for a, b in zip(W, ref[-1][0]))
    for i, l in enumerate(layers):  # a gpool's sums fill the int8 range after the requantisation
        if l["gpool"]:
            assert all(int(np.abs(rec["gp"][i][0]).max()) >= 64 for _, rec, _, _ in ref)


def test_without_the_new_keys_the_reference_is_strided_cases():
    layers = SC.derive(SC.NET_M)
    W, S = SC.init_weights(layers, seed=3)
    (x, labels), = SC.batches(layers, 3, 1, 1)
    a, ra = SC.chain_step_ref(layers, W, S, x, -3, labels)
    b, rb = K.chain_step_ref(K.derive(SC.NET_M), W, S, x, -3, labels)
    assert all(np.array_equal(u, v) for u, v in zip(a, b)) and np.array_equal(ra["logits"], rb["logits"])
    assert all(np.array_equal(u, v) for u, v in zip(ra["dy"], rb["dy"]))
