"""Host-side checks of the depthwise conv layers (no device call anywhere here): the tests' references
against the direct sums of the definition, the op-level inputs' rule classes, niti_model_chain_check2's
refusals and its agreement with the seven-field entry point, the chain step reference with such layers
against the one without, and the spec / snapshot record forms."""
import ctypes as C
import json

import numpy as np
import pytest

import chain_cases as CC
import depthwise_cases as DC
import niti_oracle as O
from niti_amd._lib import INVALID_VALUE as INVALID, NOT_SUPPORT

OLD_NETS = ["LENET", "VGG11", "NET_A", "NET_B", "NET_C", "NET_D", "NET_D2", "NET_E", "NET_F", "NET_G"]


@pytest.fixture(scope="module")
def L():
    from niti_amd import _lib
    return _lib


# ------------------------------------------------------------------------------------ references
@pytest.mark.parametrize("shape", DC.OP_SHAPES)
def test_refs_equal_the_direct_sums(shape):
    n, c, h, k, pad = shape
    g = DC.geom_of(shape)
    x, dy, w = DC.wgrad_inputs(shape, "large")
    assert g.oh == h + 2 * pad - k + 1 and dy.shape == (n, c, g.oh, g.oh)
    _, _, acc = DC.dw_fwd_ref(g, x, w)
    assert np.array_equal(acc, DC.dw_fwd_direct(x, w, pad))
    _, _, dacc = DC.dw_dgrad_ref(g, dy, w)
    assert np.array_equal(dacc, DC.dw_dgrad_direct(dy, w, pad, h))
    wacc, bw, _ = DC.dw_wgrad_ref(g, x, dy)
    assert wacc.shape == (c, 1, k, k) and np.array_equal(wacc, DC.dw_wgrad_direct(x, dy, k, pad))
    assert bw == O.range_estimate(wacc)


def test_diagonal_range_differs_from_the_dense_tensors():
    """What a dense emulation gets wrong: its range covers entries that are no parameters."""
    differ = []
    for shape in DC.OP_SHAPES:
        x, dy, _ = DC.wgrad_inputs(shape, "large")
        _, bw, bw_dense = DC.dw_wgrad_ref(DC.geom_of(shape), x, dy)
        assert bw <= bw_dense
        if bw != bw_dense:
            differ.append(shape)
    assert len(differ) >= 2, differ


@pytest.mark.parametrize("shape", DC.OP_SHAPES)
def test_op_inputs_hit_every_rule_class(shape):
    n, c, h, k, pad = shape
    g = DC.geom_of(shape)
    for dgrad in (False, True):
        for cls in DC.SHIFT_CLASSES:
            a, w, mask = DC.act_inputs(shape, cls, dgrad)
            acc = DC.dw_dgrad_ref(g, a, w)[2] if dgrad else DC.dw_fwd_ref(g, a, w)[2]
            shift = O.range_estimate(acc) - 7
            assert {"le0": shift <= 0, "eq1": shift == 1, "gt1": shift > 1}[cls], (dgrad, cls, shift)
            assert np.any(acc != 0) and np.any(mask > 0) and np.any(mask <= 0) and mask.shape == acc.shape
            if cls != "le0":  # the relu and the mask change something
                q = DC.requant_under(acc)[0]
                assert np.any(q < 0) and np.any(q[mask <= 0] != 0)
    want = {"bw0": lambda b: b == 0, "bw1": lambda b: b == 1, "bw2": lambda b: b == 2, "large": lambda b: b > 8}
    for cls in DC.WGRAD_CLASSES:
        x, dy, w = DC.wgrad_inputs(shape, cls)
        acc, bw, _ = DC.dw_wgrad_ref(g, x, dy)
        assert want[cls](bw), (cls, bw)
        for bits in (0, 2, 4):
            nw, g8 = DC.dw_update_ref(w, acc, bits)
            assert nw.shape == w.shape and (bits == 0 or cls == "bw0") == np.array_equal(nw, w), (cls, bits)


def test_requant_under_a_larger_range():
    acc = np.array([[-300, 5, 77, 290]], np.int32)
    q0, inc0 = DC.requant_under(acc)
    q1, inc1 = DC.requant_under(acc, 5000)
    assert inc1 > inc0 and q1.shape == acc.shape and np.max(np.abs(q1)) < np.max(np.abs(q0))
    assert np.array_equal(DC.requant_under(acc, 300)[0], q0)


# ------------------------------------------------------------------------------------ the check
def _check2(L, layers, in_c, in_hw):
    """layers: (c_out, kernel, stride, pad, relu, pool, flatten, depthwise) each -> (code, shapes)."""
    arr = (L.ChainLayer2 * len(layers))()
    for a, l in zip(arr, layers):
        a.c_out, a.kernel, a.stride, a.pad, a.relu, a.pool, a.flatten, a.depthwise = l
    shapes = ((C.c_int * 8) * len(layers))()
    code = L.lib().niti_model_chain_check2(arr, len(layers), in_c, in_hw, shapes)
    return code, [list(s) for s in shapes]


HEAD = (10, 1, 1, 0, 0, 0, 0, 0)
STEM = (16, 3, 1, 1, 1, 0, 0, 0)


@pytest.mark.parametrize("name,layers,in_hw,want", [
    ("flag2", [STEM, (16, 3, 1, 1, 1, 0, 0, 2), HEAD], 1, INVALID),
    ("flag_negative", [STEM, (16, 3, 1, 1, 1, 0, 0, -1), HEAD], 1, INVALID),
    ("c_out_other", [STEM, (24, 3, 1, 1, 1, 0, 0, 1), HEAD], 1, INVALID),
    ("c_out_negative", [STEM, (-1, 3, 1, 1, 1, 0, 0, 1), HEAD], 1, INVALID),
    ("pad_ge_kernel", [STEM, (0, 3, 1, 3, 1, 0, 0, 1), HEAD], 1, INVALID),
    ("layer0", [(3, 3, 1, 1, 1, 0, 0, 1), HEAD], 1, NOT_SUPPORT),
    ("layer0_c_out0", [(0, 3, 1, 1, 1, 0, 0, 1), HEAD], 1, NOT_SUPPORT),
    ("last", [STEM, (0, 3, 1, 1, 0, 0, 0, 1)], 1, NOT_SUPPORT),
    ("after_flatten", [(16, 3, 1, 1, 1, 0, 1, 0), (0, 3, 1, 1, 1, 0, 0, 1), HEAD], 1, NOT_SUPPORT),
    ("kernel1", [STEM, (0, 1, 1, 0, 1, 0, 0, 1), HEAD], 1, NOT_SUPPORT),
    ("kernel2", [STEM, (0, 2, 1, 1, 1, 0, 0, 1), HEAD], 1, NOT_SUPPORT),
    ("kernel7", [STEM, (0, 7, 1, 3, 1, 0, 0, 1), HEAD], 1, NOT_SUPPORT),
    ("stride2", [STEM, (0, 3, 2, 1, 1, 0, 0, 1), HEAD], 1, NOT_SUPPORT),
    ("dense_stride2_still", [(16, 3, 2, 1, 1, 0, 0, 0), HEAD], 1, NOT_SUPPORT),
    ("dense_c_out0_still", [(0, 3, 1, 1, 1, 0, 0, 0), HEAD], 1, INVALID),
])
def test_chain_check2_refusals(L, name, layers, in_hw, want):
    assert _check2(L, layers, 3, in_hw)[0] == want, name


def test_chain_check2_accepts_and_derives(L):
    # c_out 0 and c_out = c_in are the same layer; {c_in, c_out, k, pad, h_in, oh, out_h, flat_c}
    for co in (0, 16):
        code, shapes = _check2(L, [(16, 3, 1, 1, 1, 0, 0, 0), (co, 5, 1, 2, 1, 1, 1, 1), HEAD], 3, 9)
        assert code == 0
        assert shapes == [[3, 16, 3, 1, 9, 9, 9, 16], [16, 16, 5, 2, 9, 9, 1, 16 * 4 * 4], [256, 10, 1, 0, 1, 1, 1, 10]]
    import niti_amd
    for name, net in DC.NETS.items():
        got = niti_amd.chain_layers(net[2], net[0], net[1])
        want = DC.derive(net)
        assert [{**{k: v for k, v in l.items() if k != "dw"}, "depthwise": l["dw"]} for l in want] == got, name


@pytest.mark.parametrize("net", OLD_NETS)
def test_old_entry_points_agree_with_the_new(L, net):
    in_c, in_hw, spec = getattr(CC, net)
    old = (L.ChainLayer * len(spec))()
    new = [(co, k, 1, pad, relu, pool, fl, 0) for co, k, pad, relu, pool, fl in spec]
    for a, l in zip(old, new):
        a.c_out, a.kernel, a.stride, a.pad, a.relu, a.pool, a.flatten = l[:7]
    shapes = ((C.c_int * 8) * len(spec))()
    assert L.lib().niti_model_chain_check(old, len(spec), in_c, in_hw, shapes) == 0
    code, shapes2 = _check2(L, new, in_c, in_hw)
    assert code == 0 and [list(s) for s in shapes] == shapes2
    # and on a refusal: the same code
    old[0].stride = 2
    new[0] = new[0][:2] + (2,) + new[0][3:]
    assert L.lib().niti_model_chain_check(old, len(spec), in_c, in_hw, None) == _check2(L, new, in_c, in_hw)[0] == NOT_SUPPORT
    assert L.lib().niti_model_chain_check(None, len(spec), in_c, in_hw, None) == INVALID
    assert L.lib().niti_model_chain_check(old, 0, in_c, in_hw, None) == INVALID


# ------------------------------------------------------------------------------------ the step reference
@pytest.mark.parametrize("net", ["LENET", "NET_A", "NET_B", "NET_C", "NET_D", "NET_D2", "NET_E", "NET_F", "NET_G"])
def test_step_ref_without_depthwise_equals_chain_step_ref(net):
    import niti_model_ref as R
    layers = CC.derive(getattr(CC, net))
    assert DC.derive(getattr(CC, net)) == [{**l, "dw": 0} for l in layers]
    W, S = R.init_weights(layers, seed=23)
    Wa, Wb = W, W
    for x, labels in CC.batches(layers, 3, 2, seed=29):
        Wa, ra = CC.chain_step_ref(layers, Wa, S, x, -3, labels)
        Wb, rb = DC.dw_chain_step_ref(DC.derive(getattr(CC, net)), Wb, S, x, -3, labels)
        assert np.array_equal(ra["logits"], rb["logits"]) and ra["exp"] == rb["exp"]
        for key in ("inp", "y", "r", "dw", "dy"):
            for i in range(len(layers)):
                assert np.array_equal(ra[key][i], rb[key][i]), (key, i)
        for i in range(len(layers)):
            assert np.array_equal(Wa[i], Wb[i]), i


@pytest.mark.parametrize("name", sorted(DC.NETS))
def test_step_ref_with_depthwise_runs_and_trains_every_layer(name):
    layers = DC.derive(DC.NETS[name])
    W, S = DC.init_weights(layers, seed=3)
    for l, w in zip(layers, W):
        assert w.shape == DC.weight_shape(l) and (w.shape[1] == 1) == bool(l["dw"] or l["ci"] == 1)
    data = DC.batches(layers, 3, 2, seed=1)
    steps = DC.ref_steps(layers, W, S, data)
    for (newW, rec, _, _) in steps:
        for i, l in enumerate(layers):
            assert rec["dw"][i].shape == DC.weight_shape(l) and newW[i].shape == DC.weight_shape(l)
    assert all(np.any(d != 0) for d in steps[0][1]["dw"])
    # a frozen depthwise layer keeps its weights; 4 bits move it differently from 2
    dw = [i for i, l in enumerate(layers) if l["dw"]]
    bits = [2] * len(layers)
    bits[dw[0]] = 0
    bits[dw[-1]] = 4
    frozen = DC.ref_steps(layers, W, S, data[:1], bits=bits)[0]
    assert np.array_equal(frozen[0][dw[0]], W[dw[0]]) and not np.any(frozen[1]["dw"][dw[0]])
    if len(dw) > 1 and frozen[1]["bw"][dw[-1]] > 2:
        assert not np.array_equal(frozen[1]["dw"][dw[-1]], steps[0][1]["dw"][dw[-1]])


# ------------------------------------------------------------------------------------ specs and records
def test_normalize_spec_round_trips():
    from niti_amd import normalize_spec
    spec = DC.NET_S[2]
    norm = normalize_spec(spec)
    assert all(set(d) == {"c_out", "kernel", "pad", "relu", "pool", "flatten", "depthwise"} for d in norm)
    assert [d["c_out"] for d in norm] == [16, 16, 24, 24, 40, 10]  # a depthwise layer's 0: its input's channels
    assert [d["depthwise"] for d in norm] == [0, 1, 0, 1, 0, 0]
    assert normalize_spec(norm) == norm  # dicts in, the same dicts out
    # c_out given, left out of a dict, or 0: one spec
    as_dicts = [dict(kernel=l[1], pad=l[2], relu=l[3], pool=l[4], flatten=l[5], depthwise=1) if l[6] else
                dict(c_out=l[0], kernel=l[1], pad=l[2], relu=l[3], pool=l[4], flatten=l[5]) for l in spec]
    assert normalize_spec(as_dicts) == norm
    assert normalize_spec([(16, 3, 1, 1, 0, 0, 0), (16, 3, 1, 1, 0, 0, 1)] + list(spec[2:])) == norm
    with pytest.raises(ValueError):
        normalize_spec([dict(kernel=3)])  # c_out may be left out of a depthwise layer only
    with pytest.raises(ValueError):
        normalize_spec([(16, 3, 1, 1, 0, 0, 0, 0)])  # eight entries


@pytest.mark.parametrize("net", OLD_NETS + ["VGG16_32"])
def test_records_of_lists_without_depthwise_are_unchanged(net, tmp_path):
    """Byte for byte what they were: no `depthwise` key anywhere, in either snapshot's record."""
    from niti_amd import checkpoint, normalize_spec
    in_c, in_hw, spec = getattr(CC, net)
    want = [dict(c_out=l[0], kernel=l[1], pad=l[2], relu=l[3], pool=l[4], flatten=l[5]) for l in spec]
    assert normalize_spec(spec) == want
    assert normalize_spec([tuple(l) + (0,) for l in spec]) == want and normalize_spec([{**d, "depthwise": 0} for d in want]) == want
    rec = checkpoint.chain_record(spec, in_c, in_hw)
    assert json.dumps(rec, sort_keys=True) == json.dumps({"spec": want, "in_c": in_c, "in_hw": in_hw}, sort_keys=True)


def test_records_differ_in_a_depthwise_flag(tmp_path):
    from niti_amd import checkpoint, mnn_snapshot
    in_c, in_hw, spec = DC.NET_S
    layers = DC.derive(DC.NET_S)
    W, S = DC.init_weights(layers, seed=3)
    rec = checkpoint.chain_record(spec, in_c, in_hw)
    dense = [l[:6] + (0,) if l[6] else l for l in [(16 if i == 1 else 24 if i == 3 else l[0],) + l[1:] for i, l in enumerate(spec)]]
    other = checkpoint.chain_record(dense, in_c, in_hw)
    assert rec != other and "depthwise" in rec["spec"][0] and "depthwise" not in other["spec"][0]
    p, q = str(tmp_path / "s.safetensors"), str(tmp_path / "s.mnn")
    checkpoint.save_params(p, W, S, 5, in_hw=in_hw, chain=rec)
    mnn_snapshot.save(q, W, S, meta={"arch": 5, "in_hw": in_hw, "chain": rec})
    assert checkpoint.load_chain(p) == rec and mnn_snapshot.chain_of(mnn_snapshot.load(q)[2]) == rec
    got, _, _ = checkpoint.load_params(p)
    assert [w.shape for w in got] == [DC.weight_shape(l) for l in layers]
    assert all(np.array_equal(a, b) for a, b in zip(mnn_snapshot.load(q)[0], W))
    for found in (checkpoint.load_chain(p), mnn_snapshot.chain_of(mnn_snapshot.load(q)[2])):
        with pytest.raises(ValueError):
            checkpoint.expect_chain(found, other, p)
