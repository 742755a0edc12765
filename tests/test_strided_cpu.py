"""Host-side checks of the strided chain layers (no device call anywhere here): the stride-2 depthwise
references against the direct triple-loop sums of the three formulas of include/niti_hip.h, the op-level
inputs' rule classes, niti_model_chain_check3's table and the older entry points' kept refusal, and the
spec / record forms."""
import ctypes as C
import json

import numpy as np
import pytest

import chain_cases as CC
import depthwise_cases as DC
import niti_oracle as O
import strided_cases as SC
from niti_amd._lib import INVALID_VALUE as INVALID, NOT_SUPPORT

OLD_NETS = ["LENET", "VGG11", "VGG16_32", "NET_A", "NET_B", "NET_C", "NET_D", "NET_D2", "NET_E", "NET_F", "NET_G"]


@pytest.fixture(scope="module")
def L():
    from niti_amd import _lib
    return _lib


# ------------------------------------------------------------------------------------ references
@pytest.mark.parametrize("sid", SC.SHAPE_IDS)
def test_refs_equal_the_direct_sums(sid):
    n, c, h, k, pad = SC.OP_SHAPES[sid]
    g = SC.geom_of(SC.OP_SHAPES[sid])
    x, dy, w = SC.wgrad_inputs(sid, "large")
    assert g.oh == g.ow == (h + 2 * pad - k) // 2 + 1 and dy.shape == (n, c, g.oh, g.oh)  # the oracle's geometry
    _, _, acc = SC.dw_fwd_ref(g, x, w)
    assert np.array_equal(acc, SC.dw2_fwd_direct(x, w, pad))
    _, _, dacc = SC.dw_dgrad_ref(g, dy, w)
    assert dacc.shape == x.shape and np.array_equal(dacc, SC.dw2_dgrad_direct(dy, w, pad, h))
    wacc, bw, _ = SC.dw_wgrad_ref(g, x, dy)
    assert wacc.shape == (c, 1, k, k) and np.array_equal(wacc, SC.dw2_wgrad_direct(x, dy, k, pad))
    assert bw == O.range_estimate(wacc)


def test_shape_b_has_a_row_and_column_no_output_reads():
    n, c, h, k, pad = SC.OP_SHAPES["B"]
    assert (h + 2 * pad - k) % 2 == 1
    for cls in SC.SHIFT_CLASSES:
        dy, w, _ = SC.act_inputs("B", cls, True)
        acc = SC.dw_dgrad_ref(SC.geom_of(SC.OP_SHAPES["B"]), dy, w)[2]
        assert not np.any(acc[:, :, 7, :]) and not np.any(acc[:, :, :, 7]) and np.any(acc[:, :, :7, :7])


def test_parity_classes_have_their_tap_counts():
    count = lambda k, pad: [len(SC.dgrad_taps(k, pad, py, px)) for py in (0, 1) for px in (0, 1)]  # noqa: E731
    assert sorted(count(3, 1), reverse=True) == [4, 2, 2, 1]
    assert sorted(count(5, 2), reverse=True) == [9, 6, 6, 4]
    for k in (3, 5):
        for pad in range(k):
            assert sum(count(k, pad)) == k * k


@pytest.mark.parametrize("sid", SC.SHAPE_IDS)
def test_op_inputs_hit_every_rule_class(sid):
    g = SC.geom_of(SC.OP_SHAPES[sid])
    for dgrad in (False, True):
        for cls in SC.SHIFT_CLASSES:
            a, w, mask = SC.act_inputs(sid, cls, dgrad)
            acc = SC.dw_dgrad_ref(g, a, w)[2] if dgrad else SC.dw_fwd_ref(g, a, w)[2]
            shift = O.range_estimate(acc) - 7
            assert {"le0": shift <= 0, "eq1": shift == 1, "gt1": shift > 1}[cls], (dgrad, cls, shift)
            assert np.any(acc != 0) and mask.shape == acc.shape
    want = {"bw0": lambda b: b == 0, "bw1": lambda b: b == 1, "bw2": lambda b: b == 2, "large": lambda b: b > 8}
    for cls in SC.WGRAD_CLASSES:
        x, dy, w = SC.wgrad_inputs(sid, cls)
        acc, bw, _ = SC.dw_wgrad_ref(g, x, dy)
        assert want[cls](bw), (cls, bw)
        for bits in (0, 2, 4):
            nw, _ = SC.dw_update_ref(w, acc, bits)
            assert (bits == 0 or cls == "bw0") == np.array_equal(nw, w), (cls, bits)


# ------------------------------------------------------------------------------------ the check
def _check(L, fn, layers, in_c, in_hw):
    """layers: (c_out, kernel, stride, pad, relu, pool, flatten, depthwise) each -> (code, shapes)."""
    arr = (L.ChainLayer2 * len(layers))()
    for a, l in zip(arr, layers):
        a.c_out, a.kernel, a.stride, a.pad, a.relu, a.pool, a.flatten, a.depthwise = l
    shapes = ((C.c_int * 8) * len(layers))()
    code = getattr(L.lib(), fn)(arr, len(layers), in_c, in_hw, shapes)
    return code, [list(s) for s in shapes]


def _check1(L, layers, in_c, in_hw):
    arr = (L.ChainLayer * len(layers))()
    for a, l in zip(arr, layers):
        a.c_out, a.kernel, a.stride, a.pad, a.relu, a.pool, a.flatten = l[:7]
    return L.lib().niti_model_chain_check(arr, len(layers), in_c, in_hw, None)


HEAD = (10, 1, 1, 0, 0, 0, 0, 0)
STEM = (16, 3, 1, 1, 1, 0, 0, 0)


def _oracle_shapes(layers, in_c, in_hw):
    """{c_in, c_out, k, pad, h_in, oh, out_h, flat_c} per layer from the oracle's geometry."""
    out, c, h = [], in_c, in_hw
    for co, k, s, pad, _, pool, flatten, dw in layers:
        co = c if dw else co
        g = O.geom(1, c, h, h, co, k, stride=s, pad=pad)
        ph = (g.oh - 2) // 2 + 1 if pool else g.oh
        fc = co * ph * ph if flatten else co
        out.append([c, co, k, pad, h, g.oh, 1 if flatten else ph, fc])
        c, h = fc, (1 if flatten else ph)
    return out


ACCEPTED = {
    "first_layer": ([(16, 3, 2, 1, 1, 0, 1, 0), HEAD], 3, 2),
    "first_layer_to_flatten": ([(16, 3, 2, 1, 1, 0, 1, 0), HEAD], 3, 16),
    "strided_1x1": ([STEM, (24, 1, 2, 0, 0, 0, 1, 0), HEAD], 3, 8),
    "strided_and_pool": ([STEM, (24, 3, 2, 0, 1, 1, 1, 0), HEAD], 3, 9),
    "depthwise_3x3": ([STEM, (0, 3, 2, 1, 1, 0, 1, 1), HEAD], 3, 8),
    "depthwise_5x5": ([STEM, (16, 5, 2, 2, 1, 0, 1, 1), HEAD], 3, 9),
    "depthwise_5x5_pad0_and_pool": ([STEM, (0, 5, 2, 0, 0, 1, 1, 1), HEAD], 3, 9),
    "odd_map_drops_a_row": ([STEM, (24, 3, 2, 0, 1, 0, 1, 0), HEAD], 3, 8),
}


@pytest.mark.parametrize("name", sorted(ACCEPTED))
def test_chain_check3_accepts_and_derives(L, name):
    layers, in_c, in_hw = ACCEPTED[name]
    code, shapes = _check(L, "niti_model_chain_check3", layers, in_c, in_hw)
    assert code == 0 and shapes == _oracle_shapes(layers, in_c, in_hw), name
    # the entry points that refuse stride != 1 still do
    assert _check(L, "niti_model_chain_check2", layers, in_c, in_hw)[0] == NOT_SUPPORT
    if not any(l[7] for l in layers):
        assert _check1(L, layers, in_c, in_hw) == NOT_SUPPORT


@pytest.mark.parametrize("name,layers,in_hw,want", [
    ("stride0", [(16, 3, 0, 1, 1, 0, 0, 0), HEAD], 1, INVALID),
    ("stride_negative", [STEM, (16, 3, -1, 1, 1, 0, 0, 0), HEAD], 1, INVALID),
    ("depthwise_stride0", [STEM, (0, 3, 0, 1, 1, 0, 0, 1), HEAD], 1, INVALID),
    ("stride3", [(16, 3, 3, 1, 1, 0, 0, 0), HEAD], 1, NOT_SUPPORT),
    ("depthwise_stride3", [STEM, (0, 3, 3, 1, 1, 0, 0, 1), HEAD], 1, NOT_SUPPORT),
    ("after_flatten", [(16, 3, 1, 1, 1, 0, 1, 0), (24, 1, 2, 0, 1, 0, 0, 0), HEAD], 1, NOT_SUPPORT),
    ("below_1x1", [STEM, (24, 5, 2, 0, 1, 0, 0, 0), HEAD], 4, INVALID),
    ("pool_below_2x2", [(16, 3, 2, 1, 1, 1, 0, 0), HEAD], 2, INVALID),
    # today's refusals hold through the new entry point
    ("depthwise_layer0", [(3, 3, 2, 1, 1, 0, 0, 1), HEAD], 1, NOT_SUPPORT),
    ("depthwise_kernel1", [STEM, (0, 1, 2, 0, 1, 0, 0, 1), HEAD], 1, NOT_SUPPORT),
    ("kernel8", [(16, 8, 2, 1, 1, 0, 0, 0), HEAD], 6, NOT_SUPPORT),
    ("map_left_at_the_head", [(16, 3, 2, 1, 1, 0, 0, 0), HEAD], 8, NOT_SUPPORT),
])
def test_chain_check3_refusals(L, name, layers, in_hw, want):
    assert _check(L, "niti_model_chain_check3", layers, 3, in_hw)[0] == want, name


@pytest.mark.parametrize("net", OLD_NETS)
def test_check3_agrees_with_check2_on_stride_1_lists(L, net):
    in_c, in_hw, spec = getattr(CC, net)
    new = [(co, k, 1, pad, relu, pool, fl, 0) for co, k, pad, relu, pool, fl in spec]
    assert _check(L, "niti_model_chain_check3", new, in_c, in_hw) == _check(L, "niti_model_chain_check2", new, in_c, in_hw)


@pytest.mark.parametrize("name", sorted(SC.NETS))
def test_chain_layers_of_the_test_nets(name):
    import niti_amd
    in_c, in_hw, spec = SC.NETS[name]
    got = niti_amd.chain_layers(spec, in_c, in_hw)
    want = SC.derive(SC.NETS[name])
    has_dw = any(l["dw"] for l in want)
    for g, l in zip(got, want):
        exp = {k: v for k, v in l.items() if k != "dw"}
        if has_dw:
            exp["depthwise"] = l["dw"]
        assert g == exp, name
    # the oracle's geometry under each layer's stride
    for l, nxt in zip(want, want[1:]):
        g = SC.layer_geom(1, l)
        ph = (g.oh - 2) // 2 + 1 if l["pool"] else g.oh
        assert nxt["h"] == (1 if l["flatten"] else ph)


# ------------------------------------------------------------------------------------ specs and records
@pytest.mark.parametrize("net", OLD_NETS)
def test_records_of_lists_without_a_stride_are_unchanged(net):
    from niti_amd import chain_layers, checkpoint, normalize_spec
    in_c, in_hw, spec = getattr(CC, net)
    want = [dict(c_out=l[0], kernel=l[1], pad=l[2], relu=l[3], pool=l[4], flatten=l[5]) for l in spec]
    assert normalize_spec(spec) == want
    assert normalize_spec([tuple(l) + (0, 1) for l in spec]) == want
    assert normalize_spec([{**d, "stride": 1} for d in want]) == want
    rec = checkpoint.chain_record(spec, in_c, in_hw)
    assert json.dumps(rec, sort_keys=True) == json.dumps({"spec": want, "in_c": in_c, "in_hw": in_hw}, sort_keys=True)
    assert all(set(l) == {"ci", "co", "k", "pad", "h", "relu", "pool", "flatten"} for l in chain_layers(spec, in_c, in_hw))


@pytest.mark.parametrize("name", sorted(DC.NETS))
def test_records_of_depthwise_lists_are_unchanged(name):
    from niti_amd import chain_layers, normalize_spec
    in_c, in_hw, spec = DC.NETS[name]
    norm = normalize_spec(spec)
    assert all(set(d) == {"c_out", "kernel", "pad", "relu", "pool", "flatten", "depthwise"} for d in norm)
    assert all("stride" not in l for l in chain_layers(spec, in_c, in_hw))


def test_a_strided_list_round_trips():
    from niti_amd import normalize_spec
    spec = SC.NET_M[2]
    norm = normalize_spec(spec)
    assert all(set(d) == {"c_out", "kernel", "pad", "relu", "pool", "flatten", "depthwise", "stride"} for d in norm)
    assert [d["stride"] for d in norm] == [2, 1, 1, 2, 1, 2, 1, 1]
    assert [d["c_out"] for d in norm] == [16, 16, 32, 32, 64, 64, 64, 10]
    assert normalize_spec(norm) == norm
    back = [tuple(d[k] for k in ("c_out", "kernel", "pad", "relu", "pool", "flatten", "depthwise", "stride")) for d in norm]
    assert normalize_spec(back) == norm
    as_dicts = [{k: v for k, v in d.items() if not (k == "stride" and v == 1) and not (k == "depthwise" and v == 0)}
                for d in norm]
    assert normalize_spec(as_dicts) == norm
    # strided, no depthwise layer: the stride key alone is added
    t = normalize_spec(SC.NET_T[2])
    assert all(set(d) == {"c_out", "kernel", "pad", "relu", "pool", "flatten", "stride"} for d in t)
    for bad in (0, -1):
        with pytest.raises(ValueError):
            normalize_spec([dict(c_out=16, kernel=3, stride=bad)])


def test_records_differ_in_a_stride(tmp_path):
    from niti_amd import checkpoint, mnn_snapshot
    in_c, in_hw, spec = SC.NET_T
    layers = SC.derive(SC.NET_T)
    W, S = SC.init_weights(layers, seed=3)
    rec = checkpoint.chain_record(spec, in_c, in_hw)
    # the stride moved from layer 1 to layer 2 (a pool dropped to keep the maps): the same weight shapes
    moved = [spec[0], spec[1][:7] + (1,), spec[2][:4] + (0,) + spec[2][5:7] + (2,), (64, 3, 1, 1, 1, 1, 0, 1), spec[4]]
    other = checkpoint.chain_record(moved, in_c, in_hw)
    assert [SC.weight_shape(l) for l in SC.derive((in_c, in_hw, moved))] == [SC.weight_shape(l) for l in layers]
    assert rec != other and rec["spec"][1]["stride"] == 2
    p, q = str(tmp_path / "s.safetensors"), str(tmp_path / "s.mnn")
    checkpoint.save_params(p, W, S, 5, in_hw=in_hw, chain=rec)
    mnn_snapshot.save(q, W, S, meta={"arch": 5, "in_hw": in_hw, "chain": rec})
    assert checkpoint.load_chain(p) == rec and mnn_snapshot.chain_of(mnn_snapshot.load(q)[2]) == rec
    for found in (checkpoint.load_chain(p), mnn_snapshot.chain_of(mnn_snapshot.load(q)[2])):
        with pytest.raises(ValueError):
            checkpoint.expect_chain(found, other, p)


# ------------------------------------------------------------------------------------ the step reference
@pytest.mark.parametrize("net", ["LENET", "NET_A", "NET_D"])
def test_step_ref_at_stride_1_equals_chain_step_ref(net):
    import niti_model_ref as R
    layers = CC.derive(getattr(CC, net))
    assert SC.derive(getattr(CC, net)) == [{**l, "dw": 0, "stride": 1} for l in layers]
    W, S = R.init_weights(layers, seed=23)
    Wa, Wb = W, W
    for x, labels in CC.batches(layers, 3, 2, seed=29):
        Wa, ra = CC.chain_step_ref(layers, Wa, S, x, -3, labels)
        Wb, rb = SC.chain_step_ref(SC.derive(getattr(CC, net)), Wb, S, x, -3, labels)
        assert np.array_equal(ra["logits"], rb["logits"]) and ra["exp"] == rb["exp"]
        for i in range(len(layers)):
            assert np.array_equal(Wa[i], Wb[i]), i


@pytest.mark.parametrize("name", sorted(SC.NETS))
def test_step_ref_trains_every_layer(name):
    layers = SC.derive(SC.NETS[name])
    W, S = SC.init_weights(layers, seed=3)
    steps = SC.ref_steps(layers, W, S, SC.batches(layers, 3, 2, seed=1))
    for (newW, rec, _, _) in steps:
        for i, l in enumerate(layers):
            assert rec["dw"][i].shape == SC.weight_shape(l) and newW[i].shape == SC.weight_shape(l)
    assert all(np.any(d != 0) for d in steps[0][1]["dw"]), name
