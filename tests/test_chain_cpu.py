"""Host-side checks of the user-defined chain networks (no device call anywhere here):
niti_model_chain_check's refusals and derived shapes, the tests' own oracle step for un-pooled
flattens pinned to the oracle's, the product-side initialiser against the oracle's, and the chain
record in both snapshot formats."""
import ctypes as C

import numpy as np
import pytest

import chain_cases as CC
from niti_amd._lib import INVALID_VALUE as INVALID, NOT_SUPPORT


@pytest.fixture(scope="module")
def L():
    from niti_amd import _lib
    return _lib


def _check(L, layers, in_c, in_hw, n=None, null=False):
    """layers: (c_out, kernel, stride, pad, relu, pool, flatten) each; returns (code, shapes)."""
    arr = (L.ChainLayer * max(1, len(layers)))()
    for a, l in zip(arr, layers):
        a.c_out, a.kernel, a.stride, a.pad, a.relu, a.pool, a.flatten = l
    n = len(layers) if n is None else n
    shapes = ((C.c_int * 8) * max(1, len(layers)))()
    code = L.lib().niti_model_chain_check(None if null else arr, n, in_c, in_hw, shapes)
    return code, [list(s) for s in shapes]


OK_HEAD = (10, 1, 1, 0, 0, 0, 0)


@pytest.mark.parametrize("name,layers,in_c,in_hw,kw,want", [
    ("null", [OK_HEAD], 3, 1, dict(null=True), INVALID),
    ("n0", [OK_HEAD], 3, 1, dict(n=0), INVALID),
    ("in_c0", [OK_HEAD], 0, 1, {}, INVALID),
    ("in_hw0", [OK_HEAD], 3, 0, {}, INVALID),
    ("c_out0", [(0, 1, 1, 0, 0, 0, 0)], 3, 1, {}, INVALID),
    ("kernel0", [(10, 0, 1, 0, 0, 0, 0)], 3, 1, {}, INVALID),
    ("pad_negative", [(10, 1, 1, -1, 0, 0, 0)], 3, 1, {}, INVALID),
    ("pad_ge_kernel", [(10, 3, 1, 3, 0, 0, 0)], 3, 1, {}, INVALID),
    ("conv_below_1x1", [(10, 3, 1, 0, 0, 0, 0)], 3, 2, {}, INVALID),
    ("pool_on_1x1", [(8, 1, 1, 0, 1, 1, 0), OK_HEAD], 3, 1, {}, INVALID),
    ("n25", [(8, 1, 1, 0, 1, 0, 0)] * 24 + [OK_HEAD], 3, 1, {}, NOT_SUPPORT),
    ("stride2", [(8, 3, 2, 1, 1, 0, 0), OK_HEAD], 3, 1, {}, NOT_SUPPORT),
    ("kernel8", [(8, 8, 1, 0, 1, 0, 0), OK_HEAD], 3, 8, {}, NOT_SUPPORT),
    ("classes2049", [(2049, 1, 1, 0, 0, 0, 0)], 3, 1, {}, NOT_SUPPORT),
    ("last_pools", [(10, 3, 1, 1, 0, 1, 0)], 3, 2, {}, NOT_SUPPORT),
    ("last_flattens", [(10, 1, 1, 0, 0, 0, 1)], 3, 1, {}, NOT_SUPPORT),
    ("last_out_h2", [(10, 3, 1, 1, 0, 0, 0)], 3, 2, {}, NOT_SUPPORT),
    ("k3_after_flatten", [(8, 3, 1, 1, 1, 0, 1), (8, 3, 1, 1, 1, 0, 0), OK_HEAD], 3, 4, {}, NOT_SUPPORT),
    ("k2_pad1_after_flatten", [(8, 3, 1, 1, 1, 0, 1), (10, 2, 1, 1, 0, 0, 0)], 3, 4, {}, NOT_SUPPORT),
    ("tensor_past_2_29", [(64, 3, 1, 1, 1, 0, 0)] + [(8, 1, 1, 0, 1, 1, 0)] * 12 + [OK_HEAD], 4, 4096, {}, NOT_SUPPORT),
    ("weights_past_2_29", [(40000, 1, 1, 0, 1, 0, 0), (40000, 1, 1, 0, 1, 0, 0), OK_HEAD], 3, 1, {}, NOT_SUPPORT),
    # sizes whose products pass 2^63: refused, not wrapped
    ("products_past_int64", [(256, 1, 1, 0, 1, 1, 1), OK_HEAD], 64, 1 << 29, {}, NOT_SUPPORT),
    ("c_out_past_int", [(2 ** 31 - 1, 1, 1, 0, 1, 0, 0), OK_HEAD], 3, 1, {}, NOT_SUPPORT),
    ("fused_input_too_wide", [(8, 3, 1, 1, 1, 1, 0)] + [(8, 1, 1, 0, 1, 1, 0)] * 10 + [OK_HEAD], 3, 2729, {},
     NOT_SUPPORT),
])
def test_chain_check_refusals(L, name, layers, in_c, in_hw, kw, want):
    code, _ = _check(L, layers, in_c, in_hw, **kw)
    assert code == want, name


def test_chain_check_accepts_24_layers_and_kernel_7(L):
    assert _check(L, [(8, 1, 1, 0, 1, 0, 0)] * 23 + [OK_HEAD], 3, 1)[0] == 0
    assert _check(L, [(8, 7, 1, 3, 1, 0, 0), (10, 7, 1, 0, 0, 0, 0)], 3, 7)[0] == 0
    # (the widest input the fused first-layer pass takes; one pixel more is refused above)
    assert _check(L, [(8, 3, 1, 1, 1, 1, 0)] + [(8, 1, 1, 0, 1, 1, 0)] * 10 + [OK_HEAD], 3, 2728)[0] == 0
    # an over-padded fused-shape first layer (2 pad >= kernel) is taken, by the unfused input path, and
    # so is not bound by the fused pass's LDS rows
    assert _check(L, [(8, 3, 1, 2, 1, 1, 0)] + [(8, 1, 1, 0, 1, 1, 0)] * 10 + [OK_HEAD], 3, 2729)[0] == 0
    assert _check(L, [(8, 5, 1, 4, 1, 0, 0), (10, 5, 1, 0, 0, 0, 0)], 1, 1)[0] == 0
    code, shapes = _check(L, [(8, 3, 1, 1, 1, 1, 1), OK_HEAD], 5, 9)
    # {c_in, c_out, k, pad, h_in, oh, out_h, flat_c}
    assert code == 0 and shapes == [[5, 8, 3, 1, 9, 9, 1, 8 * 4 * 4], [128, 10, 1, 0, 1, 1, 1, 10]]


def test_python_refusals():
    import niti_amd
    from niti_amd._lib import NitiError  # (looked up now: a test that reloads the module leaves a new class)
    with pytest.raises(ValueError):
        niti_amd.chain_layers([(10, 3, 3)], 3, 1)          # pad >= kernel: malformed
    with pytest.raises(ValueError):
        niti_amd.chain_layers([], 3, 1)
    with pytest.raises(ValueError):
        niti_amd.chain_layers([dict(c_out=10)], 3, 1)     # no kernel
    with pytest.raises(NitiError) as e:
        niti_amd.chain_layers([(2049, 1)], 3, 1)
    assert e.value.code == NOT_SUPPORT


@pytest.mark.parametrize("net,ref", [("LENET", "lenet_layers"), ("VGG11", "vgg11_layers"), ("VGG16_32", "vgg16_layers")])
def test_derived_shapes_equal_the_oracle_lists(net, ref):
    import niti_amd
    import niti_model_ref as R
    in_c, in_hw, spec = getattr(CC, net)
    want = R.vgg16_layers(32) if net == "VGG16_32" else getattr(R, ref)()
    got = niti_amd.chain_layers(spec, in_c, in_hw)
    assert got == want
    assert CC.derive(getattr(CC, net)) == want  # (the tests' own derivation, used where no library is)
    # dict and tuple specs are the same spec
    as_dicts = [dict(c_out=l[0], kernel=l[1], pad=l[2], relu=l[3], pool=l[4], flatten=l[5]) for l in spec]
    assert niti_amd.chain_layers(as_dicts, in_c, in_hw) == want


@pytest.mark.parametrize("net", ["LENET", "NET_A", "NET_B", "NET_C", "NET_E", "NET_F", "NET_G"])
def test_chain_step_ref_equals_the_oracle_step(net):
    """Two steps at batch 4: every record field and every weight."""
    import niti_model_ref as R
    layers = CC.derive(getattr(CC, net))
    classes = layers[-1]["co"]
    W, S = R.init_weights(layers, seed=23)
    Wa, Wb = W, W
    for x, labels in CC.batches(layers, 4, 2, seed=29):
        Wa, ra = R.train_step(layers, Wa, S, x, -3, labels, classes=classes)
        Wb, rb = CC.chain_step_ref(layers, Wb, S, x, -3, labels)
        assert np.array_equal(ra["logits"], rb["logits"]) and ra["exp"] == rb["exp"]
        for key in ("inp", "y", "r", "dw", "dy"):
            for i in range(len(layers)):
                assert np.array_equal(ra[key][i], rb[key][i]), (key, i)
        for i in range(len(layers)):
            assert (ra["p"][i] is None) == (rb["p"][i] is None)
            assert ra["p"][i] is None or np.array_equal(ra["p"][i], rb["p"][i])
            assert np.array_equal(Wa[i], Wb[i]), i
        assert any(np.any(d != 0) for d in rb["dw"])


def test_chain_step_ref_runs_an_unpooled_flatten():
    import niti_model_ref as R
    for net in (CC.NET_D, CC.NET_D2):
        layers = CC.derive(net)
        W, S = R.init_weights(layers, seed=3)
        (x, labels), = CC.batches(layers, 4, 1, seed=4)
        newW, rec = CC.chain_step_ref(layers, W, S, x, -3, labels)
        fl = [i for i, l in enumerate(layers) if l["flatten"]][0]
        assert rec["dy"][fl].shape == rec["r"][fl].shape and rec["inp"][fl + 1].shape[2:] == (1, 1)
        # the flatten's order: channel-major over the map, index (c * h + y) * w + x
        assert np.array_equal(rec["inp"][fl + 1].reshape(rec["r"][fl].shape), rec["r"][fl])
        assert all(np.any(d != 0) for d in rec["dw"])


@pytest.mark.parametrize("shape", [(20, 6, 5, 5), (36, 1440, 1, 1), (1, 1, 1, 1)])
def test_xavier_int8_equals_the_oracle_initialiser(shape):
    import niti_oracle as O
    from niti_amd.init import xavier_int8
    for seed in (0, 7):
        w, s = xavier_int8(shape, np.random.default_rng(seed))
        wo, so = O.synth_w(np.random.default_rng(seed), shape)
        assert w.dtype == np.int8 and w.shape == shape and np.array_equal(w, wo) and s == so
    with pytest.raises(ValueError):
        xavier_int8((3, 3), np.random.default_rng(0))


def _arrays(layers, seed):
    from niti_amd.init import xavier_int8
    rng = np.random.default_rng(seed)
    ws = [xavier_int8((l["co"], l["ci"], l["k"], l["k"]), rng) for l in layers]
    return [w for w, _ in ws], [s for _, s in ws]


def test_chain_record_round_trips_through_both_snapshots(tmp_path):
    import niti_amd
    from niti_amd import checkpoint, mnn_snapshot
    in_c, in_hw, spec = CC.NET_A
    W, S = _arrays(CC.derive(CC.NET_A), 5)
    rec = checkpoint.chain_record(spec, in_c, in_hw)
    other = checkpoint.chain_record(CC.NET_A[2][:-1] + [(21, 1, 0, 0, 0, 0)], in_c, in_hw)
    assert rec != other and rec == checkpoint.chain_record([dict(c_out=l[0], kernel=l[1], pad=l[2], relu=l[3],
                                                                 pool=l[4], flatten=l[5]) for l in spec], in_c, in_hw)
    # safetensors
    p = str(tmp_path / "a.safetensors")
    checkpoint.save_params(p, W, S, niti_amd.ARCH_CHAIN, in_hw=in_hw, chain=rec)
    w2, s2, arch = checkpoint.load_params(p)
    assert arch == niti_amd.ARCH_CHAIN and s2 == S and all(np.array_equal(a, b) for a, b in zip(W, w2))
    assert checkpoint.load_chain(p) == rec
    checkpoint.expect_chain(checkpoint.load_chain(p), rec, p)
    with pytest.raises(ValueError):
        checkpoint.expect_chain(checkpoint.load_chain(p), other, p)
    with pytest.raises(ValueError):  # another input is another network
        checkpoint.expect_chain(checkpoint.load_chain(p), checkpoint.chain_record(spec, in_c, in_hw + 1), p)
    # .mnn + side-car
    q = str(tmp_path / "a.mnn")
    mnn_snapshot.save(q, W, S, meta={"arch": niti_amd.ARCH_CHAIN, "in_hw": in_hw, "chain": rec})
    w3, s3, meta = mnn_snapshot.load(q)
    assert s3 == S and all(np.array_equal(a, b) for a, b in zip(W, w3))
    assert mnn_snapshot.chain_of(meta) == rec
    with pytest.raises(ValueError):
        checkpoint.expect_chain(mnn_snapshot.chain_of(meta), other, q)


def test_builtin_snapshots_are_unchanged(tmp_path):
    """No chain record: the file holds exactly the metadata it always did, and reads back."""
    import json

    import niti_amd
    import niti_model_ref as R
    from niti_amd import checkpoint, mnn_snapshot
    from safetensors import safe_open
    W, S = _arrays(R.lenet_layers(), 6)
    p = str(tmp_path / "l.safetensors")
    checkpoint.save_params(p, W, S, niti_amd.ARCH_LENET, in_hw=28)
    with safe_open(p, framework="numpy") as f:
        assert f.metadata() == {"format": checkpoint.FORMAT, "arch": "1", "num_layers": "4", "in_hw": "28"}
    assert checkpoint.load_chain(p) is None
    w2, s2, arch = checkpoint.load_params(p)
    assert arch == niti_amd.ARCH_LENET and s2 == S and all(np.array_equal(a, b) for a, b in zip(W, w2))
    checkpoint.expect_chain(None, None, p)  # a built-in model asks for no record
    with pytest.raises(ValueError):        # a chain model refuses a snapshot without one
        checkpoint.expect_chain(None, checkpoint.chain_record(CC.LENET[2], 1, 28), p)
    q = str(tmp_path / "l.mnn")
    mnn_snapshot.save(q, W, S, meta={"arch": niti_amd.ARCH_LENET, "in_hw": 28})
    assert json.load(open(q + ".wscale.json")) == {"format": "niti-mnn-snapshot-wscale", "wscale": S, "arch": 1,
                                                   "in_hw": 28}
    assert mnn_snapshot.chain_of(mnn_snapshot.load(q)[2]) is None


def test_symbols_are_exported(L):
    import niti_amd
    assert niti_amd.ARCH_CHAIN == 5
    names = L.header_functions()
    assert "niti_model_chain_check" in names and "niti_model_create_chain" in names
    for n in ("niti_model_chain_check", "niti_model_create_chain"):
        getattr(L.lib(), n)
    assert callable(niti_amd.chain_layers)
