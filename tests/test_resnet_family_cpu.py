"""Host-side checks of the user-defined residual networks (no device call anywhere here):
niti_model_resnet_check's refusals and derived shapes, the tests' own oracle step with an optional
stem pool pinned to the oracle's ResNet step, the properties every GPU case relies on (no overflow,
non-zero logits, no all-zero weight gradient), and the spec record in both snapshot formats."""
import ctypes as C

import numpy as np
import pytest

import resnet_family_cases as FC
from niti_amd._lib import INVALID_VALUE as INVALID, NOT_SUPPORT


@pytest.fixture(scope="module")
def L():
    from niti_amd import _lib
    return _lib


BASE = dict(in_c=3, stem_kernel=7, stem_stride=2, stem_pad=3, stem_pool=1, width=64, n_stages=4, depths=(2, 2, 2, 2),
            classes=10)
CIFAR = dict(BASE, stem_kernel=3, stem_stride=1, stem_pad=1, stem_pool=0)


def _check(L, in_hw=32, null=False, **kw):
    f = dict(BASE, **kw)
    cs = L.ResnetSpec()
    for k, v in f.items():
        if k != "depths":
            setattr(cs, k, v)
    for i, d in enumerate(f["depths"]):
        cs.depths[i] = d
    n = C.c_int(-1)
    shapes = ((C.c_int * 8) * L.RESNET_MAX_LAYERS)()
    code = L.lib().niti_model_resnet_check(None if null else C.byref(cs), in_hw, C.byref(n), shapes)
    return code, n.value, [list(s) for s in shapes[:max(n.value, 0)]]


@pytest.mark.parametrize("name,kw,want", [
    ("null", dict(null=True), INVALID),
    ("in_hw0", dict(in_hw=0), INVALID),
    ("in_c0", dict(in_c=0), INVALID),
    ("stem_kernel0", dict(stem_kernel=0, stem_pad=0), INVALID),
    ("stem_stride0", dict(stem_stride=0), INVALID),
    ("stem_pad_negative", dict(stem_pad=-1), INVALID),
    ("stem_pad_ge_kernel", dict(stem_pad=7), INVALID),
    ("stem_pool2", dict(stem_pool=2), INVALID),
    ("width0", dict(width=0), INVALID),
    ("n_stages0", dict(n_stages=0), INVALID),
    ("n_stages9", dict(n_stages=9), INVALID),
    ("depth0", dict(depths=(2, 0, 2, 2)), INVALID),
    ("classes0", dict(classes=0), INVALID),
    ("stem_below_1x1", dict(stem_pad=0, in_hw=6), INVALID),
    ("in_c5", dict(in_c=5), NOT_SUPPORT),
    # 37 * 37 * 3 = 4107 columns (its one output row's 37 * 37 * 3 staged bytes fit in LDS)
    ("stem_columns_past_4096", dict(stem_kernel=37, stem_stride=1, stem_pad=0, in_hw=37), NOT_SUPPORT),
    # 7 rows of (800 - 1) * 2 + 7 pixels of 3 bytes = 33705 > 16384
    ("stem_rows_past_lds", dict(in_hw=1600), NOT_SUPPORT),
    ("classes2049", dict(classes=2049), NOT_SUPPORT),
    ("layers257", dict(n_stages=1, depths=(128,)), NOT_SUPPORT),  # 2 + 2 * 128 = 258
    # a 1800-px map of 256 channels: 829 M elements (the stem's 3 * 1802 * 3 staged bytes fit)
    ("tensor_past_2_29", dict(CIFAR, width=256, in_hw=1800), NOT_SUPPORT),
    ("width_1_shl_30", dict(width=1 << 30, n_stages=3, depths=(1, 1, 1)), NOT_SUPPORT),
    ("products_past_int64", dict(CIFAR, width=2 ** 31 - 1, n_stages=8, depths=(1,) * 8, in_hw=1800), NOT_SUPPORT),
])
def test_resnet_check_refusals(L, name, kw, want):
    code, n, _ = _check(L, **kw)
    assert code == want and n == -1, name


def test_resnet_check_accepts_the_edges(L):
    assert _check(L, n_stages=1, depths=(127,))[:2] == (0, 256)          # the layer cap itself
    assert _check(L, in_hw=224, classes=2048)[:2] == (0, 21)
    assert _check(L, in_hw=33)[0] == 0                                   # no multiple of 16 asked for
    assert _check(L, in_c=4, stem_kernel=31, stem_stride=1, stem_pad=0, in_hw=31)[0] == 0  # 3844 -> 3872 columns
    assert _check(L, n_stages=8, depths=(1,) * 8, width=8)[0] == 0
    # ignored: depths past n_stages
    assert _check(L, n_stages=2, depths=(1, 1, 0, -5))[:2] == (0, 7)
    code, n, sh = _check(L, in_hw=32, **dict(CIFAR, n_stages=2, depths=(1, 1), width=16, in_c=1))
    # {c_in, c_out, k, stride, pad, h_in, oh, relu}
    assert code == 0 and sh == [[1, 16, 3, 1, 1, 32, 32, 1], [16, 16, 3, 1, 1, 32, 32, 1], [16, 16, 3, 1, 1, 32, 32, 0],
                                [16, 32, 3, 2, 1, 32, 16, 1], [32, 32, 3, 1, 1, 16, 16, 0], [16, 32, 1, 2, 0, 32, 16, 0],
                                [32, 10, 1, 1, 0, 1, 1, 0]]


def test_python_refusals():
    import niti_amd
    from niti_amd._lib import NitiError
    with pytest.raises(ValueError):
        niti_amd.resnet_layers(dict(depths=(1,), classes=10, stem=(3, 1, 3, 0)), 32)   # pad >= kernel: malformed
    with pytest.raises(ValueError):
        niti_amd.resnet_layers(dict(depths=(), classes=10), 32)
    with pytest.raises(ValueError):
        niti_amd.resnet_layers(dict(depths=(1,)), 32)                                  # no classes
    with pytest.raises(ValueError):
        niti_amd.resnet_layers(dict(depths=(1,), classes=10, stem="mnist"), 32)
    with pytest.raises(ValueError):
        niti_amd.resnet_layers(dict(depths=(1,), classes=10, blocks=3), 32)            # an unknown key
    with pytest.raises(NitiError) as e:
        niti_amd.resnet_layers(dict(depths=(1,), classes=2049), 32)
    assert e.value.code == NOT_SUPPORT
    a = niti_amd.normalize_resnet_spec(depths=(3, 3, 3), width=16, classes=10, stem="cifar")
    assert a == niti_amd.normalize_resnet_spec(dict(depths=[3, 3, 3], width=16, classes=10, stem=(3, 1, 1, 0), in_c=3))
    assert a == {"in_c": 3, "stem": [3, 1, 1, 0], "width": 16, "depths": [3, 3, 3], "classes": 10}
    assert niti_amd.normalize_resnet_spec(depths=(2,), classes=5)["stem"] == [7, 2, 3, 1]


@pytest.mark.parametrize("hw", [32, 64, 224])
def test_resnet18_spec_equals_the_oracle_list(hw):
    import niti_amd
    import niti_resnet_ref as RR
    want = RR.resnet18_convs(hw, 1000)
    assert niti_amd.resnet_layers(dict(FC.RESNET18, classes=1000), hw) == want
    assert FC.family_convs(dict(FC.RESNET18, classes=1000), hw) == want


@pytest.mark.parametrize("name", list(FC.CASES))
def test_derived_layers_of_every_case(name):
    import niti_amd
    import niti_resnet_ref as RR
    spec, in_hw, _, _ = FC.CASES[name]
    got = niti_amd.resnet_layers(spec, in_hw)
    assert got == FC.family_convs(spec, in_hw) and len(got) == FC.N_LAYERS[name]
    n_blocks = sum(spec["depths"])
    assert len(RR.blocks(got)) == n_blocks
    assert sum(l["name"].endswith("proj") for l in got) == len(spec["depths"]) - 1


def test_derived_sizes():
    import niti_amd
    sizes = lambda name: [(l["ci"], l["co"], l["stride"], l["h"]) for l in niti_amd.resnet_layers(*FC.CASES[name][:2])]  # noqa: E731
    # odd maps: 48 -> conv1 24 -> pool 12 -> 6 -> 3
    assert sizes("odd_maps_w16") == [(3, 16, 2, 48), (16, 16, 1, 12), (16, 16, 1, 12), (16, 16, 1, 12), (16, 16, 1, 12),
                                     (16, 32, 2, 12), (32, 32, 1, 6), (16, 32, 2, 12), (32, 64, 2, 6), (64, 64, 1, 3),
                                     (32, 64, 2, 6), (64, 7, 1, 1)]
    assert sizes("one_stage_w48") == [(3, 48, 2, 32), (48, 48, 1, 8), (48, 48, 1, 8), (48, 10, 1, 1)]
    assert sizes("two_stage_w32")[-1] == (64, 20, 1, 1) and sizes("two_stage_w32")[-2] == (64, 64, 1, 4)
    s34 = sizes("resnet34")
    assert len(s34) == 37 and s34[-1] == (512, 10, 1, 1) and [s[1] for s in s34].count(256) == 13
    assert sizes("cifar_resnet20")[1] == (16, 16, 1, 32) and sizes("cifar_gray_images")[0] == (1, 32, 1, 28)


@pytest.mark.parametrize("name", FC.POOLED)
def test_family_step_ref_equals_the_oracle_step(name):
    """The restatement, pooled stem, against RR.train_step over the case's two steps: logits,
    exponent, every fwd / exp / dy / dw and the new weights."""
    import niti_resnet_ref as RR
    spec, in_hw, batch, _ = FC.CASES[name]
    convs, W, S, steps = FC.reference(name)
    for data, labels, x, e, newW, rec in steps:
        wantW, want = RR.train_step(convs, W, S, x, e, labels, classes=spec["classes"])
        assert rec["exp_logits"] == want["exp_logits"] and np.array_equal(rec["logits"], want["logits"])
        for i, c in enumerate(convs):
            assert rec["exp"][i] == want["exp"][i], c["name"]
            for key in ("fwd", "dy", "dw"):
                assert np.array_equal(rec[key][i], want[key][i]), (key, c["name"])
            assert np.array_equal(newW[i], wantW[i]), c["name"]
        W = wantW


@pytest.mark.parametrize("name", list(FC.CASES))
def test_every_case_exercises_every_layer(name):
    """What the GPU comparison needs of a case for it to mean anything (the oracle's overflow
    counter is asserted inside the step)."""
    convs, _, _, steps = FC.reference(name)
    for _, _, _, _, _, rec in steps:
        assert np.any(rec["logits"] != 0)
    rec = steps[-1][5]
    assert all(np.any(rec["dw"][i] != 0) for i in range(len(convs)))


def _arrays(layers, seed):
    from niti_amd.init import xavier_int8
    rng = np.random.default_rng(seed)
    ws = [xavier_int8((l["co"], l["ci"], l["k"], l["k"]), rng) for l in layers]
    return [w for w, _ in ws], [s for _, s in ws]


def test_resnet_record_round_trips_through_both_snapshots(tmp_path):
    import json

    import niti_amd
    from niti_amd import checkpoint, mnn_snapshot
    from safetensors import safe_open
    spec, in_hw, _, _ = FC.CASES["cifar_gray_images"]
    W, S = _arrays(FC.family_convs(spec, in_hw), 5)
    rec = checkpoint.resnet_record(spec, in_hw)
    other = checkpoint.resnet_record(dict(spec, depths=(1, 2)), in_hw)
    assert rec != other and rec == checkpoint.resnet_record(niti_amd.normalize_resnet_spec(spec), in_hw)
    p = str(tmp_path / "r.safetensors")
    checkpoint.save_params(p, W, S, niti_amd.ARCH_RESNET, in_hw=in_hw, resnet=rec)
    with safe_open(p, framework="numpy") as f:
        assert json.loads(f.metadata()["resnet"]) == rec and "chain" not in f.metadata()
    w2, s2, arch = checkpoint.load_params(p)
    assert arch == niti_amd.ARCH_RESNET and s2 == S and all(np.array_equal(a, b) for a, b in zip(W, w2))
    assert checkpoint.load_resnet(p) == rec and checkpoint.load_chain(p) is None
    checkpoint.expect_chain(checkpoint.load_resnet(p), rec, p)
    with pytest.raises(ValueError):
        checkpoint.expect_chain(checkpoint.load_resnet(p), other, p)
    with pytest.raises(ValueError):  # another input size is another network
        checkpoint.expect_chain(checkpoint.load_resnet(p), checkpoint.resnet_record(spec, in_hw + 4), p)
    q = str(tmp_path / "r.mnn")
    mnn_snapshot.save(q, W, S, meta={"arch": niti_amd.ARCH_RESNET, "in_hw": in_hw, "resnet": rec})
    w3, s3, meta = mnn_snapshot.load(q)
    assert s3 == S and all(np.array_equal(a, b) for a, b in zip(W, w3))
    assert mnn_snapshot.resnet_of(meta) == rec and mnn_snapshot.chain_of(meta) is None
    with pytest.raises(ValueError):
        checkpoint.expect_chain(mnn_snapshot.resnet_of(meta), other, q)
    # a built-in network's snapshot carries no record, and a spec model refuses it
    b = str(tmp_path / "b.safetensors")
    checkpoint.save_params(b, W, S, niti_amd.ARCH_RESNET18, in_hw=in_hw)
    with safe_open(b, framework="numpy") as f:
        assert sorted(f.metadata()) == ["arch", "format", "in_hw", "num_layers"]
    assert checkpoint.load_resnet(b) is None
    with pytest.raises(ValueError):
        checkpoint.expect_chain(checkpoint.load_resnet(b), rec, b)


def test_symbols_are_exported(L):
    import niti_amd
    assert niti_amd.ARCH_RESNET == 6
    names = L.header_functions()
    for n in ("niti_model_resnet_check", "niti_model_create_resnet"):
        assert n in names
        getattr(L.lib(), n)
    assert callable(niti_amd.resnet_layers) and callable(niti_amd.normalize_resnet_spec)
    from niti_amd.model import NitiModel
    assert callable(NitiModel.from_resnet)
    # the struct is the header's: 7 ints, NITI_RESNET_MAX_STAGES depths, classes
    assert C.sizeof(L.ResnetSpec) == 4 * (7 + L.RESNET_MAX_STAGES + 1)
    hdr = open(L.HEADER).read()
    assert f"#define NITI_RESNET_MAX_STAGES {L.RESNET_MAX_STAGES}\n" in hdr
    assert f"#define NITI_RESNET_MAX_LAYERS {L.RESNET_MAX_LAYERS}\n" in hdr
