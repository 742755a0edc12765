"""The host-access half of the niti_model_* C ABI (set_weight / get_weight, get_tap, get_logits, layer_info,
spec_stats, set_rowconv, copy_weights_from) on both step drivers: two chain networks (NET_S: depthwise
layers behind an im2col first layer; NET_T: a stride-2 dense layer with sub-pixel weights between row-kernel
layers) and two residual ones (one stem of each kind).  Everything is compared bit for bit; the refusals are
made through the C ABI itself, with a sentinel in the host buffer that no refused call may touch.
"""
import ctypes as C

import numpy as np
import pytest

import depthwise_cases as DC
import resnet_family_cases as FC
import strided_cases as SC

pytestmark = pytest.mark.gpu

NETS = ("NET_S", "NET_T", "one_stage_w48", "cifar_resnet20")
SENTINEL = 0x5A


@pytest.fixture(scope="module")
def T():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import niti_amd  # noqa: F401
    return torch


def _chain(net):
    return net in ("NET_S", "NET_T")


def _model(net):
    """A model of the named net at the batch its own test file uses, weights from init_weights(3)."""
    from niti_amd.model import NitiModel
    if _chain(net):
        in_c, in_hw, spec = (DC.NETS if net == "NET_S" else SC.NETS)[net]
        m = NitiModel.from_chain(spec, in_c, in_hw, 3)
    else:
        spec, in_hw, batch, _ = FC.CASES[net]
        m = NitiModel.from_resnet(spec, in_hw, batch)
    m.init_weights(3)
    return m


def _data(net, steps):
    """[(x int8, labels)] and the input exponent."""
    if _chain(net):
        nets, cases = (DC.NETS, DC) if net == "NET_S" else (SC.NETS, SC)
        return cases.batches(cases.derive(nets[net]), 3, steps, 1), -3
    spec, in_hw, batch, _ = FC.CASES[net]
    return FC.draw_steps(spec, in_hw, batch, False, steps), FC.EXP_IN


def _step(T, m, x, labels, exp_in):
    m.train_step(T.from_numpy(x.copy()).cuda(), exp_in, T.from_numpy(labels.copy()).cuda())


@pytest.mark.parametrize("net", NETS)
def test_weight_round_trip(T, net):
    """Random int8 weights of weight_shape(i) come back as they went in: the im2col first layer at pitch 32,
    the stem at its own pitch, depthwise [C][1][k][k] and strided layers."""
    m = _model(net)
    rng = np.random.default_rng(7)
    W = [rng.integers(-128, 128, m.weight_shape(i)).astype(np.int8) for i in range(len(m.layers))]
    for i, w in enumerate(W):
        m.set_weight(i, w, -5 - i % 3)
    for i, w in enumerate(W):
        assert np.array_equal(m.get_weight(i), w), i


@pytest.mark.parametrize("net", NETS)
def test_rowconv_off_after_steps_rebuilds_what_the_update_skipped(T, net):
    """set_rowconv(False) after two steps on the row kernels equals a model that never used them and took
    the stepped weights through copy_weights_from: the same weights and logits after one more step."""
    data, exp_in = _data(net, 3)
    a, b = _model(net), _model(net)
    for x, labels in data[:2]:
        _step(T, a, x, labels, exp_in)
        _step(T, b, x, labels, exp_in)
    a.set_rowconv(False)
    c = _model(net)
    c.set_rowconv(False)
    c.copy_weights_from(b)
    for i in range(len(a.layers)):
        assert np.array_equal(a.get_weight(i), c.get_weight(i)), ("before", i)
    _step(T, a, *data[2], exp_in)
    _step(T, c, *data[2], exp_in)
    (la, ea), (lc, ec) = a.logits(), c.logits()
    assert ea == ec and np.array_equal(la, lc)
    for i in range(len(a.layers)):
        assert np.array_equal(a.get_weight(i), c.get_weight(i)), ("after", i)
    assert a.rowconv_error() == 0 and c.rowconv_error() == 0


@pytest.mark.parametrize("net", NETS)
def test_identities(T, net):
    m = _model(net)
    data, exp_in = _data(net, 1)
    _step(T, m, *data[0], exp_in)
    logits, _ = m.logits()
    last = len(m.layers) - 1
    assert np.array_equal(logits, m.tap(last, 0).reshape(logits.shape))
    assert len(m.spec_stats()) == len(m.layers)
    if not _chain(net):
        assert [l["pool"] for l in m.layers] == [0] * len(m.layers)


def _tap(m, layer, which, buf, nbytes):
    return m._lib.niti_model_get_tap(m._h, layer, which, buf.ctypes.data_as(C.c_void_p), nbytes, None)


@pytest.mark.parametrize("net", NETS)
def test_refusals_leave_the_host_buffer_alone(T, net):
    from niti_amd._lib import INVALID_VALUE
    m = _model(net)
    data, exp_in = _data(net, 1)
    x, labels = data[0]
    _step(T, m, x, labels, exp_in)
    nl = len(m.layers)

    def sentinel(n):
        return np.full(n, SENTINEL, np.uint8)

    # a buffer one byte short, every layer and tap (all three were written: keep_grads is on)
    for i, l in enumerate(m.layers):
        for which in (0, 1, 2):
            need = int(np.prod(m.weight_shape(i))) if which == 1 else m.batch * l["c_out"] * l["oh"] * l["ow"]
            buf = sentinel(need)
            assert _tap(m, i, which, buf, need - 1) == INVALID_VALUE, (i, which)
            assert (buf == SENTINEL).all(), (i, which)
            assert _tap(m, i, which, buf, need) == 0, (i, which)  # (and the exact size is taken)
    # which = 3, and a layer out of range
    big = max(max(m.batch * l["c_out"] * l["oh"] * l["ow"], int(np.prod(m.weight_shape(i))))
              for i, l in enumerate(m.layers))
    buf = sentinel(big)
    assert _tap(m, 0, 3, buf, big) == INVALID_VALUE
    for layer in (-1, nl):
        for which in (0, 1, 2):
            assert _tap(m, layer, which, buf, big) == INVALID_VALUE, (layer, which)
        assert m._lib.niti_model_get_weight(m._h, layer, buf.ctypes.data_as(C.c_void_p)) == INVALID_VALUE
        assert m._lib.niti_model_set_weight(m._h, layer, buf.ctypes.data_as(C.c_void_p), -6) == INVALID_VALUE
        info = (C.c_int * 12)(*([SENTINEL] * 12))
        assert m._lib.niti_model_layer_info(m._h, layer, info) == INVALID_VALUE
        assert list(info) == [SENTINEL] * 12
        assert m._lib.niti_model_layer_depthwise(m._h, layer) == -1
    assert (buf == SENTINEL).all()
    # the int8 weight gradient after a step that did not keep it
    m.keep_grads(False)
    _step(T, m, x, labels, exp_in)
    for i in range(nl):
        assert _tap(m, i, 1, buf, big) == INVALID_VALUE, i
    assert (buf == SENTINEL).all()
