"""GPU parity of chain networks with skip connections, a global pool and more than 24 layers
(NitiModel.from_chain through niti_model_create_chain4) against the oracle's step restated with the two
rules (tests/skip_cases.py: chain_step_ref).

Every check runs two steps at the net's batch (two ranks: two halves of it) with weights from
init_weights(seed=3) and data from default_rng(1), and compares logits, the exponent, taps 0 / 1 / 2 of every
layer and every weight bit for bit.
"""
import ctypes as C
import functools
import threading

import numpy as np
import pytest

import skip_cases as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def T():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import niti_amd  # noqa: F401
    return torch


@functools.lru_cache(maxsize=None)
def _ref_cached(net, steps, bits):
    layers = K.derive(K.NETS[net])
    W, S = K.init_weights(layers, seed=K.SEED_W)
    data = K.batches(layers, K.BATCH[net], steps, K.SEED_X)
    return layers, W, S, data, K.ref_steps(layers, W, S, data, bits=None if bits is None else list(bits))


def _ref(net, steps=2, bits=None):
    """(layers, W, S, data, reference steps) of a named net: computed once, shared, never written."""
    return _ref_cached(net, steps, bits)


def _model(net, batch=None):
    from niti_amd.model import NitiModel
    in_c, in_hw, spec = K.NETS[net]
    m = NitiModel.from_chain(spec, in_c, in_hw, batch or K.BATCH[net])
    m.init_weights(K.SEED_W)
    return m


def _compare(m, layers, newW, rec, step, keep_grads=True, sl=slice(None)):
    from niti_amd._lib import NitiError
    logits, e = m.logits()
    assert e == rec["exp"][-1], (step, e, rec["exp"][-1])
    assert np.array_equal(logits, rec["logits"][sl]), step
    for i in range(len(layers)):
        try:
            fwd = m.tap(i, 0)
        except NitiError:  # keep_grads(0): a pooled layer whose route went on as codes writes no pre-pool output
            assert not keep_grads and layers[i]["pool"] and not layers[i]["dw"]
            fwd = None
        assert fwd is None or np.array_equal(fwd, rec["r"][i][sl]), ("fwd", step, i)
        assert np.array_equal(m.tap(i, 2), rec["dy"][i][sl]), ("dy", step, i)
        if keep_grads:
            assert np.array_equal(m.tap(i, 1), rec["dw"][i]), ("dw", step, i)
        assert np.array_equal(m.get_weight(i), newW[i]), ("w", step, i)


def _run(T, net, steps=2, rowconv=True, keep_grads=True, graph=False, prepare=None, bits=None):
    layers, W, S, data, ref = _ref(net, steps, bits)
    m = _model(net)
    assert m.arch == 5 and [l["c_out"] for l in m.layers] == [l["co"] for l in layers]
    assert [l.get("skip", 0) for l in m.layers] == [l["skip"] for l in layers]
    assert [l.get("gpool", 0) for l in m.layers] == [l["gpool"] for l in layers]
    assert [l["oh"] for l in m.layers] == [s[5] for s in K.shapes_of(layers)]
    for i, (w, s) in enumerate(zip(W, S)):
        assert np.array_equal(m.get_weight(i), w) and m._wscale[i] == s
    m.set_graph(graph)
    m.set_rowconv(rowconv)
    m.keep_grads(keep_grads)
    if bits is not None:
        m.set_update_bits({i: b for i, b in enumerate(bits) if b != 2})
    xd = ld = None
    if prepare is not None:  # after one throwaway step; the weights are set again after it
        m.train_step(T.from_numpy(data[0][0].copy()).cuda(), -3, T.from_numpy(data[0][1].copy()).cuda())
        prepare(m)
        for i, (w, s) in enumerate(zip(W, S)):
            m.set_weight(i, w, s)
    for step, ((x, labels), (newW, rec, _, _)) in enumerate(zip(data, ref)):
        if xd is None:
            xd, ld = T.from_numpy(x.copy()).cuda(), T.from_numpy(labels.copy()).cuda()
        else:  # (the same device buffers: a captured graph replays)
            xd.copy_(T.from_numpy(x.copy()))
            ld.copy_(T.from_numpy(labels.copy()))
        m.train_step(xd, -3, ld)
        _compare(m, layers, newW, rec, step, keep_grads)
    assert m.rowconv_error() == 0
    return m


def _two_ranks(T, net):
    from niti_amd.model import LocalGroup
    layers, W, S, data, ref = _ref(net)
    half = K.BATCH[net] // 2
    assert 2 * half == K.BATCH[net]
    ranks = [_model(net, half) for _ in range(2)]
    group = LocalGroup(2)
    for r, m in enumerate(ranks):
        m.attach_local(group, r, exact=True)
    streams = [T.cuda.Stream() for _ in range(2)]
    for step, ((x, labels), (newW, rec, _, _)) in enumerate(zip(data, ref)):
        xd, ld = T.from_numpy(x.copy()).cuda(), T.from_numpy(labels.copy()).cuda()
        parts = [(xd[r * half:(r + 1) * half].contiguous(), ld[r * half:(r + 1) * half].contiguous()) for r in range(2)]
        T.cuda.synchronize()
        errs = []

        def rank_step(r):
            try:
                ranks[r].train_step(parts[r][0], -3, parts[r][1], stream=C.c_void_p(streams[r].cuda_stream))
                streams[r].synchronize()
            except BaseException as e:  # noqa: BLE001 -- re-raised in the main thread
                errs.append(e)

        ts = [threading.Thread(target=rank_step, args=(r,)) for r in range(2)]
        for t in ts:
            t.start()
        for t in ts:
            t.join(timeout=120)
        assert not any(t.is_alive() for t in ts), "a rank thread hung"
        if errs:
            raise errs[0]
        for r, m in enumerate(ranks):
            _compare(m, layers, newW, rec, (step, r), sl=slice(r * half, (r + 1) * half))
    assert all(m.rowconv_error() == 0 for m in ranks)


# ------------------------------------------------------------------------------------ every net, plainly
def test_net_v_mobilenetv2_shaped(T):
    m = _run(T, "NET_V")
    assert m.rowconv_error() == 0
    assert [l["skip"] for l in m.layers] == [0, 0, 0, 3, 0, 0, 3, 0, 0, 0, 0, 0, 3, 0, 0]
    assert m.layers[13]["gpool"] == 1 and m.layers[14]["h"] == 1 and m.layers[14]["c_in"] == 64


@pytest.mark.parametrize("net", ["NET_W", "NET_X", "NET_D", "NET_G", "NET_P", "NET_E"])
def test_net_plain(T, net):
    _run(T, net)


@pytest.mark.parametrize("net", ["NET_X", "NET_W"])
def test_net_without_the_row_kernels(T, net):
    _run(T, net, rowconv=False)


def test_net_w_equals_the_residual_driver(T):
    """The same network through the other driver: a from_resnet model with the same weights, directly."""
    from niti_amd.model import NitiModel
    layers, W, S, data, _ = _ref("NET_W")
    a = _model("NET_W")
    b = NitiModel.from_resnet(dict(depths=(2,), width=16, classes=10, stem="cifar"), 8, K.BATCH["NET_W"])
    assert len(b.layers) == len(layers)
    for i, (w, s) in enumerate(zip(W, S)):
        b.set_weight(i, w, s)
    for x, labels in data:
        for m in (a, b):
            m.train_step(T.from_numpy(x.copy()).cuda(), -3, T.from_numpy(labels.copy()).cuda())
        la, lb = a.logits(), b.logits()
        assert la[1] == lb[1] and np.array_equal(la[0], lb[0])
        for i in range(len(layers)):
            assert np.array_equal(a.get_weight(i), b.get_weight(i)), i


# ------------------------------------------------------------------------------------ NET_V through the rest
def test_net_v_graph_replay(T):
    _run(T, "NET_V", steps=3, graph=True)


def test_net_v_without_grad_tap(T):
    _run(T, "NET_V", keep_grads=False)


def test_net_v_autotune_keeps_results(T):
    from niti_amd.model import NitiModel
    try:
        _run(T, "NET_V", prepare=lambda m: m.autotune(reps=2))
    finally:
        NitiModel.reset_plans()


def test_net_v_two_local_ranks_equal_one_device(T):
    _two_ranks(T, "NET_V")


def test_net_v_evaluate_padded_tail(T):
    import eval_cases as E
    import niti_oracle as O
    layers, W, S, _, _ = _ref("NET_V")
    rng = np.random.default_rng(9)
    b = K.BATCH["NET_V"]
    img = rng.integers(0, 256, (7, 3, 16, 16)).astype(np.uint8)
    lab = rng.integers(0, 10, 7).astype(np.int32)
    m = _model("NET_V")
    got = m.evaluate(img, lab)
    want = {"images": 0, "top1": 0, "topk": 0, "loss_sum": 0.0}
    for i in range(0, 7, b):
        bi = np.concatenate([img[i:i + b], np.zeros((max(0, i + b - 7), 3, 16, 16), np.uint8)])
        bl = np.concatenate([lab[i:i + b], np.full(max(0, i + b - 7), -1, np.int32)])
        x, a = O.quantize_images(bi)
        _, rec = K.chain_step_ref(layers, W, S, x, a, np.maximum(bl, 0))
        want = E.add_totals(want, E.metrics_ref(rec["logits"], rec["exp"][-1], bl, 5))
    assert (got["images"], got["top1"], got["topk"]) == (7, want["top1"], want["topk"])
    assert E.loss_close(got["loss_sum"], want["loss_sum"])
    for i in range(len(layers)):  # evaluation writes no weight
        assert np.array_equal(m.get_weight(i), W[i])


def test_net_v_fit_epoch_equals_the_reference(T):
    from niti_amd.dataset import DeviceDataset, make_order
    layers, W, S, _, _ = _ref("NET_V")
    b = K.BATCH["NET_V"]
    rng = np.random.default_rng(10)
    img = rng.integers(0, 256, (2 * b, 3, 16, 16)).astype(np.uint8)
    lab = rng.integers(0, 10, 2 * b).astype(np.int32)
    m = _model("NET_V")
    steps = m.fit_epoch(DeviceDataset(img, lab), seed=3, epoch=1)
    assert steps == 2
    index, _ = make_order(2 * b, b, seed=3, epoch=1, drop_last=True)
    ref = K.ref_steps(layers, W, S, [(img[index[k * b:(k + 1) * b]], lab[index[k * b:(k + 1) * b]]) for k in range(steps)])
    T.cuda.synchronize()
    _compare(m, layers, ref[-1][0], ref[-1][1], steps - 1)


def test_net_v_update_bits(T):
    """A frozen adding layer keeps its weights while its sum still runs; another follows the reference at 4 bits."""
    bits = (2, 2, 2, 0, 2, 2, 4, 2, 2, 2, 2, 2, 2, 2, 2)
    m = _run(T, "NET_V", bits=bits)
    assert m.update_bits() == list(bits)
    _, W, _, _, _ = _ref("NET_V", 2, bits)
    assert np.array_equal(m.get_weight(3), W[3]) and not np.array_equal(m.get_weight(6), W[6])


def test_net_v_snapshots(T, tmp_path):
    """Both snapshot formats carry skip and gpool; a list that differs in one skip, or in gpool, is refused
    before any device write."""
    from niti_amd.model import NitiModel
    in_c, in_hw, spec = K.NET_V
    layers, W, S, _, _ = _ref("NET_V")
    m = _model("NET_V")
    assert [d["skip"] for d in m.chain] == [l["skip"] for l in layers] and [d["gpool"] for d in m.chain] == [0] * 13 + [1, 0]
    p, q = str(tmp_path / "a.safetensors"), str(tmp_path / "a.mnn")
    m.save(p)
    m.save_mnn(q)
    other_spec = [tuple(l) for l in spec]
    other_spec[6] = other_spec[6][:8] + (0, 0)  # the second block without its sum: the same weight shapes
    for load in ("load", "load_mnn"):
        path = p if load == "load" else q
        same = NitiModel.from_chain(spec, in_c, in_hw, 2)
        getattr(same, load)(path)
        for i, w in enumerate(W):
            assert np.array_equal(same.get_weight(i), w) and same._wscale[i] == S[i]
        other = NitiModel.from_chain(other_spec, in_c, in_hw, 2)
        with pytest.raises(ValueError):
            getattr(other, load)(path)
        assert not np.any(other.get_weight(0))  # refused before any device write
    # gpool: a 1x1 map pooled or not -- the same weight shapes
    pooled = [K._l(16, 3, 1, 1, stride=2, gpool=1), K._l(10, 1)]
    plain = [K._l(16, 3, 1, 1, stride=2), K._l(10, 1)]
    g = NitiModel.from_chain(pooled, 3, 2, 2)
    g.init_weights(5)
    pg, qg = str(tmp_path / "g.safetensors"), str(tmp_path / "g.mnn")
    g.save(pg)
    g.save_mnn(qg)
    for load, path in (("load", pg), ("load_mnn", qg)):
        other = NitiModel.from_chain(plain, 3, 2, 2)
        with pytest.raises(ValueError):
            getattr(other, load)(path)
        assert not np.any(other.get_weight(0))
        same = NitiModel.from_chain(pooled, 3, 2, 2)
        getattr(same, load)(path)
        assert np.array_equal(same.get_weight(0), g.get_weight(0))


def test_net_v_copy_weights(T):
    from niti_amd._lib import NitiError
    from niti_amd.model import NitiModel
    in_c, in_hw, spec = K.NET_V
    layers, W, S, _, _ = _ref("NET_V")
    b = K.BATCH["NET_V"]
    src = _model("NET_V")
    dst = NitiModel.from_chain(spec, in_c, in_hw, b)
    dst.copy_weights_from(src)
    for i, w in enumerate(W):
        assert np.array_equal(dst.get_weight(i), w), i
    (x, labels), = K.batches(layers, b, 1, seed=12)
    newW, rec, _, _ = K.ref_steps(layers, W, S, [(x, labels)])[0]
    dst.train_step(T.from_numpy(x.copy()).cuda(), -3, T.from_numpy(labels.copy()).cuda())
    _compare(dst, layers, newW, rec, 0)
    # the same weight shapes without one sum: another network
    moved = [tuple(l) for l in spec]
    moved[6] = moved[6][:8] + (0, 0)
    with pytest.raises(NitiError):
        NitiModel.from_chain(moved, in_c, in_hw, b).copy_weights_from(src)


# ------------------------------------------------------------------------------------ NET_D: 27 layers
def test_net_d_two_local_ranks_put_27_layers_in_one_bucket(T):
    _two_ranks(T, "NET_D")


def test_net_d_graph_replay(T):
    _run(T, "NET_D", steps=3, graph=True)


def test_net_d_update_runs_in_two_launches(T):
    """27 layers: the update's two launches, with a layer of each frozen and one of each at 4 bits."""
    bits = [2] * 27
    bits[1], bits[2], bits[25], bits[26] = 0, 4, 0, 4
    m = _run(T, "NET_D", bits=tuple(bits))
    _, W, _, _, _ = _ref("NET_D", 2, tuple(bits))
    assert np.array_equal(m.get_weight(1), W[1]) and np.array_equal(m.get_weight(25), W[25])
    assert not np.array_equal(m.get_weight(2), W[2]) and not np.array_equal(m.get_weight(26), W[26])
