"""GPU parity of chain networks with depthwise layers (NitiModel.from_chain) against the oracle's step
restated with such layers (tests/depthwise_cases.py: dw_chain_step_ref).

Every check runs two steps at batch 3 or 4 with weights from init_weights(seed=3) and data from
default_rng(1), and compares logits, exponents, taps 0 / 1 / 2 of every layer and every weight bit for bit.
"""
import ctypes as C
import functools
import threading

import numpy as np
import pytest

import depthwise_cases as DC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def T():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import niti_amd  # noqa: F401
    return torch


@functools.lru_cache(maxsize=None)
def _ref(net, batch, steps=2, images=False, bits=None):
    """(layers, W, S, data, reference steps) of a named net: computed once, shared, never written."""
    layers = DC.derive(DC.NETS[net])
    W, S = DC.init_weights(layers, seed=3)
    data = DC.batches(layers, batch, steps, 1, images=images)
    return layers, W, S, data, DC.ref_steps(layers, W, S, data, bits=None if bits is None else list(bits))


def _model(net, batch, W=None, S=None):
    from niti_amd.model import NitiModel
    in_c, in_hw, spec = DC.NETS[net]
    m = NitiModel.from_chain(spec, in_c, in_hw, batch)
    if W is None:
        m.init_weights(3)
    else:
        for i, (w, s) in enumerate(zip(W, S)):
            m.set_weight(i, w, s)
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


def _run(T, net, batch, steps=2, rowconv=True, keep_grads=True, graph=False, prepare=None, bits=None):
    layers, W, S, data, ref = _ref(net, batch, steps, False, bits)
    m = _model(net, batch)
    assert m.arch == 5 and [l["c_out"] for l in m.layers] == [l["co"] for l in layers]
    assert [l["depthwise"] for l in m.layers] == [l["dw"] for l in layers]
    for i, (w, s) in enumerate(zip(W, S)):  # init_weights: xavier_int8 on [C, 1, k, k] for such a layer
        assert m.weight_shape(i) == DC.weight_shape(layers[i])
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


def test_net_s_separable_blocks(T):
    m = _run(T, "NET_S", 4)
    layers = DC.derive(DC.NET_S)
    # MACs: n oh ow C k k for a depthwise layer; forward + weight gradient (+ input gradient past layer 0)
    per = [4 * (l["h"] + 2 * l["pad"] - l["k"] + 1) ** 2 * l["co"] * (1 if l["dw"] else l["ci"]) * l["k"] ** 2 for l in layers]
    assert m.step_macs() == sum(p * (2 if i == 0 else 3) for i, p in enumerate(per))
    # no GEMM plan on such a layer; the others keep theirs
    from niti_amd._lib import NOT_SUPPORT, NitiError
    for ph in (0, 1, 2):
        with pytest.raises(NitiError) as e:
            m.plan(1, ph)
        assert e.value.code == NOT_SUPPORT
        with pytest.raises(NitiError) as e:
            m.set_plan(3, ph, (128, 128, 1, 0))
        assert e.value.code == NOT_SUPPORT
    assert sorted({i for i, _ in m.plans()}) == [0, 2, 4, 5]


@pytest.mark.parametrize("rowconv", [True, False])
def test_net_r_between_row_kernel_layers(T, rowconv):
    """A pooled row-kernel layer in front of a depthwise one writes its pre-pool output and no codes, and
    hands over NHWC16; the row-kernel layer behind one converts its input and output gradient itself."""
    _run(T, "NET_R", 4, rowconv=rowconv)


def test_net_o_odd_maps_5x5_pool_and_flatten(T):
    _run(T, "NET_O", 3)


def test_net_s_without_grad_tap(T):
    _run(T, "NET_S", 4, keep_grads=False)


def test_net_s_graph_replay(T):
    _run(T, "NET_S", 4, steps=3, graph=True)


def test_net_s_autotune_keeps_results(T):
    from niti_amd.model import NitiModel
    try:
        _run(T, "NET_S", 4, prepare=lambda m: m.autotune(reps=2))
    finally:
        NitiModel.reset_plans()


def test_net_s_run_phase_and_probe(T):
    """Each phase of a depthwise layer again, alone: the same buffers; the probe times its launches."""
    layers, W, S, data, ref = _ref("NET_S", 4)
    m = _model("NET_S", 4)
    m.set_update_bits(0)  # every layer frozen: the phases run again on the weights the step ran on
    m.train_step(T.from_numpy(data[0][0].copy()).cuda(), -3, T.from_numpy(data[0][1].copy()).cuda())
    rec = ref[0][1]
    m.set_probe(1, 0, 8)
    for ph in (0, 1, 2):
        m.run_phase(1, ph)
        m.run_phase(3, ph)
    T.cuda.synchronize()
    ms, count = m.probe_read()
    assert count == 1 and ms > 0
    m.set_probe(-1, -1, 0)
    for i in (0, 1, 2, 3):
        assert np.array_equal(m.tap(i, 0), rec["r"][i]) and np.array_equal(m.tap(i, 2), rec["dy"][i]), i


def test_net_s_update_bits(T):
    """A frozen depthwise layer keeps its weights; the other follows the reference at 4 bits."""
    bits = (2, 0, 2, 4, 2, 2)
    m = _run(T, "NET_S", 4, bits=bits)
    assert m.update_bits() == list(bits)
    _, W, _, _, ref = _ref("NET_S", 4, 2, False, bits)
    assert np.array_equal(m.get_weight(1), W[1]) and not np.array_equal(m.get_weight(3), W[3])
    plain = _ref("NET_S", 4)[4]
    assert not np.array_equal(ref[0][0][3], plain[0][0][3])  # (4 bits is another update than 2 here)


def test_net_s_evaluate_padded_tail(T):
    import eval_cases as E
    import niti_oracle as O
    layers, W, S, _, _ = _ref("NET_S", 4)
    rng = np.random.default_rng(9)
    img = rng.integers(0, 256, (10, 3, 8, 8)).astype(np.uint8)
    lab = rng.integers(0, 10, 10).astype(np.int32)
    m = _model("NET_S", 4)
    got = m.evaluate(img, lab)
    want = {"images": 0, "top1": 0, "topk": 0, "loss_sum": 0.0}
    for i in range(0, 10, 4):
        bi = np.concatenate([img[i:i + 4], np.zeros((max(0, i + 4 - 10), 3, 8, 8), np.uint8)])
        bl = np.concatenate([lab[i:i + 4], np.full(max(0, i + 4 - 10), -1, np.int32)])
        x, a = O.quantize_images(bi)
        _, rec = DC.dw_chain_step_ref(layers, W, S, x, a, np.maximum(bl, 0))
        want = E.add_totals(want, E.metrics_ref(rec["logits"], rec["exp"][-1], bl, 5))
    assert (got["images"], got["top1"], got["topk"]) == (10, want["top1"], want["topk"])
    assert E.loss_close(got["loss_sum"], want["loss_sum"])
    for i in range(len(layers)):  # evaluation writes no weight
        assert np.array_equal(m.get_weight(i), W[i])


def test_net_s_fit_epoch_equals_the_reference(T):
    from niti_amd.dataset import DeviceDataset, make_order
    layers, W, S, _, _ = _ref("NET_S", 4)
    rng = np.random.default_rng(10)
    img = rng.integers(0, 256, (8, 3, 8, 8)).astype(np.uint8)
    lab = rng.integers(0, 10, 8).astype(np.int32)
    m = _model("NET_S", 4)
    steps = m.fit_epoch(DeviceDataset(img, lab), seed=3, epoch=1)
    assert steps == 2
    index, _ = make_order(8, 4, seed=3, epoch=1, drop_last=True)
    ref = DC.ref_steps(layers, W, S, [(img[index[k * 4:(k + 1) * 4]], lab[index[k * 4:(k + 1) * 4]]) for k in range(steps)])
    T.cuda.synchronize()
    _compare(m, layers, ref[-1][0], ref[-1][1], steps - 1)


def test_net_s_snapshots(T, tmp_path):
    """save / load and save_mnn / load_mnn carry [C, 1, k, k] weights and the list; a list that differs
    only in a depthwise flag is refused before any device write."""
    from niti_amd.model import NitiModel
    in_c, in_hw, spec = DC.NET_S
    layers, W, S, _, _ = _ref("NET_S", 4)
    m = _model("NET_S", 4)
    assert m.chain[1]["c_out"] == 16 and m.chain[1]["depthwise"] == 1
    p, q = str(tmp_path / "a.safetensors"), str(tmp_path / "a.mnn")
    m.save(p)
    m.save_mnn(q)
    # the same network with layer 3 dense (24 -> 24, 3x3): same layer count, another weight shape
    dense = [tuple(l) for l in spec]
    dense[3] = (24, 3, 1, 1, 1, 0, 0)
    for load in ("load", "load_mnn"):
        path = p if load == "load" else q
        same = NitiModel.from_chain(spec, in_c, in_hw, 2)
        getattr(same, load)(path)
        for i, w in enumerate(W):
            assert np.array_equal(same.get_weight(i), w) and same._wscale[i] == S[i]
        other = NitiModel.from_chain(dense, in_c, in_hw, 2)
        with pytest.raises(ValueError):
            getattr(other, load)(path)
        assert not np.any(other.get_weight(0))  # refused before any device write


def test_net_s_copy_weights(T):
    from niti_amd._lib import NitiError
    from niti_amd.model import NitiModel
    in_c, in_hw, spec = DC.NET_S
    layers, W, S, _, _ = _ref("NET_S", 4)
    src = _model("NET_S", 4)
    dst = NitiModel.from_chain(spec, in_c, in_hw, 3)
    dst.copy_weights_from(src)
    for i, w in enumerate(W):
        assert np.array_equal(dst.get_weight(i), w), i
    dense = [tuple(l) for l in spec]
    dense[1] = (16, 3, 1, 1, 0, 0, 0)  # the same geometry, dense: another network
    with pytest.raises(NitiError):
        NitiModel.from_chain(dense, in_c, in_hw, 3).copy_weights_from(src)
    (x, labels), = DC.batches(layers, 3, 1, seed=12)
    newW, rec, _, _ = DC.ref_steps(layers, W, S, [(x, labels)])[0]
    dst.train_step(T.from_numpy(x.copy()).cuda(), -3, T.from_numpy(labels.copy()).cuda())
    _compare(dst, layers, newW, rec, 0)


def test_net_s_two_local_ranks_equal_one_device(T):
    from niti_amd.model import LocalGroup
    layers, W, S, data, ref = _ref("NET_S", 4)
    ranks = [_model("NET_S", 2) for _ in range(2)]
    group = LocalGroup(2)
    for r, m in enumerate(ranks):
        m.attach_local(group, r, exact=True)
    streams = [T.cuda.Stream() for _ in range(2)]
    for step, ((x, labels), (newW, rec, _, _)) in enumerate(zip(data, ref)):
        xd, ld = T.from_numpy(x.copy()).cuda(), T.from_numpy(labels.copy()).cuda()
        parts = [(xd[r * 2:(r + 1) * 2].contiguous(), ld[r * 2:(r + 1) * 2].contiguous()) for r in range(2)]
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
            _compare(m, layers, newW, rec, (step, r), sl=slice(r * 2, (r + 1) * 2))
    assert all(m.rowconv_error() == 0 for m in ranks)


def test_vgg11_by_name_and_through_create_chain2(T):
    """The built-in network and the same list through the eight-field entry point: two steps' results,
    plans and MACs."""
    import chain_cases as CC
    import niti_amd
    import niti_model_ref as R
    from niti_amd import _lib as L
    from niti_amd.model import NitiModel
    layers = CC.derive(CC.VGG11)
    W, S = R.init_weights(layers, seed=31)
    a = NitiModel(niti_amd.ARCH_VGG11, 8)
    arr = (L.ChainLayer2 * len(CC.VGG11[2]))()
    for s, (co, k, pad, relu, pool, fl) in zip(arr, CC.VGG11[2]):
        s.c_out, s.kernel, s.stride, s.pad, s.relu, s.pool, s.flatten, s.depthwise = co, k, 1, pad, relu, pool, fl, 0
    h = C.c_void_p()
    assert L.lib().niti_model_create_chain2(arr, len(arr), 3, 32, 8, C.byref(h)) == 0
    b = NitiModel.__new__(NitiModel)
    b._lib = L.lib()
    b._adopt(h, L.ARCH_CHAIN, 8)
    for m in (a, b):
        for i, (w, s) in enumerate(zip(W, S)):
            m.set_weight(i, w, s)
    assert a.layers == b.layers and not any(l["depthwise"] for l in a.layers)
    assert a.plans() == b.plans() and a.step_macs() == b.step_macs()
    rng = np.random.default_rng(32)
    for step in range(2):
        x = T.from_numpy(rng.integers(-127, 128, (8, 3, 32, 32)).astype(np.int8)).cuda()
        lab = T.from_numpy(rng.integers(0, 10, 8).astype(np.int32)).cuda()
        a.train_step(x, -3, lab)
        b.train_step(x, -3, lab)
        (la, ea), (lb, eb) = a.logits(), b.logits()
        assert ea == eb and np.array_equal(la, lb), step
        for i in range(len(layers)):
            assert np.array_equal(a.get_weight(i), b.get_weight(i)), (step, i)
            assert np.array_equal(a.tap(i, 2), b.tap(i, 2)), (step, i)
    assert a.plans() == b.plans() and b.rowconv_error() == 0
