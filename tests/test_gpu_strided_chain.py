"""GPU parity of chain networks with strided layers (NitiModel.from_chain through niti_model_create_chain3)
against the oracle's step restated with each layer's stride (tests/strided_cases.py: chain_step_ref).

Every check runs two steps at batch 3 (two ranks: 2 x 2) with weights from init_weights(seed=3) and data from
default_rng(1), and compares logits, exponents, taps 0 / 1 / 2 of every layer and every weight bit for bit.
"""
import ctypes as C
import functools
import threading

import numpy as np
import pytest

import strided_cases as SC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def T():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import niti_amd  # noqa: F401
    return torch


@functools.lru_cache(maxsize=None)
def _ref(net, batch, steps=2, bits=None):
    """(layers, W, S, data, reference steps) of a named net: computed once, shared, never written."""
    layers = SC.derive(SC.NETS[net])
    W, S = SC.init_weights(layers, seed=3)
    data = SC.batches(layers, batch, steps, 1)
    return layers, W, S, data, SC.ref_steps(layers, W, S, data, bits=None if bits is None else list(bits))


def _model(net, batch):
    from niti_amd.model import NitiModel
    in_c, in_hw, spec = SC.NETS[net]
    m = NitiModel.from_chain(spec, in_c, in_hw, batch)
    m.init_weights(3)
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


def _run(T, net, batch=3, steps=2, rowconv=True, keep_grads=True, graph=False, prepare=None, bits=None):
    layers, W, S, data, ref = _ref(net, batch, steps, bits)
    m = _model(net, batch)
    assert m.arch == 5 and [l["c_out"] for l in m.layers] == [l["co"] for l in layers]
    assert [l["depthwise"] for l in m.layers] == [l["dw"] for l in layers]
    assert [l["stride"] for l in m.layers] == [l["stride"] for l in layers]
    assert [l["oh"] for l in m.layers] == [SC.out_hw(l["h"], l["k"], l["pad"], l["stride"]) for l in layers]
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


def test_net_m_mobilenet_shaped(T):
    m = _run(T, "NET_M")
    layers = SC.derive(SC.NET_M)
    assert [l["stride"] for l in m.layers] == [2, 1, 1, 2, 1, 2, 1, 1]
    assert [l["h"] for l in m.layers] == [16, 8, 8, 8, 4, 4, 2, 1]
    # MACs count the strided oh ow: forward + weight gradient (+ input gradient past layer 0)
    per = [3 * SC.out_hw(l["h"], l["k"], l["pad"], l["stride"]) ** 2 * l["co"] * (1 if l["dw"] else l["ci"]) * l["k"] ** 2
           for l in layers]
    assert m.step_macs() == sum(p * (2 if i == 0 else 3) for i, p in enumerate(per))
    # plans: the dense layers (the strided first one among them) have theirs, the depthwise ones none
    from niti_amd._lib import NOT_SUPPORT, NitiError
    assert sorted({i for i, _ in m.plans()}) == [0, 2, 4, 6, 7]
    for i in (1, 3, 5):
        with pytest.raises(NitiError) as e:
            m.plan(i, 0)
        assert e.value.code == NOT_SUPPORT


@pytest.mark.parametrize("rowconv", [True, False])
def test_net_t_strided_between_row_kernel_layers(T, rowconv):
    """The row-kernel layer in front of the strided one hands over NHWC16 and the one behind converts its
    input and output gradient itself; the strided layer's input gradient runs as the sub-pixel class GEMMs."""
    m = _run(T, "NET_T", rowconv=rowconv)
    assert 1 in {i for i, _ in m.plans()}  # the strided layer has GEMM plans either way


def test_net_u_odd_maps_strided_1x1_and_5x5(T):
    _run(T, "NET_U")


def test_net_up_strided_layer_that_pools(T):
    _run(T, "NET_UP")


def test_net_m_without_grad_tap(T):
    _run(T, "NET_M", keep_grads=False)


def test_net_m_graph_replay(T):
    _run(T, "NET_M", steps=3, graph=True)


def test_net_t_graph_replay(T):
    _run(T, "NET_T", steps=3, graph=True)


def test_net_m_autotune_keeps_results(T):
    from niti_amd.model import NitiModel
    try:
        _run(T, "NET_M", prepare=lambda m: m.autotune(reps=2))
    finally:
        NitiModel.reset_plans()


def test_net_t_autotune_keeps_results(T):
    from niti_amd.model import NitiModel
    try:
        _run(T, "NET_T", prepare=lambda m: m.autotune(reps=2))
    finally:
        NitiModel.reset_plans()


def test_net_m_run_phase_and_probe(T):
    """Each phase of the strided layers again, alone: the same buffers; the probe times its launches."""
    layers, W, S, data, ref = _ref("NET_M", 3)
    m = _model("NET_M", 3)
    m.set_update_bits(0)  # every layer frozen: the phases run again on the weights the step ran on
    m.train_step(T.from_numpy(data[0][0].copy()).cuda(), -3, T.from_numpy(data[0][1].copy()).cuda())
    rec = ref[0][1]
    m.set_probe(3, 1, 8)
    for ph in (0, 1, 2):
        m.run_phase(3, ph)
        m.run_phase(5, ph)
        if ph != 1:
            m.run_phase(0, ph)
    T.cuda.synchronize()
    ms, count = m.probe_read()
    assert count == 1 and ms > 0
    m.set_probe(-1, -1, 0)
    for i in range(6):
        assert np.array_equal(m.tap(i, 0), rec["r"][i]) and np.array_equal(m.tap(i, 2), rec["dy"][i]), i


def test_net_m_update_bits(T):
    """A frozen strided depthwise layer keeps its weights; the strided first layer follows the reference at 4 bits."""
    bits = (4, 2, 2, 0, 2, 4, 2, 2)
    m = _run(T, "NET_M", bits=bits)
    assert m.update_bits() == list(bits)
    _, W, _, _, ref = _ref("NET_M", 3, 2, bits)
    assert np.array_equal(m.get_weight(3), W[3]) and not np.array_equal(m.get_weight(0), W[0])


def test_net_t_update_bits_keep_the_class_weights_current(T):
    """The strided layer's sub-pixel class weights follow a 4-bit update: the second step's input gradient reads them."""
    _run(T, "NET_T", bits=(2, 4, 2, 2, 2))


def test_net_m_evaluate_padded_tail(T):
    import eval_cases as E
    import niti_oracle as O
    layers, W, S, _, _ = _ref("NET_M", 3)
    rng = np.random.default_rng(9)
    img = rng.integers(0, 256, (7, 3, 16, 16)).astype(np.uint8)
    lab = rng.integers(0, 10, 7).astype(np.int32)
    m = _model("NET_M", 3)
    got = m.evaluate(img, lab)
    want = {"images": 0, "top1": 0, "topk": 0, "loss_sum": 0.0}
    for i in range(0, 7, 3):
        bi = np.concatenate([img[i:i + 3], np.zeros((max(0, i + 3 - 7), 3, 16, 16), np.uint8)])
        bl = np.concatenate([lab[i:i + 3], np.full(max(0, i + 3 - 7), -1, np.int32)])
        x, a = O.quantize_images(bi)
        _, rec = SC.chain_step_ref(layers, W, S, x, a, np.maximum(bl, 0))
        want = E.add_totals(want, E.metrics_ref(rec["logits"], rec["exp"][-1], bl, 5))
    assert (got["images"], got["top1"], got["topk"]) == (7, want["top1"], want["topk"])
    assert E.loss_close(got["loss_sum"], want["loss_sum"])
    for i in range(len(layers)):  # evaluation writes no weight
        assert np.array_equal(m.get_weight(i), W[i])


def test_net_m_fit_epoch_equals_the_reference(T):
    from niti_amd.dataset import DeviceDataset, make_order
    layers, W, S, _, _ = _ref("NET_M", 3)
    rng = np.random.default_rng(10)
    img = rng.integers(0, 256, (6, 3, 16, 16)).astype(np.uint8)
    lab = rng.integers(0, 10, 6).astype(np.int32)
    m = _model("NET_M", 3)
    steps = m.fit_epoch(DeviceDataset(img, lab), seed=3, epoch=1)
    assert steps == 2
    index, _ = make_order(6, 3, seed=3, epoch=1, drop_last=True)
    ref = SC.ref_steps(layers, W, S, [(img[index[k * 3:(k + 1) * 3]], lab[index[k * 3:(k + 1) * 3]]) for k in range(steps)])
    T.cuda.synchronize()
    _compare(m, layers, ref[-1][0], ref[-1][1], steps - 1)


def test_net_m_snapshots(T, tmp_path):
    """Both snapshot formats carry the strides; a list that differs only in one stride is refused before
    any device write."""
    from niti_amd.model import NitiModel
    in_c, in_hw, spec = SC.NET_M
    layers, W, S, _, _ = _ref("NET_M", 3)
    m = _model("NET_M", 3)
    assert [d["stride"] for d in m.chain] == [2, 1, 1, 2, 1, 2, 1, 1]
    p, q = str(tmp_path / "a.safetensors"), str(tmp_path / "a.mnn")
    m.save(p)
    m.save_mnn(q)
    # the same weight shapes under other strides
    other_spec = [tuple(l) for l in spec]
    other_spec[1] = other_spec[1][:7] + (2,)   # the first depthwise layer strided too (8 -> 4)
    other_spec[3] = other_spec[3][:7] + (1,)   # and the second one not: every later map as before
    assert [SC.weight_shape(l) for l in SC.derive((in_c, in_hw, other_spec))] == [SC.weight_shape(l) for l in layers]
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


def test_net_m_and_net_t_copy_weights(T):
    from niti_amd._lib import NitiError
    from niti_amd.model import NitiModel
    for net in ("NET_M", "NET_T"):
        in_c, in_hw, spec = SC.NETS[net]
        layers, W, S, _, _ = _ref(net, 3)
        src = _model(net, 3)
        dst = NitiModel.from_chain(spec, in_c, in_hw, 3)
        dst.copy_weights_from(src)
        for i, w in enumerate(W):
            assert np.array_equal(dst.get_weight(i), w), i
        (x, labels), = SC.batches(layers, 3, 1, seed=12)
        newW, rec, _, _ = SC.ref_steps(layers, W, S, [(x, labels)])[0]
        dst.train_step(T.from_numpy(x.copy()).cuda(), -3, T.from_numpy(labels.copy()).cuda())
        _compare(dst, layers, newW, rec, 0)
    # the same weight shapes under other strides: another network
    in_c, in_hw, spec = SC.NET_M
    moved = [tuple(l) for l in spec]
    moved[1] = moved[1][:7] + (2,)
    moved[3] = moved[3][:7] + (1,)
    with pytest.raises(NitiError):
        NitiModel.from_chain(moved, in_c, in_hw, 3).copy_weights_from(_model("NET_M", 3))


def test_net_m_two_local_ranks_equal_one_device(T):
    from niti_amd.model import LocalGroup
    layers, W, S, data, ref = _ref("NET_M", 4)
    ranks = [_model("NET_M", 2) for _ in range(2)]
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


def test_old_entry_point_still_refuses_and_stride_1_lists_take_it(T):
    """from_chain sends only lists with a strided layer through niti_model_create_chain3."""
    from niti_amd import _lib as L
    in_c, in_hw, spec = SC.NET_T
    arr = (L.ChainLayer2 * len(spec))()
    for s, (co, k, pad, relu, pool, fl, dw, st) in zip(arr, spec):
        s.c_out, s.kernel, s.stride, s.pad, s.relu, s.pool, s.flatten, s.depthwise = co, k, st, pad, relu, pool, fl, dw
    h = C.c_void_p()
    assert L.lib().niti_model_create_chain2(arr, len(arr), in_c, in_hw, 3, C.byref(h)) == L.NOT_SUPPORT and not h
    assert L.lib().niti_model_create_chain3(arr, len(arr), in_c, in_hw, 3, C.byref(h)) == 0 and h
    L.lib().niti_model_destroy(h)
