"""GPU parity of user-defined chain networks (NitiModel.from_chain) against the oracle's NITI_SGD step.

Every case compares logits, exponents, taps 0 / 1 / 2 and every layer's weights bit for bit over
two steps at batch 6 unless said otherwise, as tests/test_gpu_model.py::_run does for the built-in
networks.  The nets (tests/chain_cases.py) are the smallest that reach each path of the chain
driver no built-in network runs.
"""
import ctypes as C
import functools
import threading

import numpy as np
import pytest

import chain_cases as CC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def T():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import niti_amd  # noqa: F401
    return torch


@functools.lru_cache(maxsize=None)
def _ref(net, batch, steps, seed, images=False, own_step=False):
    """(layers, W, S, data, oracle steps) of a named net: computed once, shared, never written."""
    import niti_model_ref as R
    layers = CC.derive(getattr(CC, net))
    W, S = R.init_weights(layers, seed=seed)
    data = CC.batches(layers, batch, steps, seed + 1, images=images)
    return layers, W, S, data, CC.ref_steps(layers, W, S, data, step_fn=CC.chain_step_ref if own_step else None)


def _model(net, batch, W, S):
    from niti_amd.model import NitiModel
    in_c, in_hw, spec = getattr(CC, net)
    m = NitiModel.from_chain(spec, in_c, in_hw, batch)
    for i, (w, s) in enumerate(zip(W, S)):
        m.set_weight(i, w, s)
    return m


def _compare(m, layers, newW, rec, step, keep_grads=True, rowconv=True):
    from niti_amd._lib import NitiError
    logits, e = m.logits()
    assert e == rec["exp"][-1], (step, e, rec["exp"][-1])
    assert np.array_equal(logits, rec["logits"]), step
    for i in range(len(layers)):
        if not keep_grads and layers[i]["pool"] and rowconv:
            # keep_grads(0): a pooled layer whose 2x2 route went on as codes writes no pre-pool output
            try:
                fwd = m.tap(i, 0)
            except NitiError:
                fwd = None
            assert fwd is None or np.array_equal(fwd, rec["r"][i]), ("fwd", step, i)
        else:
            assert np.array_equal(m.tap(i, 0), rec["r"][i]), ("fwd", step, i)
        assert np.array_equal(m.tap(i, 2), rec["dy"][i]), ("dy", step, i)
        if keep_grads:
            assert np.array_equal(m.tap(i, 1), rec["dw"][i]), ("dw", step, i)
        assert np.array_equal(m.get_weight(i), newW[i]), ("w", step, i)


def _run(T, net, batch=6, steps=2, seed=5, images=False, own_step=False, rowconv=True, keep_grads=True, graph=False,
         prepare=None):
    layers, W, S, data, ref = _ref(net, batch, steps, seed, images, own_step)
    m = _model(net, batch, W, S)
    assert m.arch == 5 and [l["c_out"] for l in m.layers] == [l["co"] for l in layers]
    m.set_graph(graph)
    m.set_rowconv(rowconv)
    m.keep_grads(keep_grads)
    xd = ld = None
    if prepare is not None:  # after one throwaway step; the weights are set again after it
        m.train_step(T.from_numpy(data[0][0]).cuda(), -3, T.from_numpy(data[0][1]).cuda())
        prepare(m)
        for i, (w, s) in enumerate(zip(W, S)):
            m.set_weight(i, w, s)
    for step, ((x, labels), (newW, rec, xq, e_in)) in enumerate(zip(data, ref)):
        if xd is None:
            xd, ld = T.from_numpy(x).cuda(), T.from_numpy(labels).cuda()
        else:  # (the same device buffers: a captured graph replays)
            xd.copy_(T.from_numpy(x))
            ld.copy_(T.from_numpy(labels))
        if images:
            m.train_step_images(xd, ld)
            xin, a = m.input()
            assert a == e_in and np.array_equal(xin, xq), step
        else:
            m.train_step(xd, -3, ld)
        _compare(m, layers, newW, rec, step, keep_grads, rowconv)
    assert m.rowconv_error() == 0
    return m


@pytest.mark.parametrize("images", [False, True])
def test_net_a_general_first_layer_odd_pool_wide_head(T, images):
    """c_in k k = 36 > 32: no im2col copy, layer 0 on the implicit GEMM; a 2x2 pool on a 9-px map
    (the unfused pool and pool-gradient kernels); a 20-class head behind a 36-wide layer."""
    _run(T, "NET_A", images=images)


@pytest.mark.parametrize("images", [False, True])
@pytest.mark.parametrize("rowconv", [True, False])
def test_net_b_im2col32_rows_7_class_head(T, images, rowconv):
    """1 x 3 x 3 first layer: an im2col copy the fused input pass does not write (the generic
    im2col32 kernel); row kernels on 8 / 4 / 2 px; a 7-class head through the pooled 1x1 route."""
    _run(T, "NET_B", images=images, rowconv=rowconv)


def test_net_b_without_grad_tap(T):
    _run(T, "NET_B", seed=6, keep_grads=False)


def test_net_b_graph_replay(T):
    _run(T, "NET_B", steps=3, seed=7, graph=True)


def test_net_c_5x5_100_classes(T):
    _run(T, "NET_C")


@pytest.mark.parametrize("images", [False, True])
def test_net_f_pads_past_half_the_kernel(T, images):
    """A 3 x 3 x 3 first layer with pad 2 must not take the fused input pass (its staged rows hold
    w + 2 columns): the quantiser / layout pass and im2col32 feed it; then 5x5 / pad 3 on the GEMM."""
    _run(T, "NET_F", images=images)


def test_net_g_7x7(T):
    """49 taps: the per-lane loaders, forward, input gradient and weight gradient."""
    _run(T, "NET_G")


@pytest.mark.parametrize("net", ["NET_D", "NET_D2"])
def test_net_d_flatten_without_pool(T, net):
    """The flatten reads the conv (+relu) output itself and its gradient goes through the relu
    gradient alone: on the GEMM path (D) and behind a row-kernel layer (D2)."""
    _run(T, net, own_step=True)


@pytest.mark.parametrize("net,arch,batch", [("LENET", "ARCH_LENET", 16), ("VGG11", "ARCH_VGG11", 8)])
def test_builtins_through_the_list(T, net, arch, batch):
    """The same network by name and by list: identical results and plans, step after step."""
    import niti_amd
    import niti_model_ref as R
    from niti_amd.model import NitiModel
    layers = CC.derive(getattr(CC, net))
    W, S = R.init_weights(layers, seed=31)
    a = NitiModel(getattr(niti_amd, arch), batch)
    for i, (w, s) in enumerate(zip(W, S)):
        a.set_weight(i, w, s)
    b = _model(net, batch, W, S)
    assert a.layers == b.layers and a.plans() == b.plans() and a.step_macs() == b.step_macs()
    rng = np.random.default_rng(32)
    l0 = layers[0]
    for step in range(2):
        x = T.from_numpy(rng.integers(-127, 128, (batch, l0["ci"], l0["h"], l0["h"])).astype(np.int8)).cuda()
        lab = T.from_numpy(rng.integers(0, 10, batch).astype(np.int32)).cuda()
        a.train_step(x, -3, lab)
        b.train_step(x, -3, lab)
        (la, ea), (lb, eb) = a.logits(), b.logits()
        assert ea == eb and np.array_equal(la, lb), step
        for i in range(len(layers)):
            assert np.array_equal(a.get_weight(i), b.get_weight(i)), (step, i)
            assert np.array_equal(a.tap(i, 2), b.tap(i, 2)), (step, i)
    assert a.plans() == b.plans() and b.rowconv_error() == 0


def test_net_b_autotune_keeps_results(T):
    from niti_amd.model import NitiModel
    try:
        _run(T, "NET_B", batch=32, seed=8, prepare=lambda m: m.autotune(reps=2))
    finally:
        NitiModel.reset_plans()


def test_net_b_evaluate_padded_tail(T):
    """13 images at batch 6: three batches, the last padded; totals against eval_cases' reference on
    the oracle's logits of each batch's own quantised input."""
    import eval_cases as E
    import niti_model_ref as R
    import niti_oracle as O
    layers, W, S, _, _ = _ref("NET_B", 6, 2, 5)
    rng = np.random.default_rng(9)
    img = rng.integers(0, 256, (13, 1, 8, 8)).astype(np.uint8)
    lab = rng.integers(0, 7, 13).astype(np.int32)
    m = _model("NET_B", 6, W, S)
    got = m.evaluate(img, lab)
    want = {"images": 0, "top1": 0, "topk": 0, "loss_sum": 0.0}
    for i in range(0, 13, 6):
        bi = np.concatenate([img[i:i + 6], np.zeros((max(0, i + 6 - 13), 1, 8, 8), np.uint8)])
        bl = np.concatenate([lab[i:i + 6], np.full(max(0, i + 6 - 13), -1, np.int32)])
        x, a = O.quantize_images(bi)
        _, rec = R.train_step(layers, W, S, x, a, np.maximum(bl, 0), classes=7)
        want = E.add_totals(want, E.metrics_ref(rec["logits"], rec["exp"][-1], bl, 5))
    assert (got["images"], got["top1"], got["topk"]) == (13, want["top1"], want["topk"])
    assert E.loss_close(got["loss_sum"], want["loss_sum"])
    for i in range(len(layers)):  # evaluation writes no weight
        assert np.array_equal(m.get_weight(i), W[i])
    assert m.rowconv_error() == 0


def test_net_b_fit_epoch_equals_host_fed_steps(T):
    from niti_amd.dataset import DeviceDataset, make_order
    layers, W, S, _, _ = _ref("NET_B", 6, 2, 5)
    rng = np.random.default_rng(10)
    img = rng.integers(0, 256, (24, 1, 8, 8)).astype(np.uint8)
    lab = rng.integers(0, 7, 24).astype(np.int32)
    a, b = _model("NET_B", 6, W, S), _model("NET_B", 6, W, S)
    steps = a.fit_epoch(DeviceDataset(img, lab), seed=3, epoch=1)
    assert steps == 4
    index, _ = make_order(24, 6, seed=3, epoch=1, drop_last=True)
    for k in range(steps):
        sel = index[k * 6:(k + 1) * 6]
        b.train_step_images(T.from_numpy(img[sel]).cuda(), T.from_numpy(lab[sel]).cuda())
    T.cuda.synchronize()
    (la, ea), (lb, eb) = a.logits(), b.logits()
    assert ea == eb and np.array_equal(la, lb)
    for i in range(len(layers)):
        assert np.array_equal(a.get_weight(i), b.get_weight(i)), i
    assert a.rowconv_error() == 0


def test_copy_weights_between_chain_models(T):
    import niti_amd
    from niti_amd._lib import NitiError
    from niti_amd.model import NitiModel
    layers, W, S, _, _ = _ref("NET_B", 6, 2, 5)
    src = _model("NET_B", 6, W, S)
    dst = NitiModel.from_chain(CC.NET_B[2], 1, 8, 4)
    dst.copy_weights_from(src)
    for i in range(len(layers)):
        assert np.array_equal(dst.get_weight(i), W[i]), i
    # the same geometry with another relu is another network; so is a built-in model
    other = [tuple(l) for l in CC.NET_B[2]]
    other[0] = (32, 3, 1, 0, 0, 0)
    with pytest.raises(NitiError):
        NitiModel.from_chain(other, 1, 8, 4).copy_weights_from(src)
    with pytest.raises(NitiError):
        NitiModel(niti_amd.ARCH_LENET, 4).copy_weights_from(src)
    with pytest.raises(NitiError):
        src.copy_weights_from(NitiModel(niti_amd.ARCH_LENET, 4))
    # copied weights train as set ones do
    (x, labels), = CC.batches(layers, 4, 1, seed=12)
    newW, rec, _, _ = CC.ref_steps(layers, W, S, [(x, labels)])[0]
    dst.train_step(T.from_numpy(x).cuda(), -3, T.from_numpy(labels).cuda())
    _compare(dst, layers, newW, rec, 0)
    assert dst.rowconv_error() == 0 and src.rowconv_error() == 0


def test_net_b_two_local_ranks_equal_one_device(T):
    from niti_amd.model import LocalGroup
    layers, W, S, data, ref = _ref("NET_B", 6, 2, 5)
    ranks = [_model("NET_B", 3, W, S) for _ in range(2)]
    group = LocalGroup(2)
    for r, m in enumerate(ranks):
        m.attach_local(group, r, exact=True)
    streams = [T.cuda.Stream() for _ in range(2)]
    for step, ((x, labels), (newW, rec, _, _)) in enumerate(zip(data, ref)):
        xd, ld = T.from_numpy(x).cuda(), T.from_numpy(labels).cuda()
        parts = [(xd[r * 3:(r + 1) * 3].contiguous(), ld[r * 3:(r + 1) * 3].contiguous()) for r in range(2)]
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
            sl = slice(r * 3, (r + 1) * 3)
            lg, e = m.logits()
            assert e == rec["exp"][-1] and np.array_equal(lg, rec["logits"][sl]), (step, r)
            for i in range(len(layers)):
                assert np.array_equal(m.tap(i, 0), rec["r"][i][sl]), ("fwd", step, r, i)
                assert np.array_equal(m.tap(i, 2), rec["dy"][i][sl]), ("dy", step, r, i)
                assert np.array_equal(m.tap(i, 1), rec["dw"][i]), ("dw", step, r, i)
                assert np.array_equal(m.get_weight(i), newW[i]), ("w", step, r, i)
    assert all(m.rowconv_error() == 0 for m in ranks)


def test_refused_list_allocates_nothing(T):
    """niti_model_create_chain returns the check's code and leaves *out as it was."""
    import niti_amd
    from niti_amd import _lib as L
    from niti_amd._lib import NitiError
    from niti_amd.model import NitiModel
    lib = L.lib()
    for layers, want in ([(10, 3, 2, 1, 0, 0, 0)], L.NOT_SUPPORT), ([(10, 3, 1, 3, 0, 0, 0)], L.INVALID_VALUE), ([(2049, 1, 1, 0, 0, 0, 0)], L.NOT_SUPPORT):
        arr = (L.ChainLayer * 1)()
        arr[0].c_out, arr[0].kernel, arr[0].stride, arr[0].pad = layers[0][:4]
        out = C.c_void_p(0x5a5a)
        assert lib.niti_model_chain_check(arr, 1, 3, 1, None) == want
        assert lib.niti_model_create_chain(arr, 1, 3, 1, 4, C.byref(out)) == want
        assert out.value == 0x5a5a
    # a list the check passes at batch 1 and refuses at the model's batch (a tensor past 2^29 elements)
    big = [(64, 3, 1, 1, 1, 0)] + [(8, 1, 0, 1, 1, 0)] * 9 + [(10, 1, 0, 0, 0, 0)]
    assert niti_amd.chain_layers(big, 4, 1024)[0]["h"] == 1024
    with pytest.raises(NitiError) as e:
        NitiModel.from_chain(big, 4, 1024, 16)
    assert e.value.code == L.NOT_SUPPORT
    with pytest.raises(ValueError):
        NitiModel.from_chain([(10, 3, 3)], 3, 1, 4)


def test_snapshot_round_trip_and_init(T, tmp_path):
    """init_weights is xavier_int8 in layer order; save / load carry the list and refuse another."""
    from niti_amd.init import xavier_int8
    from niti_amd.model import NitiModel
    in_c, in_hw, spec = CC.NET_A
    m = NitiModel.from_chain(spec, in_c, in_hw, 2)
    m.init_weights(4)
    rng = np.random.default_rng(4)
    want = [xavier_int8(m.weight_shape(i), rng) for i in range(len(m.layers))]
    for i, (w, s) in enumerate(want):
        assert np.array_equal(m.get_weight(i), w) and m._wscale[i] == s
    p, q = str(tmp_path / "a.safetensors"), str(tmp_path / "a.mnn")
    m.save(p)
    m.save_mnn(q)
    for load in ("load", "load_mnn"):
        path = p if load == "load" else q
        same = NitiModel.from_chain(spec, in_c, in_hw, 3)
        getattr(same, load)(path)
        for i, (w, _) in enumerate(want):
            assert np.array_equal(same.get_weight(i), w)
        other = NitiModel.from_chain([spec[0], spec[1], (36, 1, 0, 0, 0, 0), spec[3]], in_c, in_hw, 3)  # a relu less
        with pytest.raises(ValueError):
            getattr(other, load)(path)
        assert not np.any(other.get_weight(0))  # refused before any device write
