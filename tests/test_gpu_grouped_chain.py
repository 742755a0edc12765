"""GPU parity of chain networks with grouped conv layers (NitiModel.from_chain) against the step reference of
tests/grouped_cases.py: three steps at batch 4, every layer's weights after each step and the logits, bit for bit."""
import ctypes as C
import threading

import numpy as np
import pytest

import grouped_cases as GC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def T():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import niti_amd  # noqa: F401
    return torch


def _model(name, batch, spec=None, seed=3):
    from niti_amd.model import NitiModel
    net = GC.NETS[name]
    m = NitiModel.from_chain(spec or net[2], net[0], net[1], batch)
    m.init_weights(seed)
    return m


def _compare(m, newW, rec, step, sl=slice(None)):
    logits, e = m.logits()
    assert e == rec["exp"][-1], (step, e, rec["exp"][-1])
    assert np.array_equal(logits, rec["logits"][sl]), step
    for i, w in enumerate(newW):
        assert np.array_equal(m.get_weight(i), w), ("w", step, i)


@pytest.mark.parametrize("graph", (False, True))
@pytest.mark.parametrize("name", sorted(GC.NETS))
def test_three_steps(T, name, graph):
    """Eagerly with the gradient taps kept; as a captured graph (replayed twice) without them."""
    layers, W, S, data, ref = GC.reference(name)
    m = _model(name, GC.BATCH)
    assert [l.get("groups", 1) for l in m.layers] == [l["groups"] for l in layers]
    for i, (w, s) in enumerate(zip(W, S)):  # init_weights: xavier_int8 on [c_out, cg, 3, 3] for such a layer
        assert m.weight_shape(i) == GC.weight_shape(layers[i])
        assert np.array_equal(m.get_weight(i), w) and m._wscale[i] == s
    m.set_graph(graph)
    m.keep_grads(not graph)
    xd, ld = T.from_numpy(data[0][0].copy()).cuda(), T.from_numpy(data[0][1].copy()).cuda()
    for step, ((x, labels), (newW, rec)) in enumerate(zip(data, ref)):
        xd.copy_(T.from_numpy(x.copy()))  # (the same device buffers: a captured graph replays)
        ld.copy_(T.from_numpy(labels.copy()))
        m.train_step(xd, -3, ld)
        _compare(m, newW, rec, step)
    assert m.rowconv_error() == 0
    assert not any(layers[i]["groups"] > 1 for i, _ in m.plans())  # no GEMM plan on such a layer
    # MACs count cg: forward + weight gradient (+ input gradient past layer 0)
    per = [GC.BATCH * (l["h"] + 2 * l["pad"] - l["k"] + 1) ** 2 * l["co"] * (l["ci"] // l["groups"]) * l["k"] ** 2 for l in layers]
    assert m.step_macs() == sum(p * (2 if i == 0 else 3) for i, p in enumerate(per))


def test_two_local_ranks_equal_one_device(T):
    from niti_amd.model import LocalGroup
    layers, W, S, data, ref = GC.reference("NET_X")
    ranks = [_model("NET_X", 2) for _ in range(2)]
    group = LocalGroup(2)
    for r, m in enumerate(ranks):
        m.attach_local(group, r, exact=True)
    streams = [T.cuda.Stream() for _ in range(2)]
    for step, ((x, labels), (newW, rec)) in enumerate(zip(data, ref)):
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
            _compare(m, newW, rec, (step, r), sl=slice(r * 2, (r + 1) * 2))


def test_save_load_and_copy_refuse_another_groups(T, tmp_path):
    from niti_amd._lib import NitiError
    _, W, S, _, _ = GC.reference("NET_R")
    m = _model("NET_R", 2)
    assert [d["groups"] for d in m.chain] == [1, 2, 1, 4, 1]
    other_spec = list(GC.NET_R[2])
    other_spec[3] = other_spec[3][:10] + (2,)  # (64 channels in 2 groups of 32: the same list but for this)
    paths = {"load": str(tmp_path / "a.safetensors"), "load_mnn": str(tmp_path / "a.mnn")}
    m.save(paths["load"])
    m.save_mnn(paths["load_mnn"])
    for load, path in paths.items():
        same, other = _model("NET_R", 3), _model("NET_R", 2, other_spec, seed=4)
        before = other.get_weight(0)
        getattr(same, load)(path)
        assert all(np.array_equal(same.get_weight(i), w) and same._wscale[i] == S[i] for i, w in enumerate(W))
        with pytest.raises(ValueError):
            getattr(other, load)(path)
        assert np.array_equal(other.get_weight(0), before)  # refused before any device write
    with pytest.raises(NitiError):
        _model("NET_R", 2, other_spec).copy_weights_from(m)
    dst = _model("NET_R", 3)
    dst.copy_weights_from(m)
    assert all(np.array_equal(dst.get_weight(i), w) for i, w in enumerate(W))


def test_evaluate_against_the_forward_reference(T):
    import eval_cases as E
    from grouped_cases import O
    layers, W, S, _, _ = GC.reference("NET_X")
    rng = np.random.default_rng(9)
    img = rng.integers(0, 256, (8, 3, 8, 8)).astype(np.uint8)
    lab = rng.integers(0, 10, 8).astype(np.int32)
    m = _model("NET_X", GC.BATCH)
    got = m.evaluate(img, lab)
    want = {"images": 0, "top1": 0, "topk": 0, "loss_sum": 0.0}
    for i in range(0, 8, 4):
        x, a = O.quantize_images(img[i:i + 4])
        _, rec = GC.chain_step_ref(layers, W, S, x, a, lab[i:i + 4])
        want = E.add_totals(want, E.metrics_ref(rec["logits"], rec["exp"][-1], lab[i:i + 4], 5))
    assert (got["images"], got["top1"], got["topk"]) == (8, want["top1"], want["topk"])
    assert E.loss_close(got["loss_sum"], want["loss_sum"])
    assert all(np.array_equal(m.get_weight(i), w) for i, w in enumerate(W))  # evaluation writes no weight
