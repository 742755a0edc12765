"""GPU parity of the forward-only evaluation step (niti_model_eval_*) and the device-to-device
weight hand-over (niti_model_copy_weights).

The evaluation logits and their exponent must equal the oracle's forward on the same weights
(niti_model_ref / niti_resnet_ref train_step records: computed before the update) bit for bit, no
weight may change, and the predictions and running totals must equal the NumPy helper
(tests/eval_cases.py) applied to the oracle logits: integer counts exactly, loss_sum within
eval_cases.LOSS_RTOL.  Interleaved with training steps (direct launches and graph replay) both must
stay exact.
"""
import ctypes as C
import threading

import numpy as np
import pytest

import eval_cases as E

pytestmark = pytest.mark.gpu

TOPK = 5  # the models' default


@pytest.fixture(scope="module")
def T():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import niti_amd  # noqa: F401
    return torch


def _dev(T, a):
    return T.from_numpy(np.ascontiguousarray(a)).cuda()


def _set(m, W, S):
    for i, (w, s) in enumerate(zip(W, S)):
        m.set_weight(i, w, s)


def _check_totals(got, want):
    assert (got["images"], got["top1"], got["topk"]) == (want["images"], want["top1"], want["topk"]), (got, want)
    assert E.loss_close(got["loss_sum"], want["loss_sum"]), (got, want)
    if want["images"]:
        assert E.loss_close(got["loss"], want["loss_sum"] / want["images"])
        assert got["accuracy"] == want["top1"] / want["images"]


def _check_eval(m, logits, exp, labels, W):
    """the model after one eval_step (from reset totals) against the oracle's logits / exponent"""
    lg, e = m.logits()
    assert e == exp and np.array_equal(lg, logits)
    for i in range(len(m.layers)):
        assert np.array_equal(m.get_weight(i), W[i]), ("w", i)
    want = E.metrics_ref(logits, exp, labels, TOPK)
    assert np.array_equal(m.predictions(), want["pred"])
    _check_totals(m.eval_read(), want)
    assert m.rowconv_error() == 0


@pytest.mark.parametrize("arch,batch,rowconv", [("lenet", 16, True), ("vgg11", 8, True), ("vgg11", 8, False)])
def test_eval_step_matches_oracle(T, arch, batch, rowconv):
    import niti_amd
    import niti_model_ref as R
    from niti_amd.model import NitiModel
    layers = R.lenet_layers() if arch == "lenet" else R.vgg11_layers()
    W, S = R.init_weights(layers, seed=21)
    rng = np.random.default_rng(21 + batch)
    l0 = layers[0]
    x = rng.integers(-127, 128, (batch, l0["ci"], l0["h"], l0["h"])).astype(np.int8)
    labels = rng.integers(0, 10, batch).astype(np.int32)
    labels[1] = -1  # an excluded image
    _, rec = R.train_step(layers, W, S, x, -3, np.maximum(labels, 0))
    m = NitiModel(niti_amd.ARCH_LENET if arch == "lenet" else niti_amd.ARCH_VGG11, batch)
    m.set_rowconv(rowconv)
    _set(m, W, S)
    m.eval_reset()
    m.eval_step(_dev(T, x), -3, _dev(T, labels))
    _check_eval(m, rec["logits"], rec["exp"][-1], labels, W)
    # a second batch accumulates; top-k follows eval_topk
    m.eval_topk(1)
    m.eval_step(_dev(T, x), -3, _dev(T, labels))
    w5, w1 = E.metrics_ref(rec["logits"], rec["exp"][-1], labels, 5), E.metrics_ref(rec["logits"], rec["exp"][-1], labels, 1)
    _check_totals(m.eval_read(), E.add_totals(w5, w1))


@pytest.mark.parametrize("hw,batch,classes", [(32, 2, 10), (64, 3, 1000)])
def test_resnet18_eval_step_matches_oracle(T, hw, batch, classes):
    import niti_amd
    import niti_resnet_ref as RR
    from niti_amd.model import NitiModel
    convs = RR.resnet18_convs(hw, classes)
    W, S = RR.init_weights(convs, seed=hw + batch)
    rng = np.random.default_rng(hw * batch + 1)
    x = rng.integers(-127, 128, (batch, 3, hw, hw)).astype(np.int8)
    labels = rng.integers(0, classes, batch).astype(np.int32)
    _, rec = RR.train_step(convs, W, S, x, -2, labels, classes=classes)
    m = NitiModel(niti_amd.ARCH_RESNET18, batch, hw, classes)
    _set(m, W, S)
    m.eval_reset()
    m.eval_step(_dev(T, x), -2, _dev(T, labels))
    _check_eval(m, rec["logits"], rec["exp_logits"], labels, W)


_INTERLEAVE = {}


def _interleave_oracle():
    """train(x0), eval(x1), train(x2), eval(x3) on the oracle, once for both launch modes"""
    if _INTERLEAVE:
        return _INTERLEAVE
    import niti_model_ref as R
    layers = R.vgg11_layers()
    W, S = R.init_weights(layers, seed=31)
    rng = np.random.default_rng(31)
    xs = [rng.integers(-127, 128, (8, 3, 32, 32)).astype(np.int8) for _ in range(4)]
    ls = [rng.integers(0, 10, 8).astype(np.int32) for _ in range(4)]
    W1, rec0 = R.train_step(layers, W, S, xs[0], -3, ls[0])
    _, rec1 = R.train_step(layers, W1, S, xs[1], -4, ls[1])
    W2, rec2 = R.train_step(layers, W1, S, xs[2], -3, ls[2])
    _, rec3 = R.train_step(layers, W2, S, xs[3], -2, ls[3])
    _INTERLEAVE.update(layers=layers, W=[W, W1, W2], S=S, xs=xs, ls=ls, rec=[rec0, rec1, rec2, rec3])
    return _INTERLEAVE


@pytest.mark.parametrize("graph", [False, True], ids=["direct", "graph"])
def test_eval_interleaved_with_training(T, graph):
    """train, eval on other data, train, eval: the training steps match the oracle's two consecutive
    steps (logits, every tap, the weights) and the evaluation steps its forward at the then-current
    weights; taps 1 and 2 keep the last training step's data across an evaluation step.  With
    set_graph(True) the second training step replays the captured graph (same device buffers)."""
    import niti_amd
    from niti_amd.model import NitiModel
    o = _interleave_oracle()
    layers, S = o["layers"], o["S"]
    m = NitiModel(niti_amd.ARCH_VGG11, 8)
    m.set_graph(graph)
    _set(m, o["W"][0], S)
    xt, lt = _dev(T, o["xs"][0]).clone(), _dev(T, o["ls"][0]).clone()  # the training step's buffers

    def check_train(rec, newW, tag, fwd=True):
        for i in range(len(layers)):
            if fwd:
                assert np.array_equal(m.tap(i, 0), rec["r"][i]), ("fwd", tag, i)
            assert np.array_equal(m.tap(i, 2), rec["dy"][i]), ("dy", tag, i)
            assert np.array_equal(m.tap(i, 1), rec["dw"][i]), ("dw", tag, i)
            assert np.array_equal(m.get_weight(i), newW[i]), ("w", tag, i)

    for k, (exp_eval, Wk) in enumerate([(-4, o["W"][1]), (-2, o["W"][2])]):
        ti, ei = 2 * k, 2 * k + 1
        xt.copy_(_dev(T, o["xs"][ti]))
        lt.copy_(_dev(T, o["ls"][ti]))
        m.train_step(xt, -3, lt)
        lg, e = m.logits()
        assert e == o["rec"][ti]["exp"][-1] and np.array_equal(lg, o["rec"][ti]["logits"]), ti
        check_train(o["rec"][ti], Wk, ti)
        m.eval_reset()
        m.eval_step(_dev(T, o["xs"][ei]), exp_eval, _dev(T, o["ls"][ei]))
        _check_eval(m, o["rec"][ei]["logits"], o["rec"][ei]["exp"][-1], o["ls"][ei], Wk)
        xin, ein = m.input()
        assert ein == exp_eval and np.array_equal(xin, o["xs"][ei])
        for i in range(len(layers)):  # tap 0 describes the evaluation batch, taps 1 / 2 the training step
            assert np.array_equal(m.tap(i, 0), o["rec"][ei]["r"][i]), ("eval fwd", ei, i)
        check_train(o["rec"][ti], Wk, ("after eval", ti), fwd=False)


def test_eval_step_images(T):
    import niti_amd
    import niti_model_ref as R
    import niti_oracle as O
    from niti_amd.model import NitiModel
    layers = R.vgg11_layers()
    W, S = R.init_weights(layers, seed=23)
    rng = np.random.default_rng(23)
    img = rng.integers(0, 256, (8, 3, 32, 32)).astype(np.uint8)
    labels = rng.integers(0, 10, 8).astype(np.int32)
    x, a = O.quantize_images(img)
    _, rec = R.train_step(layers, W, S, x, a, labels)
    m = NitiModel(niti_amd.ARCH_VGG11, 8)
    _set(m, W, S)
    m.eval_reset()
    m.eval_step_images(_dev(T, img), _dev(T, labels))
    xd, ad = m.input()
    assert ad == a and np.array_equal(xd, x)
    _check_eval(m, rec["logits"], rec["exp"][-1], labels, W)


def test_evaluate_pads_the_last_batch(T):
    """20 images through a batch-8 model: the last batch carries 4 zero images with label -1; the
    expected logits are computed per padded batch (the quantiser's statistics and every range are
    per batch)."""
    import niti_amd
    import niti_model_ref as R
    import niti_oracle as O
    from niti_amd.model import NitiModel
    layers = R.vgg11_layers()
    W, S = R.init_weights(layers, seed=24)
    rng = np.random.default_rng(24)
    img = rng.integers(0, 256, (20, 3, 32, 32)).astype(np.uint8)
    labels = rng.integers(0, 10, 20).astype(np.int32)
    pimg = np.concatenate([img, np.zeros((4, 3, 32, 32), np.uint8)])
    plab = np.concatenate([labels, np.full(4, -1, np.int32)])
    want = {"images": 0, "top1": 0, "topk": 0, "loss_sum": 0.0}
    for i in range(0, 24, 8):
        x, a = O.quantize_images(pimg[i:i + 8])
        _, rec = R.train_step(layers, W, S, x, a, np.maximum(plab[i:i + 8], 0))
        want = E.add_totals(want, E.metrics_ref(rec["logits"], rec["exp"][-1], plab[i:i + 8], TOPK))
    m = NitiModel(niti_amd.ARCH_VGG11, 8)
    _set(m, W, S)
    got = m.evaluate(img, labels)
    assert got["images"] == 20
    _check_totals(got, want)
    _check_totals(m.evaluate(T.from_numpy(img).cuda(), T.from_numpy(labels).cuda()), want)  # (resets first)


def test_copy_weights_from(T):
    """A batch-8 model trained two steps hands its weights to a batch-4 model on the device."""
    import niti_amd
    import niti_model_ref as R
    from niti_amd._lib import NitiError
    from niti_amd.model import NitiModel
    layers = R.vgg11_layers()
    W, S = R.init_weights(layers, seed=25)
    rng = np.random.default_rng(25)
    src = NitiModel(niti_amd.ARCH_VGG11, 8)
    _set(src, W, S)
    for _ in range(2):
        x = rng.integers(-127, 128, (8, 3, 32, 32)).astype(np.int8)
        lb = rng.integers(0, 10, 8).astype(np.int32)
        W, _ = R.train_step(layers, W, S, x, -3, lb)
        src.train_step(_dev(T, x), -3, _dev(T, lb))
    dst = NitiModel(niti_amd.ARCH_VGG11, 4)
    dst.set_rowconv(True)
    dst.copy_weights_from(src)
    for i in range(len(layers)):
        assert np.array_equal(src.get_weight(i), W[i]), ("src", i)
        assert np.array_equal(dst.get_weight(i), W[i]), ("dst", i)
    x = rng.integers(-127, 128, (4, 3, 32, 32)).astype(np.int8)
    lb = rng.integers(0, 10, 4).astype(np.int32)
    _, rec = R.train_step(layers, W, S, x, -3, lb)
    dst.eval_reset()
    dst.eval_step(_dev(T, x), -3, _dev(T, lb))
    _check_eval(dst, rec["logits"], rec["exp"][-1], lb, W)
    # the copied model trains on: its derived weight copies (input-gradient layouts) are current
    newW, rec = R.train_step(layers, W, S, x, -3, lb)
    dst.train_step(_dev(T, x), -3, _dev(T, lb))
    for i in range(len(layers)):
        assert np.array_equal(dst.get_weight(i), newW[i]), ("trained", i)
    lenet = NitiModel(niti_amd.ARCH_LENET, 4)
    with pytest.raises(NitiError) as err:
        dst.copy_weights_from(lenet)
    assert err.value.code == 5  # INVALID_VALUE
    res = NitiModel(niti_amd.ARCH_RESNET18, 2, 32, 10)
    with pytest.raises(NitiError) as err:
        res.copy_weights_from(dst)
    assert err.value.code == 5
    with pytest.raises(NitiError) as err:  # (and the other way round: the two step drivers never mix)
        dst.copy_weights_from(res)
    assert err.value.code == 5


def test_resnet18_copy_weights_from(T):
    import niti_amd
    import niti_resnet_ref as RR
    from niti_amd.model import NitiModel
    hw, classes = 32, 10
    convs = RR.resnet18_convs(hw, classes)
    W, S = RR.init_weights(convs, seed=26)
    src = NitiModel(niti_amd.ARCH_RESNET18, 2, hw, classes)
    _set(src, W, S)
    dst = NitiModel(niti_amd.ARCH_RESNET18, 3, hw, classes)
    dst.copy_weights_from(src)
    rng = np.random.default_rng(26)
    x = rng.integers(-127, 128, (3, 3, hw, hw)).astype(np.int8)
    lb = rng.integers(0, classes, 3).astype(np.int32)
    newW, rec = RR.train_step(convs, W, S, x, -2, lb, classes=classes)
    dst.eval_reset()
    dst.eval_step(_dev(T, x), -2, _dev(T, lb))
    _check_eval(dst, rec["logits"], rec["exp_logits"], lb, W)
    dst.train_step(_dev(T, x), -2, _dev(T, lb))  # the input gradients read the copied derived weights
    for i in range(len(convs)):
        assert np.array_equal(dst.get_weight(i), newW[i]), i


def _in_threads(fns):
    errs = []

    def wrap(f):
        try:
            f()
        except BaseException as e:  # noqa: BLE001 -- re-raised in the main thread
            errs.append(e)

    ts = [threading.Thread(target=wrap, args=(f,)) for f in fns]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in ts), "a rank thread hung"
    if errs:
        raise errs[0]


@pytest.mark.parametrize("images", [False, True], ids=["int8", "uint8"])
def test_local_dp_eval_equals_full_batch(T, images):
    """LocalGroup(2) x batch 4 evaluates exactly as one device at batch 8: each rank's logits are
    its slice of the full model's, the ranks' (rank-local) totals add up to the full model's."""
    import niti_amd
    import niti_model_ref as R
    from niti_amd.model import LocalGroup, NitiModel
    layers = R.vgg11_layers()
    W, S = R.init_weights(layers, seed=27)
    world, b = 2, 4
    full = NitiModel(niti_amd.ARCH_VGG11, b * world)
    ranks = [NitiModel(niti_amd.ARCH_VGG11, b) for _ in range(world)]
    group = LocalGroup(world)
    for r, m in enumerate(ranks):
        m.attach_local(group, r, exact=True)
    for m in [full] + ranks:
        _set(m, W, S)
        m.eval_reset()
    rng = np.random.default_rng(27)
    labels = rng.integers(0, 10, b * world).astype(np.int32)
    labels[5] = -1
    ld = _dev(T, labels)
    if images:
        data = _dev(T, rng.integers(0, 256, (b * world, 3, 32, 32)).astype(np.uint8))
        full.eval_step_images(data, ld)
    else:
        data = _dev(T, rng.integers(-127, 128, (b * world, 3, 32, 32)).astype(np.int8))
        full.eval_step(data, -3, ld)
    T.cuda.synchronize()
    streams = [T.cuda.Stream() for _ in range(world)]
    parts = [(data[r * b:(r + 1) * b].contiguous(), ld[r * b:(r + 1) * b].contiguous()) for r in range(world)]

    def rank_step(r):
        s = C.c_void_p(streams[r].cuda_stream)
        if images:
            ranks[r].eval_step_images(parts[r][0], parts[r][1], stream=s)
        else:
            ranks[r].eval_step(parts[r][0], -3, parts[r][1], stream=s)
        streams[r].synchronize()

    _in_threads([lambda r=r: rank_step(r) for r in range(world)])
    fl, fe = full.logits()
    fp = full.predictions()
    total = {"images": 0, "top1": 0, "topk": 0, "loss_sum": 0.0}
    for r, m in enumerate(ranks):
        sl = slice(r * b, (r + 1) * b)
        lg, e = m.logits()
        assert e == fe and np.array_equal(lg, fl[sl]), r
        assert np.array_equal(m.predictions(), fp[sl]), r
        total = E.add_totals(total, m.eval_read())
        for i in range(len(layers)):
            assert np.array_equal(m.get_weight(i), W[i]), (r, i)
    want = full.eval_read()
    _check_totals({**total, "loss": total["loss_sum"] / total["images"], "accuracy": total["top1"] / total["images"]},
                  want)
    _check_totals(want, E.metrics_ref(fl, fe, labels, TOPK))
