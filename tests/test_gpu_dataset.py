"""GPU checks of the device-resident dataset: the batch gather against the NumPy statement of its
definition (dataset_cases.gather_ref, itself pinned by hand-written answers in test_dataset_cpu),
byte for byte on every kernel path; dataset training steps against the same steps on batches
gathered on the host (bit-equal weights, logits, input); evaluate_dataset against evaluate;
the opt-in training metrics against eval_cases.metrics_ref; two data-parallel ranks with their own
datasets against one full-batch model; the refusals on a live model."""
import ctypes as C
import threading

import numpy as np
import pytest

import dataset_cases as D
import eval_cases as E

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def T():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import niti_amd  # noqa: F401
    return torch


def _set(m, W, S):
    for i, (w, s) in enumerate(zip(W, S)):
        m.set_weight(i, w, s)


def _weights(m):
    return [m.get_weight(i) for i in range(len(m.layers))]


# ---------------------------------------------------------------------------------- 1. the gather
GUARD = 64  # bytes / labels on either side of the outputs


@pytest.mark.parametrize("chw", [(3, 32, 32), (1, 28, 28), (3, 7, 5), (2, 3, 17)], ids=str)
def test_gather_parity(T, chw):
    """(3,32,32): 16-byte copies / 16-byte transformed stores; (1,28,28): rows that are no multiple
    of 16 (dword transformed stores); (3,7,5): C*H*W = 105, images start unaligned; (2,3,17): odd
    rows longer than 16 -- the byte path for both."""
    from niti_amd import DeviceDataset
    c, h, w = chw
    count, first = 9, 5
    rng = np.random.default_rng(c * 1000 + h * 10 + w)
    data = rng.integers(1, 256, (count, c, h, w)).astype(np.uint8)  # (no zero pixel: zero fill shows)
    labels = rng.integers(0, 1000, count).astype(np.int32)
    index, xform = D.parity_order(count, h, w)
    n = len(index)
    # a longer order: `first` other entries ahead of the ones gathered
    full_i = np.concatenate([np.array([8, -1, 3, 3, 0], np.int32), index])
    full_x = np.concatenate([np.full(first, 0x10101, np.int32), xform])
    ds = DeviceDataset(data, labels)
    for xf in (full_x, None):
        ds.set_order(full_i, xf)
        img = T.full((GUARD + n * c * h * w + GUARD,), 0xA5, dtype=T.uint8, device="cuda")
        lab = T.full((GUARD + n + GUARD,), -77, dtype=T.int32, device="cuda")
        ds.gather(first, n, img[GUARD:], lab[GUARD:])
        T.cuda.synchronize()
        want_img, want_lab = D.gather_ref(data, labels, index, None if xf is None else xform)
        got_img, got_lab = img.cpu().numpy(), lab.cpu().numpy()
        tag = "xform" if xf is not None else "plain"
        assert (got_img[:GUARD] == 0xA5).all() and (got_img[-GUARD:] == 0xA5).all(), tag
        assert (got_lab[:GUARD] == -77).all() and (got_lab[-GUARD:] == -77).all(), tag
        assert np.array_equal(got_lab[GUARD:-GUARD], want_lab), tag
        got = got_img[GUARD:-GUARD].reshape(n, c, h, w)
        bad = [i for i in range(n) if not np.array_equal(got[i], want_img[i])]
        assert not bad, (tag, bad[:8], [(int(index[i]), hex(int(xform[i]))) for i in bad[:8]])


# ------------------------------------------------------- 2 / 4. dataset steps == host-gathered steps
CASES = {
    "lenet-b16": ("lenet", 16, False),
    "vgg11-b8": ("vgg11", 8, False),
    "vgg11-b8-graph": ("vgg11", 8, True),
    "resnet18-32px-b2": ("resnet18", 2, False),
}
_PAIR = {}
STEPS = 3


def _make(arch, batch):
    """(model factory, W, S, image shape, classes)"""
    import niti_amd
    from niti_amd.model import NitiModel
    if arch == "resnet18":
        import niti_resnet_ref as RR
        convs = RR.resnet18_convs(32, 10)
        W, S = RR.init_weights(convs, seed=51)
        return (lambda: NitiModel(niti_amd.ARCH_RESNET18, batch, 32, 10)), W, S, (3, 32, 32), 10
    import niti_model_ref as R
    layers = R.lenet_layers() if arch == "lenet" else R.vgg11_layers()
    W, S = R.init_weights(layers, seed=52)
    a_id = niti_amd.ARCH_LENET if arch == "lenet" else niti_amd.ARCH_VGG11
    shape = (1, 28, 28) if arch == "lenet" else (3, 32, 32)
    return (lambda: NitiModel(a_id, batch)), W, S, shape, 10


def _pair(T, case):
    """Model A: one train_steps(ds, 0, 3) call, training metrics on.  Model B: the same initial
    weights, three train_step_images calls on batches gathered on the host by gather_ref."""
    if case in _PAIR:
        return _PAIR[case]
    from niti_amd import DeviceDataset, make_order
    arch, batch, graph = CASES[case]
    new, W, S, shape, classes = _make(arch, batch)
    count = 3 * batch + 3
    rng = np.random.default_rng(53 + batch)
    data = rng.integers(0, 256, (count,) + shape).astype(np.uint8)
    labels = rng.integers(0, classes, count).astype(np.int32)
    index, xform = make_order(count, batch, seed=7, epoch=1, pad=2, flip=True)
    assert len(index) >= STEPS * batch  # (batch 2: the 9 images make a fourth whole batch, not run)
    ds = DeviceDataset(data, labels)
    ds.set_order(index, xform)
    a, b = new(), new()
    a.set_graph(graph)
    _set(a, W, S)
    _set(b, W, S)
    a.train_metrics(True)
    a.train_metrics_reset()
    a.train_steps(ds, 0, STEPS)
    totals = a.train_metrics_read()
    want = {"images": 0, "top1": 0, "topk": 0, "loss_sum": 0.0}
    for s in range(STEPS):
        sl = slice(s * batch, (s + 1) * batch)
        img, lab = D.gather_ref(data, labels, index[sl], xform[sl])
        b.train_step_images(T.from_numpy(img).cuda(), T.from_numpy(lab).cuda())
        lg, e = b.logits()
        want = E.add_totals(want, E.metrics_ref(lg, e, lab, min(5, classes)))
    _PAIR[case] = dict(a=a, b=b, totals=totals, want=want, W=W)
    return _PAIR[case]


@pytest.mark.parametrize("case", list(CASES))
def test_dataset_steps_equal_host_gathered_steps(T, case):
    p = _pair(T, case)
    a, b = p["a"], p["b"]
    la, ea = a.logits()
    lb, eb = b.logits()
    assert ea == eb and np.array_equal(la, lb)
    xa, xea = a.input()
    xb, xeb = b.input()
    assert xea == xeb and np.array_equal(xa, xb)
    moved = False
    for i, (wa, wb) in enumerate(zip(_weights(a), _weights(b))):
        assert np.array_equal(wa, wb), ("w", i)
        moved = moved or not np.array_equal(wa, p["W"][i])
    assert moved, "three steps changed no weight"
    assert a.rowconv_error() == 0 and b.rowconv_error() == 0


@pytest.mark.parametrize("case", list(CASES))
def test_training_metrics(T, case):
    p = _pair(T, case)
    got, want = p["totals"], p["want"]
    print(case, got, want)
    assert (got["images"], got["top1"], got["topk"]) == (want["images"], want["top1"], want["topk"]), (got, want)
    assert got["images"] == STEPS * CASES[case][1]
    assert E.loss_close(got["loss_sum"], want["loss_sum"]), (got, want)


def test_training_metrics_disabled_launch_nothing(T):
    from niti_amd import DeviceDataset, make_order
    new, W, S, shape, classes = _make("lenet", 4)
    rng = np.random.default_rng(54)
    data = rng.integers(0, 256, (8,) + shape).astype(np.uint8)
    ds = DeviceDataset(data, rng.integers(0, classes, 8).astype(np.int32))
    ds.set_order(*make_order(8, 4, seed=1, epoch=0, pad=1))
    m = new()
    _set(m, W, S)
    m.train_steps(ds, 0, 2)
    t = m.train_metrics_read()
    assert (t["images"], t["top1"], t["topk"], t["loss_sum"]) == (0, 0, 0, 0.0)
    m.train_metrics(True)
    m.train_steps(ds, 1, 1)
    assert m.train_metrics_read()["images"] == 4
    m.train_metrics_reset()
    m.train_metrics(False)
    m.train_steps(ds, 0, 1)
    assert m.train_metrics_read()["images"] == 0


# ---------------------------------------------------------------------------------- 3. evaluation
def test_evaluate_dataset_equals_evaluate(T):
    from niti_amd import DeviceDataset
    batch = 8
    new, W, S, shape, classes = _make("vgg11", batch)
    n = 2 * batch + 3
    rng = np.random.default_rng(55)
    data = rng.integers(0, 256, (n,) + shape).astype(np.uint8)
    labels = rng.integers(0, classes, n).astype(np.int32)
    m = new()
    _set(m, W, S)
    want = m.evaluate(data, labels)
    got = m.evaluate_dataset(DeviceDataset(T.from_numpy(data).cuda(), T.from_numpy(labels).cuda()))
    assert want["images"] == n
    for k in ("images", "top1", "topk"):
        assert got[k] == want[k], (k, got, want)
    assert got["loss_sum"] == want["loss_sum"], (got, want)  # the same launches in the same order
    for i, w in enumerate(_weights(m)):
        assert np.array_equal(w, W[i]), i


# ------------------------------------------------------------------------------- 5. data parallel
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


def test_local_dp_datasets_equal_full_batch(T):
    """LocalGroup(2) x batch 4, each rank with its own dataset object whose order is its half of
    every global batch, against one batch-8 model fed the full order."""
    import niti_amd
    from niti_amd import DeviceDataset, make_order
    from niti_amd.model import LocalGroup, NitiModel
    world, b, steps = 2, 4, 2
    _, W, S, shape, classes = _make("vgg11", b)
    count = steps * b * world + 3
    rng = np.random.default_rng(56)
    data = rng.integers(0, 256, (count,) + shape).astype(np.uint8)
    labels = rng.integers(0, classes, count).astype(np.int32)
    index, xform = make_order(count, b * world, seed=9, epoch=4, pad=2, flip=True)
    full = NitiModel(niti_amd.ARCH_VGG11, b * world)
    ranks = [NitiModel(niti_amd.ARCH_VGG11, b) for _ in range(world)]
    group = LocalGroup(world)
    for r, m in enumerate(ranks):
        m.attach_local(group, r, exact=True)
    for m in [full] + ranks:
        _set(m, W, S)
    dsf = DeviceDataset(data, labels)
    dsf.set_order(index, xform)
    full.train_steps(dsf, 0, steps)
    T.cuda.synchronize()
    dss = []
    for r in range(world):
        pick = np.concatenate([np.arange(s * b * world + r * b, s * b * world + (r + 1) * b) for s in range(steps)])
        ds = DeviceDataset(data, labels)
        ds.set_order(index[pick], xform[pick])
        dss.append(ds)
    streams = [T.cuda.Stream() for _ in range(world)]

    def rank_steps(r):
        ranks[r].train_steps(dss[r], 0, steps, stream=C.c_void_p(streams[r].cuda_stream))
        streams[r].synchronize()

    _in_threads([lambda r=r: rank_steps(r) for r in range(world)])
    wf = _weights(full)
    assert any(not np.array_equal(w, W[i]) for i, w in enumerate(wf))
    for r, m in enumerate(ranks):
        for i, w in enumerate(_weights(m)):
            assert np.array_equal(w, wf[i]), (r, i)


# ------------------------------------------------------------------------------------ 6. refusals
def test_refusals_leave_the_model_untouched(T):
    from niti_amd import DeviceDataset
    from niti_amd._lib import NitiError
    batch = 4
    new, W, S, shape, classes = _make("lenet", batch)
    m = new()
    _set(m, W, S)
    rng = np.random.default_rng(57)
    labels = rng.integers(0, classes, 8).astype(np.int32)
    good = DeviceDataset(rng.integers(0, 256, (8,) + shape).astype(np.uint8), labels)
    other = DeviceDataset(rng.integers(0, 256, (8, 3, 32, 32)).astype(np.uint8), labels)
    other.set_order(np.arange(8, dtype=np.int32))
    good.set_order(np.array([0, 1, 2, 3, 4, 5, 6, -1], np.int32))

    def refused(f):
        with pytest.raises(NitiError) as err:
            f()
        assert err.value.code == 5  # NITI_INVALID_VALUE
        for i, w in enumerate(_weights(m)):
            assert np.array_equal(w, W[i]), i

    refused(lambda: m.train_steps(other, 0, 1))   # another geometry than the model's input
    refused(lambda: m.eval_steps(other, 0, 1))
    refused(lambda: m.train_steps(good, 1, 1))    # a -1 in the training slice
    refused(lambda: m.train_steps(good, 0, 2))
    refused(lambda: m.train_steps(good, 1, 2))    # past the order's end
    refused(lambda: m.train_steps(good, 2, 1))
    refused(lambda: m.train_steps(good, 0, 3))
    refused(lambda: m.eval_steps(good, 0, 3))
    refused(lambda: m.train_steps(good, -1, 1))
    refused(lambda: m.train_steps(good, 0, 0))
    m.eval_reset()
    m.eval_steps(good, 1, 1)                      # (the padded slice is fine for evaluation)
    assert m.eval_read()["images"] == 3
    m.train_steps(good, 0, 1)                     # and the clean slice trains
    assert any(not np.array_equal(w, W[i]) for i, w in enumerate(_weights(m)))
