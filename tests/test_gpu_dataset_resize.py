"""GPU checks of the crop-and-resize gather of the device-resident dataset: niti_batch_gather on
orders with windows against the statement of its definition (resize_cases.resize_ref, itself
pinned by hand-written answers in test_dataset_resize_cpu), byte for byte on every store form;
dataset training steps with windows against the same steps on batches gathered by the primitive
(bit-equal weights, logits, input), also under a captured graph; evaluate_dataset with centre
windows against evaluate on the reference arrays; two data-parallel ranks with windowed datasets
against one full-batch model; the refusals on a live model; the untouched default."""
import ctypes as C
import threading

import numpy as np
import pytest

import dataset_cases as D
import resize_cases as R

pytestmark = pytest.mark.gpu

GUARD = 64  # bytes / labels on either side of the outputs


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
def _pixels(rng, count, c, h, w):
    """random bytes, plus one image of all 0 and one of all 255 (the 32-bit headroom) and one of
    only 0 and 255"""
    data = rng.integers(0, 256, (count, c, h, w)).astype(np.uint8)
    data[1] = 0
    data[2] = 255
    data[3] = rng.integers(0, 2, (c, h, w)).astype(np.uint8) * 255
    return data


def _gather_check(T, ds, data, labels, index, xform, windows, oh, ow, first, offset, tag):
    """ds's order is [`first` other entries] + (index, xform, windows); gather the latter into a
    guarded buffer that starts `offset` bytes past an aligned address and compare with resize_ref."""
    n, c = len(index), data.shape[1]
    size = n * c * oh * ow
    img = T.full((GUARD + offset + size + GUARD,), 0xA5, dtype=T.uint8, device="cuda")
    lab = T.full((GUARD + n + GUARD,), -77, dtype=T.int32, device="cuda")
    assert img.data_ptr() % 16 == 0
    ds.gather(first, n, img[GUARD + offset:], lab[GUARD:])
    T.cuda.synchronize()
    want_img, want_lab = R.resize_ref(data, labels, index, xform, windows, oh, ow)
    got_img, got_lab = img.cpu().numpy(), lab.cpu().numpy()
    assert (got_img[:GUARD + offset] == 0xA5).all() and (got_img[GUARD + offset + size:] == 0xA5).all(), tag
    assert (got_lab[:GUARD] == -77).all() and (got_lab[-GUARD:] == -77).all(), tag
    assert np.array_equal(got_lab[GUARD:-GUARD], want_lab), tag
    got = got_img[GUARD + offset:GUARD + offset + size].reshape(n, c, oh, ow)
    bad = [i for i in range(n) if not np.array_equal(got[i], want_img[i])]
    assert not bad, (tag, bad[:8], [(int(index[i]), windows[i].tolist(), hex(int(xform[i]))) for i in bad[:8]])


@pytest.mark.parametrize("geom", [((3, 13, 10), (7, 5)), ((2, 20, 24), (12, 12)), ((3, 20, 24), (16, 16))], ids=str)
def test_gather_parity(T, geom):
    """stored 3x13x10 -> 7x5: a byte per lane; 2x20x24 -> 12x12: dword stores; 3x20x24 -> 16x16:
    16-byte stores; each also into an output one byte past alignment (the byte fall-back), and at
    the output sizes 1x1 and oh x 4 (the downscale from the full width to 4)."""
    from niti_amd import DeviceDataset
    (c, h, w), (oh, ow) = geom
    count, first = 9, 4
    rng = np.random.default_rng(c * 1000 + h * 10 + w)
    data = _pixels(rng, count, c, h, w)
    labels = rng.integers(0, 1000, count).astype(np.int32)
    ds = DeviceDataset(data, labels, out_hw=(oh, ow))
    assert (ds.oh, ds.ow) == (oh, ow)

    def run(order, oh, ow, offsets, tag):
        index, xform, windows = order
        # a longer order: `first` other entries ahead of the ones gathered
        ds.set_order(np.concatenate([np.array([8, -1, 3, 3], np.int32), index]),
                     np.concatenate([np.full(first, 1 << 16, np.int32), xform]),
                     np.concatenate([np.tile(np.array([1, 1, 2, 2], np.int32), (first, 1)), windows]))
        for off in offsets:
            _gather_check(T, ds, data, labels, index, xform, windows, oh, ow, first, off, (tag, off))

    run(R.parity_order(count, h, w, oh, ow), oh, ow, (0, 1), "main")
    small = R.small_order(count, h, w)
    ds.set_output(1, 1)
    assert ds.order_len == 0
    run(small, 1, 1, (0,), "1x1")
    ds.set_output(oh, 4)
    run(small, oh, 4, (0, 2), "to-4")
    # without xform: no entry is mirrored
    index, xform, windows = small
    ds.set_order(index, None, windows)
    _gather_check(T, ds, data, labels, index, np.zeros_like(xform), windows, oh, 4, 0, 0, "no-xform")


@pytest.mark.parametrize("geom", [((1, 9, 6), (70, 3)), ((2, 5, 33), (66, 16)), ((3, 4, 40), (5, 2052)),
                                  ((2, 200, 200), (16, 16)), ((1, 150, 203), (5, 12)), ((1, 150, 203), (3, 7))], ids=str)
def test_gather_parity_more_than_one_block_per_entry(T, geom):
    """A block owns at most 64 output rows, 2048 output columns and about 16384 pixels of an entry.
    1x9x6 -> 70x3: two row strips, bytes; 2x5x33 -> 66x16: two strips, 16-byte stores;
    3x4x40 -> 5x2052: two column chunks (the second 4 wide) x three strips of 2 rows, dword stores.
    A block stages the source rows it samples in LDS where they fit 24 KB per channel, which every
    case so far does; 200x200 and 150x203 windows do not and are sampled through the cache, in the
    16-byte, dword and byte forms (the 1x1 window of the same orders is staged)."""
    from niti_amd import DeviceDataset
    (c, h, w), (oh, ow) = geom
    count = 5
    rng = np.random.default_rng(c * 1000 + h * 10 + w)
    data = _pixels(rng, count, c, h, w)
    labels = rng.integers(0, 1000, count).astype(np.int32)
    index, xform, windows = (v[[0, 1, 5, 6]] for v in R.small_order(count, h, w))
    ds = DeviceDataset(data, labels, out_hw=(oh, ow))
    ds.set_order(index, xform, windows)
    _gather_check(T, ds, data, labels, index, xform, windows, oh, ow, 0, 0, "blocks")


def test_unchanged_default(T):
    """A dataset without set_output and with a plain order gathers as dataset_cases.gather_ref
    says, also after an order with windows was replaced by a plain one."""
    from niti_amd import DeviceDataset, pack_xform
    count, c, h, w = 5, 2, 6, 8
    rng = np.random.default_rng(81)
    data = rng.integers(1, 256, (count, c, h, w)).astype(np.uint8)
    labels = rng.integers(0, 1000, count).astype(np.int32)
    index = np.array([4, 0, -1, 2, 2, 1], np.int32)
    xform = pack_xform([0, 1, 0, -2, 3, 0], [0, -1, 0, 2, 0, 0], [0, 1, 0, 0, 1, 1])
    ds = DeviceDataset(data, labels)
    assert (ds.oh, ds.ow) == (h, w)
    for xf, pre in ((xform, False), (None, False), (xform, True)):
        if pre:
            ds.set_order(index, None, np.tile(np.array([1, 1, 3, 2], np.int32), (len(index), 1)))
        ds.set_order(index, xf)
        img = T.full((len(index), c, h, w), 0xA5, dtype=T.uint8, device="cuda")
        lab = T.full((len(index),), -77, dtype=T.int32, device="cuda")
        ds.gather(0, len(index), img, lab)
        T.cuda.synchronize()
        want_img, want_lab = D.gather_ref(data, labels, index, xf)
        assert np.array_equal(img.cpu().numpy(), want_img) and np.array_equal(lab.cpu().numpy(), want_lab)


# ------------------------------------------------------------ 2. dataset steps with windows
CASES = {
    "lenet-28-from-32": ("lenet", 8, (1, 32, 32), 28, False),
    "lenet-28-from-32-graph": ("lenet", 8, (1, 32, 32), 28, True),
    "resnet18-32-from-40": ("resnet18", 2, (3, 40, 40), 32, False),
}
STEPS = 3


def _make(arch, batch):
    import niti_amd
    from niti_amd.model import NitiModel
    if arch == "resnet18":
        import niti_resnet_ref as RR
        W, S = RR.init_weights(RR.resnet18_convs(32, 10), seed=61)
        return (lambda: NitiModel(niti_amd.ARCH_RESNET18, batch, 32, 10)), W, S
    import niti_model_ref as MR
    W, S = MR.init_weights(MR.lenet_layers(), seed=62)
    return (lambda: NitiModel(niti_amd.ARCH_LENET, batch)), W, S


@pytest.mark.parametrize("case", list(CASES))
def test_steps_with_windows_equal_steps_on_gathered_batches(T, case):
    from niti_amd import DeviceDataset, make_rrc_order
    arch, batch, stored, px, graph = CASES[case]
    new, W, S = _make(arch, batch)
    c, h, w = stored
    count = STEPS * batch + 1
    rng = np.random.default_rng(63 + batch)
    data = rng.integers(0, 256, (count,) + stored).astype(np.uint8)
    labels = rng.integers(0, 10, count).astype(np.int32)
    index, xform, windows = make_rrc_order(count, batch, seed=7, epoch=1, h=h, w=w, scale=(0.3, 1.0))
    ds = DeviceDataset(data, labels, out_hw=(px, px))
    ds.set_order(index, xform, windows)
    a, b = new(), new()
    a.set_graph(graph)
    _set(a, W, S)
    _set(b, W, S)
    a.train_steps(ds, 0, STEPS)
    img = T.empty((batch, c, px, px), dtype=T.uint8, device="cuda")
    lab = T.empty(batch, dtype=T.int32, device="cuda")
    for s in range(STEPS):
        ds.gather(s * batch, batch, img, lab)
        b.train_step_images(img, lab)
    la, ea = a.logits()
    lb, eb = b.logits()
    assert ea == eb and np.array_equal(la, lb)
    xa, xea = a.input()
    xb, xeb = b.input()
    assert xea == xeb and np.array_equal(xa, xb)
    # (the last batch the primitive gathered is the definition's)
    want, _ = R.resize_ref(data, labels, index[(STEPS - 1) * batch:STEPS * batch], xform[(STEPS - 1) * batch:],
                           windows[(STEPS - 1) * batch:], px, px)
    assert np.array_equal(img.cpu().numpy(), want)
    moved = False
    for i, (wa, wb) in enumerate(zip(_weights(a), _weights(b))):
        assert np.array_equal(wa, wb), ("w", i)
        moved = moved or not np.array_equal(wa, W[i])
    assert moved, "three steps changed no weight"
    assert a.rowconv_error() == 0 and b.rowconv_error() == 0


def test_evaluate_dataset_with_centre_windows(T):
    from niti_amd import DeviceDataset, center_windows
    batch = 8
    new, W, S = _make("lenet", batch)
    n = 2 * batch + 3
    rng = np.random.default_rng(64)
    data = rng.integers(0, 256, (n, 1, 32, 32)).astype(np.uint8)
    labels = rng.integers(0, 10, n).astype(np.int32)
    m = new()
    _set(m, W, S)
    win = center_windows(n, 32, 32)  # int(32 * 0.875) = 28 from 2: the identity crop
    assert (win == [2, 2, 28, 28]).all()
    ref, _ = R.resize_ref(data, labels, np.arange(n), None, win, 28, 28)
    want = m.evaluate(ref, labels)
    ds = DeviceDataset(T.from_numpy(data).cuda(), T.from_numpy(labels).cuda(), out_hw=(28, 28))
    got = m.evaluate_dataset(ds)  # (centre windows by default: the stored size is not the output's)
    assert want["images"] == n and got == want, (got, want)
    # explicit windows that do resample: the 30 x 30 centre
    win30 = center_windows(n, 32, 32, fraction=(0.95, 0.95))
    assert (win30 == [1, 1, 30, 30]).all()
    ref30, _ = R.resize_ref(data, labels, np.arange(n), None, win30, 28, 28)
    assert not np.array_equal(ref30, ref)
    assert m.evaluate_dataset(ds, windows=win30) == m.evaluate(ref30, labels)
    for i, wt in enumerate(_weights(m)):
        assert np.array_equal(wt, W[i]), i


# ------------------------------------------------------------------------------- 3. data parallel
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


def test_local_dp_windowed_datasets_equal_full_batch(T):
    """LocalGroup(2) x batch 4, each rank with its own windowed dataset whose order is its half of
    every global batch, against one batch-8 model fed the full order."""
    import niti_amd
    from niti_amd import DeviceDataset, make_rrc_order
    from niti_amd.model import LocalGroup, NitiModel
    world, b, steps = 2, 4, 2
    _, W, S = _make("lenet", b)
    count = steps * b * world + 3
    rng = np.random.default_rng(66)
    data = rng.integers(0, 256, (count, 1, 32, 32)).astype(np.uint8)
    labels = rng.integers(0, 10, count).astype(np.int32)
    index, xform, windows = make_rrc_order(count, b * world, seed=9, epoch=4, h=32, w=32, scale=(0.3, 1.0))
    full = NitiModel(niti_amd.ARCH_LENET, b * world)
    ranks = [NitiModel(niti_amd.ARCH_LENET, b) for _ in range(world)]
    group = LocalGroup(world)
    for r, m in enumerate(ranks):
        m.attach_local(group, r, exact=True)
    for m in [full] + ranks:
        _set(m, W, S)
    dsf = DeviceDataset(data, labels, out_hw=(28, 28))
    dsf.set_order(index, xform, windows)
    full.train_steps(dsf, 0, steps)
    T.cuda.synchronize()
    dss = []
    for r in range(world):
        pick = np.concatenate([np.arange(s * b * world + r * b, s * b * world + (r + 1) * b) for s in range(steps)])
        ds = DeviceDataset(data, labels, out_hw=(28, 28))
        ds.set_order(index[pick], xform[pick], windows[pick])
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


# ------------------------------------------------------------------------------------ 4. refusals
def test_refusals_leave_the_model_untouched(T):
    from niti_amd import DeviceDataset
    from niti_amd._lib import NitiError
    batch = 4
    new, W, S = _make("lenet", batch)
    m = new()
    _set(m, W, S)
    rng = np.random.default_rng(67)
    labels = rng.integers(0, 10, 8).astype(np.int32)
    data = rng.integers(0, 256, (8, 1, 32, 32)).astype(np.uint8)
    index = np.arange(8, dtype=np.int32)
    win = np.tile(np.array([2, 2, 28, 28], np.int32), (8, 1))

    def refused(f):
        with pytest.raises(NitiError) as err:
            f()
        assert err.value.code == 5  # NITI_INVALID_VALUE
        for i, w in enumerate(_weights(m)):
            assert np.array_equal(w, W[i]), i

    # an output size that is not the model's
    ds = DeviceDataset(data, labels, out_hw=(24, 24))
    ds.set_order(index, None, win)
    refused(lambda: m.train_steps(ds, 0, 1))
    refused(lambda: m.eval_steps(ds, 0, 1))
    ds30 = DeviceDataset(data, labels, out_hw=(28, 30))
    ds30.set_order(index, None, win)
    refused(lambda: m.train_steps(ds30, 0, 1))
    # an output size different from the stored size with a plain order
    ds.set_output(28, 28)
    ds.set_order(index)
    refused(lambda: m.train_steps(ds, 0, 1))
    refused(lambda: m.eval_steps(ds, 0, 1))
    out = T.zeros((4, 1, 28, 28), dtype=T.uint8, device="cuda")
    lab = T.zeros(4, dtype=T.int32, device="cuda")
    refused(lambda: ds.gather(0, 4, out, lab))
    # xform with dx != 0 (or dy != 0) beside windows
    refused(lambda: ds.set_order(index, np.array([0, 0, 1, 0, 0, 0, 0, 0], np.int32), win))
    refused(lambda: ds.set_order(index, np.array([0] * 7 + [(1 << 16) | (2 << 8)], np.int32), win))
    # a window outside the image
    for bad in ((5, 2, 28, 28), (2, 5, 28, 28), (-1, 0, 4, 4), (0, 0, 0, 4), (0, 0, 33, 1)):
        w2 = win.copy()
        w2[5] = bad
        refused(lambda: ds.set_order(index, None, w2))
    # output sizes below 1 or beyond the 2^22 bound
    for oh, ow in ((0, 28), (28, -1), (28, (1 << 22) // 31 + 2)):
        refused(lambda: ds.set_output(oh, ow))
    ds.set_output(28, (1 << 22) // 31 + 1)  # (ow - 1) * 31 < 2^22: the largest admitted
    # and the good order trains
    ds.set_output(28, 28)
    ds.set_order(index, np.full(8, 1 << 16, np.int32), win)
    m.train_steps(ds, 0, 2)
    assert any(not np.array_equal(w, W[i]) for i, w in enumerate(_weights(m)))
