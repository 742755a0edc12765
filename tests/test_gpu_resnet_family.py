"""Residual networks from a stage list (niti_model_create_resnet, csrc/niti_resnet_model.hip) against
the oracle: RR.train_step restated with an optional stem pool (resnet_family_cases.family_step_ref,
pinned to RR.train_step in test_resnet_family_cpu.py).  Each case runs two steps and must match bit
for bit: the logits and their exponent, taps 0 / 1 / 2 of every layer, every updated weight, with
rowconv_error() == 0.  The cases and what only each of them can break are listed in DESIGN.md,
"User-defined residual networks"."""
import ctypes as C
import threading

import numpy as np
import pytest

import resnet_family_cases as FC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def T():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import niti_amd  # noqa: F401
    return torch


def _model(spec, in_hw, batch, W, S):
    from niti_amd.model import NitiModel
    m = NitiModel.from_resnet(spec, in_hw, batch)
    for i, (w, s) in enumerate(zip(W, S)):
        m.set_weight(i, w, s)
    return m


def _check_step(m, convs, rec, newW, step, sl=None, grads=True):
    import niti_oracle as O
    lg, e = m.logits()
    want = rec["logits"] if sl is None else rec["logits"][sl]
    assert e == rec["exp_logits"] and np.array_equal(lg, want), step
    for i, c in enumerate(convs):
        f = O.relu(rec["fwd"][i]) if m.layers[i]["relu"] else rec["fwd"][i]
        assert np.array_equal(m.tap(i, 0), f if sl is None else f[sl]), ("fwd", step, c["name"])
        assert np.array_equal(m.tap(i, 2), rec["dy"][i] if sl is None else rec["dy"][i][sl]), ("dy", step, c["name"])
        if grads:
            assert np.array_equal(m.tap(i, 1), rec["dw"][i]), ("dw", step, c["name"])
        assert np.array_equal(m.get_weight(i), newW[i]), ("w", step, c["name"])


def _step(T, m, data, labels, images, exp_in=FC.EXP_IN):
    if images:
        m.train_step_images(T.from_numpy(data).cuda(), T.from_numpy(labels).cuda())
    else:
        m.train_step(T.from_numpy(data).cuda(), exp_in, T.from_numpy(labels).cuda())


@pytest.mark.parametrize("name", list(FC.CASES))
def test_family_step_matches_oracle(T, name):
    import niti_amd
    spec, in_hw, batch, images = FC.CASES[name]
    convs, W, S, steps = FC.reference(name)
    m = _model(spec, in_hw, batch, W, S)
    assert m.arch == niti_amd.ARCH_RESNET and len(m.layers) == FC.N_LAYERS[name]
    assert [(l["c_in"], l["c_out"], l["kh"], l["stride"], l["pad"], l["h"]) for l in m.layers] == \
        [(c["ci"], c["co"], c["k"], c["stride"], c["pad"], c["h"]) for c in convs]
    for step, (data, labels, x, e, newW, rec) in enumerate(steps):
        _step(T, m, data, labels, images)
        if images:
            xd, ad = m.input()
            assert ad == e and np.array_equal(xd, x)
        _check_step(m, convs, rec, newW, step)
    assert m.rowconv_error() == 0


def test_resnet18_by_name_and_by_spec_agree(T):
    """The built-in network is the spec {3, 7,2,3, pool, 64, (2,2,2,2)}: the same layers, plans and
    MACs, and after two steps identical logits, exponents and weights."""
    import niti_amd
    import niti_resnet_ref as RR
    from niti_amd.model import NitiModel
    hw, batch, classes = 32, 2, 10
    convs = RR.resnet18_convs(hw, classes)
    W, S = RR.init_weights(convs, seed=FC.SEED_W)
    a = NitiModel(niti_amd.ARCH_RESNET18, batch, hw, classes)
    b = NitiModel.from_resnet(FC.RESNET18, hw, batch)
    assert a.arch == niti_amd.ARCH_RESNET18 and b.arch == niti_amd.ARCH_RESNET and a.resnet is None
    for m in (a, b):
        for i, (w, s) in enumerate(zip(W, S)):
            m.set_weight(i, w, s)
    assert a.layers == b.layers and a.plans() == b.plans() and a.step_macs() == b.step_macs()
    for data, labels in FC.draw_steps(FC.RESNET18, hw, batch, False):
        _step(T, a, data, labels, False)
        _step(T, b, data, labels, False)
        (la, ea), (lb, eb) = a.logits(), b.logits()
        assert ea == eb and np.array_equal(la, lb)
    for i in range(len(convs)):
        assert np.array_equal(a.get_weight(i), b.get_weight(i)), i
        assert np.array_equal(a.tap(i, 1), b.tap(i, 1)), i
    assert a.plans() == b.plans()
    assert a.rowconv_error() == 0 and b.rowconv_error() == 0
    # equal specs and input sizes copy both ways; another depth list does not
    b.copy_weights_from(a)
    a.copy_weights_from(b)
    with pytest.raises(niti_amd._lib.NitiError):
        NitiModel.from_resnet(dict(FC.RESNET18, depths=(2, 2, 2, 1)), hw, batch).copy_weights_from(a)


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


def test_deep_narrow_net_two_local_ranks_equal_one_device(T):
    """(3,4,6,3) at width 16: all 37 weight gradients (1.3 M elements, 5.3 MB) close one
    data-parallel bucket, whose ranges take two launches.  Two ranks of one image each equal one
    device stepping both, over two steps."""
    from niti_amd.model import LocalGroup
    import niti_resnet_ref as RR
    spec, hw, per, world = dict(depths=(3, 4, 6, 3), width=16, classes=10), 32, 1, 2
    convs = FC.family_convs(spec, hw)
    assert len(convs) == 37 and sum(c["co"] * c["ci"] * c["k"] ** 2 for c in convs) * 4 < 8 << 20
    W, S = RR.init_weights(convs, seed=FC.SEED_W)
    full = _model(spec, hw, world * per, W, S)
    ranks = [_model(spec, hw, per, W, S) for _ in range(world)]
    group = LocalGroup(world)
    for r, m in enumerate(ranks):
        m.attach_local(group, r, exact=True)
    streams = [T.cuda.Stream() for _ in range(world)]
    for step, (data, labels) in enumerate(FC.draw_steps(spec, hw, world * per, False)):
        dd, ld = T.from_numpy(data).cuda(), T.from_numpy(labels).cuda()
        full.train_step(dd, FC.EXP_IN, ld)
        T.cuda.synchronize()
        parts = [(dd[r * per:(r + 1) * per].contiguous(), ld[r * per:(r + 1) * per].contiguous()) for r in range(world)]

        def rank_step(r):
            ranks[r].train_step(parts[r][0], FC.EXP_IN, parts[r][1], stream=C.c_void_p(streams[r].cuda_stream))
            streams[r].synchronize()

        _in_threads([lambda r=r: rank_step(r) for r in range(world)])
        fl, fe = full.logits()
        assert np.any(fl != 0)
        for r, m in enumerate(ranks):
            sl = slice(r * per, (r + 1) * per)
            lg, e = m.logits()
            assert e == fe and np.array_equal(lg, fl[sl]), (step, r)
            for i, c in enumerate(convs):
                assert np.array_equal(m.tap(i, 0), full.tap(i, 0)[sl]), ("fwd", step, r, c["name"])
                assert np.array_equal(m.tap(i, 2), full.tap(i, 2)[sl]), ("dy", step, r, c["name"])
                assert np.array_equal(m.tap(i, 1), full.tap(i, 1)), ("dw", step, r, c["name"])
                assert np.array_equal(m.get_weight(i), full.get_weight(i)), ("w", step, r, c["name"])
    for m in [full] + ranks:
        assert m.rowconv_error() == 0


def test_deep_narrow_net_rccl_world1_equals_no_comm(T):
    """attach_comm on a spec model: a world of one runs every collective call site (the split
    communicator, the 37-layer bucket's SUM and its two range launches on the comm stream, every
    range MAX) and must equal the plain step, from uint8 images over two steps."""
    import os
    import niti_resnet_ref as RR
    from niti_amd.model import NitiModel
    os.environ.setdefault("NCCL_SOCKET_IFNAME", "lo")
    spec, hw, batch = dict(depths=(3, 4, 6, 3), width=16, classes=10), 32, 2
    convs = FC.family_convs(spec, hw)
    W, S = RR.init_weights(convs, seed=FC.SEED_W)
    data = FC.draw_steps(spec, hw, batch, True)
    runs = []
    for comm in (True, False):
        m = NitiModel.from_resnet(spec, hw, batch)
        if comm:
            m.attach_comm(NitiModel.unique_id(), 0, 1, exact=True)
        for i, (w, s) in enumerate(zip(W, S)):
            m.set_weight(i, w, s)
        for img, lab in data:
            _step(T, m, img, lab, True)
        T.cuda.synchronize()
        assert m.rowconv_error() == 0
        runs.append(([m.get_weight(i) for i in range(len(W))], [m.tap(i, 1) for i in range(len(W))], m.logits()))
        del m
    (wc, gc, (lc, ec)), (wn, gn, (ln, en)) = runs
    assert ec == en and np.array_equal(lc, ln) and np.any(ln != 0)
    for i in range(len(W)):
        assert np.array_equal(wc[i], wn[i]) and np.array_equal(gc[i], gn[i]), convs[i]["name"]


# ---- one small spec model through everything the step-driver base offers
SMALL = "cifar_gray_images"


def test_small_model_graph_replay_and_no_grad_tap(T):
    from niti_amd._lib import NitiError
    spec, in_hw, batch, images = FC.CASES[SMALL]
    convs, W, S, steps = FC.reference(SMALL)
    for graph, keep in ((True, True), (False, False), (True, False)):
        m = _model(spec, in_hw, batch, W, S)
        m.set_graph(graph)
        m.keep_grads(keep)
        for step, (data, labels, x, e, newW, rec) in enumerate(steps):
            _step(T, m, data, labels, images)
            _check_step(m, convs, rec, newW, step, grads=keep)  # (tap (0, 0): the pool-less stem's y0 is always there)
            if not keep:
                with pytest.raises(NitiError):
                    m.tap(1, 1)
        assert m.rowconv_error() == 0


def test_small_model_autotune_keeps_results(T):
    from niti_amd.model import NitiModel
    spec, in_hw, batch, images = FC.CASES[SMALL]
    convs, W, S, steps = FC.reference(SMALL)
    m = _model(spec, in_hw, batch, W, S)
    try:
        data, labels, _, _, newW, rec = steps[0]
        _step(T, m, data, labels, images)
        m.autotune(reps=2)
        for i, w in enumerate(newW):  # (tuning reruns phases on the last step's buffers, never the update)
            assert np.array_equal(m.get_weight(i), w), i
        data, labels, _, _, newW, rec = steps[1]
        _step(T, m, data, labels, images)
        _check_step(m, convs, rec, newW, 1)
        assert m.rowconv_error() == 0
    finally:
        NitiModel.reset_plans()


def test_small_model_evaluate_padded_tail(T):
    """5 images at batch 2: three batches, the last padded with a zero image of label -1."""
    import eval_cases as E
    import niti_oracle as O
    spec, in_hw, batch, _ = FC.CASES[SMALL]
    convs, W, S, _ = FC.reference(SMALL)
    rng = np.random.default_rng(9)
    img = rng.integers(0, 256, (5, 1, in_hw, in_hw)).astype(np.uint8)
    lab = rng.integers(0, spec["classes"], 5).astype(np.int32)
    m = _model(spec, in_hw, batch, W, S)
    got = m.evaluate(img, lab)
    want = {"images": 0, "top1": 0, "topk": 0, "loss_sum": 0.0}
    for i in range(0, 5, batch):
        pad = max(0, i + batch - 5)
        bi = np.concatenate([img[i:i + batch], np.zeros((pad, 1, in_hw, in_hw), np.uint8)])
        bl = np.concatenate([lab[i:i + batch], np.full(pad, -1, np.int32)])
        x, a = O.quantize_images(bi)
        _, rec = FC.family_step_ref(convs, W, S, x, a, np.maximum(bl, 0), spec["classes"], pool=False)
        want = E.add_totals(want, E.metrics_ref(rec["logits"], rec["exp_logits"], bl, 5))
    assert (got["images"], got["top1"], got["topk"]) == (5, want["top1"], want["topk"])
    assert E.loss_close(got["loss_sum"], want["loss_sum"])
    for i in range(len(convs)):  # evaluation writes no weight
        assert np.array_equal(m.get_weight(i), W[i])
    assert m.rowconv_error() == 0


def test_small_model_fit_epoch_equals_host_fed_steps(T):
    from niti_amd.dataset import DeviceDataset, make_order
    spec, in_hw, batch, _ = FC.CASES[SMALL]
    convs, W, S, _ = FC.reference(SMALL)
    rng = np.random.default_rng(10)
    img = rng.integers(0, 256, (7, 1, in_hw, in_hw)).astype(np.uint8)
    lab = rng.integers(0, spec["classes"], 7).astype(np.int32)
    a, b = _model(spec, in_hw, batch, W, S), _model(spec, in_hw, batch, W, S)
    steps = a.fit_epoch(DeviceDataset(img, lab), seed=3, epoch=1)
    assert steps == 3
    index, _ = make_order(7, batch, seed=3, epoch=1, drop_last=True)
    for k in range(steps):
        sel = index[k * batch:(k + 1) * batch]
        b.train_step_images(T.from_numpy(img[sel]).cuda(), T.from_numpy(lab[sel]).cuda())
    T.cuda.synchronize()
    (la, ea), (lb, eb) = a.logits(), b.logits()
    assert ea == eb and np.array_equal(la, lb) and np.any(la != 0)
    for i in range(len(convs)):
        assert np.array_equal(a.get_weight(i), b.get_weight(i)), i
    assert a.rowconv_error() == 0


def test_small_model_snapshots_init_and_copy(T, tmp_path):
    """init_weights is xavier_int8 in layer order; save / load carry the spec and refuse another
    before any device write; copy_weights_from takes an equal spec at another batch and refuses
    another spec, another input size and a built-in model."""
    import niti_amd
    from niti_amd._lib import NitiError
    from niti_amd.init import xavier_int8
    from niti_amd.model import NitiModel
    spec, in_hw, batch, images = FC.CASES[SMALL]
    m = NitiModel.from_resnet(spec, in_hw, batch)
    assert m.resnet == niti_amd.normalize_resnet_spec(spec)
    m.init_weights(4)
    rng = np.random.default_rng(4)
    want = [xavier_int8(m.weight_shape(i), rng) for i in range(len(m.layers))]
    for i, (w, s) in enumerate(want):
        assert np.array_equal(m.get_weight(i), w) and m._wscale[i] == s
    p, q = str(tmp_path / "r.safetensors"), str(tmp_path / "r.mnn")
    m.save(p)
    m.save_mnn(q)
    wider = dict(spec, depths=(1, 2))
    for load in ("load", "load_mnn"):
        path = p if load == "load" else q
        same = NitiModel.from_resnet(spec, in_hw, 3)
        getattr(same, load)(path)
        for i, (w, _) in enumerate(want):
            assert np.array_equal(same.get_weight(i), w)
        for other in (NitiModel.from_resnet(wider, in_hw, 3), NitiModel.from_resnet(spec, in_hw + 4, 3),
                      NitiModel.from_resnet(dict(spec, stem=(3, 1, 1, 1)), in_hw, 3)):
            with pytest.raises(ValueError):
                getattr(other, load)(path)
            assert not np.any(other.get_weight(0))  # refused before any device write
    dst = NitiModel.from_resnet(spec, in_hw, 3)
    dst.copy_weights_from(m)
    for i, (w, _) in enumerate(want):
        assert np.array_equal(dst.get_weight(i), w), i
    for other in (NitiModel.from_resnet(wider, in_hw, 3), NitiModel.from_resnet(spec, in_hw + 4, 3),
                  NitiModel.from_resnet(dict(spec, stem=(3, 1, 1, 1)), in_hw, 3), NitiModel(niti_amd.ARCH_LENET, 4)):
        with pytest.raises(NitiError):
            other.copy_weights_from(m)
        with pytest.raises(NitiError):
            m.copy_weights_from(other)
    # copied weights train as set ones do
    convs = FC.family_convs(spec, in_hw)
    W, S = [w for w, _ in want], [s for _, s in want]
    data, labels = FC.draw_steps(spec, in_hw, 3, images, steps=1)[0]
    import niti_oracle as O
    x, e = O.quantize_images(data)
    newW, rec = FC.family_step_ref(convs, W, S, x, e, labels, spec["classes"], pool=False)
    _step(T, dst, data, labels, images)
    _check_step(dst, convs, rec, newW, 0)
    assert dst.rowconv_error() == 0


def test_refused_spec_allocates_nothing(T):
    """niti_model_create_resnet returns the check's code and leaves *out as it was."""
    import niti_amd
    from niti_amd import _lib as L
    from niti_amd._lib import NitiError
    from niti_amd.model import NitiModel
    from niti_amd.resnet import normalize_resnet_spec, to_c
    lib = L.lib()
    for spec, want in ((dict(depths=(1,), classes=2049), L.NOT_SUPPORT), (dict(depths=(1,), classes=10, in_c=5), L.NOT_SUPPORT),
                       (dict(depths=(1,), classes=10, width=0), L.INVALID_VALUE)):
        cs = to_c(normalize_resnet_spec(spec))
        out = C.c_void_p(0x5a5a)
        assert lib.niti_model_resnet_check(C.byref(cs), 32, None, None) == want
        assert lib.niti_model_create_resnet(C.byref(cs), 32, 2, C.byref(out)) == want
        assert out.value == 0x5a5a
    # a spec the check passes at batch 1 and refuses at the model's batch (a tensor past 2^29 elements)
    big = dict(depths=(1,), width=128, classes=10, stem="cifar")
    assert niti_amd.resnet_layers(big, 1024)[1]["h"] == 1024
    with pytest.raises(NitiError) as e:
        NitiModel.from_resnet(big, 1024, 8)
    assert e.value.code == L.NOT_SUPPORT
    # the stem's im2col alone: 1100 * 112 * 112 * 160 bytes pass 2^31, while every other tensor of the
    # width-8 net stays under 2^29 elements (its stem output: 1100 * 112 * 112 * 32)
    with pytest.raises(NitiError) as e:
        NitiModel.from_resnet(dict(depths=(1,), width=8, classes=10), 224, 1100)
    assert e.value.code == L.NOT_SUPPORT
    with pytest.raises(ValueError):
        NitiModel.from_resnet(dict(depths=(1,), classes=10, stem=(3, 1, 3, 0)), 32, 2)
