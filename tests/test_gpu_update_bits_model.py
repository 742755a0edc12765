"""The update bits through whole training steps (niti_model_set_update_bits), bit for bit against
chain_step_ref / family_step_ref with the update substituted by the rule as the tests restate it
(update_bits_cases.step_update: each layer's int32 gradient recomputed from the record's input and
output gradient).  Two steps per case: every weight and kept gradient, every output gradient, the
logits and their exponent after each -- the second step reads the first one's weights and every
derived copy of them, so a copy a frozen layer's update disturbed, or one an updated layer left
stale, shows there.
"""
import ctypes as C
import functools
import threading

import numpy as np
import pytest

import chain_cases as CC
import resnet_family_cases as FC
import update_bits_cases as UB

pytestmark = pytest.mark.gpu

# a first layer, a 32 -> 32 3x3 layer the row kernels take, a 32 -> 24 layer on the GEMM path whose
# pooled 2 x 2 map is flattened, the head
NET_ROWS_GEMM = (3, 8, [(32, 3, 1, 1, 0, 0), (32, 3, 1, 1, 1, 0), (24, 3, 1, 1, 1, 1), (10, 1, 0, 0, 0, 0)])
# the same ending in fully connected layers whose weight gradient is recomputed with the update in
# its GEMM epilogue: 96 -> 48 (not the head), and a head whose 48 inputs keep it off the <= 32-output
# head's own path
NET_FC = (3, 8, NET_ROWS_GEMM[2][:3] + [(48, 1, 0, 1, 0, 0), (10, 1, 0, 0, 0, 0)])
BATCH = 8
# two stages at 16 px, the second opening with a stride-2 block and its projection
RES_SMALL = (dict(depths=(1, 1), width=16, classes=10, stem="cifar"), 16, 2)
# 26 parameter layers at width 16: the update runs as two launches (24 + 2 jobs)
RES_DEEP = (dict(depths=(3, 4, 4), width=16, classes=10, stem="cifar"), 16, 2)


@pytest.fixture(scope="module")
def T():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import niti_amd  # noqa: F401
    return torch


def _tup(bits, n):
    return tuple(bits) if isinstance(bits, (list, tuple)) else (bits,) * n


# ------------------------------------------------------------------------------------ references
@functools.lru_cache(maxsize=None)
def _chain_ref(net_name, bits_per_step, seed=5, images=False):
    """(layers, W0, S, [(data, labels, newW, rec)]): chain_step_ref with step k's update under
    bits_per_step[k] (a tuple per step); rec["dw"] holds the kept gradients."""
    import niti_model_ref as R
    import niti_oracle as O
    layers = CC.derive(globals()[net_name])
    W, S = R.init_weights(layers, seed=seed)
    W0 = W
    out = []
    for (data, labels), bits in zip(CC.batches(layers, BATCH, len(bits_per_step), seed + 1, images=images),
                                    bits_per_step):
        x, e = O.quantize_images(data) if images else (data, -3)
        _, rec = CC.chain_step_ref(layers, W, S, x, e, labels)
        newW, kept = UB.step_update(rec["geom"], rec["inp"], rec["dy"], W, bits)
        rec["dw"] = kept
        out.append((data, labels, newW, rec))
        W = newW
    return layers, W0, S, out


@functools.lru_cache(maxsize=None)
def _res_ref(case_name, bits_per_step):
    import niti_oracle as O
    import niti_resnet_ref as RR
    spec, in_hw, batch = globals()[case_name]
    convs = FC.family_convs(spec, in_hw)
    W, S = RR.init_weights(convs, seed=FC.SEED_W)
    W0 = W
    out = []
    for (data, labels), bits in zip(FC.draw_steps(spec, in_hw, batch, False, steps=len(bits_per_step)), bits_per_step):
        _, rec = FC.family_step_ref(convs, W, S, data, FC.EXP_IN, labels, spec["classes"], pool=False)
        G = [O.geom(batch, l["ci"], l["h"], l["h"], l["co"], l["k"], stride=l["stride"], pad=l["pad"]) for l in convs]
        newW, kept = UB.step_update(G, rec["inp"], rec["dy"], W, bits)
        rec["dw"] = kept
        out.append((data, labels, newW, rec))
        W = newW
    return convs, W0, S, out


def _chain_model(net_name, W, S, batch=BATCH):
    from niti_amd.model import NitiModel
    in_c, in_hw, spec = globals()[net_name]
    m = NitiModel.from_chain(spec, in_c, in_hw, batch)
    for i, (w, s) in enumerate(zip(W, S)):
        m.set_weight(i, w, s)
    return m


def _res_model(case_name, W, S):
    from niti_amd.model import NitiModel
    spec, in_hw, batch = globals()[case_name]
    m = NitiModel.from_resnet(spec, in_hw, batch)
    for i, (w, s) in enumerate(zip(W, S)):
        m.set_weight(i, w, s)
    return m


def _check(m, newW, rec, step, logits_key="logits", exp=None, sl=None):
    lg, e = m.logits()
    want = rec[logits_key] if sl is None else rec[logits_key][sl]
    assert e == exp and np.array_equal(lg, want), ("logits", step)
    for i in range(len(newW)):
        dy = rec["dy"][i] if sl is None else rec["dy"][i][sl]
        assert np.array_equal(m.tap(i, 2), dy), ("dy", step, i)
        assert np.array_equal(m.tap(i, 1), rec["dw"][i]), ("dw", step, i)
        assert np.array_equal(m.get_weight(i), newW[i]), ("w", step, i)


def _run_chain(T, net_name, bits, set_bits=True, images=False):
    n = len(globals()[net_name][2])
    per = _tup(bits, n)
    layers, W, S, steps = _chain_ref(net_name, (per, per), images=images)
    m = _chain_model(net_name, W, S)
    if set_bits:
        m.set_update_bits(bits)
        assert m.update_bits() == list(per)
    for step, (data, labels, newW, rec) in enumerate(steps):
        xd, ld = T.from_numpy(data).cuda(), T.from_numpy(labels).cuda()
        if images:
            m.train_step_images(xd, ld)
        else:
            m.train_step(xd, -3, ld)
        _check(m, newW, rec, step, exp=rec["exp"][-1])
        for i, b in enumerate(per):
            if b == 0:
                assert np.array_equal(m.get_weight(i), W[i]) and not m.tap(i, 1).any(), ("frozen", i)
    assert m.rowconv_error() == 0
    return m


def _run_res(T, case_name, bits, set_bits=True):
    spec, in_hw, batch = globals()[case_name]
    n = len(FC.family_convs(spec, in_hw))
    per = _tup(bits, n)
    convs, W, S, steps = _res_ref(case_name, (per, per))
    m = _res_model(case_name, W, S)
    assert len(m.layers) == n
    if set_bits:
        m.set_update_bits(bits)
        assert m.update_bits() == list(per)
    for step, (data, labels, newW, rec) in enumerate(steps):
        m.train_step(T.from_numpy(data).cuda(), FC.EXP_IN, T.from_numpy(labels).cuda())
        _check(m, newW, rec, step, exp=rec["exp_logits"])
        for i, b in enumerate(per):
            if b == 0:
                assert np.array_equal(m.get_weight(i), W[i]) and not m.tap(i, 1).any(), ("frozen", i)
    assert m.rowconv_error() == 0
    return m


# ------------------------------------------------------------------------------------ the rule in a step
@pytest.mark.parametrize("bits", [1, 5, [4, 0, 3, 7]])
def test_chain_rows_and_gemm_layers(T, bits):
    _run_chain(T, "NET_ROWS_GEMM", bits)


@pytest.mark.parametrize("bits", [1, 4, 7, [0, 3, 5, 0, 6]])
def test_chain_fused_fc_update(T, bits):
    m = _run_chain(T, "NET_FC", bits)
    # the two fully connected layers are on 1 x 1 maps and off the P16 weight gradient (tile 16):
    # their update is the GEMM epilogue's
    for i in (3, 4):
        l = m.layers[i]
        assert (l["kh"], l["h"], l["oh"]) == (1, 1, 1) and m.plan(i, 2)[0] != 16


def test_chain_from_images(T):
    _run_chain(T, "NET_ROWS_GEMM", [3, 6, 0, 1], images=True)


@pytest.mark.parametrize("bits", [5, [4, 0, 3, 1, 0, 7, 6]])
def test_residual_two_stages_with_a_stride_2_block(T, bits):
    spec, in_hw, _ = RES_SMALL
    convs = FC.family_convs(spec, in_hw)
    assert len(convs) == 7 and [c["stride"] for c in convs] == [1, 1, 1, 2, 1, 2, 1]
    _run_res(T, "RES_SMALL", bits)


def test_residual_two_update_launches(T):
    """26 layers: jobs 0..23 and 24..25 go in two launches; the bits differ on both sides of the
    boundary, with a frozen layer on each."""
    bits = [(3, 5, 1, 4, 6, 7, 2)[i % 7] for i in range(26)]
    bits[22], bits[23], bits[24], bits[25] = 0, 6, 0, 4
    _run_res(T, "RES_DEEP", bits)


def test_default_models_equal_the_unmodified_oracle(T):
    """Never touched by the setter: the reference's rule 2, chain_step_ref's and family_step_ref's
    own O.conv_wgrad + O.sgd_update."""
    import niti_model_ref as R
    import niti_resnet_ref as RR
    m = _run_chain(T, "NET_FC", 2, set_bits=False)
    assert m.update_bits() == [2] * 5
    layers = CC.derive(NET_FC)
    W, S = R.init_weights(layers, seed=5)
    for (x, labels), (_, _, newW, rec) in zip(CC.batches(layers, BATCH, 2, 6), _chain_ref("NET_FC", ((2,) * 5,) * 2)[3]):
        want, wrec = CC.chain_step_ref(layers, W, S, x, -3, labels)
        for i in range(5):
            assert np.array_equal(want[i], newW[i]) and np.array_equal(wrec["dw"][i], rec["dw"][i])
        W = want
    m = _run_res(T, "RES_SMALL", 2, set_bits=False)
    assert m.update_bits() == [2] * 7
    spec, in_hw, batch = RES_SMALL
    convs = FC.family_convs(spec, in_hw)
    W, S = RR.init_weights(convs, seed=FC.SEED_W)
    for (data, labels), (_, _, newW, rec) in zip(FC.draw_steps(spec, in_hw, batch, False), _res_ref("RES_SMALL", ((2,) * 7,) * 2)[3]):
        want, wrec = FC.family_step_ref(convs, W, S, data, FC.EXP_IN, labels, spec["classes"], pool=False)
        for i in range(7):
            assert np.array_equal(want[i], newW[i]) and np.array_equal(wrec["dw"][i], rec["dw"][i])
        W = want


def test_refusals(T, tmp_path):
    from niti_amd import _lib as L
    from niti_amd.model import NitiModel
    layers, W, S, _ = _chain_ref("NET_ROWS_GEMM", ((2,) * 4,))
    m = _chain_model("NET_ROWS_GEMM", W, S)
    m.set_update_bits({1: 6})
    lib = L.lib()
    for layer, bits in ((-1, 8), (0, 8), (0, -1), (4, 3), (-2, 3), (99, 0)):
        assert lib.niti_model_set_update_bits(m._h, layer, bits, None) == L.INVALID_VALUE
    for bad in (8, -1, [2, 2, 2], [2, 2, 2, 2, 2], {4: 3}, {0: 9}, [2, 2, 2, 2.5], "2222"):
        with pytest.raises(ValueError):
            m.set_update_bits(bad)
    assert m.update_bits() == [2, 6, 2, 2]  # nothing was written
    # a snapshot whose list has the wrong length is refused before any device write
    from niti_amd import checkpoint, mnn_snapshot
    p, q = str(tmp_path / "bad.safetensors"), str(tmp_path / "bad.mnn")
    other = [np.full_like(w, 9) for w in W]
    checkpoint.save_params(p, other, S, m.arch, in_hw=8, chain=m._chain_record(), update_bits=[4, 4, 4])
    mnn_snapshot.save(q, other, S, meta=dict(m._mnn_meta(), update_bits=[4, 4, 4, 4, 4]))
    for load, path in (("load", p), ("load_mnn", q)):
        with pytest.raises(ValueError):
            getattr(m, load)(path)
        assert m.update_bits() == [2, 6, 2, 2]
        for i, w in enumerate(W):
            assert np.array_equal(m.get_weight(i), w)
    # copy_weights_from leaves the destination's bits alone
    dst = NitiModel.from_chain(NET_ROWS_GEMM[2], 3, 8, 2)
    dst.set_update_bits(3)
    dst.copy_weights_from(m)
    assert dst.update_bits() == [3] * 4 and np.array_equal(dst.get_weight(1), W[1])


# ------------------------------------------------------------------------------------ ordering
def test_change_between_replays_of_a_captured_step(T):
    """set_graph(True): step, set_update_bits(5), step -- the replayed update launches read the
    new words (the same device buffers feed both steps: the graph is captured once)."""
    n = 4
    layers, W, S, steps = _chain_ref("NET_ROWS_GEMM", ((2,) * n, (5,) * n, (5,) * n))
    m = _chain_model("NET_ROWS_GEMM", W, S)
    m.set_graph(True)
    xd = ld = None
    for step, (data, labels, newW, rec) in enumerate(steps):
        if xd is None:
            xd, ld = T.from_numpy(data).cuda(), T.from_numpy(labels).cuda()
        else:
            xd.copy_(T.from_numpy(data))
            ld.copy_(T.from_numpy(labels))
        if step == 1:
            m.set_update_bits(5)
        m.train_step(xd, -3, ld)
        _check(m, newW, rec, step, exp=rec["exp"][-1])
    assert m.update_bits() == [5] * n and m.rowconv_error() == 0


def test_change_between_enqueued_dataset_steps(T):
    """train_steps(ds, 0, 2), set_update_bits(3), train_steps(ds, 2, 2) with no host
    synchronisation in between: four reference steps, the change after the second."""
    import niti_model_ref as R
    import niti_oracle as O
    from niti_amd.dataset import DeviceDataset
    layers = CC.derive(NET_ROWS_GEMM)
    n = len(layers)
    W, S = R.init_weights(layers, seed=5)
    rng = np.random.default_rng(21)
    img = rng.integers(0, 256, (4 * BATCH, 3, 8, 8)).astype(np.uint8)
    lab = rng.integers(0, 10, 4 * BATCH).astype(np.int32)
    m = _chain_model("NET_ROWS_GEMM", W, S)
    ds = DeviceDataset(img, lab)
    ds.set_order(np.arange(4 * BATCH, dtype=np.int32))
    m.train_steps(ds, 0, 2)
    m.set_update_bits(3)
    m.train_steps(ds, 2, 2)
    for k in range(4):
        x, e = O.quantize_images(img[k * BATCH:(k + 1) * BATCH])
        _, rec = CC.chain_step_ref(layers, W, S, x, e, lab[k * BATCH:(k + 1) * BATCH])
        W, kept = UB.step_update(rec["geom"], rec["inp"], rec["dy"], W, (2 if k < 2 else 3,) * n)
    T.cuda.synchronize()
    lg, e = m.logits()
    assert e == rec["exp"][-1] and np.array_equal(lg, rec["logits"])
    for i in range(n):
        assert np.array_equal(m.get_weight(i), W[i]), i
        assert np.array_equal(m.tap(i, 1), kept[i]), i
    assert m.rowconv_error() == 0


def test_fit_epoch_sets_the_bits_ahead_of_its_steps(T):
    from niti_amd.dataset import DeviceDataset
    layers, W, S, _ = _chain_ref("NET_ROWS_GEMM", ((2,) * 4,))
    rng = np.random.default_rng(22)
    img = rng.integers(0, 256, (2 * BATCH, 3, 8, 8)).astype(np.uint8)
    lab = rng.integers(0, 10, 2 * BATCH).astype(np.int32)
    a, b = _chain_model("NET_ROWS_GEMM", W, S), _chain_model("NET_ROWS_GEMM", W, S)
    assert a.fit_epoch(DeviceDataset(img, lab), seed=3, epoch=0, update_bits=[4, 0, 6, 1]) == 2
    b.set_update_bits([4, 0, 6, 1])
    b.fit_epoch(DeviceDataset(img, lab), seed=3, epoch=0)
    T.cuda.synchronize()
    assert a.update_bits() == [4, 0, 6, 1]
    for i in range(4):
        assert np.array_equal(a.get_weight(i), b.get_weight(i)), i
    assert np.array_equal(a.get_weight(1), W[1]) and not np.array_equal(a.get_weight(0), W[0])


def test_two_local_ranks_equal_one_device(T):
    from niti_amd.model import LocalGroup
    n = 4
    layers, W, S, steps = _chain_ref("NET_ROWS_GEMM", ((4,) * n, (4,) * n))
    half = BATCH // 2
    ranks = [_chain_model("NET_ROWS_GEMM", W, S, batch=half) for _ in range(2)]
    group = LocalGroup(2)
    for r, m in enumerate(ranks):
        m.attach_local(group, r, exact=True)
        m.set_update_bits(4)
    streams = [T.cuda.Stream() for _ in range(2)]
    for step, (data, labels, newW, rec) in enumerate(steps):
        xd, ld = T.from_numpy(data).cuda(), T.from_numpy(labels).cuda()
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
            _check(m, newW, rec, (step, r), exp=rec["exp"][-1], sl=slice(r * half, (r + 1) * half))
    assert all(m.rowconv_error() == 0 for m in ranks)


# ------------------------------------------------------------------------------------ snapshots
def test_snapshots_restore_the_bits(T, tmp_path):
    from niti_amd.model import NitiModel
    layers, W, S, _ = _chain_ref("NET_ROWS_GEMM", ((2,) * 4,))
    m = _chain_model("NET_ROWS_GEMM", W, S)
    m.set_update_bits([5, 0, 2, 7])
    p, q = str(tmp_path / "b.safetensors"), str(tmp_path / "b.mnn")
    m.save(p)
    m.save_mnn(q)
    for load, path in (("load", p), ("load_mnn", q)):
        other = NitiModel.from_chain(NET_ROWS_GEMM[2], 3, 8, 2)
        other.set_update_bits(3)
        getattr(other, load)(path)
        assert other.update_bits() == [5, 0, 2, 7]
        for i, w in enumerate(W):
            assert np.array_equal(other.get_weight(i), w)


def test_default_snapshot_bytes_are_unchanged(T, tmp_path):
    """A model at the default writes the files it always wrote: no update_bits key, byte for byte
    what the snapshot helpers write when they are not given the bits; and such a snapshot leaves a
    model's own bits alone."""
    from niti_amd import checkpoint, mnn_snapshot
    from niti_amd.model import NitiModel
    layers, W, S, _ = _chain_ref("NET_ROWS_GEMM", ((2,) * 4,))
    m = _chain_model("NET_ROWS_GEMM", W, S)
    m.set_update_bits(6)
    m.set_update_bits(2)  # back at the default: still no key
    p, q = str(tmp_path / "d.safetensors"), str(tmp_path / "d.mnn")
    p0, q0 = str(tmp_path / "d0.safetensors"), str(tmp_path / "d0.mnn")
    m.save(p)
    m.save_mnn(q)
    checkpoint.save_params(p0, W, S, m.arch, in_hw=8, chain=m._chain_record())
    mnn_snapshot.save(q0, W, S, meta={"arch": int(m.arch), "in_hw": 8, "chain": m._chain_record()})
    read = lambda path: open(path, "rb").read()  # noqa: E731

    def parts(path):
        # a safetensors file: the header's length, the JSON header, the tensor bytes.  The writer
        # keeps the metadata in a hash map whose order differs from one call to the next, so the
        # header is compared as the JSON object it is and everything after it byte for byte.
        import json
        raw = read(path)
        n = int.from_bytes(raw[:8], "little")
        return json.loads(raw[8:8 + n]), raw[8 + n:]

    assert parts(p) == parts(p0) and b"update_bits" not in read(p)
    assert "update_bits" not in parts(p)[0]["__metadata__"]
    assert read(q) == read(q0)
    assert read(q + ".wscale.json") == read(q0 + ".wscale.json") and b"update_bits" not in read(q + ".wscale.json")
    other = NitiModel.from_chain(NET_ROWS_GEMM[2], 3, 8, 2)
    other.set_update_bits([1, 3, 5, 7])
    other.load(p)
    other.load_mnn(q)
    assert other.update_bits() == [1, 3, 5, 7]
