"""GPU parity of niti_head_metrics (csrc/niti_metrics.hip) and of the 710 Execution
(NITI_LOSS_Int8) against the NumPy float64 helper tests/eval_cases.py.

pred and the integer totals must be exactly equal; the per-image loss and loss_sum within
eval_cases.LOSS_RTOL (1e-9 relative, absolute below 1: derived there, not measured); loss_sum
bit-identical between two runs on the same inputs.  The 710 output must equal float32(mean loss_i)
within one float32 ulp.

The 710 slot returns the reference's value, *outputPtr = average_sum / ib * (-1) with average_sum
the sum of the rows' log-softmax at the target (NITI_CPULoss_Int8.cpp:103-125): the positive batch
mean of loss_i = -log softmax(z)[label].
"""
import numpy as np
import pytest

import eval_cases as E

pytestmark = pytest.mark.gpu

# (batch, classes, ld): smallest batch; batch not a multiple of the 4 rows per block; classes not a
# multiple of 16; ImageNet head; the class limit; more than one block
SHAPES = [(1, 10, 16), (5, 10, 16), (16, 37, 48), (3, 1000, 1008), (2, 2048, 2048), (257, 10, 16)]
KINDS = ["random", "constant", "all_min", "negative_pad127", "dup_max", "label_last", "some_excluded"]


@pytest.fixture(scope="module")
def T():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import niti_amd  # noqa: F401
    return torch


@pytest.fixture(scope="module")
def ops(T):
    from niti_amd import ops
    return ops


def _case(kind, batch, classes, ld, seed):
    rng = np.random.default_rng(seed)
    lg = rng.integers(-128, 128, (batch, ld), dtype=np.int8)  # (padding lanes random: never read)
    labels = rng.integers(0, classes, batch).astype(np.int32)
    if kind == "constant":
        lg[:, :classes] = rng.integers(-128, 128, (batch, 1), dtype=np.int8)
        labels[::2] = 0  # first-max gives pred 0: top-1 only where the label is 0
    elif kind == "all_min":
        lg[:, :classes] = -128
    elif kind == "negative_pad127":
        lg[:, :classes] = rng.integers(-128, 0, (batch, classes), dtype=np.int8)
        lg[:, classes:] = 127
    elif kind == "dup_max":
        lg[:, :classes] = rng.integers(-128, 100, (batch, classes), dtype=np.int8)
        a = rng.integers(0, classes - 1, batch)
        b = np.minimum(a + 1 + rng.integers(0, classes, batch), classes - 1)
        lg[np.arange(batch), a] = 101
        lg[np.arange(batch), b] = 101
        labels = np.where(np.arange(batch) % 2 == 0, a, b).astype(np.int32)  # the first and the second maximum
    elif kind == "label_last":
        labels[:] = classes - 1
    elif kind == "some_excluded":
        labels[rng.random(batch) < 0.4] = -1
        labels[0] = -1
    return lg, labels


def _run(T, ops, lg, labels, classes, ascale, topk, totals=None):
    pred, loss, totals = ops.head_metrics(T.from_numpy(lg).cuda(), classes, T.tensor([ascale], dtype=T.int8).cuda(),
                                          T.from_numpy(labels).cuda(), topk=topk, totals=totals)
    T.cuda.synchronize()
    return pred.cpu().numpy(), loss.cpu().numpy(), totals


def _check(T, ops, lg, labels, classes, ascale, topk):
    want = E.metrics_ref(lg, ascale, labels, topk, classes)
    pred, loss, totals = _run(T, ops, lg, labels, classes, ascale, topk)
    got = ops.read_eval_totals(totals)
    tag = (lg.shape, classes, ascale, topk)
    assert np.array_equal(pred, want["pred"]), tag
    assert (got["images"], got["top1"], got["topk"]) == (want["images"], want["top1"], want["topk"]), tag
    counted = labels >= 0
    assert got["top1"] == int(np.sum(pred[counted] == labels[counted])), tag
    assert E.loss_close(loss, want["loss"]), (tag, np.abs(loss - want["loss"]).max())
    assert E.loss_close(got["loss_sum"], want["loss_sum"]), (tag, got["loss_sum"], want["loss_sum"])
    return totals, got


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_head_metrics_matches_reference(T, ops, shape, kind):
    batch, classes, ld = shape
    lg, labels = _case(kind, batch, classes, ld, seed=batch * 7 + classes + KINDS.index(kind))
    if kind == "random":
        for ascale in (-7, -3, 0, 4):
            for topk in (1, 5):
                _check(T, ops, lg, labels, classes, ascale, topk)
    else:
        _check(T, ops, lg, labels, classes, -3, 5)
        _check(T, ops, lg, labels, classes, 0, 1)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_head_metrics_deterministic_and_accumulating(T, ops, shape):
    batch, classes, ld = shape
    lg, labels = _case("some_excluded" if batch > 1 else "random", batch, classes, ld, seed=99 + batch)
    t1, g1 = _check(T, ops, lg, labels, classes, -3, 5)
    t2, g2 = _check(T, ops, lg, labels, classes, -3, 5)
    assert np.array_equal(t1.cpu().numpy(), t2.cpu().numpy())  # fresh totals: bit-identical loss_sum
    _run(T, ops, lg, labels, classes, -3, 5, totals=t1)  # the same totals again: everything doubles
    g = ops.read_eval_totals(t1)
    assert (g["images"], g["top1"], g["topk"]) == (2 * g1["images"], 2 * g1["top1"], 2 * g1["topk"])
    assert g["loss_sum"] == 2 * g1["loss_sum"]  # s + s is exact


def test_head_metrics_unaligned_rows(T, ops):
    """ld not a multiple of 16 (the 710 slot's rows are [batch][classes]): the byte-load path."""
    lg, labels = _case("some_excluded", 9, 10, 10, seed=3)
    _check(T, ops, lg, labels, 10, -6, 5)
    lg, labels = _case("negative_pad127", 6, 37, 41, seed=4)
    _check(T, ops, lg, labels, 37, -2, 1)


def _onehot(labels, tc):
    oh = np.zeros((len(labels), tc), np.int32)
    oh[np.arange(len(labels)), labels] = 1
    return oh


@pytest.mark.parametrize("on_host", [False, True], ids=["device", "host"])
@pytest.mark.parametrize("batch,classes,tc,ascale", [(9, 10, 10, -6), (5, 37, 37, -3), (7, 12, 10, 0), (3, 1000, 1000, -4)])
def test_loss_execution_710(T, ops, batch, classes, tc, ascale, on_host):
    """{logits, ascale, one-hot target} -> float32 mean loss; tc < classes: the classes at and beyond
    tc never are the label."""
    import niti_amd
    rng = np.random.default_rng(710 + batch)
    logits = rng.integers(-128, 128, (batch, classes), dtype=np.int8)
    labels = rng.integers(0, tc, batch)
    want = np.float32(E.metrics_ref(logits, ascale, labels, 1)["loss"].mean())
    put = (lambda a: T.from_numpy(np.ascontiguousarray(a).copy())) if on_host else \
        (lambda a: T.from_numpy(np.ascontiguousarray(a)).cuda())
    out = put(np.full(1, -1.0, np.float32))
    ins = [ops.tensor(put(logits), (batch, classes)), ops.tensor(put(np.array([ascale], np.int8)), (1, 1, 1, 1)),
           ops.tensor(put(_onehot(labels, tc)), (batch, tc))]
    ex = ops.NITIExecution(niti_amd.OP_LOSS_INT8, None)
    assert ex.resize(ins, [ops.tensor(out, (1, 1, 1, 1))]) == 0
    for _ in range(2):  # (a second execute starts from zeroed totals again)
        assert ex.execute(ins, [ops.tensor(out, (1, 1, 1, 1))]) == 0
        T.cuda.synchronize()
        got = np.float32(out.cpu().numpy()[0])
        assert abs(float(got) - float(want)) <= 2.0 ** -23 * abs(float(want)), (got, want)


def test_loss_execution_710_rejects(T, ops):
    import niti_amd
    z = T.zeros(4 * 4096, dtype=T.int8).cuda()
    f = T.zeros(1, dtype=T.float32).cuda()
    t = T.zeros(4 * 4096, dtype=T.int32).cuda()
    ex = ops.NITIExecution(niti_amd.OP_LOSS_INT8, None)
    a = ops.tensor(z, (1, 1, 1, 1))
    assert ex.resize([ops.tensor(z, (4, 4096)), a, ops.tensor(t, (4, 4096))], [ops.tensor(f, (1, 1, 1, 1))]) == 2
    assert ex.resize([ops.tensor(z, (4, 12, 1, 1), niti_amd.FORMAT_NC4HW4), a, ops.tensor(t, (4, 12))],
                     [ops.tensor(f, (1, 1, 1, 1))]) == 2  # NOT_SUPPORT, as 711
