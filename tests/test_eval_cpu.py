"""CPU-side checks of the evaluation pass's C ABI: the 710 (NITI_LOSS_Int8) slot exists,
niti_head_metrics validates its arguments on the host before any device call, the model entry
points are exported and bound -- and the NumPy expected-value helper the GPU tests compare
against agrees with hand-computed values."""
import ctypes as C
import math

import numpy as np
import pytest

import eval_cases as E


@pytest.fixture(scope="module")
def L():
    from niti_amd import _lib
    return _lib


def test_loss_execution_creates_without_common(L):
    lib = L.lib()
    assert L.OP_LOSS_INT8 == 710
    h = C.c_void_p()
    assert lib.niti_create_execution(710, None, C.byref(h)) == 0
    assert lib.niti_execution_workspace_bytes(h) == 0
    lib.niti_destroy_execution(h)


def test_head_metrics_validation(L):
    """Every rejected argument of niti_head_metrics with its code; the pointers are small integers
    that are never dereferenced (the calls fail validation first)."""
    lib = L.lib()
    INVALID, NOT_SUPPORT = 5, 2
    p = lambda v: C.c_void_p(v)  # noqa: E731
    nbytes = C.c_size_t()
    assert lib.niti_head_metrics_workspace(16, C.byref(nbytes)) == 0 and nbytes.value >= 16 * 12
    assert lib.niti_head_metrics_workspace(0, C.byref(nbytes)) == INVALID
    assert lib.niti_head_metrics_workspace(16, None) == INVALID
    assert lib.niti_head_metrics_workspace(16, C.byref(nbytes)) == 0

    def call(logits=256, batch=16, classes=10, ld=16, ascale=512, labels=768, topk=5, totals=1024, ws=2048,
             ws_bytes=None):
        return lib.niti_head_metrics(p(logits) if logits else None, batch, classes, ld, p(ascale) if ascale else None,
                                     p(labels) if labels else None, topk, None, None, p(totals) if totals else None,
                                     p(ws) if ws else None, nbytes.value if ws_bytes is None else ws_bytes, None)

    for kw in ({"logits": 0}, {"ascale": 0}, {"labels": 0}, {"totals": 0}):
        assert call(**kw) == INVALID, kw
    for kw in ({"batch": 0}, {"batch": -3}, {"classes": 0}, {"classes": -1}, {"classes": 17, "ld": 16}):
        assert call(**kw) == INVALID, kw
    for kw in ({"topk": 0}, {"topk": -1}, {"topk": 11}):
        assert call(**kw) == INVALID, kw
    assert call(classes=2049, ld=2064) == NOT_SUPPORT
    assert call(classes=4096, ld=4096, topk=5) == NOT_SUPPORT
    for kw in ({"ws_bytes": nbytes.value - 1}, {"ws_bytes": 0}, {"ws": 0}):
        assert call(**kw) == INVALID, kw


def test_eval_entry_points_are_bound(L):
    lib = L.lib()
    for name in ("niti_model_eval_step", "niti_model_eval_step_images", "niti_model_eval_reset", "niti_model_eval_read",
                 "niti_model_eval_topk", "niti_model_get_predictions", "niti_model_copy_weights", "niti_head_metrics",
                 "niti_head_metrics_workspace"):
        assert name in L.header_functions(), name
        assert getattr(lib, name).argtypes is not None, name
    assert lib.niti_model_copy_weights.argtypes == [C.c_void_p, C.c_void_p, C.c_void_p]
    assert lib.niti_model_copy_weights(None, None, None) == 5  # INVALID_VALUE, no device call
    assert lib.niti_model_eval_step(None, None, 0, None, None) == 5
    assert lib.niti_model_eval_topk(None, 5) == 5
    assert C.sizeof(L.EvalTotals) == 32


def test_metrics_ref_hand_values():
    """The expected-value helper on rows whose metrics are known in closed form."""
    # a constant row: first-max 0, loss log(classes) whatever the scale; top-1 only for label 0
    lg = np.full((3, 16), 7, np.int8)
    r = E.metrics_ref(lg, -3, [0, 4, -1], topk=5, classes=10)
    assert list(r["pred"]) == [0, 0, 0] and list(r["rank"]) == [0, 4, -1]
    assert (r["images"], r["top1"], r["topk"]) == (2, 1, 2)
    assert E.loss_close(r["loss"], [math.log(10), math.log(10), 0.0])
    assert E.loss_close(r["loss_sum"], 2 * math.log(10))
    # two classes one step apart at scale 2^0: loss = log(1 + e^-1) for the larger, + 1 for the smaller
    lg = np.array([[5, 4], [5, 4]], np.int8)
    r = E.metrics_ref(lg, 0, [0, 1], topk=1)
    assert E.loss_close(r["loss"], [math.log1p(math.exp(-1)), 1 + math.log1p(math.exp(-1))])
    assert (r["top1"], r["topk"]) == (1, 1)
    # a duplicated maximum: the first index wins, the second has rank 1
    lg = np.array([[-3, 9, 2, 9]], np.int8)
    assert E.metrics_ref(lg, -7, [3], topk=1)["top1"] == 0 and E.metrics_ref(lg, -7, [3], topk=2)["topk"] == 1
    assert E.metrics_ref(lg, -7, [1], topk=1)["top1"] == 1
    # all-negative rows with +127 beyond `classes`: the padding is not a class
    lg = np.full((1, 16), 127, np.int8)
    lg[0, :10] = np.arange(-20, -10)
    assert E.metrics_ref(lg, -3, [9], topk=1, classes=10)["pred"][0] == 9
    assert not E.loss_close(1.0, 1.0 + 1e-8) and E.loss_close(1e-12, 0.0) and E.loss_close(4000.0, 4000.0 + 1e-6)
