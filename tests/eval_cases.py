"""Expected values of the evaluation metrics (niti_head_metrics, the 710 Execution, the models'
eval_* calls): NumPy, float64, from the definitions in include/niti_hip.h.

  pred_i  the first index of the row maximum over the first `classes` lanes
  rank_i  #{j : l[j] > l[label] or (l[j] == l[label] and j < label)}
  loss_i  log(sum_j exp(z_j - z_max)) - (z_label - z_max),  z = l * 2^ascale
An image whose label is negative is counted nowhere (its loss is reported as 0).

LOSS_RTOL is derived, not measured: at most 2048 terms summed in double, each within a few ulp of
exp / log (about 1e-12 in all), leaving three orders of margin; absolute where the value is below 1.
"""
import math

import numpy as np

LOSS_RTOL = 1e-9


def loss_close(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return bool(np.all(np.abs(got - want) <= LOSS_RTOL * np.maximum(1.0, np.abs(want))))


def metrics_ref(logits, ascale, labels, topk, classes=None):
    """logits int8 [batch][ld] (the first `classes` lanes count), labels int [batch]."""
    logits = np.asarray(logits)
    b = logits.shape[0]
    classes = logits.shape[1] if classes is None else classes
    l = logits[:, :classes].astype(np.int64)
    labels = np.asarray(labels).astype(np.int64)
    pred = np.argmax(l, axis=1).astype(np.int32)  # the first maximum
    mx = l.max(axis=1, keepdims=True)
    d = np.ldexp((l - mx).astype(np.float64), int(ascale))  # exact
    lse = np.log(np.exp(d).sum(axis=1))
    loss = np.zeros(b, np.float64)
    rank = np.full(b, -1, np.int64)
    idx = np.arange(classes)
    for i in range(b):
        t = labels[i]
        if t < 0:
            continue
        loss[i] = lse[i] - d[i, t]
        rank[i] = int(np.sum(l[i] > l[i, t]) + np.sum((l[i] == l[i, t]) & (idx < t)))
    counted = labels >= 0
    return {"pred": pred, "loss": loss, "rank": rank, "images": int(counted.sum()),
            "top1": int(np.sum(counted & (rank == 0))), "topk": int(np.sum(counted & (rank < topk))),
            "loss_sum": math.fsum(loss[counted])}


def add_totals(a, b):
    return {k: a[k] + b[k] for k in ("images", "top1", "topk", "loss_sum")}
