"""Shared cases of the depthwise conv tests (importable without a GPU).

A depthwise layer (include/niti_hip.h, niti_dwconv_*) is NITI_Conv_Int8 over the block-diagonal dense
weight dense_of(w), except that its weight gradient's range is taken over the C k k parameters only.
The references below are therefore the existing oracle's: O.conv_fwd / O.conv_dgrad over dense_of(w),
and the diagonal of O.conv_wgrad_acc with O.range_estimate / O.psto / O.sgd_update through the
update-bits rule of tests/update_bits_cases.py.  test_depthwise_cpu.py pins them to the direct sums of
the definition (dw_*_direct).

Op shapes are (n, C, h, k, pad); chain specs are (c_out, k, pad, relu, pool, flatten, depthwise).
"""
from __future__ import annotations

import functools
import os
import sys

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(_ROOT, "oracle"), os.path.join(_ROOT, "mandheling-dsp-training_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import niti_oracle as O  # noqa: E402
import update_bits_cases as UB  # noqa: E402

OP_SHAPES = (
    (1, 16, 1, 3, 1),   # a 1x1 map: every tap but the centre is padding
    (2, 24, 2, 3, 1),   # 8 pad channels, a 2x2 map
    (3, 40, 5, 3, 1),   # odd batch, odd map, cp 48
    (2, 64, 8, 3, 1),
    (2, 20, 7, 5, 2),   # 5x5
    (2, 16, 4, 3, 0),   # the output is smaller than the input
    (2, 16, 3, 3, 2),   # the output is larger than the input; the input gradient's pad is 0
    (1, 16, 13, 3, 1),  # a row that is no multiple of a wave's pixels
    (4, 32, 16, 3, 1),  # more than one workgroup, more than one weight-gradient slab
)
MULTI_SLAB = (4, 32, 16, 3, 1)
SHIFT_CLASSES = ("le0", "eq1", "gt1")  # NITI_Conv_Int8's rule: shift = bw - 7 <= 0, == 1, > 1
WGRAD_CLASSES = ("bw0", "bw1", "bw2", "large")


def r16(x):
    return (x + 15) // 16 * 16


def geom_of(shape):
    n, c, h, k, pad = shape
    return O.geom(n, c, h, h, c, k, pad=pad)


def dense_of(w):
    """[C, 1, k, k] -> the block-diagonal [C, C, k, k]."""
    w = np.asarray(w)
    c = w.shape[0]
    d = np.zeros((c, c) + w.shape[2:], w.dtype)
    d[np.arange(c), np.arange(c)] = w[:, 0]
    return d


def diag_of(acc):
    """[C, C, k, k] -> its diagonal as [C, 1, k, k]."""
    c = acc.shape[0]
    return np.ascontiguousarray(acc[np.arange(c), np.arange(c)][:, None])


# ------------------------------------------------------------------------------------ the definition
def dw_fwd_direct(x, w, pad):
    n, c, h, _ = x.shape
    k = w.shape[2]
    oh = h + 2 * pad - k + 1
    xp = np.zeros((n, c, h + 2 * pad, h + 2 * pad), np.int64)
    xp[:, :, pad:pad + h, pad:pad + h] = x
    acc = np.zeros((n, c, oh, oh), np.int64)
    for ky in range(k):
        for kx in range(k):
            acc += xp[:, :, ky:ky + oh, kx:kx + oh] * w[None, :, 0, ky, kx, None, None].astype(np.int64)
    return acc.astype(np.int32)


def dw_dgrad_direct(dy, w, pad, h):
    n, c, oh, _ = dy.shape
    k = w.shape[2]
    acc = np.zeros((n, c, h + 2 * pad, h + 2 * pad), np.int64)  # over the padded input; the border is dropped
    for ky in range(k):
        for kx in range(k):
            acc[:, :, ky:ky + oh, kx:kx + oh] += dy.astype(np.int64) * w[None, :, 0, ky, kx, None, None].astype(np.int64)
    return acc[:, :, pad:pad + h, pad:pad + h].astype(np.int32)


def dw_wgrad_direct(x, dy, k, pad):
    n, c, h, _ = x.shape
    oh = dy.shape[2]
    xp = np.zeros((n, c, h + 2 * pad, h + 2 * pad), np.int64)
    xp[:, :, pad:pad + h, pad:pad + h] = x
    acc = np.zeros((c, 1, k, k), np.int64)
    for ky in range(k):
        for kx in range(k):
            acc[:, 0, ky, kx] = (xp[:, :, ky:ky + oh, kx:kx + oh] * dy.astype(np.int64)).sum(axis=(0, 2, 3))
    return acc.astype(np.int32)


# ------------------------------------------------------------------------------------ the references
def requant_under(acc, amax=None):
    """(int8 in acc's shape, inc) of NITI_Conv_Int8's rule; amax: the range's max|.| where it is larger
    than acc's own (what a MAX all-reduce over the ranks leaves in the range words)."""
    if amax is None:
        return O.requant_fwd(acc)
    assert amax >= int(np.abs(acc.astype(np.int64)).max())
    q, inc = O.requant_fwd(np.concatenate([acc.ravel(), np.array([amax], np.int32)]))
    return q[:-1].reshape(acc.shape), inc


def _e8(v):
    return int(np.int8(np.int32(v).astype(np.int8)))


def dw_fwd_ref(g, x, w, exp_in=-7, wscale=-7, relu=False, amax=None):
    """(y int8, exponent, acc int32) of the forward."""
    acc, st = O.conv_fwd_acc(g, x, dense_of(w))
    assert st.overflow == 0
    y, inc = requant_under(acc, amax)
    return (O.relu(y) if relu else y), _e8(exp_in + wscale + inc), acc


def dw_dgrad_ref(g, dy, w, relu_mask=None, amax=None):
    """(dx int8, inc, acc int32) of the input gradient; relu_mask: dx = mask > 0 ? q : 0."""
    acc, st = O.conv_dgrad_acc(g, dy, dense_of(w))
    assert st.overflow == 0
    dx, inc = requant_under(acc, amax)
    return (O.relu_grad(relu_mask, dx) if relu_mask is not None else dx), inc, acc


def dw_wgrad_ref(g, x, dy):
    """(acc int32 [C, 1, k, k], bw over these values only, bw of the dense emulation's tensor)."""
    dense, st = O.conv_wgrad_acc(g, x, dy)
    assert st.overflow == 0
    acc = diag_of(dense)
    return acc, O.range_estimate(acc), O.range_estimate(dense)


def dw_update_ref(w, acc, bits=2):
    """(new weights, kept int8 gradient) under the layer's update bits."""
    return UB.apply_update(w, acc, bits)


# ------------------------------------------------------------------------------------ op-level inputs
def _ro(*arrays):
    for a in arrays:
        a.flags.writeable = False
    return arrays


def _bw(acc):
    return O.range_estimate(np.ascontiguousarray(acc, np.int32))


def _in_class(bw, cls):
    return {"le0": bw <= 7, "eq1": bw == 8, "gt1": bw > 8}[cls]


@functools.lru_cache(maxsize=None)
def act_inputs(shape, cls, dgrad=False):
    """(a, w, mask): the conv's input (x, or dy for the input gradient), weights [C, 1, k, k] and a relu
    mask of the output's shape, scaled so the accumulators' bit width falls in the shift class: fixed
    uniform draws times the smallest amplitude that gets there."""
    n, c, h, k, pad = shape
    oh = h + 2 * pad - k + 1
    rng = np.random.default_rng(1000 + 7 * OP_SHAPES.index(shape) + (1 if dgrad else 0))
    ua = rng.uniform(-1, 1, (n, c, oh, oh) if dgrad else (n, c, h, h))
    uw = rng.uniform(-1, 1, (c, 1, k, k))
    mask = rng.integers(-3, 4, (n, c, h, h) if dgrad else (n, c, oh, oh)).astype(np.int8)
    for amp in range(1, 128):
        a, w = np.rint(ua * amp).astype(np.int8), np.rint(uw * amp).astype(np.int8)
        acc = dw_dgrad_direct(a, w, pad, h) if dgrad else dw_fwd_direct(a, w, pad)
        if _in_class(_bw(acc), cls):
            return _ro(a, w, mask)
    raise AssertionError(f"no amplitude puts {shape} in {cls}")


@functools.lru_cache(maxsize=None)
def wgrad_inputs(shape, cls):
    """(x, dy, w) of a weight-gradient case.  bw0: dy all zero.  bw1 / bw2: dy is one pixel of value 1 / 2
    and x in -2..2 with a 2 under the window's centre tap, so max|acc| is 2 / 4.  large: random."""
    n, c, h, k, pad = shape
    oh = h + 2 * pad - k + 1
    rng = np.random.default_rng(2000 + 11 * OP_SHAPES.index(shape) + WGRAD_CLASSES.index(cls))
    w = rng.integers(-127, 128, (c, 1, k, k)).astype(np.int8)
    if cls == "large":
        return _ro(O.synth_x(rng, (n, c, h, h)), O.synth_dy(rng, (n, c, oh, oh), zero_frac=0.3), w)
    x = rng.integers(-2, 3, (n, c, h, h)).astype(np.int8)
    dy = np.zeros((n, c, oh, oh), np.int8)
    if cls != "bw0":
        o = min(pad, oh - 1)  # the output pixel; its centre tap ky = kx = pad reads input pixel (o, o)
        dy[n - 1, :, o, o] = 1 if cls == "bw1" else 2
        x[n - 1, :, o, o] = 2
    return _ro(x, dy, w)


# ------------------------------------------------------------------------------------ chain nets
# S: separable blocks (dw 3x3 then 1x1) on the GEMM path
NET_S = (3, 8, [(16, 3, 1, 1, 0, 0, 0), (0, 3, 1, 1, 0, 0, 1), (24, 1, 0, 1, 1, 0, 0), (0, 3, 1, 1, 1, 0, 1),
                (40, 1, 0, 1, 0, 1, 0), (10, 1, 0, 0, 0, 0, 0)])
# R: depthwise layers between row-kernel layers, a pooled row-kernel layer in front of the first
NET_R = (1, 8, [(32, 3, 1, 1, 1, 0, 0), (0, 3, 1, 1, 0, 0, 1), (64, 3, 1, 1, 1, 0, 0), (0, 3, 1, 0, 0, 0, 1),
                (32, 3, 1, 1, 1, 0, 0), (7, 1, 0, 0, 0, 0, 0)])
# O: odd maps, 5x5, a pool on an odd map after a depthwise layer, a flatten on one
NET_O = (4, 9, [(24, 3, 1, 1, 0, 0, 0), (0, 5, 2, 1, 1, 0, 1), (0, 3, 0, 1, 0, 1, 1), (20, 1, 0, 0, 0, 0, 0)])
NETS = {"NET_S": NET_S, "NET_R": NET_R, "NET_O": NET_O}


def derive(net):
    """The layer dicts of a (in_c, in_hw, spec) net whose spec tuples may carry `depthwise`."""
    c, h, spec = net
    out = []
    for l in spec:
        co, k, pad, relu, pool, flatten = l[:6]
        dw = l[6] if len(l) > 6 else 0
        co = c if dw else co
        out.append(dict(ci=c, co=co, k=k, pad=pad, h=h, relu=relu, pool=pool, flatten=flatten, dw=dw))
        oh = h + 2 * pad - k + 1
        ph = (oh - 2) // 2 + 1 if pool else oh
        c, h = (co * ph * ph, 1) if flatten else (co, ph)
    return out


def weight_shape(l):
    return (l["co"], 1 if l.get("dw") else l["ci"], l["k"], l["k"])


def init_weights(layers, seed):
    """niti_amd.init.xavier_int8 on every layer's shape, one default_rng(seed) in layer order (what
    NitiModel.init_weights does)."""
    from niti_amd.init import xavier_int8
    rng = np.random.default_rng(seed)
    ws = [xavier_int8(weight_shape(l), rng) for l in layers]
    return [w for w, _ in ws], [s for _, s in ws]


def dw_chain_step_ref(layers, W, S, x, exp_in, labels, bits=None):
    """chain_cases.chain_step_ref with depthwise layers (weights [C, 1, k, k]) and per-layer update
    bits (None: 2 everywhere).  rec["dw"] is the kept int8 gradient, rec["bw"] each gradient's range."""
    import niti_model_ref as R
    n = x.shape[0]
    rec = dict(inp=[], y=[], r=[], p=[], exp=[], dw=[], dy=[], geom=[], bw=[])
    a, exp = x, exp_in
    dense = [dense_of(w) if l.get("dw") else w for l, w in zip(layers, W)]
    for i, l in enumerate(layers):
        g = O.geom(n, l["ci"], l["h"], l["h"], l["co"], l["k"], pad=l["pad"])
        rec["geom"].append(g)
        rec["inp"].append(a)
        y, exp, _, st = O.conv_fwd(g, a, dense[i], exp, S[i])
        assert st.overflow == 0
        r = O.relu(y) if l["relu"] else y
        p = O.maxpool(r) if l["pool"] else None
        rec["y"].append(y)
        rec["r"].append(r)
        rec["p"].append(p)
        rec["exp"].append(exp)
        a = r if p is None else p
        if l["flatten"]:
            a = a.reshape(n, -1, 1, 1)
    last = layers[-1]
    logits = rec["r"][-1].reshape(n, last["co"])
    d = O.loss_grad(logits, rec["exp"][-1], R.onehot(labels, last["co"])).reshape(n, last["co"], 1, 1)
    dy = [None] * len(layers)
    dy[-1] = d
    newW = list(W)
    for i in range(len(layers) - 1, -1, -1):
        g = rec["geom"][i]
        acc, st = O.conv_wgrad_acc(g, rec["inp"][i], dy[i])
        assert st.overflow == 0
        if layers[i].get("dw"):
            acc = diag_of(acc)
        rec["bw"].insert(0, O.range_estimate(acc))
        if i > 0:
            dx, _, _, _ = O.conv_dgrad(g, dy[i], dense[i])
            pl = layers[i - 1]
            if pl["flatten"]:
                dx = dx.reshape((rec["p"] if pl["pool"] else rec["r"])[i - 1].shape)
            if pl["pool"]:
                dx = O.maxpool_grad(rec["r"][i - 1], rec["p"][i - 1], dx)
            if pl["relu"]:
                dx = O.relu_grad(rec["y"][i - 1], dx)
            dy[i - 1] = dx
        newW[i], g8 = UB.apply_update(W[i], acc, 2 if bits is None else bits[i])
        rec["dw"].insert(0, g8)
    rec["dy"] = dy
    rec["logits"] = logits
    return newW, rec


def batches(layers, batch, steps, seed, images=False):
    import chain_cases as CC
    return CC.batches(layers, batch, steps, seed, images=images)


def ref_steps(layers, W, S, data, exp_in=-3, bits=None):
    """dw_chain_step_ref over `data`: [(new weights, record, x, exponent)] per step."""
    out = []
    for x, labels in data:
        e = exp_in
        if x.dtype == np.uint8:
            x, e = O.quantize_images(x)
        W, rec = dw_chain_step_ref(layers, W, S, x, e, labels, bits=bits)
        out.append((W, rec, x, e))
    return out
