"""Shared cases of the strided-layer tests (importable without a GPU).

A stride-2 depthwise layer (include/niti_hip.h, niti_dwconv2_*) is NITI_Conv_Int8 over the block-diagonal
dense weight with stride_h = stride_w = 2, so the references are the existing oracle's O.conv_fwd_acc /
conv_dgrad_acc / conv_wgrad_acc over O.geom(..., stride=2) and depthwise_cases.dense_of(w), with the
requantise, range and update helpers of depthwise_cases.  test_strided_cpu.py pins them to the direct
triple-loop sums of the three formulas (dw2_*_direct).  The chain reference is depthwise_cases' step
restated with each layer's stride in its geometry.

Op shapes are (n, C, h, k, pad) at stride 2; chain specs are (c_out, k, pad, relu, pool, flatten,
depthwise, stride).
"""
from __future__ import annotations

import functools

import numpy as np

import depthwise_cases as DC
from depthwise_cases import O, UB  # noqa: F401

OP_SHAPES = {
    "A": (2, 16, 8, 3, 1),    # even map, all four parity classes
    "B": (3, 24, 8, 3, 0),    # pad channels, odd batch; a last row / column no output reads
    "C": (1, 16, 7, 3, 1),    # odd map
    "D": (2, 40, 9, 5, 2),    # 5x5
    "E": (1, 16, 2, 3, 1),    # 1x1 output
    "F": (2, 16, 6, 5, 0),    # 5x5 to 1x1, pad 0
    "G": (4, 32, 32, 3, 1),   # oh = 16: two row bands, several workgroups, more than one slab
}
SHAPE_IDS = tuple(OP_SHAPES)
MULTI_SLAB = "G"
BUMP_SHAPES = ("B", "D", "G")
SHIFT_CLASSES = DC.SHIFT_CLASSES
WGRAD_CLASSES = DC.WGRAD_CLASSES


def out_hw(h, k, pad, stride=2):
    return (h + 2 * pad - k) // stride + 1


def geom_of(shape, stride=2):
    n, c, h, k, pad = shape
    return O.geom(n, c, h, h, c, k, stride=stride, pad=pad)


# ------------------------------------------------------------------------------------ the definition
def dw2_fwd_direct(x, w, pad):
    """acc[n][c][oy][ox] = sum x[n][c][2 oy + ky - pad][2 ox + kx - pad] w[c][ky][kx]"""
    n, c, h, _ = x.shape
    k = w.shape[2]
    oh = out_hw(h, k, pad)
    acc = np.zeros((n, c, oh, oh), np.int64)
    for oy in range(oh):
        for ox in range(oh):
            for ky in range(k):
                for kx in range(k):
                    iy, ix = 2 * oy + ky - pad, 2 * ox + kx - pad
                    if 0 <= iy < h and 0 <= ix < h:
                        acc[:, :, oy, ox] += x[:, :, iy, ix].astype(np.int64) * w[None, :, 0, ky, kx].astype(np.int64)
    return acc.astype(np.int32)


def dw2_dgrad_direct(dy, w, pad, h):
    """acc[n][c][y][x] = sum over (ky, kx) with y + pad - ky, x + pad - kx even and inside the output of
    dy[n][c][(y + pad - ky) / 2][(x + pad - kx) / 2] w[c][ky][kx]"""
    n, c, oh, _ = dy.shape
    k = w.shape[2]
    acc = np.zeros((n, c, h, h), np.int64)
    for y in range(h):
        for x in range(h):
            for ky in range(k):
                for kx in range(k):
                    ny, nx = y + pad - ky, x + pad - kx
                    if ny % 2 or nx % 2 or not (0 <= ny // 2 < oh and 0 <= nx // 2 < oh):
                        continue
                    acc[:, :, y, x] += dy[:, :, ny // 2, nx // 2].astype(np.int64) * w[None, :, 0, ky, kx].astype(np.int64)
    return acc.astype(np.int32)


def dw2_wgrad_direct(x, dy, k, pad):
    """acc[c][ky][kx] = sum dy[n][c][oy][ox] x[n][c][2 oy + ky - pad][2 ox + kx - pad]"""
    n, c, h, _ = x.shape
    oh = dy.shape[2]
    acc = np.zeros((c, 1, k, k), np.int64)
    for ky in range(k):
        for kx in range(k):
            for oy in range(oh):
                for ox in range(oh):
                    iy, ix = 2 * oy + ky - pad, 2 * ox + kx - pad
                    if 0 <= iy < h and 0 <= ix < h:
                        acc[:, 0, ky, kx] += (dy[:, :, oy, ox].astype(np.int64) * x[:, :, iy, ix].astype(np.int64)).sum(axis=0)
    return acc.astype(np.int32)


def dgrad_taps(k, pad, py, px):
    """The taps (ky, kx) a pixel of parity (py, px) sums."""
    return [(ky, kx) for ky in range(k) for kx in range(k) if (py + pad - ky) % 2 == 0 and (px + pad - kx) % 2 == 0]


# ------------------------------------------------------------------------------------ the references
# (depthwise_cases' own, on the strided geometry: they take any geometry the oracle does)
dw_fwd_ref = DC.dw_fwd_ref
dw_dgrad_ref = DC.dw_dgrad_ref
dw_wgrad_ref = DC.dw_wgrad_ref
dw_update_ref = DC.dw_update_ref


# ------------------------------------------------------------------------------------ op-level inputs
@functools.lru_cache(maxsize=None)
def act_inputs(sid, cls, dgrad=False):
    """(a, w, mask) as depthwise_cases.act_inputs, for the stride-2 shape `sid`."""
    n, c, h, k, pad = OP_SHAPES[sid]
    oh = out_hw(h, k, pad)
    g = geom_of(OP_SHAPES[sid])
    rng = np.random.default_rng(5000 + 7 * SHAPE_IDS.index(sid) + (1 if dgrad else 0))
    ua = rng.uniform(-1, 1, (n, c, oh, oh) if dgrad else (n, c, h, h))
    uw = rng.uniform(-1, 1, (c, 1, k, k))
    mask = rng.integers(-3, 4, (n, c, h, h) if dgrad else (n, c, oh, oh)).astype(np.int8)
    for amp in range(1, 128):
        a, w = np.rint(ua * amp).astype(np.int8), np.rint(uw * amp).astype(np.int8)
        acc = (O.conv_dgrad_acc if dgrad else O.conv_fwd_acc)(g, a, DC.dense_of(w))[0]
        if DC._in_class(DC._bw(acc), cls):
            return DC._ro(a, w, mask)
    raise AssertionError(f"no amplitude puts {sid} in {cls}")


@functools.lru_cache(maxsize=None)
def wgrad_inputs(sid, cls):
    """(x, dy, w) as depthwise_cases.wgrad_inputs: bw0 dy all zero; bw1 / bw2 one dy pixel of 1 / 2 over x in
    -2..2 with a 2 under its centre tap (input pixel 2 o + (k - 1) / 2 - pad), so max|acc| is 2 / 4; large random."""
    n, c, h, k, pad = OP_SHAPES[sid]
    oh = out_hw(h, k, pad)
    rng = np.random.default_rng(6000 + 11 * SHAPE_IDS.index(sid) + WGRAD_CLASSES.index(cls))
    w = rng.integers(-127, 128, (c, 1, k, k)).astype(np.int8)
    if cls == "large":
        return DC._ro(O.synth_x(rng, (n, c, h, h)), O.synth_dy(rng, (n, c, oh, oh), zero_frac=0.3), w)
    x = rng.integers(-2, 3, (n, c, h, h)).astype(np.int8)
    dy = np.zeros((n, c, oh, oh), np.int8)
    if cls != "bw0":
        o = oh - 1
        i = 2 * o + (k - 1) // 2 - pad
        assert 0 <= i < h
        dy[n - 1, :, o, o] = 1 if cls == "bw1" else 2
        x[n - 1, :, i, i] = 2
    return DC._ro(x, dy, w)


# ------------------------------------------------------------------------------------ chain nets
# (c_out, k, pad, relu, pool, flatten, depthwise, stride)
# M: MobileNet-shaped
NET_M = (3, 16, [(16, 3, 1, 1, 0, 0, 0, 2), (0, 3, 1, 0, 0, 0, 1, 1), (32, 1, 0, 1, 0, 0, 0, 1),
                 (0, 3, 1, 0, 0, 0, 1, 2), (64, 1, 0, 1, 0, 0, 0, 1), (0, 3, 1, 0, 0, 0, 1, 2),
                 (64, 1, 0, 1, 0, 1, 0, 1), (10, 1, 0, 0, 0, 0, 0, 1)])
# T: a strided layer between row-kernel layers (sub-pixel input gradient)
NET_T = (1, 8, [(32, 3, 1, 1, 0, 0, 0, 1), (64, 3, 1, 1, 0, 0, 0, 2), (64, 3, 1, 1, 1, 0, 0, 1),
                (64, 3, 1, 1, 0, 1, 0, 1), (7, 1, 0, 0, 0, 0, 0, 1)])
# U: odd maps, a first layer on the GEMM (36 > 32), a strided 1x1, a strided 5x5 depthwise down to 1x1
NET_U = (4, 9, [(24, 3, 0, 1, 0, 0, 0, 2), (40, 1, 0, 0, 0, 0, 0, 2), (0, 5, 2, 1, 0, 0, 1, 2), (20, 1, 0, 0, 0, 0, 0, 1)])
# UP: a strided layer that also pools (9 -> 4 -> 2), then a flatten
NET_UP = (4, 9, [(24, 3, 0, 1, 1, 1, 0, 2), (20, 1, 0, 0, 0, 0, 0, 1)])
NETS = {"NET_M": NET_M, "NET_T": NET_T, "NET_U": NET_U, "NET_UP": NET_UP}


def derive(net):
    """The layer dicts of a (in_c, in_hw, spec) net whose spec tuples may carry `depthwise` and `stride`."""
    c, h, spec = net
    out = []
    for l in spec:
        co, k, pad, relu, pool, flatten = l[:6]
        dw = l[6] if len(l) > 6 else 0
        s = l[7] if len(l) > 7 else 1
        co = c if dw else co
        out.append(dict(ci=c, co=co, k=k, pad=pad, h=h, relu=relu, pool=pool, flatten=flatten, dw=dw, stride=s))
        oh = out_hw(h, k, pad, s)
        ph = (oh - 2) // 2 + 1 if pool else oh
        c, h = (co * ph * ph, 1) if flatten else (co, ph)
    return out


weight_shape = DC.weight_shape
init_weights = DC.init_weights
batches = DC.batches


def layer_geom(n, l):
    return O.geom(n, l["ci"], l["h"], l["h"], l["co"], l["k"], stride=l.get("stride", 1), pad=l["pad"])


def macs(layers, n):
    return sum(n * out_hw(l["h"], l["k"], l["pad"], l["stride"]) ** 2 * l["co"] * (1 if l["dw"] else l["ci"]) * l["k"] ** 2
               for l in layers)


def chain_step_ref(layers, W, S, x, exp_in, labels, bits=None):
    """depthwise_cases.dw_chain_step_ref with each layer's stride in its geometry."""
    import niti_model_ref as R
    n = x.shape[0]
    rec = dict(inp=[], y=[], r=[], p=[], exp=[], dw=[], dy=[], geom=[], bw=[])
    a, exp = x, exp_in
    dense = [DC.dense_of(w) if l.get("dw") else w for l, w in zip(layers, W)]
    for i, l in enumerate(layers):
        g = layer_geom(n, l)
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
            acc = DC.diag_of(acc)
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


def ref_steps(layers, W, S, data, exp_in=-3, bits=None):
    """chain_step_ref over `data`: [(new weights, record, x, exponent)] per step."""
    out = []
    for x, labels in data:
        e = exp_in
        if x.dtype == np.uint8:
            x, e = O.quantize_images(x)
        W, rec = chain_step_ref(layers, W, S, x, e, labels, bits=bits)
        out.append((W, rec, x, e))
    return out
