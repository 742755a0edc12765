"""Shared cases of the skip-connection, global-pool and deep-chain tests (importable without a GPU).

The chain reference is strided_cases.chain_step_ref extended with the two rules of niti_chain_layer3
(include/niti_hip.h), restated from the oracle's primitives -- RR.residual_add / RR.requant of
oracle/niti_resnet_ref.py and the gradient exponents as its train_step tracks them -- and not read from
the library:

  skip = d on layer i   y = the layer's requantised conv output (exponent e_y), u = the final output of
                        layer i - d (after its own add and relu, exponent e_u);
                        z, e_z = residual_add(y, e_y, u, e_u); q, e = requant(z, e_z); the layer's relu,
                        pool, flatten and gpool follow on q, and q is its relu mask.
                        Backward: dz, the gradient at q after the layer's relu mask, is the conv's output
                        gradient and, unchanged, the skip's.  At the source, layer s + 1's input gradient
                        is taken unmasked; residual_add(dgrad, e_dgrad, dz, e_dz), requant, then the
                        source's relu mask give the source's output gradient.
  gpool = 1             after the relu the map is summed per image and channel (int32, the exponent kept)
                        and requantised by the forward rule into a 1x1 map; its gradient hands the pooled
                        gradient to every pixel, then the relu mask.
  gradient exponents    the loss gradient has 0, an input gradient e_dy + wscale + inc; relu, pool,
                        flatten and gpool gradients keep theirs.

Spec tuples are (c_out, k, pad, relu, pool, flatten, depthwise, stride, skip, gpool), the tail optional.
"""
from __future__ import annotations

import numpy as np

import depthwise_cases as DC
import strided_cases as SC
from depthwise_cases import O, UB  # noqa: F401

import niti_resnet_ref as RR


def _l(co, k, pad=0, relu=0, pool=0, flatten=0, dw=0, stride=1, skip=0, gpool=0):
    return (co, k, pad, relu, pool, flatten, dw, stride, skip, gpool)


def _block(mid, out, skip, stride=1):
    """1x1 -> mid relu, depthwise 3x3 relu, 1x1 -> out linear (+ skip)"""
    return [_l(mid, 1, 0, 1), _l(0, 3, 1, 1, dw=1, stride=stride), _l(out, 1, 0, 0, skip=skip)]


# V: MobileNetV2-shaped.  The first block's source has a relu, the second block's source is the first
# block's adding layer; 24 channels (cp 32) cover pad lanes; a gpool before the head.
NET_V = (3, 16, [_l(16, 3, 1, 1, stride=2)] + _block(48, 16, 3) + _block(48, 16, 3) + _block(48, 24, 0, stride=2) +
         _block(72, 24, 3) + [_l(64, 1, 0, 1, gpool=1), _l(10, 1)])
# W: a pool-less-stem ResNet (depths (2,), width 16) as a chain
NET_W = (3, 8, [_l(16, 3, 1, 1), _l(16, 3, 1, 1), _l(16, 3, 1, 1, skip=2), _l(16, 3, 1, 1),
                _l(16, 3, 1, 1, skip=2, gpool=1), _l(10, 1)])
# X: odd maps, cp 48, d = 1 on a depthwise layer; an adding layer that pools after its add, between
# row-kernel shaped neighbours
NET_X = (1, 9, [_l(40, 3, 1, 1), _l(0, 3, 1, 1, dw=1, skip=1), _l(64, 3, 1, 1), _l(64, 3, 1, 1, pool=1, skip=1),
                _l(32, 3, 1, 1, flatten=1), _l(7, 1)])
# D: depth -- a stem, eight skip blocks of three narrow layers, a gpool layer, fc: 27 layers
NET_D = (3, 8, [_l(16, 3, 1, 1)] + sum((_block(32, 16, 3) for _ in range(8)), []) + [_l(32, 1, 0, 1, gpool=1), _l(10, 1)])
# G: the global pool alone (no skip): an odd 7x7 map of 24 channels (cp 32: pad lanes) summed after a relu,
# and before it a linear gpool-free layer; then two layers on the 1x1 map
NET_G = (3, 14, [_l(16, 3, 1, 1, stride=2), _l(24, 3, 1, 1, gpool=1), _l(40, 1, 0, 1), _l(10, 1)])
# P: a gpool without a relu on a depthwise layer, behind a pooled row-kernel shaped layer
NET_P = (1, 8, [_l(32, 3, 1, 1, pool=1), _l(0, 3, 1, 0, dw=1, gpool=1), _l(7, 1)])
# E: depth without a skip -- 27 layers, the eight blocks of NET_D without their sums
NET_E = (3, 8, [_l(16, 3, 1, 1)] + sum((_block(32, 16, 0) for _ in range(8)), []) + [_l(32, 1, 0, 1, gpool=1), _l(10, 1)])
NETS = {"NET_V": NET_V, "NET_W": NET_W, "NET_X": NET_X, "NET_D": NET_D, "NET_G": NET_G, "NET_P": NET_P, "NET_E": NET_E}
BATCH = {"NET_V": 4, "NET_W": 3, "NET_X": 3, "NET_D": 2, "NET_G": 3, "NET_P": 3, "NET_E": 2}
SKIP_NETS = ("NET_V", "NET_W", "NET_X", "NET_D")
SEED_W, SEED_X = 3, 1


def derive(net):
    """The layer dicts of a (in_c, in_hw, spec) net: strided_cases.derive's keys and skip, gpool."""
    c, h, spec = net
    out = []
    for l in spec:
        l = tuple(l) + (0,) * (10 - len(l))
        co, k, pad, relu, pool, flatten, dw = l[:7]
        s = l[7] or 1
        co = c if dw else co
        out.append(dict(ci=c, co=co, k=k, pad=pad, h=h, relu=relu, pool=pool, flatten=flatten, dw=dw, stride=s,
                        skip=l[8], gpool=l[9]))
        oh = SC.out_hw(h, k, pad, s)
        ph = (oh - 2) // 2 + 1 if pool else oh
        c, h = (co * ph * ph, 1) if flatten else (co, 1) if l[9] else (co, ph)
    return out


def shapes_of(layers):
    """What niti_model_chain_check4 reports: {c_in, c_out, k, pad, h_in, oh, out_h, flat_c} per layer."""
    out = []
    for l in layers:
        oh = SC.out_hw(l["h"], l["k"], l["pad"], l["stride"])
        ph = (oh - 2) // 2 + 1 if l["pool"] else oh
        one = l["flatten"] or l["gpool"]
        out.append([l["ci"], l["co"], l["k"], l["pad"], l["h"], oh, 1 if one else ph,
                    l["co"] * ph * ph if l["flatten"] else l["co"]])
    return out


weight_shape = DC.weight_shape
init_weights = DC.init_weights
batches = DC.batches
layer_geom = SC.layer_geom


def chain_step_ref(layers, W, S, x, exp_in, labels, bits=None):
    """strided_cases.chain_step_ref with skip and gpool.  The record's y is the relu mask (q of an adding
    layer), r the forward tap, exp the layer's exponent (before a gpool's requantisation), edy each output
    gradient's exponent, sums [(direction, layer, e_a, e_b, max|z|)] of every residual sum."""
    import niti_model_ref as R
    n = x.shape[0]
    nl = len(layers)
    rec = dict(inp=[], y=[], r=[], p=[], exp=[], dw=[], dy=[], geom=[], bw=[], sums=[], gp=[None] * nl)
    a, exp = x, exp_in
    dense = [DC.dense_of(w) if l.get("dw") else w for l, w in zip(layers, W)]
    src_of = {i - l["skip"]: i for i, l in enumerate(layers) if l["skip"]}
    for i, l in enumerate(layers):
        g = layer_geom(n, l)
        rec["geom"].append(g)
        rec["inp"].append(a)
        y, exp, _, st = O.conv_fwd(g, a, dense[i], exp, S[i])
        assert st.overflow == 0
        if l["skip"]:
            s = i - l["skip"]
            u, eu = rec["r"][s], rec["exp"][s]
            z, ez = RR.residual_add(y, exp, u, eu)
            rec["sums"].append(("fwd", i, exp, eu, int(np.abs(z.astype(np.int64)).max())))
            y, exp = RR.requant(z, ez)
        r = O.relu(y) if l["relu"] else y
        p = O.maxpool(r) if l["pool"] else None
        rec["y"].append(y)
        rec["r"].append(r)
        rec["p"].append(p)
        rec["exp"].append(exp)
        a = r if p is None else p
        if l["flatten"]:
            a = a.reshape(n, -1, 1, 1)
        if l["gpool"]:
            gsum = r.astype(np.int32).sum(axis=(2, 3)).astype(np.int32)
            g8, exp = RR.requant(gsum, exp)
            rec["gp"][i] = (g8, exp)
            a = g8.reshape(n, -1, 1, 1)
    last = layers[-1]
    logits = rec["r"][-1].reshape(n, last["co"])
    d = O.loss_grad(logits, rec["exp"][-1], R.onehot(labels, last["co"])).reshape(n, last["co"], 1, 1)
    dy = [None] * nl
    edy = [None] * nl
    dy[-1], edy[-1] = d, 0
    newW = list(W)
    for i in range(nl - 1, -1, -1):
        g = rec["geom"][i]
        acc, st = O.conv_wgrad_acc(g, rec["inp"][i], dy[i])
        assert st.overflow == 0
        if layers[i].get("dw"):
            acc = DC.diag_of(acc)
        rec["bw"].insert(0, O.range_estimate(acc))
        if i > 0:
            dx, inc, _, _ = O.conv_dgrad(g, dy[i], dense[i])
            e = RR._e8(edy[i] + S[i] + inc)
            pl = layers[i - 1]
            if pl["flatten"]:
                dx = dx.reshape((rec["p"] if pl["pool"] else rec["r"])[i - 1].shape)
            if pl["gpool"]:
                dx = np.broadcast_to(dx.reshape(n, -1, 1, 1), rec["r"][i - 1].shape).astype(np.int8).copy()
            if pl["pool"]:
                dx = O.maxpool_grad(rec["r"][i - 1], rec["p"][i - 1], dx)
            if i - 1 in src_of:  # (a source neither pools, flattens nor gpools: dx is the unmasked input gradient)
                j = src_of[i - 1]
                z, ez = RR.residual_add(dx, e, dy[j], edy[j])
                rec["sums"].append(("bwd", i - 1, e, edy[j], int(np.abs(z.astype(np.int64)).max())))
                dx, e = RR.requant(z, ez)
            if pl["relu"]:
                dx = O.relu_grad(rec["y"][i - 1], dx)
            dy[i - 1], edy[i - 1] = dx, e
        newW[i], g8 = UB.apply_update(W[i], acc, 2 if bits is None else bits[i])
        rec["dw"].insert(0, g8)
    rec["dy"] = dy
    rec["edy"] = edy
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
