"""Shared cases of the grouped conv tests (importable without a GPU).

A grouped layer (include/niti_hip.h, niti_gconv_*) is NITI_Conv_Int8 over the block-diagonal dense weight
dense_of(w, groups), except that its weight gradient's range is taken over the c_out cg 9 parameters only.
The references are therefore the existing oracle's over dense_of, and the diagonal blocks (blocks_of) of
O.conv_wgrad_acc.  Op shapes are (n, C, G, h, pad); net spec tuples are skip_cases' with `groups` as the
eleventh entry, which NitiModel.from_chain takes as they are.
"""
from __future__ import annotations

import functools

import numpy as np

import depthwise_cases as DC
import skip_cases as SK
from depthwise_cases import O, UB  # noqa: F401

OP_SHAPES = (
    (1, 32, 2, 1, 1),    # a 1x1 map: every tap but the centre is padding, cg 16
    (2, 64, 2, 5, 1),    # cg 32, an odd map, 5 K-steps with two zero slots
    (3, 128, 2, 7, 1),   # cg 64, odd batch, the weight fragments from LDS
    (2, 48, 3, 4, 0),    # three groups, the output smaller than the input
    (2, 32, 2, 3, 2),    # the output larger; the input gradient's pad is 0
    (1, 32, 2, 19, 1),   # a row of one whole and one partial 16-pixel strip
    (4, 64, 4, 16, 1),   # several workgroups per group, more than one weight-gradient slab
)
MULTI_SLAB = OP_SHAPES[-1]
SHIFT_CLASSES = DC.SHIFT_CLASSES


def geom_of(shape):
    n, c, _, h, pad = shape
    return O.geom(n, c, h, h, c, 3, pad=pad)


def dense_of(w, groups):
    """[c_out, cg, k, k] -> the block-diagonal [c_out, groups * cg, k, k]."""
    w = np.asarray(w)
    co, cg = w.shape[:2]
    d = np.zeros((co, groups * cg) + w.shape[2:], w.dtype)
    og = co // groups
    for g in range(groups):
        d[g * og:(g + 1) * og, g * cg:(g + 1) * cg] = w[g * og:(g + 1) * og]
    return d


def blocks_of(acc, groups):
    """[c_out, c_in, k, k] -> its diagonal blocks as [c_out, c_in / groups, k, k]."""
    co, ci = acc.shape[:2]
    og, cg = co // groups, ci // groups
    return np.ascontiguousarray(np.concatenate([acc[g * og:(g + 1) * og, g * cg:(g + 1) * cg] for g in range(groups)]))


def absmax(acc):
    return int(np.abs(acc.astype(np.int64)).max())


def act_ref(g, groups, a, w, dgrad=False, amax=None):
    """(q int8, inc, acc int32) of the forward of x = a, or of the input gradient of dy = a, ahead of the relu /
    relu_mask; amax: a larger range than acc's own (DC.requant_under)."""
    acc, st = (O.conv_dgrad_acc if dgrad else O.conv_fwd_acc)(g, a, dense_of(w, groups))
    assert st.overflow == 0
    return DC.requant_under(acc, amax) + (acc,)


def wgrad_ref(g, groups, x, dy):
    """acc int32 [c_out, cg, 3, 3]: the diagonal blocks of the dense weight gradient."""
    dense, st = O.conv_wgrad_acc(g, x, dy)
    assert st.overflow == 0
    return blocks_of(dense, groups)


@functools.lru_cache(maxsize=None)
def act_inputs(shape, cls, dgrad=False):
    """(a, w, mask) as depthwise_cases.act_inputs draws them: fixed uniform draws (so every group's inputs and
    weights differ) times the smallest amplitude that puts the accumulators' bit width in the shift class."""
    n, c, groups, h, pad = shape
    oh = h + 2 * pad - 2
    rng = np.random.default_rng(3000 + 7 * OP_SHAPES.index(shape) + (1 if dgrad else 0))
    ua = rng.uniform(-1, 1, (n, c, oh, oh) if dgrad else (n, c, h, h))
    uw = rng.uniform(-1, 1, (c, c // groups, 3, 3))
    mask = rng.integers(-3, 4, (n, c, h, h) if dgrad else (n, c, oh, oh)).astype(np.int8)
    for amp in range(1, 128):
        a, w = np.rint(ua * amp).astype(np.int8), np.rint(uw * amp).astype(np.int8)
        if DC._in_class(DC._bw(act_ref(geom_of(shape), groups, a, w, dgrad)[2]), cls):
            return DC._ro(a, w, mask)
    raise AssertionError(f"no amplitude puts {shape} in {cls}")


@functools.lru_cache(maxsize=None)
def wgrad_inputs(shape):
    n, c, groups, h, pad = shape
    oh = h + 2 * pad - 2
    rng = np.random.default_rng(4000 + 11 * OP_SHAPES.index(shape))
    w = rng.integers(-127, 128, (c, c // groups, 3, 3)).astype(np.int8)
    return DC._ro(O.synth_x(rng, (n, c, h, h)), O.synth_dy(rng, (n, c, oh, oh), zero_frac=0.3), w)


# ------------------------------------------------------------------------------------ chain nets
def _l(co, k, pad=0, relu=0, pool=0, flatten=0, skip=0, gpool=0, groups=1):
    return (co, k, pad, relu, pool, flatten, 0, 1, skip, gpool, groups)


# X: ResNeXt-style -- a 3x3 stem, a block (1x1, grouped 3x3 cg 16, 1x1 + skip), a pooled 3x3 layer, a second block
# at 64 channels with cg 32 (its source is the block's own 1x1 layer: the pooled layer in front cannot be one),
# the global pool, fc
NET_X = (3, 8, [_l(32, 3, 1, 1), _l(32, 1, 0, 1), _l(32, 3, 1, 1, groups=2), _l(32, 1, 0, 0, skip=3), _l(64, 3, 1, 1, pool=1),
                _l(64, 1, 0, 1), _l(64, 3, 1, 1, groups=2), _l(64, 1, 0, 1, skip=2, gpool=1), _l(10, 1)])
# R: a grouped layer between row-kernel layers, one with pool = 1 and a flatten behind it
NET_R = (1, 8, [_l(32, 3, 1, 1), _l(32, 3, 1, 1, groups=2), _l(64, 3, 1, 1), _l(64, 3, 1, 1, pool=1, flatten=1, groups=4),
                _l(7, 1)])
NETS = {"NET_X": NET_X, "NET_R": NET_R}
BATCH = 4


def derive(net):
    """skip_cases.derive's layer dicts with `groups`."""
    out = SK.derive((net[0], net[1], [l[:10] for l in net[2]]))
    for d, l in zip(out, net[2]):
        d["groups"] = l[10]
    return out


def weight_shape(l):
    return (l["co"], l["ci"] // l["groups"], l["k"], l["k"])


def init_weights(layers, seed):
    from niti_amd.init import xavier_int8
    rng = np.random.default_rng(seed)
    ws = [xavier_int8(weight_shape(l), rng) for l in layers]
    return [w for w, _ in ws], [s for _, s in ws]


def chain_step_ref(layers, W, S, x, exp_in, labels):
    """skip_cases.chain_step_ref over the block-diagonal weights: the forward, every gradient and the dense layers'
    updates are the step's.  A grouped layer's update is then made again from the diagonal blocks of its weight
    gradient alone, with their own range (update bits 2), on its [c_out, cg, 3, 3] weight."""
    dense = [dense_of(w, l["groups"]) for l, w in zip(layers, W)]
    newW, rec = SK.chain_step_ref(layers, dense, S, x, exp_in, labels)
    for i, l in enumerate(layers):
        if l["groups"] > 1:
            assert O.conv_dgrad_acc(rec["geom"][i], rec["dy"][i], dense[i])[1].overflow == 0  # (not asserted in there)
            newW[i], _ = UB.apply_update(W[i], wgrad_ref(rec["geom"][i], l["groups"], rec["inp"][i], rec["dy"][i]), 2)
    return newW, rec


@functools.lru_cache(maxsize=None)
def reference(name, steps=3, seed_w=3, seed_x=1):
    """(layers, W0, S, data, [(weights after the step, record)]) of a net, computed once and shared."""
    layers = derive(NETS[name])
    W, S = init_weights(layers, seed_w)
    data = DC.batches(layers, BATCH, steps, seed_x)
    out, cur = [], W
    for x, labels in data:
        cur, rec = chain_step_ref(layers, cur, S, x, -3, labels)
        out.append((cur, rec))
    return layers, W, S, data, out
