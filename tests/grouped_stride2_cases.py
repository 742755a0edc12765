"""Shared cases of the stride-2 grouped conv tests (importable without a GPU): grouped_cases' references over
O.geom(..., stride=2, pad=pad).  Op shapes are (n, C, G, h, pad), each the smallest that hits its hazard."""
from __future__ import annotations

import functools

import numpy as np

import grouped_cases as GC
from grouped_cases import DC, O

OP_SHAPES = (
    (1, 32, 2, 2, 1),    # a 1x1 output; dx classes with every tap but one outside
    (2, 64, 2, 5, 1),    # cg 32, odd map, 3x3 output
    (3, 128, 2, 8, 1),   # cg 64, even map, 4x4 output; the last dx row / column is read by one tap only
    (2, 48, 3, 6, 0),    # pad 0, three groups; h - 3 odd: the last dx row and column are all zeros
    (2, 32, 2, 7, 2),    # pad 2, 4x4 output; the parity planes swapped against pad 1
    (1, 32, 2, 35, 1),   # 18 output columns: one whole and one partial strip; 5 row bands
    (4, 64, 4, 32, 1),   # several workgroups per group, more than one weight-gradient slab
)
MULTI_SLAB = OP_SHAPES[-1]


def geom_of(shape, stride=2):
    n, c, _, h, pad = shape
    return O.geom(n, c, h, h, c, 3, stride=stride, pad=pad)


@functools.lru_cache(maxsize=None)
def act_inputs(shape, cls, dgrad=False):
    """grouped_cases.act_inputs' draws and amplitude search over the strided geometry."""
    n, c, groups, h, pad = shape
    g = geom_of(shape)
    rng = np.random.default_rng(5000 + 7 * OP_SHAPES.index(shape) + (1 if dgrad else 0))
    ua = rng.uniform(-1, 1, (n, c, g.oh, g.ow) if dgrad else (n, c, h, h))
    uw = rng.uniform(-1, 1, (c, c // groups, 3, 3))
    mask = rng.integers(-3, 4, (n, c, h, h) if dgrad else (n, c, g.oh, g.ow)).astype(np.int8)
    for amp in range(1, 128):
        a, w = np.rint(ua * amp).astype(np.int8), np.rint(uw * amp).astype(np.int8)
        if DC._in_class(DC._bw(GC.act_ref(g, groups, a, w, dgrad)[2]), cls):
            return DC._ro(a, w, mask)
    raise AssertionError(f"no amplitude puts {shape} in {cls}")


@functools.lru_cache(maxsize=None)
def wgrad_inputs(shape):
    n, c, groups, h, pad = shape
    g = geom_of(shape)
    rng = np.random.default_rng(6000 + 11 * OP_SHAPES.index(shape))
    w = rng.integers(-127, 128, (c, c // groups, 3, 3)).astype(np.int8)
    return DC._ro(O.synth_x(rng, (n, c, h, h)), O.synth_dy(rng, (n, c, g.oh, g.ow), zero_frac=0.3), w)


# ------------------------------------------------------------------------------------ the chain net
def _l(co, k, pad=0, relu=0, stride=1, gpool=0, groups=1):
    return (co, k, pad, relu, 0, 0, 0, stride, 0, gpool, groups)


# 3 x 16 px: a stem, 1x1, grouped 3x3 / 2 (cg 16), 1x1 to 64, a 3x3 row-kernel layer behind the strided one,
# grouped 3x3 / 2 (cg 32) with the global pool, fc
NET_S = (3, 16, [_l(32, 3, 1, 1), _l(32, 1, 0, 1), _l(32, 3, 1, 1, stride=2, groups=2), _l(64, 1, 0, 1), _l(64, 3, 1, 1),
                 _l(64, 3, 1, 1, stride=2, gpool=1, groups=2), _l(10, 1)])
BATCH = 4


@functools.lru_cache(maxsize=None)
def reference(steps=3):
    """(layers, W0, S, data, [(weights after the step, record)]) of NET_S, computed once and shared."""
    layers = GC.derive(NET_S)
    W, S = GC.init_weights(layers, 3)
    data = DC.batches(layers, BATCH, steps, 1)
    out, cur = [], W
    for x, labels in data:
        cur, rec = GC.chain_step_ref(layers, cur, S, x, -3, labels)
        out.append((cur, rec))
    return layers, W, S, data, out
