"""Inputs and CPU references of tests/test_gpu_first_layer.py (importable without a GPU).

Every reference is the CPU oracle (oracle/niti_oracle.py) or plain numpy index arithmetic; none is
a GPU kernel.  Each is built once per case (lru_cache) and handed out read-only.
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

BATCH = 3


def _ro(*arrays):
    for a in arrays:
        a.flags.writeable = False
    return arrays


def xcol_of(x, k, pad):
    """The K = 32 im2col copy [n * oh * ow][32] of int8 NCHW x: byte (ky k + kx) C + c of a pixel's
    row is x[c] at tap (ky, kx), zero outside the image and past C k k."""
    n, c, h, w = x.shape
    oh, ow = h + 2 * pad - k + 1, w + 2 * pad - k + 1
    xp = np.zeros((n, c, h + 2 * pad, w + 2 * pad), np.int8)
    xp[:, :, pad:pad + h, pad:pad + w] = x
    out = np.zeros((n, oh, ow, 32), np.int8)
    for ky in range(k):
        for kx in range(k):
            for ch in range(c):
                out[..., (ky * k + kx) * c + ch] = xp[:, ch, ky:ky + oh, kx:kx + ow]
    return out.reshape(n * oh * ow, 32)


def wcol_of(w, rows):
    """OIHW weights as the im2col conv's [rows][32] (xcol_of's byte order; rows >= co, the rest 0)."""
    co, c, k, _ = w.shape
    out = np.zeros((rows, 32), np.int8)
    out[:co, :c * k * k] = w.transpose(0, 2, 3, 1).reshape(co, -1)
    return out


def r32(x):
    return (x + 31) // 32 * 32


# ------------------------------------------------------------------------------------ conv0
CONV0_COUT = (20, 64, 96)  # one tile with co < cop; two tiles; three (the general kernel)
CONV0_CLASSES = ("raw", "one", "psto")
CONV0_EXP = (-3, -6)  # exp_in, and the weight scale of the pinned classes


@functools.lru_cache(maxsize=None)
def conv0_inputs(c_out, cls):
    """(x int8 [3][3][32][32], w OIHW, wscale).  raw: one +-1 tap per output channel, so max|acc|
    <= 128 (x holds a -128 under a -1 weight: acc = 128 wraps to -128 in the raw cast); one: two
    +-1 taps, max|acc| in 129..256; psto: Xavier weights."""
    rng = np.random.default_rng([c_out, CONV0_CLASSES.index(cls)])
    x = rng.integers(-127, 128, (BATCH, 3, 32, 32)).astype(np.int8)
    if cls == "psto":
        w, ws = O.synth_w(rng, (c_out, 3, 3, 3))
        return _ro(x, w) + (ws,)
    w = np.zeros((c_out, 27), np.int8)
    for o in range(c_out):
        taps = rng.choice(27, 1 if cls == "raw" else 2, replace=False)
        w[o, taps] = rng.choice([-1, 1], taps.size)
    w = w.reshape(c_out, 3, 3, 3)
    if cls == "raw":
        w[0] = 0
        w[0, 1, 1, 1] = -1
        x[0, 1, 5, 7] = -128
    else:
        x[1, :, 8:11, 8:11] = 127  # a patch where both taps of any channel meet 127
    return _ro(x, w) + (CONV0_EXP[1],)


def pool_code_of(r, p, relu):
    """pool_code4's byte per pooled element: bit t for the first window element (0,0), (0,1),
    (1,0), (1,1) that is >= the pooled value; 0 under relu where the pooled value is <= 0."""
    t = [r[:, :, dy::2, dx::2].astype(np.int32) for dy in (0, 1) for dx in (0, 1)]
    m = p.astype(np.int32)
    code = np.zeros(p.shape, np.int8)
    done = np.zeros(p.shape, bool)
    for k in range(4):
        take = (t[k] >= m) & ~done
        code[take] = 1 << k
        done |= take
    assert done.all()
    if relu:
        code[m <= 0] = 0
    return code


@functools.lru_cache(maxsize=None)
def conv0_reference(c_out, cls, relu):
    """dict(range, shift, exp, out NCHW, pool NCHW, code NCHW) of the oracle's conv (+ relu, 2x2 pool)."""
    x, w, ws = conv0_inputs(c_out, cls)
    g = O.geom(BATCH, 3, 32, 32, c_out, 3, pad=1)
    y, e, acc, st = O.conv_fwd(g, x, w, CONV0_EXP[0], ws)
    assert st.overflow == 0
    r = O.relu(y) if relu else y
    p = O.maxpool(r)
    ref = dict(range=int(np.abs(acc.astype(np.int64)).max()), shift=O.range_estimate(acc) - 7, exp=e, out=r, pool=p,
               code=pool_code_of(r, p, relu))
    _ro(*(v for v in ref.values() if isinstance(v, np.ndarray)))
    return ref


def nhwc_of(a, cop):
    """NCHW -> [n * h * w][cop], pad channels 0."""
    n, c, h, w = a.shape
    out = np.zeros((n, h, w, cop), np.int8)
    out[..., :c] = a.transpose(0, 2, 3, 1)
    return out.reshape(n * h * w, cop)


def c32_of(a, cop):
    """NCHW -> the row kernels' C32 [n][cop / 32][h][w][32], pad channels 0."""
    n, c, h, w = a.shape
    t = np.zeros((n, cop, h, w), np.int8)
    t[:, :c] = a
    return np.ascontiguousarray(t.reshape(n, cop // 32, 32, h, w).transpose(0, 1, 3, 4, 2))


# ------------------------------------------------------------------------------------ input_im2col
# (channels, image size, kernel, pad, the first conv's channel count)
IM2COL_SHAPES = [
    (3, 32, 3, 1, 64),   # the step's: 16-byte aligned rows, two bands per image
    (1, 28, 5, 0, 20),   # 28-byte rows (images 16-byte aligned)
    (3, 17, 3, 1, 40),   # 17-byte rows of 289-byte planes: aligned to nothing
]


@functools.lru_cache(maxsize=None)
def im2col_reference(c, hw, k, pad, co, quant):
    """dict(inp uint8 images or int8 x, x int8, ascale, xcol, w OIHW, range): the oracle's quantiser
    (quant) or the int8 pixels as they are, xcol_of's copy, max|oracle conv| of Xavier weights."""
    rng = np.random.default_rng([c, hw, k, co, int(quant)])
    if quant:
        inp = rng.integers(0, 256, (BATCH, c, hw, hw)).astype(np.uint8)
        x, a = O.quantize_images(inp)
    else:
        inp = rng.integers(-128, 128, (BATCH, c, hw, hw)).astype(np.int8)
        x, a = inp, None
    w, _ = O.synth_w(rng, (co, c, k, k))
    g = O.geom(BATCH, c, hw, hw, co, k, pad=pad)
    acc, st = O.conv_fwd_acc(g, x, w)
    ref = dict(inp=inp, x=x, ascale=a, xcol=xcol_of(x, k, pad), w=w, range=int(np.abs(acc.astype(np.int64)).max()))
    _ro(*(v for v in ref.values() if isinstance(v, np.ndarray)))
    return ref


# ------------------------------------------------------------------------------------ whole step
# a 20-channel first layer (one tile, co < cop) on the fused input pass and conv0, pooled into a
# row-kernel layer
FIRST_NET = (3, 32, [(20, 3, 1, 1, 1, 0), (32, 3, 1, 1, 1, 1), (10, 1, 0, 0, 0, 0)])
