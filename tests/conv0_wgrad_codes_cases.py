"""Inputs and CPU references of tests/test_gpu_conv0_wgrad_codes.py (importable without a GPU).

Every expected value is the CPU oracle's (oracle/niti_oracle.py, oracle/niti_model_ref.py) or plain
numpy index arithmetic; none is a GPU kernel.  The weight gradient of the first layer is the oracle's
own chain: conv_fwd_acc -> requant_fwd -> relu -> maxpool forward, maxpool_grad and relu_grad of a
random pooled gradient, conv_wgrad_acc over the expanded gradient.  Each reference is built once per
case (lru_cache) and handed out read-only.

The VGG-11 model references take the oracle 9 s (batch 4) and over a minute (batch 36), so their two
steps are recorded in tests/golden/conv0_wgrad_codes_vgg11_b{4,36}.npz (logits, exponents and a sha256
of every layer's updated weights per step); `python tests/conv0_wgrad_codes_cases.py --write-golden`
rebuilds the files from the oracle, and tests/test_conv0_wgrad_codes_cpu.py holds the batch-4 file's
first step against the oracle.
"""
from __future__ import annotations

import functools
import hashlib
import os
import sys

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(_ROOT, "oracle"), os.path.join(_ROOT, "mandheling-dsp-training_amd"),
           os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import first_layer_cases as F  # noqa: E402
import niti_oracle as O  # noqa: E402

# ------------------------------------------------------------------------------------ op level
BATCHES = (1, 3, 5, 16)
# (channels, image size, kernel, pad): 3x3 pad 1 at 4x4 (4 pooled pixels an image: every batch a partial
# step), 8x8, 32x32 (4 steps an image; the only one conv0_fwd records codes for) and LeNet's 5x5 at
# 12x12 (an 8x8 output, 25 of the 32 columns)
GEOMS = ((3, 4, 3, 1), (3, 8, 3, 1), (3, 32, 3, 1), (1, 12, 5, 0))
PAIRS = ((64, 64), (33, 64), (20, 32))  # (c_out, cop)
BLOCKS = (0, 1, 3)
KINDS = ("random", "zero_grad", "dead_relu", "route0", "route1", "route2", "route3", "tie", "extreme")


def _ro(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.flags.writeable = False
    return d


def dw_cols(dw, rows=None):
    """The oracle's weight gradient [co][ci][kh][kw] as the im2col conv's [co][32] (xcol_of's order)."""
    co, c, k, _ = dw.shape
    out = np.zeros((co if rows is None else rows, 32), dw.dtype)
    out[:co, :c * k * k] = dw.transpose(0, 2, 3, 1).reshape(co, -1)
    return out


def formula(g0, code, xcol, n, oh, ow):
    """The issue's sum, straight from the three operands (numpy, int64): g0 / code [n*ph*pw][cop],
    xcol [n*oh*ow][32] -> [cop][32]."""
    ph, pw = oh // 2, ow // 2
    cop = g0.shape[1]
    g = g0.reshape(n, ph, pw, cop).astype(np.int64)
    c = code.reshape(n, ph, pw, cop).astype(np.int64)
    x = xcol.reshape(n, oh, ow, 32).astype(np.int64)
    out = np.zeros((cop, 32), np.int64)
    for t in range(4):
        m = g * ((c >> t) & 1)
        out += np.einsum("nyxc,nyxk->ck", m, x[:, t >> 1::2, t & 1::2])
    return out


@functools.lru_cache(maxsize=None)
def op_case(batch, geom, pair, kind="random"):
    """dict(x, w, ws, xcol, g0 [n*ph*pw][cop], code (the oracle's route, pad channels 0), dy (expanded,
    NCHW), ref int32 [co][32], oh, ow) for one op-level case."""
    c, hw, k, pad = geom
    co, cop = pair
    rng = np.random.default_rng([batch, c, hw, k, co, KINDS.index(kind)])
    g = O.geom(batch, c, hw, hw, co, k, pad=pad)
    oh, ow = g.oh, g.ow
    x = rng.integers(-127, 128, (batch, c, hw, hw)).astype(np.int8)
    w, ws = O.synth_w(rng, (co, c, k, k))
    g0 = O.synth_dy(rng, (batch, co, oh // 2, ow // 2), zero_frac=0.3)
    if kind == "zero_grad":
        g0 = np.zeros_like(g0)
    elif kind == "dead_relu":  # x >= 0 under w <= 0: every output <= 0, every pooled value 0 after relu
        x = np.abs(x)
        w = (-np.abs(w.astype(np.int16))).astype(np.int8)
    elif kind.startswith("route") or kind == "tie":
        # the centre tap of channel 0 alone, weight 1: the conv is x[:, 0] itself (max 100 < 128: the raw
        # cast), so the window's maximum sits where x's does -- element t, or all four equal (tie: the
        # first element takes the route, NITI_CPUPoolGrad_Int8)
        assert pad == (k - 1) // 2 or hw - k + 1 == oh
        w = np.zeros((co, c, k, k), np.int8)
        w[:, 0, k // 2, k // 2] = 1
        x = np.full((batch, c, hw, hw), 10, np.int8)
        if kind != "tie":
            t = int(kind[-1])
            off = 0 if pad else k // 2  # the output pixel (0, 0) reads x at (off, off)
            x[:, 0, off + (t >> 1)::2, off + (t & 1)::2] = 100
    elif kind == "extreme":
        x = rng.choice(np.array([-127, 127], np.int8), (batch, c, hw, hw))
        g0 = rng.choice(np.array([-127, 127], np.int8), g0.shape)
    acc, st = O.conv_fwd_acc(g, x, w)
    assert st.overflow == 0
    y, _ = O.requant_fwd(acc)
    r = O.relu(y)
    p = O.maxpool(r)
    dy = O.relu_grad(y, O.maxpool_grad(r, p, g0))
    dw, st = O.conv_wgrad_acc(g, x, dy)
    code = F.pool_code_of(r, p, True)
    return _ro(dict(x=x, w=w, ws=ws, xcol=F.xcol_of(x, k, pad), g0=F.nhwc_of(g0, cop), code=F.nhwc_of(code, cop),
                    code_nchw=code, dy=dy, ref=dw_cols(dw).astype(np.int32), oh=oh, ow=ow, k=c * k * k))


# ------------------------------------------------------------------------------------ model level
STEPS = 2
GOLDEN_BATCHES = (4, 36)


def golden_path(batch):
    return os.path.join(_ROOT, "tests", "golden", f"conv0_wgrad_codes_vgg11_b{batch}.npz")


# conv 3 -> 32 at 8x8, pool, conv 32 -> 32, pool (flattened: 2 x 2 x 32), head.  The first layer's
# forward records no codes at this width (conv0_fwd takes rows of 32 pixels), so the route does not apply.
CHAIN_8 = (3, 8, [(32, 3, 1, 1, 1, 0), (32, 3, 1, 1, 1, 1), (10, 1, 0, 0, 0, 0)])
# the same at 32x32 with 20 first-layer channels (cop 32): the route applies (first_layer_cases.FIRST_NET)
CHAIN_32 = F.FIRST_NET


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def vgg11_data(batch):
    rng = np.random.default_rng([batch, 1311])
    return [(rng.integers(-127, 128, (batch, 3, 32, 32)).astype(np.int8), rng.integers(0, 10, batch).astype(np.int32))
            for _ in range(STEPS)]


def vgg11_oracle(batch, steps=STEPS):
    import niti_model_ref as R
    layers = R.vgg11_layers()
    W, S = R.init_weights(layers, seed=13)
    out = []
    for x, labels in vgg11_data(batch)[:steps]:
        W, rec = R.train_step(layers, W, S, x, -3, labels)
        out.append(dict(logits=np.array(rec["logits"]), exp=int(rec["exp"][-1]), w=[sha(w) for w in W]))
    return out


@functools.lru_cache(maxsize=None)
def vgg11_ref(batch):
    """[dict(logits, exp, w: sha256 per layer)] per step: the oracle's, as recorded."""
    if batch in GOLDEN_BATCHES:
        z = np.load(golden_path(batch))
        return [dict(logits=z[f"logits{s}"], exp=int(z[f"exp{s}"]), w=[str(h) for h in z[f"w{s}"]]) for s in range(STEPS)]
    return vgg11_oracle(batch)


def vgg11_weights():
    import niti_model_ref as R
    return R.init_weights(R.vgg11_layers(), seed=13)


if __name__ == "__main__":
    if "--write-golden" in sys.argv:
        for b in GOLDEN_BATCHES:
            ref = vgg11_oracle(b)
            np.savez(golden_path(b), **{f"logits{s}": r["logits"] for s, r in enumerate(ref)},
                     **{f"exp{s}": np.int32(r["exp"]) for s, r in enumerate(ref)},
                     **{f"w{s}": np.array(r["w"]) for s, r in enumerate(ref)})
            print("wrote", golden_path(b))
