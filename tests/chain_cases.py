"""Shared cases of the user-defined chain network tests (importable without a GPU).

Specs are lists of (c_out, kernel, pad, relu, pool, flatten); each named net is the smallest that
reaches a path of the chain driver no built-in network runs ("User-defined chains").

chain_step_ref is the oracle's NITI_SGD step (oracle/niti_model_ref.py train_step, "naive")
restated from the same niti_oracle primitives for lists that loop cannot run: it reshapes a
flatten's gradient to the pooled output's shape and so needs a pool on every flattening layer.
Here the flatten's gradient takes the shape of whatever was flattened -- the pooled map, or the
conv (+relu) output itself.  test_chain_cpu.py pins it to train_step on every list both can run.
"""
import numpy as np

import niti_oracle as O

LENET = (1, 28, [(20, 5, 0, 1, 1, 0), (52, 5, 0, 1, 1, 1), (500, 1, 0, 1, 0, 0), (12, 1, 0, 0, 0, 0)])
VGG11 = (3, 32, [(64, 3, 1, 1, 1, 0), (128, 3, 1, 1, 1, 0), (256, 3, 1, 1, 0, 0), (256, 3, 1, 1, 1, 0),
                 (512, 3, 1, 1, 0, 0), (512, 3, 1, 1, 1, 0), (512, 3, 1, 1, 0, 0), (512, 3, 1, 1, 1, 0),
                 (12, 1, 0, 0, 0, 0)])
_V16 = [(64, 0), (64, 1), (128, 0), (128, 1), (256, 0), (256, 0), (256, 1), (512, 0), (512, 0), (512, 1), (512, 0),
        (512, 0), (512, 1)]
VGG16_32 = (3, 32, [(c, 3, 1, 1, p, int(i == 12)) for i, (c, p) in enumerate(_V16)] +
            [(4096, 1, 0, 1, 0, 0), (4096, 1, 0, 1, 0, 0), (1000, 1, 0, 0, 0, 0)])

# A: non-im2col first layer (4 * 3 * 3 = 36 > 32), a 2x2 pool on an odd map (9 -> 4), 20 classes
NET_A = (4, 9, [(24, 3, 1, 1, 1, 0), (40, 3, 0, 1, 1, 1), (36, 1, 0, 1, 0, 0), (20, 1, 0, 0, 0, 0)])
# B: an im2col first layer the fused input pass refuses (1 * 3 * 3), row kernels, a 7-class head
# behind a pooled 1x1 map
NET_B = (1, 8, [(32, 3, 1, 1, 0, 0), (64, 3, 1, 1, 1, 0), (64, 3, 1, 1, 1, 0), (32, 3, 1, 1, 1, 0), (7, 1, 0, 0, 0, 0)])
# C: 5x5 / pad 2, 100 classes behind a 288-wide flatten
NET_C = (3, 12, [(16, 5, 2, 1, 1, 0), (32, 3, 1, 1, 1, 1), (100, 1, 0, 0, 0, 0)])
# D: flatten without a pool (on the GEMM path; D2: on a layer the row kernel takes)
NET_D = (3, 4, [(8, 3, 1, 1, 0, 1), (10, 1, 0, 0, 0, 0)])
NET_D2 = (3, 4, [(32, 3, 1, 1, 0, 0), (32, 3, 1, 1, 0, 1), (10, 1, 0, 0, 0, 0)])
# F: pads past (kernel - 1) / 2 -- a 3 x 3 x 3 first layer with pad 2 (the fused input pass stages too few
# columns for it: the unfused quantiser + im2col32) and a 5x5 / pad 3 layer on the implicit GEMM
NET_F = (3, 6, [(16, 3, 2, 1, 1, 0), (24, 5, 3, 1, 1, 1), (10, 1, 0, 0, 0, 0)])
# G: 7x7 / pad 3, the largest kernel taken: 49 taps (past the tap-mask loader's 32), first layer and deeper
NET_G = (2, 9, [(8, 7, 3, 1, 1, 0), (12, 7, 3, 1, 1, 1), (10, 1, 0, 0, 0, 0)])
# a further pooled-flatten net (the chain_step_ref pin only)
NET_E = (4, 9, [(24, 3, 1, 1, 1, 0), (40, 3, 0, 1, 1, 1), (36, 1, 0, 1, 0, 0), (20, 1, 0, 0, 0, 0)])


def derive(net):
    """The oracle's layer dicts of a (in_c, in_hw, spec) net, derived here (no library call)."""
    c, h, spec = net
    out = []
    for co, k, pad, relu, pool, flatten in spec:
        out.append(dict(ci=c, co=co, k=k, pad=pad, h=h, relu=relu, pool=pool, flatten=flatten))
        oh = h + 2 * pad - k + 1
        ph = (oh - 2) // 2 + 1 if pool else oh
        c, h = (co * ph * ph, 1) if flatten else (co, ph)
    return out


def chain_step_ref(layers, W, S, x, exp_in, labels):
    """(new weights, record) of one NITI_SGD step; the record has train_step's fields."""
    import niti_model_ref as R
    n = x.shape[0]
    rec = dict(inp=[], y=[], r=[], p=[], exp=[], dw=[], dy=[], geom=[])
    a, exp = x, exp_in
    for i, l in enumerate(layers):
        g = O.geom(n, l["ci"], l["h"], l["h"], l["co"], l["k"], pad=l["pad"])
        rec["geom"].append(g)
        rec["inp"].append(a)
        y, exp, _, st = O.conv_fwd(g, a, W[i], exp, S[i])
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
        dw, _, _, _ = O.conv_wgrad(g, rec["inp"][i], dy[i])
        rec["dw"].insert(0, dw)
        if i > 0:
            dx, _, _, _ = O.conv_dgrad(g, dy[i], W[i])
            pl = layers[i - 1]
            if pl["flatten"]:  # the shape of what was flattened
                dx = dx.reshape((rec["p"] if pl["pool"] else rec["r"])[i - 1].shape)
            if pl["pool"]:
                dx = O.maxpool_grad(rec["r"][i - 1], rec["p"][i - 1], dx)
            if pl["relu"]:
                dx = O.relu_grad(rec["y"][i - 1], dx)
            dy[i - 1] = dx
        newW[i] = O.sgd_update(W[i], dw)
    rec["dy"] = dy
    rec["logits"] = logits
    return newW, rec


def batches(layers, batch, steps, seed, images=False):
    """[(x or images, labels)] of `steps` batches for a derived layer list."""
    rng = np.random.default_rng(seed)
    l0, classes = layers[0], layers[-1]["co"]
    out = []
    for _ in range(steps):
        shape = (batch, l0["ci"], l0["h"], l0["h"])
        x = rng.integers(0, 256, shape).astype(np.uint8) if images else rng.integers(-127, 128, shape).astype(np.int8)
        out.append((x, rng.integers(0, classes, batch).astype(np.int32)))
    return out


def ref_steps(layers, W, S, data, exp_in=-3, step_fn=None):
    """The oracle over `data` (int8 x with exp_in, or uint8 images through the oracle's input
    quantiser): [(new weights, record, x, exponent)] per step."""
    import niti_model_ref as R
    out = []
    for x, labels in data:
        e = exp_in
        if x.dtype == np.uint8:
            x, e = O.quantize_images(x)
        if step_fn is None:
            W, rec = R.train_step(layers, W, S, x, e, labels, classes=layers[-1]["co"])
        else:
            W, rec = step_fn(layers, W, S, x, e, labels)
        out.append((W, rec, x, e))
    return out
