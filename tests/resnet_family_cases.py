"""Shared cases of the user-defined residual network tests (importable without a GPU).

family_convs builds the oracle's conv list (oracle/niti_resnet_ref.py's dict keys and names) of a
stage list by the header's rule, restated here and not read from the library.

family_step_ref is RR.train_step restated from the same oracle primitives with the stem's max pool
optional: without it block 0 reads u = relu(y0), and conv1's output gradient is d0 =
relu_grad(y0, du).  test_resnet_family_cpu.py pins it to RR.train_step on every pooled-stem case
before the GPU tests trust it for the pool-less stem.

Every case draws its weights from RR.init_weights(seed=3), its inputs and labels from
default_rng(1), int8 inputs with exponent -2 (the uint8 case: through the oracle's quantiser).  On
the CPU each runs two steps with the oracle's overflow counter at 0, non-zero logits and no
all-zero weight gradient in the second step (checked in test_resnet_family_cpu.py).
"""
import functools

import numpy as np

import niti_oracle as O
import niti_resnet_ref as RR
from niti_model_ref import onehot

SEED_W, SEED_X, EXP_IN = 3, 1, -2
STEMS = {"imagenet": (7, 2, 3, 1), "cifar": (3, 1, 1, 0)}

# name: (spec, in_hw, batch, uint8 images); the first four are the issue's pooled-stem lists
CASES = {
    "resnet34": (dict(depths=(3, 4, 6, 3), width=64, classes=10), 32, 2, False),
    "two_stage_w32": (dict(depths=(1, 3), width=32, classes=20), 32, 3, False),
    "odd_maps_w16": (dict(depths=(2, 1, 1), width=16, classes=7), 48, 2, False),
    "one_stage_w48": (dict(depths=(1,), width=48, classes=10), 32, 2, False),
    "cifar_resnet20": (dict(depths=(3, 3, 3), width=16, classes=10, stem="cifar"), 32, 2, False),
    "cifar_gray_images": (dict(depths=(1, 1), width=32, classes=10, stem="cifar", in_c=1), 28, 2, True),
}
POOLED = [k for k, v in CASES.items() if v[0].get("stem", "imagenet") == "imagenet"]
N_LAYERS = {"resnet34": 37, "two_stage_w32": 11, "odd_maps_w16": 12, "one_stage_w48": 4, "cifar_resnet20": 22,
            "cifar_gray_images": 7}
RESNET18 = dict(depths=(2, 2, 2, 2), width=64, classes=10)


def stem_of(spec):
    s = spec.get("stem", "imagenet")
    return STEMS[s] if isinstance(s, str) else tuple(s)


def family_convs(spec, in_hw):
    k, s, p, pool = stem_of(spec)
    w, in_c = spec.get("width", 64), spec.get("in_c", 3)
    L = [dict(name="conv1", ci=in_c, co=w, k=k, stride=s, pad=p, h=in_hw)]
    h = (in_hw + 2 * p - k) // s + 1
    if pool:
        h = (h + 2 - 3) // 2 + 1
    ci = w
    for stage, dep in enumerate(spec["depths"]):
        co = w << stage
        for blk in range(dep):
            st = 2 if stage > 0 and blk == 0 else 1
            L.append(dict(name=f"layer{stage + 1}.{blk}.a", ci=ci, co=co, k=3, stride=st, pad=1, h=h))
            ho = (h + 2 - 3) // st + 1
            L.append(dict(name=f"layer{stage + 1}.{blk}.b", ci=co, co=co, k=3, stride=1, pad=1, h=ho))
            if st != 1 or ci != co:
                L.append(dict(name=f"layer{stage + 1}.{blk}.proj", ci=ci, co=co, k=1, stride=st, pad=0, h=h))
            ci, h = co, ho
    L.append(dict(name="fc", ci=ci, co=spec["classes"], k=1, stride=1, pad=0, h=1))
    return L


def family_step_ref(convs, W, S, x, exp_in, labels, classes, pool=True):
    """RR.train_step with the stem pool optional; the same record (fwd / exp / dy / dw per layer,
    logits, exp_logits)."""
    n = x.shape[0]
    nl = len(convs)
    rec = dict(fwd=[None] * nl, exp=[None] * nl, inp=[None] * nl, dy=[None] * nl, dw=[None] * nl)
    G = [O.geom(n, l["ci"], l["h"], l["h"], l["co"], l["k"], stride=l["stride"], pad=l["pad"]) for l in convs]

    def conv_fwd(i, a, ea):
        y, e, _, st = O.conv_fwd(G[i], a, W[i], ea, S[i])
        assert st.overflow == 0
        rec["fwd"][i], rec["exp"][i], rec["inp"][i] = y, e, a
        return y, e

    y, e = conv_fwd(0, x, exp_in)
    r0 = O.relu(y)
    p0 = O.maxpool(r0, 3, 2, 1) if pool else r0
    u, eu = p0, e
    BL = RR.blocks(convs)
    saved = []
    for (ia, ib, ip) in BL:
        ya, ea = conv_fwd(ia, u, eu)
        h = O.relu(ya)
        yb, eb = conv_fwd(ib, h, ea)
        sc, es = conv_fwd(ip, u, eu) if ip is not None else (u, eu)
        z, ez = RR.residual_add(yb, eb, sc, es)
        q, eo = RR.requant(z, ez)
        saved.append(dict(ya=ya, q=q))
        u, eu = O.relu(q), eo
    gsum = u.astype(np.int32).sum(axis=(2, 3)).astype(np.int32)
    g8, eg = RR.requant(gsum, eu)
    fc = nl - 1
    logits4, el = conv_fwd(fc, g8.reshape(n, -1, 1, 1), eg)
    logits = logits4.reshape(n, classes)
    rec["logits"], rec["exp_logits"] = logits, el
    d = O.loss_grad(logits, el, onehot(labels, classes)).reshape(n, classes, 1, 1)
    dW = [None] * nl

    def wgrad(i, dy):
        dw, _, _, _ = O.conv_wgrad(G[i], rec["inp"][i], dy)
        rec["dy"][i], rec["dw"][i] = dy, dw
        dW[i] = dw

    def dgrad(i, dy, edy):
        dx, inc, _, _ = O.conv_dgrad(G[i], dy, W[i])
        return dx, RR._e8(edy + S[i] + inc)

    wgrad(fc, d)
    dg, edu = dgrad(fc, d, 0)
    hh = u.shape[2]
    du = np.broadcast_to(dg.reshape(n, -1, 1, 1), (n, dg.shape[1], hh, hh)).astype(np.int8).copy()
    for k in range(len(BL) - 1, -1, -1):
        ia, ib, ip = BL[k]
        dz = O.relu_grad(saved[k]["q"], du)
        wgrad(ib, dz)
        dh, edh = dgrad(ib, dz, edu)
        dh = O.relu_grad(saved[k]["ya"], dh)
        wgrad(ia, dh)
        dua, edua = dgrad(ia, dh, edh)
        if ip is not None:
            wgrad(ip, dz)
            dus, edus = dgrad(ip, dz, edu)
        else:
            dus, edus = dz, edu
        zsum, ez = RR.residual_add(dua, edua, dus, edus)
        du, edu = RR.requant(zsum, ez)
    dp = O.maxpool_grad(r0, p0, du, 3, 2, 1) if pool else du
    wgrad(0, O.relu_grad(rec["fwd"][0], dp))
    return [O.sgd_update(W[i], dW[i]) for i in range(nl)], rec


def draw_steps(spec, in_hw, batch, images, steps=2):
    """The inputs of a case: [(data, labels)] -- int8 x, or uint8 images."""
    rng = np.random.default_rng(SEED_X)
    in_c = spec.get("in_c", 3)
    out = []
    for _ in range(steps):
        if images:
            data = rng.integers(0, 256, (batch, in_c, in_hw, in_hw)).astype(np.uint8)
        else:
            data = rng.integers(-127, 128, (batch, in_c, in_hw, in_hw)).astype(np.int8)
        out.append((data, rng.integers(0, spec["classes"], batch).astype(np.int32)))
    return out


@functools.lru_cache(maxsize=None)
def reference(name, steps=2):
    """(convs, W0, S, [(data, labels, x, exp, newW, rec)]) of a case: the oracle's steps, computed
    once per process and shared (nothing in it is written afterwards)."""
    spec, in_hw, batch, images = CASES[name]
    convs = family_convs(spec, in_hw)
    W, S = RR.init_weights(convs, seed=SEED_W)
    W0 = W
    out = []
    for data, labels in draw_steps(spec, in_hw, batch, images, steps):
        x, e = O.quantize_images(data) if images else (data, EXP_IN)
        newW, rec = family_step_ref(convs, W, S, x, e, labels, spec["classes"], pool=bool(stem_of(spec)[3]))
        out.append((data, labels, x, e, newW, rec))
        W = newW
    return convs, W0, S, out
