"""The update-bits rule restated for the tests (importable without a GPU), and the inputs of the
op-level cases of tests/test_gpu_update_bits_op.py.

The rule (include/niti_hip.h, "Update bits") from the oracle's own primitives: bw =
O.range_estimate(acc); bits == 2 is the reference's rule 2, g = O.psto(acc, bw - 2) at any shift
(bw == 1 included: the shift -1 through the reference's PSTO), 0 for bw == 0; any other bits in
1..7 gives g = O.psto(acc, bw - bits) for a shift >= 0 and clip(acc, +-127) below; bits == 0 leaves
the layer as it is.  O.sgd_update applies g.  test_update_bits_cpu.py pins the bits == 2 form to
O.conv_wgrad + O.sgd_update.

Op-level inputs: acc = O.conv_wgrad_acc of a small random conv, scaled so that its largest
magnitude is exactly 2^bw (bw >= 1; then O.range_estimate is bw) or 1 (bw == 0).  A case is a
(shape, bits) pair crossed with the shift classes of SHIFTS: bw = bits + shift.
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
import update_op_cases as U  # noqa: E402

FILL = 77
BITS = tuple(range(8))
# bw - bits: negative, 0, 1, an odd and an even shift; None: bw == 0 (a zero gradient)
SHIFTS = (-1, 0, 1, 5, 12, None)

# name: co, ci, kernel, stride, pad, input size, and which copies the job carries
SHAPES = {
    "tile64": dict(co=64, ci=64, k=1, stride=1, pad=0, h=2),                  # one full 64 x 64 tile, one tap
    "ragged": dict(co=40, ci=24, k=3, stride=1, pad=1, h=3),                  # cip = 32, cop = 48
    "wf": dict(co=32, ci=32, k=3, stride=1, pad=1, h=3, wf=True),             # the fragment-major copies
    "wT": dict(co=20, ci=72, k=1, stride=1, pad=0, h=2, wT=True),             # two tiles along ci
    "subw": dict(co=24, ci=16, k=3, stride=2, pad=1, h=4, wT=True, subw=True),
    "slab": dict(co=24, ci=16, k=3, stride=1, pad=1, h=3, splits=4),          # a deferred combine
}
THREE_JOBS = (("ragged", 4, 0), ("wf", 0, 5), ("tile64", 7, -1))  # (shape, bits, shift) in one launch


def r16(x):
    return (x + 15) // 16 * 16


def bw_of(bits, shift):
    """The gradient bit width a (bits, shift class) pair asks for; None where the class does not
    exist (a negative shift needs 1 <= bw < bits)."""
    if shift is None:
        return 0
    if bits == 3 and shift == -1:
        # bw == 2 is the one width at which a negative-shift class says nothing: bits == 2 has the
        # shift 0 there and applies the gradient as it is too.  bits == 3 takes bw == 1 (shift -2).
        return 1
    bw = bits + shift
    return bw if bw >= 1 else None


def classes_of(bits):
    """[(shift, bw)] of one bits value, without duplicates of the bw == 0 class."""
    return [(s, bw_of(bits, s)) for s in SHIFTS if bw_of(bits, s) is not None]


# ------------------------------------------------------------------------------------ the rule
def clip127(a):
    return np.clip(np.asarray(a, np.int64), -127, 127).astype(np.int8)


def rule_gradient(acc, bits):
    """(g int8 in acc's shape or None for a frozen layer, bw)."""
    assert 0 <= bits <= 7
    acc = np.ascontiguousarray(acc, np.int32)
    bw = O.range_estimate(acc)
    if bits == 0:
        return None, bw
    if bw == 0:
        return np.zeros(acc.shape, np.int8), bw
    sh = bw - bits
    if bits == 2 or sh >= 0:
        return O.psto(acc, sh).astype(np.int8), bw  # (PSTO clips to +-127)
    return clip127(acc), bw


def apply_update(w, acc, bits):
    """(new weights, g as the kept int8 gradient reads: zeros for a frozen layer)."""
    g, _ = rule_gradient(acc, bits)
    if g is None:
        return np.array(w, np.int8), np.zeros(np.shape(acc), np.int8)
    return O.sgd_update(w, g).reshape(np.shape(w)), g


def step_update(G, rec_inp, rec_dy, W, bits):
    """A whole step's update under per-layer bits from the step reference's record: layer i's
    int32 gradient recomputed from its input and output gradient (the backward pass reads the old
    weights only, so nothing else of the step depends on the update).  Returns (new weights, kept
    gradients)."""
    newW, kept = [], []
    for i, g in enumerate(G):
        acc, st = O.conv_wgrad_acc(g, rec_inp[i], rec_dy[i])
        assert st.overflow == 0
        w, g8 = apply_update(W[i], acc, bits[i])
        newW.append(w)
        kept.append(g8)
    return newW, kept


# ------------------------------------------------------------------------------------ op-level inputs
def _ro(*arrays):
    for a in arrays:
        a.flags.writeable = False
    return arrays


@functools.lru_cache(maxsize=None)
def raw_acc(name):
    """The unscaled int32 gradient of a shape: O.conv_wgrad_acc of random x / dy, OIHW."""
    s = SHAPES[name]
    rng = np.random.default_rng([len(name), s["co"], s["ci"], s["k"]])
    g = O.geom(2, s["ci"], s["h"], s["h"], s["co"], s["k"], stride=s["stride"], pad=s["pad"])
    x = rng.integers(-127, 128, (2, s["ci"], s["h"], s["h"])).astype(np.int8)
    dy = rng.integers(-127, 128, (2, s["co"], g.oh, g.ow)).astype(np.int8)
    acc, st = O.conv_wgrad_acc(g, x, dy)
    assert st.overflow == 0 and np.abs(acc).max() > 1000
    return _ro(acc)[0]


@functools.lru_cache(maxsize=None)
def inputs(name, bw):
    """(acc OIHW int32 with range exactly bw, w OIHW int8 over the whole range with -128 cells)."""
    s = SHAPES[name]
    a = raw_acc(name).astype(np.int64)
    top = (1 << bw) if bw >= 1 else 1
    m = int(np.abs(a).max())
    acc = np.sign(a) * ((np.abs(a) * top + m // 2) // m)
    acc.flat[0], acc.flat[-1] = top, -top
    acc = acc.astype(np.int32)
    assert O.range_estimate(acc) == bw
    rng = np.random.default_rng([len(name), bw, 7])
    w = rng.integers(-127, 128, acc.shape, dtype=np.int64)
    for pos in {0, w.size // 3, w.size - 1}:
        w.flat[pos] = -128
    return _ro(acc, w.astype(np.int8))


def ohwi16(a):
    """OIHW -> [co][kh][kw][cip], pad input channels 0."""
    co, ci, kh, kw = a.shape
    out = np.zeros((co, kh, kw, r16(ci)), a.dtype)
    out[..., :ci] = a.transpose(0, 2, 3, 1)
    return out


def _taps(kn, pad, par):
    k0 = (par + pad) & 1
    return (kn - k0 + 1) // 2 if k0 < kn else 0


def subw_of(w, pad):
    """A stride-2 layer's sub-pixel class weights from OIHW w: class (py, px) = ((ky - pad) & 1,
    (kx - pad) & 1) in the order py * 2 + px, each [ci][jy][jx][cop] with (jy, jx) = (ky >> 1,
    kx >> 1), pad output channels 0 (SgdJob::subw, csrc/niti_kernels.hpp)."""
    co, ci, kh, kw = w.shape
    cop = r16(co)
    parts = []
    for cl in range(4):
        py, px = cl >> 1, cl & 1
        ny, nx = _taps(kh, pad, py), _taps(kw, pad, px)
        blk = np.zeros((ci, ny, nx, cop), np.int8)
        for ky in range(kh):
            for kx in range(kw):
                if ((ky - pad) & 1, (kx - pad) & 1) == (py, px):
                    blk[:, ky >> 1, kx >> 1, :co] = w[:, :, ky, kx].T
        parts.append(blk.ravel())
    return np.concatenate(parts)


def expected(name, bw, bits):
    """dict(w, g, wT, wf, wft, subw) in the device layouts after the update (None: the job has no
    such copy); frozen: w as it was, g zeros, the copies absent (the caller keeps the sentinel)."""
    s = SHAPES[name]
    acc, w = inputs(name, bw)
    w_new, g = apply_update(w, acc, bits)
    co, ci, k = s["co"], s["ci"], s["k"]
    out = dict(w=ohwi16(w_new), g=ohwi16(g), wT=None, wf=None, wft=None, subw=None, frozen=bits == 0)
    if s.get("wT"):
        out["wT"] = np.zeros((ci, k, k, r16(co)), np.int8)
        out["wT"][..., :co] = w_new.transpose(1, 2, 3, 0)
    if s.get("wf"):
        w9 = w_new.transpose(0, 2, 3, 1).reshape(co, 9, ci)
        out["wf"] = np.full(U.wf_bytes(co, ci), FILL, np.int8)
        out["wf"][U.wf_index(co, ci).ravel()] = w9.ravel()
        out["wft"] = np.full(U.wf_bytes(co, ci), FILL, np.int8)
        out["wft"][U.wft_index(co, ci).ravel()] = w9.ravel()
    if s.get("subw"):
        out["subw"] = subw_of(w_new, s["pad"])
    return out


def slabs_of(acc16, splits, seed):
    """int32 [splits][n] slabs that sum to acc16.ravel() (random parts, the last the remainder)."""
    rng = np.random.default_rng([splits, seed])
    flat = acc16.ravel().astype(np.int64)
    parts = rng.integers(-(1 << 20), 1 << 20, (splits - 1, flat.size))
    last = flat - parts.sum(axis=0)
    out = np.concatenate([parts, last[None]]).astype(np.int32)
    assert np.array_equal(out.astype(np.int64).sum(axis=0), flat)
    return out


# ------------------------------------------------------------------------------------ bw-pinned convs
# (n, max |x|, max |dy|) of a 1x1 conv over a 1x1 map whose weight gradient has the bit width: its
# largest element is n * ax * ad
BW_CONVS = {0: (1, 1, 1), 1: (1, 2, 1), 2: (1, 4, 1), 7: (1, 127, 1), 20: (64, 127, 127)}


@functools.lru_cache(maxsize=None)
def bw_conv(bw):
    """(geom, x, dy, w) of an 8 -> 8 channel 1x1 conv whose int32 weight gradient has range bw."""
    n, ax, ad = BW_CONVS[bw]
    rng = np.random.default_rng([bw, 11])
    x = rng.integers(-ax, ax + 1, (n, 8, 1, 1)).astype(np.int8)
    dy = rng.integers(-ad, ad + 1, (n, 8, 1, 1)).astype(np.int8)
    x[:, 0], dy[:, 0] = ax, ad
    x[:, 1], dy[:, 1] = -ax, ad
    w = rng.integers(-127, 128, (8, 8, 1, 1)).astype(np.int8)
    return O.geom(n, 8, 1, 1, 8, 1), x, dy, w
