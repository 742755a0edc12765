"""Case tables and CPU references of tests/test_gpu_update_ops.py (and, without a GPU, of
tests/test_update_op_cases.py, which checks that the tables reach the branches they are meant to).

Every reference here is the CPU oracle (oracle/niti_oracle.py, oracle/niti_resnet_ref.py) or plain
numpy on int64 / int32; none is a GPU kernel.  Inputs and references are built once per case
(lru_cache) and handed out read-only.

What each group guards (file:line of mandheling-dsp-training_amd/csrc at the time of writing):

A. SGD update (niti_sgd_update, niti_sgd_update_wf)
   niti_sgd.hpp:92    g = PSTO(acc, bw - rule), 0 when bw == 0: the pinned ranges 0 / 1 (bw == 0),
                      2 / 3 / 5 (shifts -2 .. 1, the negative ones through psto_generic) and
                      2^31 - 1 (the top shift), rules 2 and 3
   niti_sgd.hpp:95    w <- clip(w - g, +-127): weights over the whole int8 range with -128 cells, so
                      every random case clips (a +-128 clip or a wrapping cast flips w16 / wT / wf)
   niti_sgd.hpp:68,85 the tile guards: co = 40 / 12 / 1 rows and cip = 32 / 512 / 16 columns inside
                      64 x 64 tiles, a 32-wide remainder tile at 96 and 160 channels
   niti_sgd.hpp:100   the WF byte index (an off-by-one in any factor moves at least one byte)
   niti_sgd.hpp:104   zero rows co..cop of the tile -> zero columns co..cop of wT (:113)
   niti_sgd.hpp:129   the transposed WF byte index, tap 8 - k
   niti_kernels.hip:4193, :4247   the update's grid-stride loop: 896 x 896 x 9 has 1764 tiles on a
                      1536-block grid, so 228 blocks take a second tile (a dropped or repeated
                      tile leaves the 77 fill or a twice-updated weight)
   niti_capi.hip:536  wf with ci % 32 != 0 is NOT_SUPPORT

B. Residual ops (niti_residual_add, niti_residual_requant, niti_residual_requant_relu_grad)
   niti_kernels.hip:3537   raw = shift <= 0: amp 1 / 40 / 64 / 3 cases (amp 64: 128 wraps to -128)
   niti_kernels.hip:3536   shift == 1 runs PSTO 2: amp 127 gap 0 (max 254)
   niti_device.hpp:122     rr = min(r, 7): gaps 31 / 32 / 64 / 127 / 200 / 255 have r = 8 .. 232
                           (without the min the bit-field extract leaves lo's byte)
   niti_device.hpp:142     min(.., 127): hi = -128 at gap >= 23 gives |z| = 2^30 -> q = 128
   niti_device.hpp:252     residual_z's r >= 31 arm: gaps 55 .. 255 (r = 32 .. 232); a 32-bit shift
                           takes r mod 32, which is 0 at gaps 55 and 87 (lo unshifted: wrong z)
                           (hi * 2^23 + (0 or -1) requantises to the same byte either way, so at
                           large gaps lo's exact value shows in residual_add's z, not in out)
   niti_resnet.hip:32, niti_kernels.hip:3540-3541   ez / exp_out as int8: e_hi = 127 cases
   niti_kernels.hip:3558, :3579   the relu-gradient mask (> 0: -128 and 0 drop, 1 and 127 keep)
   niti_resnet.hip:34, niti_kernels.hip:3549, :3565   the 2048-block grid-stride loops: n =
                           2048 * 256 * 16 + 16 * 300 makes a second, ragged pass of 300 chunks
   niti_kernels.hip:3544, :3565   NITI_RES_PK=0 sends PSTO cases down the 32-bit loop too

C. niti_requant_act (requant_quad_kernel<RQ_PLAIN>)
   niti_kernels.hip:3203-3204   raw / shift 1 / PSTO by the pinned range
   niti_kernels.hip:3209        exp_out = int8(exp_in + wscale + inc) wraps (120 + 5 + 9)
   niti_kernels.hip:3213        the outer loop: 2,099,200 quads = one full pass of 4 loads per
                                thread on 2048 blocks plus a 2048-quad tail
   niti_kernels.hip:3227, :3232 the tail's load guard and break (an unmasked tail reads and
                                writes past the tensor or leaves quads unwritten)
   niti_kernels.hip:3184, :3238 relu, and the mask's > 0

D. Layout helpers and the sum pool
   niti_kernels.hip:4857        nchw_to_chwn16: pad channels and pad images 0
   niti_kernels.hip:4777, :4786 nhwc16_to_chwn16: the 64 x 64 tile guards (n = 70, cp = 144)
   niti_kernels.hip:4939, :4889 ohwi16_to_oihw, nhwc16_to_nchw index maps
   niti_resnet.hip:194-208      sum_pool over 5 blocks publishing one range
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
import niti_resnet_ref as RR  # noqa: E402


def r16(x):
    return (x + 15) // 16 * 16


def _ro(*arrays):
    for a in arrays:
        a.flags.writeable = False
    return arrays


def branch_of(acc):
    """The forward rule's branch for an int32 tensor: (name, bit width)."""
    bw = O.range_estimate(acc)
    return ("raw" if bw - 7 <= 0 else "one" if bw - 7 == 1 else "psto"), bw


# ------------------------------------------------------------------------------------ A. SGD update
# (co, ci, kk, with wf / wft)
SGD_LAYERS = [
    (96, 96, 9, True),      # a 64 x 64 tile and a 32-wide remainder in both directions
    (32, 160, 9, True),
    (160, 32, 9, True),
    (40, 24, 9, False),     # ragged: cip = 32, cop = 48
    (12, 500, 1, False),    # FC
    (1, 1, 1, False),
    (896, 896, 9, True),    # 14 * 14 * 9 = 1764 tiles > the 1536-block grid (29 MB of accumulators)
]
SGD_RULES = (2, 3)
SGD_SMALL_LAYERS = [(96, 96, 9, True), (12, 500, 1, False)]
SGD_SMALL_MAX = [0, 1, 2, 3, 5, 2**31 - 1]  # bw 0, 0, 1, 2, 3, 31
SGD_RANDOM_TOP = 2**20
SGD_FILL = 77


@functools.lru_cache(maxsize=None)
def sgd_inputs(co, ci, kk, pin=None):
    """(acc int32 [co][k][k][cip], w16 int8 [co][k][k][cip]), pad input channels 0.
    acc: uniform in +-2^20 (pin None) or in +-pin, its first cell +max and its last -max so the
    range is known.  w: uniform in [-127, 127] with a few cells -128; the first of them sits on the
    positive first cell of acc, where w - g < -127 whenever g > 0."""
    rng = np.random.default_rng([co, ci, kk, 0 if pin is None else 1 + pin % 1000003])
    k = 3 if kk == 9 else 1
    assert k * k == kk
    top = SGD_RANDOM_TOP if pin is None else pin
    a = rng.integers(-top, top + 1, (co, k, k, ci), dtype=np.int64)
    a.flat[-1] = -top
    a.flat[0] = top
    w = rng.integers(-127, 128, (co, k, k, ci), dtype=np.int64)
    for pos in {0, w.size // 3, w.size // 2, w.size - 1}:
        w.flat[pos] = -128
    acc = np.zeros((co, k, k, r16(ci)), np.int32)
    acc[..., :ci] = a
    w16 = np.zeros((co, k, k, r16(ci)), np.int8)
    w16[..., :ci] = w
    return _ro(acc, w16)


def wf_index(co, ci):
    """Byte of w[o][k][i] in WF [co/32][ci/32][9][2][32][16] (niti_sgd.hpp), shape [co][9][ci]."""
    o = np.arange(co, dtype=np.int64)[:, None, None]
    k = np.arange(9, dtype=np.int64)[None, :, None]
    i = np.arange(ci, dtype=np.int64)[None, None, :]
    cb = ci // 32
    return (((((o >> 5) * cb + (i >> 5)) * 9 + k) * 2 + ((i >> 4) & 1)) * 32 + (o & 31)) * 16 + (i & 15)


def wft_index(co, ci):
    """Byte of w[o][k][i] in the input gradient's WF [ci/32][co/32][9][2][32][16], tap 8 - k."""
    o = np.arange(co, dtype=np.int64)[:, None, None]
    k = np.arange(9, dtype=np.int64)[None, :, None]
    i = np.arange(ci, dtype=np.int64)[None, None, :]
    ob = co // 32
    return (((((i >> 5) * ob + (o >> 5)) * 9 + (8 - k)) * 2 + ((o >> 4) & 1)) * 32 + (i & 31)) * 16 + (o & 15)


def wf_bytes(co, ci):
    return (co // 32) * (ci // 32) * 9 * 1024


@functools.lru_cache(maxsize=None)
def sgd_reference(co, ci, kk, rule, with_wf, pin=None):
    """dict(g, w, wT, wf, wft, clipped): the oracle's gradient and weights in the device layouts."""
    acc, w16 = sgd_inputs(co, ci, kk, pin)
    g, _ = (O.requant_wgrad if rule == 2 else O.requant_matmul)(acc)
    w_new = O.sgd_update(w16, g).reshape(w16.shape)
    k = acc.shape[1]
    wT = np.zeros((ci, k, k, r16(co)), np.int8)
    wT[..., :co] = w_new[..., :ci].transpose(3, 1, 2, 0)
    ref = dict(g=g, w=w_new, wT=wT, wf=None, wft=None,
               clipped=int((np.abs(w16.astype(np.int32) - g.astype(np.int32)) > 127).sum()))
    if with_wf:
        w9 = w_new[..., :ci].reshape(co, 9, ci)
        ref["wf"] = np.full(wf_bytes(co, ci), SGD_FILL, np.int8)
        ref["wf"][wf_index(co, ci).ravel()] = w9.ravel()
        ref["wft"] = np.full(wf_bytes(co, ci), SGD_FILL, np.int8)
        ref["wft"][wft_index(co, ci).ravel()] = w9.ravel()
    _ro(*(v for v in ref.values() if isinstance(v, np.ndarray)))
    return ref


# ------------------------------------------------------------------------------------ B. residual ops
# (amp, gap, e_hi, branch, inc, r): branch / inc / r as the reference gives them
# (tests/test_update_op_cases.py asserts them)
RES_N = 4096
RES_N_BIG = 2048 * 256 * 16 + 16 * 300
RES_CASES = (
    [(amp, 0, -5, "raw", 0, 0) for amp in (1, 40, 64)] +
    [(3, gap, -5, "raw", 0, 0) for gap in (1, 2, 5)] +
    [(127, 0, -5, "one", 2, 0), (127, 1, -5, "psto", 2, 0)] +
    # (55 and 87: r = 32 and 64, where a 32-bit shift that takes r mod 32 shifts by 0 -- at
    # every other r >= 31 here r mod 32 >= 7 and would give lo's sign all the same)
    [(127, gap, -5, "psto", 23, gap - 23) for gap in (23, 24, 30, 31, 32, 55, 64, 87)] +
    [(127, gap, 127, "psto", 23, gap - 23) for gap in (127, 200, 255)]
)
RES_BIG_CASES = [c for c in RES_CASES if (c[0], c[1]) in ((40, 0), (127, 24))]
MASK_VALUES = np.array([-128, 0, 1, 127], np.int8)


@functools.lru_cache(maxsize=None)
def res_inputs(amp, gap, e_hi, swap, n=RES_N):
    """(a, ea, b, eb, mask): operands in +-amp with +amp / -amp pinned in both, the high-exponent
    one first unless swap; amp 127: some -128 cells, none where it would move the range (a -128 high
    cell meets a non-negative low one)."""
    rng = np.random.default_rng([amp, gap, n])
    x = rng.integers(-amp, amp + 1, n).astype(np.int8)   # the high operand
    y = rng.integers(-amp, amp + 1, n).astype(np.int8)
    x[0] = y[0] = amp
    x[1] = y[1] = -amp
    if amp == 127:
        # (hi = -128 with lo < 0 at gap >= 23 would give |z| > 2^30, one more bit of range)
        x[2:5] = [-128, 5, -128]
        y[2:5] = [0, -128, 127]
    mask = MASK_VALUES[rng.integers(0, 4, n)]
    mask[:4] = MASK_VALUES
    mask[4:8] = MASK_VALUES[::-1]
    e_lo = e_hi - gap
    assert -128 <= e_lo <= e_hi <= 127
    _ro(x, y, mask)
    return (y, e_lo, x, e_hi, mask) if swap else (x, e_hi, y, e_lo, mask)


@functools.lru_cache(maxsize=None)
def res_reference(amp, gap, e_hi, swap, n=RES_N):
    """dict(z, ez, range, out, out_relu, out_mask, exp_out, branch, bw)."""
    a, ea, b, eb, mask = res_inputs(amp, gap, e_hi, swap, n)
    z, ez = RR.residual_add(a, ea, b, eb)
    q, eo = RR.requant(z, ez)
    branch, bw = branch_of(z)
    ref = dict(z=z, ez=int(np.int8(ez)), range=int(np.abs(z.astype(np.int64)).max()), out=q,
               out_relu=np.maximum(q, 0).astype(np.int8), out_mask=np.where(mask > 0, q, 0).astype(np.int8),
               exp_out=eo, branch=branch, bw=bw)
    _ro(*(v for v in ref.values() if isinstance(v, np.ndarray)))
    return ref


RES_MODES = ("plain", "relu", "mask")


def residual_requant_mismatch(T, ops, case, swap, n=RES_N, modes=RES_MODES):
    """Runs niti_residual_requant (relu off / on) and niti_residual_requant_relu_grad on one case;
    returns the list of mismatches against res_reference (empty: all equal)."""
    amp, gap, e_hi = case[:3]
    a, ea, b, eb, mask = res_inputs(amp, gap, e_hi, swap, n)
    ref = res_reference(amp, gap, e_hi, swap, n)
    dev = lambda v: T.from_numpy(np.array(v)).cuda()  # noqa: E731
    i8 = lambda v: T.tensor([v], dtype=T.int8, device="cuda")  # noqa: E731
    da, db, dm = dev(a), dev(b), dev(mask)
    bad = []
    for mode in modes:
        amax = ops.new_range()
        ops.residual_range(da, i8(ea), db, i8(eb), amax)
        got, ez, eo = ops.residual_requant(da, i8(ea), db, i8(eb), amax, relu=mode == "relu",
                                           relu_mask=dm if mode == "mask" else None)
        want = ref[{"plain": "out", "relu": "out_relu", "mask": "out_mask"}[mode]]
        if ops.range_max(amax) != ref["range"]:
            bad.append((case, swap, mode, "range", ops.range_max(amax), ref["range"]))
        if not np.array_equal(got.cpu().numpy(), want):
            bad.append((case, swap, mode, "out", int((got.cpu().numpy() != want).sum())))
        if int(ez.item()) != ref["ez"] or int(eo.item()) != ref["exp_out"]:
            bad.append((case, swap, mode, "exp", int(ez.item()), int(eo.item()), ref["ez"], ref["exp_out"]))
    return bad


def residual_table_mismatch(T, ops):
    """The whole n = 4096 table through residual_requant_mismatch (the NITI_RES_PK=0 child's body)."""
    bad = []
    for case in RES_CASES:
        for swap in (False, True):
            bad += residual_requant_mismatch(T, ops, case, swap)
    return bad


# ------------------------------------------------------------------------------------ C. requant_act
RQ_SHAPES = [(1, 16), (257, 48), (65600, 128)]   # the last: 2,099,200 quads
RQ_PINS = [("raw", 128), ("one", 200), ("psto", 40000)]   # raw: 128 wraps to -128
RQ_EXP = (3, -7)
RQ_WRAP = dict(shape=(257, 48), pin=40000, exp_in=120, wscale=5)   # 120 + 5 + 9 wraps


@functools.lru_cache(maxsize=None)
def rq_inputs(rows, ldc, pin):
    rng = np.random.default_rng([rows, ldc, pin])
    acc = rng.integers(-pin, pin + 1, (rows, ldc)).astype(np.int32)
    acc[0, 0] = pin
    acc[-1, -1] = -pin
    mask = MASK_VALUES[rng.integers(0, 4, (rows, ldc))]
    mask[0, :4] = MASK_VALUES
    mask[-1, -4:] = MASK_VALUES
    return _ro(acc, mask)


@functools.lru_cache(maxsize=None)
def rq_reference(rows, ldc, pin):
    """dict(out, out_relu, out_mask, inc, branch)."""
    acc, mask = rq_inputs(rows, ldc, pin)
    q, inc = O.requant_fwd(acc)
    ref = dict(out=q, out_relu=np.maximum(q, 0).astype(np.int8), out_mask=np.where(mask > 0, q, 0).astype(np.int8),
               inc=inc, branch=branch_of(acc)[0])
    _ro(*(v for v in ref.values() if isinstance(v, np.ndarray)))
    return ref


# ------------------------------------------------------------------------------------ D. layouts, sum pool
LAYOUT_SHAPES = [(5, 3, 2, 3), (70, 130, 1, 2), (17, 64, 3, 3)]   # (n, c, h, w)
POOL_SHAPE = (20, 7, 7, 64)   # 1280 (image, channel) threads: five blocks


@functools.lru_cache(maxsize=None)
def layout_inputs(n, c, h, w):
    """(x NCHW, x NHWC16 with zero pad channels), values over the whole int8 range."""
    rng = np.random.default_rng([n, c, h, w])
    x = rng.integers(-128, 128, (n, c, h, w)).astype(np.int8)
    x.flat[0] = -128
    x16 = np.zeros((n, h, w, r16(c)), np.int8)
    x16[..., :c] = x.transpose(0, 2, 3, 1)
    return _ro(x, x16)


def chwn16_of(x):
    """NCHW -> CHWN16 [r16(c)][h][w][r16(n)], pads 0."""
    n, c, h, w = x.shape
    out = np.zeros((r16(c), h, w, r16(n)), np.int8)
    out[:c, :, :, :n] = x.transpose(1, 2, 3, 0)
    return out
