"""Case tables and CPU references of tests/test_gpu_fused_requant.py (and, without a GPU, of
tests/test_fused_requant_cases.py, which checks that the tables reach what they are meant to).

The fused forms of the requantisation pass (niti_requant_act_fused) and the stem pool pair
(niti_maxpool_arg, niti_maxpool_grad_arg) against the CPU oracle (oracle/niti_oracle.py: psto,
maxpool, maxpool_grad, relu_grad) or plain numpy on int32 / int64; none is a GPU kernel.  The P16
and C32 layouts are restated here in numpy.  Inputs and references are built once per case
(lru_cache) and handed out read-only.

Every requantise case pins the range in word 0 of a zeroed range buffer (PINS: bw 7 raw, bw 8
shift 1, bw 9 / 16 / 31 PSTO); accumulators stay inside it and every seventh one is an exact
half-way value of PSTO's rounding.

What each group guards (file:line of mandheling-dsp-training_amd/csrc at the time of writing):

every group
   niti_kernels.hip:3201-3210, :3355-3364, :3430-3439, :3859-3868   each variant's own copy of the
                      prologue: raw / shift 1 runs PSTO 2 / PSTO by the pinned range, and exp_out =
                      int8(exp_in + wscale + inc), which wraps in one case per group (120 + 5 + 9)

A. pool forward (requant_quad_kernel<RQ_POOL_FWD>)
   niti_kernels.hip:3252-3258   unit -> (pooled pixel, quad) -> window rows by three fast divisions:
                      2 x 6 x 10 x 48 divides by 12, 5 and 3
   niti_kernels.hip:3276-3284   bmax4 from -128 and the pre-pool store of all four corners
   niti_kernels.hip:3213, :3269, :3275   the outer loop's second, ragged pass (2,097,456 units)

B. pool backward (requant_quad_kernel<RQ_POOL_BWD>)
   niti_kernels.hip:3313-3314   first max wins (done): windows with a tie at a positive max and
                      all-equal windows
   niti_kernels.hip:3315        the relu gradient's x <= 0: windows whose max is 0
   niti_kernels.hip:3305        the optional requantised dy
   niti_kernels.hip:3319-3324   the C32 copy's index (three channel blocks at ldc 96)
   niti_kernels.hip:3213, :3291, :3303   the ragged second pass

C. P16 plain (requant_p16_plain_kernel)
   niti_kernels.hip:3442-3446   (block, quad, quarter) of a unit; ldc 80 divides by 20
   niti_kernels.hip:3456-3463   relu and the mask's > 0
   niti_kernels.hip:3467-3475   the v_perm transposes and the P16 address
   niti_kernels.hip:3441        the grid-stride loop (524,336 units on 2048 blocks)

D. P16 pool backward (requant_p16_kernel<RQ_POOL_BWD, W>)
   niti_kernels.hip:3344-3348   p16_loc of W = 2 (four images per run), 4 (one image), 8 and 16
                      (one pooled row); more than one run per image and more than one image
   niti_kernels.hip:3393-3398   the same first-max / relu routing, kept for the transposes
   niti_kernels.hip:3403-3420   4 x 4 byte transposes into P16 blocks; NPX / 16 = 2 blocks at W = 16

E. zero_cls (requant_quad_kernel<RQ_PLAIN>)
   niti_kernels.hip:3221-3225   the class of a unit's pixel: rows by zc_w, then by zc_h; bit
                      2 (y & 1) + (x & 1); the skipped accumulators hold 0x7fffffff / INT32_MIN,
                      which requantise to -1 / 0 raw and to +-127 otherwise if they are read
   niti_kernels.hip:3226        no load where skipped

F. 3x3 / 2 pool (requant_pool3_kernel<RELU>)
   niti_kernels.hip:3886-3889   c0 / c2: the last window's right column outside an odd-width image
   niti_kernels.hip:3894, :3910 r2: the bottom row outside an odd-height image
   niti_kernels.hip:3920        the relu form's first position (oy > 0 ? 0 : 3) + (c0 ? 0 : 1)
   niti_kernels.hip:3835-3845   rq4_relu against PSTO + relu
   niti_kernels.hip:3849-3854   pool3_take_u7's strict >: the first maximum stays
   niti_kernels.hip:3884, :3902-3908, :3946-3948   strips: the carried top row, a one-row last strip
                      (OH = 9 in strips of 4; NITI_RQ3_ROWS = 1 and 3 in child processes)
   niti_kernels.hip:3937-3944   each pre-pool pixel written once
   niti_kernels.hip:3872, :3880 NITI_RQ3_REMAP=1: one unit per thread on remapped blocks

G. stem pool pair (maxpool_kernel's arg, maxpool_grad_gather_kernel, maxpool3_grad_pooled_kernel)
   niti_kernels.hip:4287-4296   the first-max position beside the max
   niti_kernels.hip:4299-4312   on a map smaller than the kernel (1 x 1 and 2 x 2 under 3 x 3 and
                      5 x 5) the reference clips the forward's window but not the gradient's scan:
                      y is the clipped window's max, arg the element the gradient routes to
   niti_kernels.hip:4506-4520   the gather's window range and pooled > 0
   niti_kernels.hip:4549-4553   the packed kernel's window range and position word
   niti_kernels.hip:4560-4564   first-max match, pooled > 0 (0, 1, 127, negative bytes) and the
                      carry-less int8 sum: four windows of 127 add to 508 -> -4
"""
from __future__ import annotations

import functools

import numpy as np

import update_op_cases as U
from update_op_cases import O, _ro

FILL = 77       # every output buffer's sentinel
GUARD = 256     # sentinel bytes kept on both sides of every output buffer

# (branch, max|acc| pinned in the range buffer): bw 7, 8, 9, 16, 31
PINS = [("raw", 128), ("one", 200), ("psto", 300), ("psto", 40000), ("psto", 2**31 - 1)]
EXP = (3, -7)
WRAP = dict(pin=40000, exp_in=120, wscale=5)   # 120 + 5 + 9 wraps to -122
BIG_PIN = 40000


def rule(pin):
    """(branch, PSTO shift, exponent step) of the forward rule at max|acc| = pin."""
    branch, bw = U.branch_of(np.array([pin], np.int32))
    shift = bw - 7
    return branch, (shift if shift > 1 else 2), (shift if shift > 1 else 2 if shift == 1 else 0)


def requant_ref(acc, pin, relu=False):
    """The forward rule on acc with the range pinned at pin: the oracle's psto, or the raw cast."""
    branch, s, _ = rule(pin)
    q = acc.astype(np.int8) if branch == "raw" else O.psto(acc, s).astype(np.int8)
    return np.maximum(q, 0) if relu else q


def exp_ref(pin, exp_in, wscale):
    return int(np.int32(exp_in + wscale + rule(pin)[2]).astype(np.int8))   # the int8 exponent wraps


def acc_about(q, pin, rng):
    """int32 accumulators within +-pin that the rule at max|acc| = pin requantises to about q
    (exactly q on the raw branch): q * 2^s plus a fraction in +-2^(s-1), every seventh cell an
    exact half-way value; the first cell is +pin and the last -pin."""
    branch, s, _ = rule(pin)
    a = q.astype(np.int64)
    if branch != "raw":
        half = 1 << (s - 1)
        frac = rng.integers(-half, half + 1, q.shape)
        frac.reshape(-1)[::7] = half
        frac.reshape(-1)[3::7] = -half
        a = np.clip(a * (1 << s) + frac, -pin, pin)
    a.reshape(-1)[0] = pin
    a.reshape(-1)[-1] = -pin
    return a.astype(np.int32)


def q_span(pin):
    """The widest requantised magnitude accumulators inside +-pin reach."""
    branch, s, _ = rule(pin)
    return 127 if branch == "raw" else min(127, pin >> s)


def p16_of(x):
    """[pixels][ldc] -> P16 [pixels / 16][ldc][16]."""
    rows, ldc = x.shape
    return np.ascontiguousarray(x.reshape(rows // 16, 16, ldc).transpose(0, 2, 1))


def c32_of(x):
    """NHWC [n][H][W][ldc] -> C32 [n][ldc / 32][H][W][32]."""
    n, h, w, ldc = x.shape
    return np.ascontiguousarray(x.reshape(n, h, w, ldc // 32, 32).transpose(0, 3, 1, 2, 4))


def nchw(x):
    return np.ascontiguousarray(x.transpose(0, 3, 1, 2))


def nhwc(x):
    return np.ascontiguousarray(x.transpose(0, 2, 3, 1))


def pool2_ref(x):
    """The oracle's 2x2 / 2 max pool of x NHWC."""
    return nhwc(O.maxpool(nchw(x), 2, 2, 0))


def pool_first_max(x, k, s, p, oh, ow):
    """(y, arg) of the k x k / s pad-p max pool of x NHWC: the window max over its in-image
    elements and ky * k + kx of the first of them equal to it, in (ky, kx) order (a window with
    no element in the image: -128 and -1)."""
    n, h, w, c = x.shape
    y = np.full((n, oh, ow, c), -129, np.int16)
    arg = np.full((n, oh, ow, c), -1, np.int8)
    for ky in range(k):
        for kx in range(k):
            sy, sx = np.arange(oh) * s - p + ky, np.arange(ow) * s - p + kx
            vy, vx = np.nonzero((sy >= 0) & (sy < h))[0], np.nonzero((sx >= 0) & (sx < w))[0]
            if not len(vy) or not len(vx):
                continue
            sub = np.ix_(np.arange(n), vy, vx, np.arange(c))
            v = x[np.ix_(np.arange(n), sy[vy], sx[vx], np.arange(c))].astype(np.int16)
            take = v > y[sub]
            y[sub] = np.where(take, v, y[sub])
            arg[sub] = np.where(take, ky * k + kx, arg[sub])
    y[y == -129] = -128
    return y.astype(np.int8), arg


def oracle_pool(x, k, s, p, oh, ow):
    """The oracle's max pool of x NHWC at a given pooled size (niti_ref_maxpool: as the reference,
    the window is clipped to min(k, h) x min(k, w), which matters on a map smaller than the kernel)."""
    xc = nchw(x)
    n, c, h, w = xc.shape
    y = np.empty((n, c, oh, ow), np.int8)
    O.lib().niti_ref_maxpool(O._p(xc), n, c, h, w, k, s, p, O._p(y), oh, ow)
    return nhwc(y)


def oracle_pool_grad(x, y, dy, k, s, p):
    """The oracle's pool gradient (niti_ref_maxpool_grad) of NHWC tensors."""
    xc, yc, dc = nchw(x), nchw(y), nchw(dy)
    n, c, h, w = xc.shape
    dx = np.empty_like(xc)
    O.lib().niti_ref_maxpool_grad(O._p(xc), O._p(yc), O._p(dc), n, c, h, w, k, s, p, yc.shape[2], yc.shape[3], O._p(dx))
    return nhwc(dx)


def first_at_least(x, y, k, s, p):
    """ky * k + kx of each window's first in-image element >= y, in (ky, kx) order over the whole
    k x k window (-1: none): the element the reference's pool gradient routes to.  Where y is the
    max of that same window -- every map at least as large as the kernel -- it is the first
    element equal to the window max."""
    n, h, w, c = x.shape
    oh, ow = y.shape[1:3]
    arg = np.full(y.shape, -1, np.int8)
    for ky in range(k):
        for kx in range(k):
            sy, sx = np.arange(oh) * s - p + ky, np.arange(ow) * s - p + kx
            vy, vx = np.nonzero((sy >= 0) & (sy < h))[0], np.nonzero((sx >= 0) & (sx < w))[0]
            if not len(vy) or not len(vx):
                continue
            sub = np.ix_(np.arange(n), vy, vx, np.arange(c))
            v = x[np.ix_(np.arange(n), sy[vy], sx[vx], np.arange(c))]
            arg[sub] = np.where((arg[sub] < 0) & (v >= y[sub]), ky * k + kx, arg[sub])
    return arg


def pool_grad_sums(arg, dy, h, w, k, s, p, pooled=None):
    """int64 [n][h][w][c]: dy summed over the windows whose first max is the pixel (with pooled:
    only the windows with pooled > 0).  The int8 gradient is its wrapping cast."""
    n, oh, ow, c = dy.shape
    term = dy.astype(np.int64)
    if pooled is not None:
        term = np.where(pooled > 0, term, 0)
    dx = np.zeros((n, h, w, c), np.int64)
    b, oy, ox, ch = np.nonzero(arg >= 0)
    a = arg[b, oy, ox, ch].astype(np.int64)
    np.add.at(dx, (b, oy * s - p + a // k, ox * s - p + a % k, ch), term[b, oy, ox, ch])
    return dx


def _seed(*parts):
    return np.random.default_rng([int(v) & 0x7fffffff for v in parts])


# --------------------------------------------------------------------------------- A. pool forward
PF_SHAPES = [(3, 2, 2, 16), (2, 6, 10, 48)]        # (n, H, W, ldc)
PF_BIG = (174788, 2, 6, 16)                        # 2,097,456 units: 2048 x 256 x 4 and 304 more
PF_WRAP_SHAPE = PF_SHAPES[1]


@functools.lru_cache(maxsize=4)
def pf_case(shape, pin, relu):
    """dict(acc [rows][ldc], out [rows][ldc], pool [n][H/2][W/2][ldc])."""
    n, h, w, ldc = shape
    rng = _seed(1, *shape, pin)
    acc = acc_about(rng.integers(-2, 6, (n * h * w, ldc)), pin, rng)
    out = requant_ref(acc, pin, relu)
    pool = pool2_ref(out.reshape(n, h, w, ldc))
    return dict(zip(("acc", "out", "pool"), _ro(acc, out, pool)))


# -------------------------------------------------------------------- B, D. pool backward (+ P16)
# (n, H, W, ldc, dx_c32)
PB_SHAPES = [(5, 2, 2, 32, True), (2, 6, 10, 96, True)]   # one and three C32 channel blocks
PB_BIG = (174788, 2, 6, 16, False)
PB_WRAP_SHAPE = PB_SHAPES[1]
# D: (n, W = H, ldc)
P16B_SHAPES = [(n, w, ldc) for w, ns in ((2, (4, 12)), (4, (1, 3)), (8, (1, 3)), (16, (1, 2))) for n in ns
               for ldc in (16, 48)]


@functools.lru_cache(maxsize=None)
def pool_x(n, h, w, ldc, relu):
    """(x, y): the forward's pre-pool output NHWC in -2 .. 5 (relu: 0 .. 5) and its 2x2 pool.  The
    first three windows are planted in every channel: a tie at a positive max (5 5 / 1 5), an
    all-equal window (3, which the fourth window repeats at 0 or -2) and a window whose max is 0."""
    rng = _seed(2, n, h, w, ldc, relu)
    x = rng.integers(0 if relu else -2, 6, (n, h, w, ldc)).astype(np.int8)
    wins = [(b, py, px) for b in range(n) for py in range(h // 2) for px in range(w // 2)]
    plants = [(5, 5, 1, 5), (3, 3, 3, 3), (0, 0, 0, 0) if relu else (-1, 0, -2, 0),
              (0, 0, 0, 0) if relu else (-2, -2, -2, -2)]
    for (b, py, px), v in zip(wins, plants):
        x[b, 2 * py:2 * py + 2, 2 * px:2 * px + 2, :] = np.array(v, np.int8).reshape(2, 2, 1)
    return _ro(x, pool2_ref(x))


@functools.lru_cache(maxsize=4)
def pb_case(n, h, w, ldc, pin, relu):
    """dict(acc [pooled pixels][ldc], x, y, q (the requantised dy), dx [n][H][W][ldc])."""
    x, y = pool_x(n, h, w, ldc, relu)
    rng = _seed(3, n, h, w, ldc, pin, relu)
    span = q_span(pin)
    acc = acc_about(rng.integers(-span, span + 1, (n * (h // 2) * (w // 2), ldc)), pin, rng)
    q = requant_ref(acc, pin)
    dx = O.maxpool_grad(nchw(x), nchw(y), nchw(q.reshape(y.shape)), 2, 2, 0)
    if relu:
        dx = O.relu_grad(nchw(x), dx)
    return dict(zip(("acc", "x", "y", "q", "dx"), (*_ro(acc), x, y, *_ro(q, nhwc(dx)))))


def window_kinds(x, y):
    """How many 2x2 windows (per channel) have a tie at a positive max, are all equal, have a
    max <= 0."""
    n, h, w, c = x.shape
    wv = x.reshape(n, h // 2, 2, w // 2, 2, c).transpose(0, 1, 3, 5, 2, 4).reshape(n, h // 2, w // 2, c, 4)
    at_max = (wv == y[..., None]).sum(-1)
    return dict(tie=int(((at_max >= 2) & (y > 0)).sum()), equal=int((at_max == 4).sum()), nonpos=int((y <= 0).sum()))


# --------------------------------------------------------------------------------- C. P16 plain
P16_SHAPES = [(16, 16), (48, 80)]     # (rows, ldc)
P16_BIG = (524336, 16)                # 524,336 units: 2048 x 256 and 48 more
P16_WRAP_SHAPE = P16_SHAPES[1]


@functools.lru_cache(maxsize=4)
def p16_case(rows, ldc, pin):
    """dict(acc, mask, out, out_relu, out_mask), each output [rows][ldc] (its P16 copy: p16_of)."""
    rng = _seed(4, rows, ldc, pin)
    span = q_span(pin)
    acc = acc_about(rng.integers(-span, span + 1, (rows, ldc)), pin, rng)
    mask = U.MASK_VALUES[rng.integers(0, 4, (rows, ldc))]
    mask[0, :4] = U.MASK_VALUES
    mask[-1, -4:] = U.MASK_VALUES
    q = requant_ref(acc, pin)
    return dict(zip(("acc", "mask", "out", "out_relu", "out_mask"),
                    _ro(acc, mask, q, np.maximum(q, 0), np.where(mask > 0, q, 0).astype(np.int8))))


# --------------------------------------------------------------------------------- E. zero_cls
ZC_SHAPES = [(3, 5, 7, 32), (2, 4, 6, 16)]    # (n, zc_h, zc_w, ldc)
ZC_MASKS = list(range(1, 15))
ZC_WRAP_SHAPE = ZC_SHAPES[0]
POISON = (np.int32(0x7fffffff), np.int32(-2**31))


def zc_classes(n, h, w):
    """[n][h][w]: each pixel's class bit 2 (y & 1) + (x & 1)."""
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    return np.broadcast_to(2 * (yy & 1) + (xx & 1), (n, h, w))


@functools.lru_cache(maxsize=None)
def zc_case(shape, cls, pin):
    """dict(acc (the skipped classes' accumulators poisoned), mask, skip [rows] bool, out,
    out_mask)."""
    n, h, w, ldc = shape
    rng = _seed(5, *shape, pin)   # (the same clean accumulators for every class mask)
    clean = acc_about(rng.integers(-2, 6, (n * h * w, ldc)), pin, rng)
    mask = U.MASK_VALUES[rng.integers(0, 4, (n * h * w, ldc))]
    skip = ((cls >> zc_classes(n, h, w).reshape(-1)) & 1).astype(bool)
    acc = clean.copy()
    poison = np.where((np.arange(clean.size).reshape(clean.shape) & 1) == 0, POISON[0], POISON[1])
    acc[skip] = poison[skip]
    q = requant_ref(clean, pin)
    q[skip] = 0
    return dict(zip(("acc", "mask", "skip", "out", "out_mask"),
                    _ro(acc, mask, skip, q, np.where(mask > 0, q, 0).astype(np.int8))))


# --------------------------------------------------------------------------------- F. 3x3 / 2 pool
P3_SHAPES = [(2, 1, 1, 16), (1, 2, 3, 16), (3, 7, 9, 48), (2, 10, 6, 16), (1, 17, 12, 32)]   # (n, H, W, ldc)
P3_CHILD_SHAPES = [(3, 7, 9, 48), (1, 17, 12, 32)]
P3_CHILD_ENVS = [dict(NITI_RQ3_ROWS="1"), dict(NITI_RQ3_ROWS="3"), dict(NITI_RQ3_REMAP="1")]
P3_WRAP_SHAPE = P3_SHAPES[2]
# windows (oy, ox) of image 0 whose pixels are planted <= 0 where the map has them: a corner, an
# edge and an interior window
P3_ZERO_WINDOWS = [(0, 0), (0, 2), (2, 1)]


def p3_out(h):
    return (h - 1) // 2 + 1


@functools.lru_cache(maxsize=None)
def p3_case(shape, pin, relu):
    """dict(acc [rows][ldc], pre [n][H][W][ldc] (the requantised image), out, arg
    [n][OH][OW][ldc])."""
    n, h, w, ldc = shape
    rng = _seed(6, *shape, pin)   # (relu on and off share the accumulators)
    q = rng.integers(-2, 6, (n, h, w, ldc))
    for oy, ox in P3_ZERO_WINDOWS:
        if oy < p3_out(h) and ox < p3_out(w):
            q[0, max(0, 2 * oy - 1):2 * oy + 2, max(0, 2 * ox - 1):2 * ox + 2, :] = -1
    acc = acc_about(q.reshape(n * h * w, ldc), pin, rng)
    pre = requant_ref(acc, pin, relu).reshape(n, h, w, ldc)
    out, arg = pool_first_max(pre, 3, 2, 1, p3_out(h), p3_out(w))
    return dict(zip(("acc", "pre", "out", "arg"), _ro(acc, pre, out, arg)))


def window_place(oy, ox, oh, ow):
    """corner / edge / interior of the pooled map's window (oy, ox)."""
    on_y, on_x = oy in (0, oh - 1), ox in (0, ow - 1)
    return "corner" if on_y and on_x else "edge" if on_y or on_x else "interior"


# --------------------------------------------------------------------------------- G. stem pool pair
PP_MAPS = [(2, 1, 1), (1, 2, 2), (3, 7, 9), (2, 10, 6)]   # (n, H, W)
PP_CPS = (16, 48)
PP_POOLS = [(3, 2, 1), (2, 2, 0)]   # (k, s, p)
PP_GENERIC_POOL = (5, 2, 2)         # overlapping, and never the packed kernel's
PP_WRAP_MAPS = [(3, 7, 9), (2, 10, 6)]   # maps with the planted four-window pixel (3, 3) of image 0
# F's cases G's arg is compared with: relu, on the maps the two groups share
PP_SHARED_WITH_F = [(2, 1, 1, 16), (3, 7, 9, 48), (2, 10, 6, 16)]
POOLED_VALUES = np.array([0, 1, 127, -128, -1, 5, 0, 2], np.int8)


def pp_out(h, k, s, p):
    """Pooled size: the stem pool's (h - 1) / 2 + 1 at 3x3 / 2 / 1, else the oracle's."""
    return p3_out(h) if (k, s, p) == (3, 2, 1) else O.pool_out(h, k, s, p)


@functools.lru_cache(maxsize=None)
def pp_case(n, h, w, cp, k, s, p, relu):
    """dict(x NHWC in -2 .. 5 (relu: 0 .. 5), y (oracle_pool), arg (first_at_least), dy over the
    whole int8 range, pooled (bytes 0, 1, 127 and negative ones), sums / sums_pooled (int64,
    pool_grad_sums; the wrapped sums equal oracle_pool_grad).  On the PP_WRAP_MAPS
    pixel (3, 3) of image 0 is the strict max of its four 3x3 / 2 windows, whose dy is 127."""
    rng = _seed(7, n, h, w, cp, k, s, p, relu)
    x = rng.integers(0 if relu else -2, 6, (n, h, w, cp)).astype(np.int8)
    oh, ow = pp_out(h, k, s, p), pp_out(w, k, s, p)
    dy = rng.integers(-128, 128, (n, oh, ow, cp)).astype(np.int8)
    dy.reshape(-1)[:2] = (-128, 127)
    if (n, h, w) in PP_WRAP_MAPS and (k, s, p) == (3, 2, 1):
        x[0, 1:6, 1:6, :] = np.minimum(x[0, 1:6, 1:6, :], 4)
        x[0, 3, 3, :] = 5
        dy[0, 1:3, 1:3, :] = 127
    pooled = POOLED_VALUES[rng.integers(0, len(POOLED_VALUES), dy.shape)]
    pooled.reshape(-1)[:len(POOLED_VALUES)] = POOLED_VALUES
    y = oracle_pool(x, k, s, p, oh, ow)
    arg = first_at_least(x, y, k, s, p)
    sums = pool_grad_sums(arg, dy, h, w, k, s, p)
    sums_pooled = pool_grad_sums(arg, dy, h, w, k, s, p, pooled)
    return dict(zip(("x", "y", "arg", "dy", "pooled", "sums", "sums_pooled"),
                    _ro(x, y, arg, dy, pooled, sums, sums_pooled)))


# ===================================================================================== GPU runners
# Each runs one case through niti_amd.ops and returns the list of mismatches against the reference
# (empty: all equal).  T is torch.
class Buf:
    """An int8 device buffer of `shape` filled with FILL between two GUARD-byte runs of it."""

    def __init__(self, T, shape):
        self.shape = tuple(shape)
        n = int(np.prod(self.shape))
        self.all = T.full((n + 2 * GUARD,), FILL, dtype=T.int8, device="cuda")
        self.t = self.all[GUARD:GUARD + n].view(self.shape)

    def check(self, want, name, bad, tag):
        got = self.all.cpu().numpy()
        if (got[:GUARD] != FILL).any() or (got[-GUARD:] != FILL).any():
            bad.append((tag, name, "wrote outside the buffer"))
        got = got[GUARD:-GUARD].reshape(self.shape)
        if want is None:
            want = np.full(self.shape, FILL, np.int8)
        if not np.array_equal(got, want.reshape(self.shape)):
            diff = np.argwhere(got != want.reshape(self.shape))
            bad.append((tag, name, f"{len(diff)} bytes differ, first at {tuple(int(v) for v in diff[0])}: "
                        f"{got[tuple(diff[0])]} for {want.reshape(self.shape)[tuple(diff[0])]}"))


def dev(T, a):
    return T.from_numpy(np.array(a)).cuda()   # (a copy: the cached cases are read-only)


def pinned_range(T, ops, pin):
    amax = ops.new_range()
    amax[0] = int(np.int32(np.uint32(pin)))
    return amax


def _exps(T, exp_in, wscale):
    i8 = lambda v: T.tensor([v], dtype=T.int8, device="cuda")  # noqa: E731
    return dict(exp_in=i8(exp_in), wscale=i8(wscale), exp_out=i8(99))


def _check_exp(e, pin, exp_in, wscale, bad, tag):
    if int(e["exp_out"].item()) != exp_ref(pin, exp_in, wscale):
        bad.append((tag, "exp_out", int(e["exp_out"].item()), exp_ref(pin, exp_in, wscale)))


def run_pool_fwd(T, ops, shape, pin, relu, exp=EXP):
    n, h, w, ldc = shape
    c = pf_case(shape, pin, relu)
    tag, bad = ("A", shape, pin, relu), []
    out, pool = Buf(T, c["out"].shape), Buf(T, c["pool"].shape)
    e = _exps(T, *exp)
    ops.requant_act_fused(dev(T, c["acc"]), pinned_range(T, ops, pin), relu=relu, out=out.t, pool_out=pool.t,
                          pool_hw=(h, w), **e)
    out.check(c["out"], "out", bad, tag)
    pool.check(c["pool"], "pool_out", bad, tag)
    _check_exp(e, pin, *exp, bad, tag)
    return bad


def run_pool_bwd(T, ops, geo, pin, relu, with_out, c32=False, p16=False, exp=EXP):
    n, h, w, ldc = geo
    c = pb_case(n, h, w, ldc, pin, relu)
    tag, bad = ("D" if p16 else "B", geo, pin, relu, with_out), []
    dx = Buf(T, c["dx"].shape)
    out = Buf(T, c["q"].shape)
    dc32 = Buf(T, c["dx"].shape) if c32 else None
    dp16 = Buf(T, c["dx"].shape) if p16 else None
    e = _exps(T, *exp)
    ops.requant_act_fused(dev(T, c["acc"]), pinned_range(T, ops, pin), out=out.t if with_out else None,
                          pool_x=dev(T, c["x"]), pool_y=dev(T, c["y"]), pool_dx=dx.t, pool_relu=relu, pool_hw=(h, w),
                          pool_dx_c32=dc32.t if c32 else None, out_p16=dp16.t if p16 else None, **e)
    dx.check(c["dx"], "dx", bad, tag)
    out.check(c["q"] if with_out else None, "out", bad, tag)
    if c32:
        dc32.check(c32_of(c["dx"]), "dx_c32", bad, tag)
    if p16:
        dp16.check(p16_of(c["dx"].reshape(-1, ldc)), "out_p16", bad, tag)
    _check_exp(e, pin, *exp, bad, tag)
    return bad


P16_MODES = (("out", {}), ("out_relu", dict(relu=True)), ("out_mask", None))


def run_p16_plain(T, ops, rows, ldc, pin, exp=EXP, modes=P16_MODES):
    c = p16_case(rows, ldc, pin)
    bad = []
    acc, mask, amax = dev(T, c["acc"]), dev(T, c["mask"]), pinned_range(T, ops, pin)
    for key, kw in modes:
        tag = ("C", rows, ldc, pin, key)
        kw = dict(relu_mask=mask) if kw is None else kw
        out, p16 = Buf(T, (rows, ldc)), Buf(T, (rows // 16, ldc, 16))
        e = _exps(T, *exp)
        ops.requant_act_fused(acc, amax, out=out.t, out_p16=p16.t, **kw, **e)
        out.check(c[key], "out", bad, tag)
        p16.check(p16_of(c[key]), "out_p16", bad, tag)
        _check_exp(e, pin, *exp, bad, tag)
    return bad


def run_zero_cls(T, ops, shape, cls, pin, with_mask, exp=EXP):
    n, h, w, ldc = shape
    c = zc_case(shape, cls, pin)
    tag, bad = ("E", shape, cls, pin, with_mask), []
    out = Buf(T, c["out"].shape)
    e = _exps(T, *exp)
    ops.requant_act_fused(dev(T, c["acc"]), pinned_range(T, ops, pin), out=out.t, zero_cls=cls, zc_hw=(h, w),
                          relu_mask=dev(T, c["mask"]) if with_mask else None, **e)
    out.check(c["out_mask" if with_mask else "out"], "out", bad, tag)
    _check_exp(e, pin, *exp, bad, tag)
    return bad


def run_pool3(T, ops, shape, pin, relu, with_pre, exp=EXP):
    n, h, w, ldc = shape
    c = p3_case(shape, pin, relu)
    tag, bad = ("F", shape, pin, relu, with_pre), []
    out, arg, pre = Buf(T, c["out"].shape), Buf(T, c["arg"].shape), Buf(T, c["pre"].shape)
    e = _exps(T, *exp)
    ops.requant_act_fused(dev(T, c["acc"]), pinned_range(T, ops, pin), relu=relu, out=pre.t if with_pre else None,
                          pool3_out=out.t, pool3_arg=arg.t, pool3_hw=(h, w), pool3_ohw=(p3_out(h), p3_out(w)), **e)
    out.check(c["out"], "pool3_out", bad, tag)
    arg.check(c["arg"], "pool3_arg", bad, tag)
    pre.check(c["pre"] if with_pre else None, "out", bad, tag)
    _check_exp(e, pin, *exp, bad, tag)
    return bad


def pool3_table_mismatch(T, ops, shapes):
    """Every pin, relu on and off, with and without the pre-pool output, on `shapes` (the strip-size
    children's body)."""
    bad, runs = [], 0
    for shape in shapes:
        for _, pin in PINS:
            for relu in (False, True):
                for with_pre in (False, True):
                    bad += run_pool3(T, ops, shape, pin, relu, with_pre)
                    runs += 1
    return bad, runs
