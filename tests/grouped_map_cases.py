"""Shared cases of the grouped conv map tests (importable without a GPU): maps wider than one column segment of
the kernels of csrc/niti_grouped.hip and csrc/niti_grouped_narrow.hip, non-square maps with their transposes, and
weight gradients with more (image, band, segment) units than slabs, so that a workgroup takes a second unit.

The reference is the grouped conv's definition in NumPy int64, per group a sum over the taps of shifted (strided)
slices, as depthwise_cases.dw_*_direct: the oracle over the block-diagonal dense weight would cost giga-MACs at these
sizes.  tests/test_grouped_map_cpu.py pins it to that oracle at the old op shapes and proves, from the tile sizes
named here, that every case reaches the hazard its comment names.  Shapes are (n, C, G, h, w, pad, stride).
"""
from __future__ import annotations

import functools

import numpy as np

import grouped_cases as GC
from grouped_cases import DC, O  # noqa: F401

# ------------------------------------------------------------------------------------ the kernels' tiles
ROWS = 4              # output rows of a band, every family
STRIP = 16            # the wide families (cg 16 / 32 / 64): columns of a strip
NARROW_COLS = 32      # the narrow family (cg 4 / 8): columns of a segment, 8 quads of 4
QUAD = 4
SLAB_BYTES = 4 << 20  # the plan rule: cap = max(64, min(1024, SLAB_BYTES / slab bytes)), slabs = min(cap, units)
MAX_SLABS, MIN_SLABS = 1024, 64
NARROW_MIN_WORKGROUPS = 256  # the narrow family's cap is also at least this over the 64-channel chunks


def cg_of(shape):
    return shape[1] // shape[2]


def narrow(shape):
    return cg_of(shape) < 16


def seg_cols(shape):
    """Columns of a segment: 4 strips in the wide families, 2 at stride 2 with cg 64; 32 in the narrow one."""
    if narrow(shape):
        return NARROW_COLS
    return STRIP * (2 if shape[6] == 2 and cg_of(shape) == 64 else 4)


def out_hw(shape):
    n, c, groups, h, w, pad, stride = shape
    return (h + 2 * pad - 3) // stride + 1, (w + 2 * pad - 3) // stride + 1


def unit_grid(shape, op):
    """(rows, columns) a launch tiles: the output for the forward and the weight gradient, dx for the input
    gradient at stride 1, and at stride 2 its ((y + pad) / 2, (x + pad) / 2)."""
    n, c, groups, h, w, pad, stride = shape
    if op != "dgrad":
        return out_hw(shape)
    return (h, w) if stride == 1 else ((h - 1 + pad) // 2 + 1, (w - 1 + pad) // 2 + 1)


def tiling(shape, op):
    """dict(bands, segs, units, last: columns of the last segment, full: a segment uses every strip / quad,
    part_band: the last band has fewer than 4 rows) of launch `op` in ("fwd", "dgrad", "wgrad")."""
    rows, cols = unit_grid(shape, op)
    sc, piece = seg_cols(shape), QUAD if narrow(shape) else STRIP
    bands, segs = -(-rows // ROWS), -(-cols // sc)
    last = cols - (segs - 1) * sc
    return dict(bands=bands, segs=segs, units=shape[0] * bands * segs, last=last,
                full=segs > 1 or -(-last // piece) == sc // piece, part_band=rows % ROWS != 0)


def slabs_of(shape):
    """The weight gradient's slab count, from the plan rule."""
    n, c, groups, h, w, pad, stride = shape
    one = c * 9 * (16 if narrow(shape) else cg_of(shape)) * 4
    cap = max(MIN_SLABS, min(MAX_SLABS, SLAB_BYTES // one))
    if narrow(shape):
        cap = max(cap, NARROW_MIN_WORKGROUPS // (-(-c // 64)))
    return max(1, min(cap, tiling(shape, "wgrad")["units"]))


def transposed(shape):
    n, c, groups, h, w, pad, stride = shape
    return (n, c, groups, w, h, pad, stride)


# ------------------------------------------------------------------------------------ the cases
SEG_CASES = (  # a. two segments or more, the last partial, on a non-square map with a partial last band
    (2, 32, 2, 6, 83, 1, 1),     # cg 16: 6 strips = a segment of 4, then one whole and one 3-pixel strip; bands 4 + 2
    (2, 64, 2, 6, 83, 1, 1),     # cg 32, the same map
    (2, 128, 2, 6, 83, 1, 1),    # cg 64, the same map
    (2, 32, 2, 11, 133, 1, 2),   # cg 16 / 2: 67 output columns and 67 columns of b, 6 rows of either
    (2, 64, 2, 11, 133, 1, 2),   # cg 32 / 2
    (2, 128, 2, 11, 133, 1, 2),  # cg 64 / 2: three segments of 2 strips, the last of 3 pixels
    (2, 128, 2, 11, 69, 1, 2),   # cg 64 / 2: 35 columns, two 32-column segments
    (2, 80, 20, 3, 45, 1, 1),    # cg 4: 32 + 13 columns, a partial 64-channel chunk, a 3-row band
    (2, 48, 6, 3, 45, 1, 1),     # cg 8, the same map; a partial chunk
    (2, 80, 20, 11, 69, 1, 2),   # cg 4 / 2: 35 columns = 32 + 3, 6 rows
    (2, 48, 6, 11, 69, 1, 2),    # cg 8 / 2
)
TWIN_CASES = tuple(transposed(s) for s in SEG_CASES)  # d. h and w exchanged: many bands, one narrow segment
FULL_CASES = (  # b. every strip or quad of a segment in use, and the widths of the workload
    (1, 32, 2, 8, 56, 1, 1),     # cg 16 at 56 px: 4 strips, the last of 8 pixels
    (1, 64, 2, 8, 56, 1, 1),     # cg 32
    (1, 128, 2, 8, 56, 1, 1),    # cg 64
    (1, 32, 2, 5, 64, 1, 1),     # cg 16: exactly 4 whole strips
    (1, 64, 2, 5, 64, 1, 1),     # cg 32
    (1, 128, 2, 5, 64, 1, 1),    # cg 64
    (1, 32, 2, 8, 112, 1, 2),    # cg 16 / 2 from 112 to 56 px: 4 strips; 57 columns of b
    (1, 64, 2, 8, 112, 1, 2),    # cg 32 / 2
    (1, 128, 2, 8, 112, 1, 2),   # cg 64 / 2: two segments, both of 2 strips
    (1, 64, 16, 8, 56, 1, 1),    # cg 4 at 56 px: a whole 32-column segment, then 24 columns
    (1, 64, 8, 8, 56, 1, 1),     # cg 8
    (1, 64, 16, 5, 65, 0, 2),    # cg 4 / 2: 32 output columns, one segment exactly full; 33 columns of b
    (1, 64, 8, 5, 65, 0, 2),     # cg 8 / 2
)
UNIT_CASES = (  # c. the weight gradient: 3 x 23 bands = 69 units over 64 slabs, 5 workgroups take two units
    (3, 128, 8, 90, 9, 1, 1),    # cg 16
    (3, 128, 4, 90, 9, 1, 1),    # cg 32
    (3, 128, 2, 90, 9, 1, 1),    # cg 64
    (3, 128, 8, 181, 9, 1, 2),   # cg 16 / 2: 91 output rows
    (3, 128, 4, 181, 9, 1, 2),   # cg 32 / 2
    (3, 128, 2, 181, 9, 1, 2),   # cg 64 / 2
    (3, 256, 64, 90, 9, 1, 1),   # cg 4: four chunks, cap 256 / 4
    (3, 256, 32, 90, 9, 1, 1),   # cg 8
    (3, 256, 64, 181, 9, 1, 2),  # cg 4 / 2
    (3, 256, 32, 181, 9, 1, 2),  # cg 8 / 2
)
EQ1_CASES = (  # e. the narrow kernels' shift class eq1: bit width 8, shift 1, the exponent up by 2
    (3, 80, 20, 5, 5, 1, 1),     # cg 4
    (2, 32, 4, 7, 5, 0, 1),      # cg 8, the input gradient's pad 2
    (2, 64, 16, 9, 7, 1, 2),     # cg 4 / 2
    (3, 48, 6, 8, 6, 1, 2),      # cg 8 / 2
)
ACT_CASES = SEG_CASES + TWIN_CASES + FULL_CASES
WGRAD_CASES = SEG_CASES + TWIN_CASES + FULL_CASES + UNIT_CASES
ALL_CASES = WGRAD_CASES + EQ1_CASES
INSTANTIATIONS = tuple((cg, s) for s in (1, 2) for cg in (4, 8, 16, 32, 64))


def case_id(shape):
    n, c, groups, h, w, pad, stride = shape
    return f"n{n}-C{c}-cg{c // groups}-{h}x{w}-p{pad}-s{stride}"


# ------------------------------------------------------------------------------------ the definition
def _fits(acc):
    assert int(np.abs(acc).max(initial=0)) < 2 ** 31
    return acc.astype(np.int32)


def _windows(a, oh, ow, stride):
    """The nine (ky, kx, view) of the padded map a [..., H, W]: view[..., oy, ox] = a[..., stride oy + ky, stride ox + kx]."""
    for ky in range(3):
        for kx in range(3):
            yield ky, kx, a[..., ky:ky + stride * (oh - 1) + 1:stride, kx:kx + stride * (ow - 1) + 1:stride]


def _padded(x, groups, pad):
    n, c, h, w = x.shape
    xp = np.zeros((n, groups, c // groups, h + 2 * pad, w + 2 * pad), np.int64)
    xp[..., pad:pad + h, pad:pad + w] = x.reshape(n, groups, c // groups, h, w)
    return xp


def _wg(w, groups):
    """[C, cg, 3, 3] -> int64 [G, og, cg, 3, 3]: output channel g og + o reads input channels g cg .."""
    return w.astype(np.int64).reshape(groups, w.shape[0] // groups, w.shape[1], 3, 3)


def g_fwd_direct(x, w, groups, pad, stride):
    """acc[n][g og + o][oy][ox] = sum over i, ky, kx of x[n][g cg + i][stride oy + ky - pad][stride ox + kx - pad]
    w[g og + o][i][ky][kx], as int32 [n, C, oh, ow]."""
    n, c, h, wd = x.shape
    oh, ow = (h + 2 * pad - 3) // stride + 1, (wd + 2 * pad - 3) // stride + 1
    xp, wg = _padded(x, groups, pad), _wg(w, groups)
    acc = np.zeros((n, groups, c // groups, oh, ow), np.int64)
    for ky, kx, win in _windows(xp, oh, ow, stride):
        acc += np.einsum("ngihw,goi->ngohw", win, wg[..., ky, kx])
    return _fits(acc.reshape(n, c, oh, ow))


def g_dgrad_direct(dy, w, groups, pad, stride, h, wd):
    """dx[n][g cg + i][y][x] = the sum of dy[n][g og + o][oy][ox] w[g og + o][i][ky][kx] over the (o, oy, ox, ky, kx)
    with stride oy + ky - pad = y, stride ox + kx - pad = x, as int32 [n, C, h, wd]."""
    n, c, oh, ow = dy.shape
    d, wg = dy.astype(np.int64).reshape(n, groups, c // groups, oh, ow), _wg(w, groups)
    acc = np.zeros((n, groups, c // groups, h + 2 * pad, wd + 2 * pad), np.int64)  # over the padded input
    for ky, kx, win in _windows(acc, oh, ow, stride):
        win += np.einsum("ngohw,goi->ngihw", d, wg[..., ky, kx])
    return _fits(np.ascontiguousarray(acc[..., pad:pad + h, pad:pad + wd]).reshape(n, c, h, wd))


def g_wgrad_direct(x, dy, groups, pad, stride):
    """dw[g og + o][i][ky][kx] = sum over n, oy, ox of dy[n][g og + o][oy][ox] x[n][g cg + i][stride oy + ky - pad][..],
    as int32 [C, cg, 3, 3]."""
    n, c, oh, ow = dy.shape
    xp, d = _padded(x, groups, pad), dy.astype(np.int64).reshape(n, groups, c // groups, oh, ow)
    acc = np.zeros((groups, c // groups, c // groups, 3, 3), np.int64)
    for ky, kx, win in _windows(xp, oh, ow, stride):
        acc[..., ky, kx] = np.einsum("ngohw,ngihw->goi", d, win)
    return _fits(acc.reshape(c, c // groups, 3, 3))


def act_direct(shape, a, w, dgrad):
    n, c, groups, h, wd, pad, stride = shape
    return g_dgrad_direct(a, w, groups, pad, stride, h, wd) if dgrad else g_fwd_direct(a, w, groups, pad, stride)


# ------------------------------------------------------------------------------------ inputs and references
def _seed(shape, k):
    return 9000 + 13 * ALL_CASES.index(shape) + k


def _act_shapes(shape, dgrad):
    """(the conv's input, the relu mask): x and the output's shape, or dy and x's shape."""
    n, c, groups, h, wd, pad, stride = shape
    xs, ys = (n, c, h, wd), (n, c) + out_hw(shape)
    return (ys, xs) if dgrad else (xs, ys)


@functools.lru_cache(maxsize=None)
def act_case(shape, dgrad):
    """(a, w, mask, acc): the input over the whole int8 range, -128 included, weights in -127..127, a mask with
    non-positive entries, and the direct accumulators."""
    sa, sm = _act_shapes(shape, dgrad)
    rng = np.random.default_rng(_seed(shape, 1 if dgrad else 0))
    a = rng.integers(-128, 128, sa).astype(np.int8)
    w = rng.integers(-127, 128, (shape[1], cg_of(shape), 3, 3)).astype(np.int8)
    mask = rng.integers(-3, 4, sm).astype(np.int8)
    return DC._ro(a, w, mask, act_direct(shape, a, w, dgrad))


@functools.lru_cache(maxsize=None)
def eq1_case(shape, dgrad):
    """act_case with grouped_cases.act_inputs' search: fixed uniform draws times the smallest amplitude that puts
    the accumulators' bit width at 8."""
    sa, sm = _act_shapes(shape, dgrad)
    rng = np.random.default_rng(_seed(shape, 1 if dgrad else 0))
    ua, uw = rng.uniform(-1, 1, sa), rng.uniform(-1, 1, (shape[1], cg_of(shape), 3, 3))
    mask = rng.integers(-3, 4, sm).astype(np.int8)
    for amp in range(1, 128):
        a, w = np.rint(ua * amp).astype(np.int8), np.rint(uw * amp).astype(np.int8)
        acc = act_direct(shape, a, w, dgrad)
        if DC._in_class(DC._bw(acc), "eq1"):
            return DC._ro(a, w, mask, acc)
    raise AssertionError(f"no amplitude puts {shape} in eq1")


@functools.lru_cache(maxsize=None)
def wgrad_case(shape):
    """(x, dy, acc): x over the whole int8 range, dy too with three values in ten zero, and the direct sums."""
    n, c, groups, h, wd, pad, stride = shape
    rng = np.random.default_rng(_seed(shape, 2))
    x = rng.integers(-128, 128, (n, c, h, wd)).astype(np.int8)
    dy = rng.integers(-128, 128, (n, c) + out_hw(shape)).astype(np.int8)
    dy[rng.random(dy.shape) < 0.3] = 0
    return DC._ro(x, dy, g_wgrad_direct(x, dy, groups, pad, stride))
