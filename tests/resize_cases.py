"""Expected values of the crop-and-resize gather (niti_batch_gather on an order with windows): the
definition in include/niti_hip.h stated directly in NumPy and plain integers, one pixel at a
time; it never calls the library.

Entry i of an order, s = index[i], window (x0, y0, cw, ch), flip = xform[i] >> 16 & 1:
  s == -1: a zero image, label -1
  else  pos(o, n_out, cn) = 0 if n_out == 1 else (2*o*(cn-1)*256 + (n_out-1)) // (2*(n_out-1))
        px = pos(ow-1-x if flip else x, ow, cw); ix = x0 + (px >> 8); fx = px & 255; ix1 = min(ix+1, x0+cw-1)
        py = pos(y, oh, ch);                     iy = y0 + (py >> 8); fy = py & 255; iy1 = min(iy+1, y0+ch-1)
        out = (((256-fx)*A + fx*B)*(256-fy) + ((256-fx)*C + fx*D)*fy + 32768) >> 16
        with A, B = data[s][c][iy][ix, ix1] and C, D = data[s][c][iy1][ix, ix1]; the label is labels[s].
"""
import numpy as np


def pos(o, n_out, cn):
    if n_out == 1:
        return 0
    return (2 * o * (cn - 1) * 256 + (n_out - 1)) // (2 * (n_out - 1))


def resize_ref(data, labels, index, xform, windows, oh, ow):
    data = np.asarray(data)
    c = data.shape[1]
    n = len(index)
    out = np.zeros((n, c, oh, ow), np.uint8)
    lab = np.full(n, -1, np.int32)
    for i in range(n):
        s = int(index[i])
        if s == -1:
            continue
        flip = 0 if xform is None else (int(xform[i]) >> 16) & 1
        x0, y0, cw, ch = (int(v) for v in windows[i])
        lab[i] = labels[s]
        for y in range(oh):
            py = pos(y, oh, ch)
            iy, fy = y0 + (py >> 8), py & 255
            iy1 = min(iy + 1, y0 + ch - 1)
            for x in range(ow):
                px = pos(ow - 1 - x if flip else x, ow, cw)
                ix, fx = x0 + (px >> 8), px & 255
                ix1 = min(ix + 1, x0 + cw - 1)
                for k in range(c):
                    a, b = int(data[s, k, iy, ix]), int(data[s, k, iy, ix1])
                    cc, d = int(data[s, k, iy1, ix]), int(data[s, k, iy1, ix1])
                    v = ((256 - fx) * a + fx * b) * (256 - fy) + ((256 - fx) * cc + fx * d) * fy + 32768
                    assert v < 1 << 32  # (the 32-bit headroom the definition claims)
                    out[i, k, y, x] = v >> 16
    return out, lab


def bilinear_f64(plane, window, oh, ow):
    """The real-valued corner-to-corner bilinear resize of one window of one 2-D plane (float64)."""
    x0, y0, cw, ch = (int(v) for v in window)
    src = np.asarray(plane, np.float64)[y0:y0 + ch, x0:x0 + cw]
    ys = np.zeros(oh) if oh == 1 else np.arange(oh) * (ch - 1) / (oh - 1)
    xs = np.zeros(ow) if ow == 1 else np.arange(ow) * (cw - 1) / (ow - 1)
    iy = np.minimum(np.floor(ys).astype(int), ch - 1)
    ix = np.minimum(np.floor(xs).astype(int), cw - 1)
    fy, fx = (ys - iy)[:, None], (xs - ix)[None, :]
    iy1, ix1 = np.minimum(iy + 1, ch - 1), np.minimum(ix + 1, cw - 1)
    top = src[iy][:, ix] * (1 - fx) + src[iy][:, ix1] * fx
    bot = src[iy1][:, ix] * (1 - fx) + src[iy1][:, ix1] * fx
    return top * (1 - fy) + bot * fy


def parity_order(count, h, w, oh, ow):
    """The order of the GPU parity test for one geometry (needs h >= oh, w >= ow, w >= 5, h >= 3):
    the full image, the identity window (oh x ow), 1x1, 1 x ch and cw x 1 windows, windows flush
    with the right and bottom edges, an upscale from 3 px, wide flat windows (a downscale along x,
    an upscale along y) -- each with and without flip -- then a repeated index under two windows
    and an index -1.  (The outputs of 1x1 and of width 4 are other output sizes: small_order.)
    Returns (index, xform, windows) as int32 arrays."""
    wins = [
        (0, 0, w, h),                   # the full image
        (1, 2, ow, oh),                 # the identity window
        (w - ow, h - oh, ow, oh),       # ... flush with both far edges
        (2, 1, 1, 1),                   # 1x1
        (w - 1, h - 1, 1, 1),
        (3, 0, 1, h),                   # 1 x ch
        (0, 2, w, 1),                   # cw x 1
        (w - 3, h - 2, 3, 2),           # flush right and bottom: ix1 / iy1 clamp
        (w - 2, 0, 2, h),
        (1, 1, 3, 3),                   # upscale from 3 px
        (0, 0, w, 4 if h >= 4 else h),  # wide and flat
        (0, 1, w, 2),
    ]
    ent = [(wd, f) for wd in wins for f in (0, 1)]
    ent += [((0, 0, w, h), 0), ((1, 0, 4, 3), 1), ((0, 0, 2, 2), 1)]
    n = len(ent)
    index = (np.arange(n) * 5 % count).astype(np.int32)
    index[-2] = index[-3]  # a repeated index, under two windows
    index[-1] = -1
    windows = np.array([e[0] for e in ent], np.int32)
    xform = np.array([e[1] << 16 for e in ent], np.int32)
    return index, xform, windows


def small_order(count, h, w):
    """Entries for the outputs of 1x1 and of (oh, 4): the full image (the downscale from the full
    width to 4), a 1x1 window and an inner window, with and without flip, and an index -1."""
    ent = [(wd, f) for wd in ((0, 0, w, h), (w - 1, 0, 1, 1), (1, 1, w - 2, h - 2)) for f in (0, 1)]
    index = (np.arange(len(ent) + 1) * 3 % count).astype(np.int32)
    index[-1] = -1
    windows = np.array([e[0] for e in ent] + [(0, 0, 1, 1)], np.int32)
    xform = np.array([e[1] << 16 for e in ent] + [0], np.int32)
    return index, xform, windows
