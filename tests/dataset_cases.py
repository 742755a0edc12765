"""Expected values of the device-resident dataset's batch gather (niti_batch_gather): the
definition in include/niti_hip.h stated directly in NumPy, one pixel at a time; it never calls the
library.

Entry i of an order, s = index[i], t = xform[i] (0 without xform):
  s == -1: a zero image, label -1
  else dx = (int8)(t & 0xff), dy = (int8)(t >> 8 & 0xff), flip = t >> 16 & 1 and
       out[i][ch][y][x] = data[s][ch][y + dy][(W - 1 - x if flip else x) + dx], 0 outside the image;
       the label is labels[s].
"""
import numpy as np


def _s8(v):
    v &= 0xff
    return v - 256 if v >= 128 else v


def gather_ref(data, labels, index, xform=None):
    data = np.asarray(data)
    _, c, h, w = data.shape
    n = len(index)
    out = np.zeros((n, c, h, w), np.uint8)
    lab = np.full(n, -1, np.int32)
    for i in range(n):
        s = int(index[i])
        if s == -1:
            continue
        t = 0 if xform is None else int(xform[i]) & 0xffffffff
        dx, dy, flip = _s8(t), _s8(t >> 8), (t >> 16) & 1
        lab[i] = labels[s]
        for y in range(h):
            ys = y + dy
            if not 0 <= ys < h:
                continue
            for x in range(w):
                xs = (w - 1 - x if flip else x) + dx
                if 0 <= xs < w:
                    out[i, :, y, x] = data[s, :, ys, xs]
    return out, lab


def parity_order(count, h, w):
    """The order of the GPU parity test for one geometry: every dx in [-w-1, w+1] x flip {0, 1} at
    dy = 0, every dy in [-h-1, h+1] at dx = 2 with flip, the extremes dx, dy in {-128, 127}, a
    repeated index and an index -1.  Returns (index, xform) as int32 arrays."""
    from niti_amd import pack_xform
    ent = [(dx, 0, f) for dx in range(-w - 1, w + 2) for f in (0, 1)]
    ent += [(2, dy, 1) for dy in range(-h - 1, h + 2)]
    ent += [(dx, dy, f) for dx in (-128, 127) for dy in (-128, 127, 0) for f in (0, 1)]
    ent += [(0, dy, 0) for dy in (-128, 127)]
    ent += [(1, -1, 0), (0, 0, 0), (0, 0, 1)]
    n = len(ent)
    index = (np.arange(n) * 7 % count).astype(np.int32)
    index[-2] = index[-3]  # a repeated index, under two transforms
    index[-1] = -1
    dx, dy, f = (np.array(v) for v in zip(*ent))
    return index, pack_xform(dx, dy, f)
