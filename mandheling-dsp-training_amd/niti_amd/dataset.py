"""Device-resident dataset (niti_dataset_* of include/niti_hip.h): the whole training or test set
in device memory, an epoch's order (a permutation plus per-image crop offset and flip, or -- for
images stored at another size than the model's input -- a crop window each, resized on the device)
set once per epoch, and every batch gathered out of it on the device -- see NitiModel.fit_epoch /
evaluate_dataset."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib as L
from ._lib import check


def pack_xform(dx, dy, flip):
    """int32 transform words: dx, dy in [-128, 127] as two's-complement bytes 0 and 1, flip bit 16."""
    dx, dy, flip = np.asarray(dx, np.int64), np.asarray(dy, np.int64), np.asarray(flip, np.int64)
    if np.any((dx < -128) | (dx > 127) | (dy < -128) | (dy > 127)):
        raise ValueError("dx, dy must lie in [-128, 127]")
    return ((dx & 0xff) | ((dy & 0xff) << 8) | ((flip != 0).astype(np.int64) << 16)).astype(np.int32)


def unpack_xform(xform):
    """(dx, dy, flip) of transform words (the inverse of pack_xform)."""
    x = np.asarray(xform).astype(np.int64)
    return (x & 0xff).astype(np.uint8).view(np.int8).astype(np.int32).reshape(x.shape), \
        ((x >> 8) & 0xff).astype(np.uint8).view(np.int8).astype(np.int32).reshape(x.shape), \
        ((x >> 16) & 1).astype(np.int32)


def make_order(count: int, batch: int, seed: int, epoch: int, pad: int = 0, flip: bool = False,
               drop_last: bool = True):
    """One epoch's order over `count` images, deterministic in (seed, epoch): (index, xform), two
    int32 arrays whose length is a multiple of `batch`.  index is a seeded permutation, cut to whole
    batches (drop_last) or filled up with -1 entries; xform packs dx, dy uniform in [-pad, pad]
    (zero-pad by `pad`, random crop) and, with flip, a fair coin."""
    if count <= 0 or batch <= 0 or not 0 <= pad <= 127:
        raise ValueError("count and batch must be positive, pad in [0, 127]")
    rng = np.random.default_rng([int(seed), int(epoch)])
    index = rng.permutation(count).astype(np.int32)
    if drop_last:
        index = index[:count // batch * batch]
    else:
        index = np.concatenate([index, np.full((-count) % batch, -1, np.int32)])
    n = len(index)
    dx = rng.integers(-pad, pad + 1, n)
    dy = rng.integers(-pad, pad + 1, n)
    fl = rng.integers(0, 2, n) if flip else np.zeros(n, np.int64)
    return index, pack_xform(dx, dy, fl)


def center_windows(n: int, h: int, w: int, fraction=(0.875, 0.875)):
    """n equal crop windows (x0, y0, cw, ch), int32 [n][4]: the reference's centre crop
    (ImageDataset.cpp:154-159), int(h * fraction[0]) x int(w * fraction[1]) pixels starting at
    ((h - ch) // 2, (w - cw) // 2)."""
    ch, cw = int(h * fraction[0]), int(w * fraction[1])
    if n <= 0 or not (1 <= ch <= h and 1 <= cw <= w):
        raise ValueError("the crop must lie inside the image")
    return np.tile(np.array([(w - cw) // 2, (h - ch) // 2, cw, ch], np.int32), (n, 1))


def random_fraction_windows(n: int, h: int, w: int, fraction=(0.875, 0.875), seed: int = 0, epoch: int = 0):
    """The reference's centerOrRandomCrop = true (ImageDataset.cpp:161-170): center_windows' size,
    the start uniform in [0, h - ch] x [0, w - cw]; deterministic in (seed, epoch)."""
    win = center_windows(n, h, w, fraction)
    rng = np.random.default_rng([int(seed), int(epoch)])
    win[:, 1] = rng.integers(0, h - win[:, 3] + 1)
    win[:, 0] = rng.integers(0, w - win[:, 2] + 1)
    return win


def make_rrc_order(count: int, batch: int, seed: int, epoch: int, h: int, w: int, scale=(0.08, 1.0),
                   ratio=(3 / 4, 4 / 3), flip: bool = True, drop_last: bool = True):
    """One epoch's random-resized-crop order over `count` images stored at h x w, deterministic in
    (seed, epoch): (index, xform, windows).  index is make_order's (the same seeded permutation);
    xform carries the flip bit only.  Each window takes the first of 10 draws -- an area of
    h * w * U(scale), an aspect ratio cw / ch log-uniform in `ratio`, both sides rounded -- that fits
    the image, at a uniform position; if none fits, the centred largest crop whose aspect is
    clamped into `ratio`.  Every window lies inside the image by construction."""
    if count <= 0 or batch <= 0 or h <= 0 or w <= 0 or not (0 < scale[0] <= scale[1]) or not (0 < ratio[0] <= ratio[1]):
        raise ValueError("count, batch, h, w must be positive, scale and ratio ascending positive pairs")
    rng = np.random.default_rng([int(seed), int(epoch)])
    index = rng.permutation(count).astype(np.int32)
    if drop_last:
        index = index[:count // batch * batch]
    else:
        index = np.concatenate([index, np.full((-count) % batch, -1, np.int32)])
    n = len(index)
    area = h * w * rng.uniform(scale[0], scale[1], (n, 10))
    ar = np.exp(rng.uniform(math.log(ratio[0]), math.log(ratio[1]), (n, 10)))
    cw = np.rint(np.sqrt(area * ar)).astype(np.int64)
    ch = np.rint(np.sqrt(area / ar)).astype(np.int64)
    fits = (cw >= 1) & (cw <= w) & (ch >= 1) & (ch <= h)
    first = np.argmax(fits, axis=1)
    rows = np.arange(n)
    hit = fits[rows, first]
    # the fall-back: the whole image, cut to the nearest admitted aspect, centred
    if w / h < ratio[0]:
        fw, fh = w, min(h, max(1, int(round(w / ratio[0]))))
    elif w / h > ratio[1]:
        fw, fh = min(w, max(1, int(round(h * ratio[1])))), h
    else:
        fw, fh = w, h
    cw = np.where(hit, cw[rows, first], fw)
    ch = np.where(hit, ch[rows, first], fh)
    x0 = np.where(hit, np.floor(rng.random(n) * (w - cw + 1)).astype(np.int64), (w - cw) // 2)
    y0 = np.where(hit, np.floor(rng.random(n) * (h - ch + 1)).astype(np.int64), (h - ch) // 2)
    x0, y0 = np.minimum(x0, w - cw), np.minimum(y0, h - ch)
    fl = rng.integers(0, 2, n) if flip else np.zeros(n, np.int64)
    windows = np.stack([x0, y0, cw, ch], axis=1).astype(np.int32)
    return index, pack_xform(np.zeros(n, np.int64), np.zeros(n, np.int64), fl), windows


class DeviceDataset:
    """uint8 images [count][C][H][W] and int labels [count] (numpy arrays or torch tensors, host or
    device) copied into device memory once.  out_hw = (oh, ow) is the size of a gathered image when
    it is not the stored one: orders then carry crop windows (set_order(..., windows=))."""

    def __init__(self, images, labels, out_hw=None):
        import torch
        self._lib = L.lib()
        self._h = None
        img = images if isinstance(images, torch.Tensor) else np.ascontiguousarray(images)
        if isinstance(labels, torch.Tensor):
            lab = labels.to(torch.int32).contiguous()
        else:
            lab = np.ascontiguousarray(np.asarray(labels).astype(np.int32))
        if isinstance(img, torch.Tensor):
            img = img.contiguous()
        if str(img.dtype).split(".")[-1] != "uint8" or len(img.shape) != 4 or img.shape[0] != lab.shape[0]:
            raise ValueError("images must be uint8 [count][C][H][W] with one label each")
        ptr = lambda a: C.c_void_p(a.data_ptr() if isinstance(a, torch.Tensor) else a.ctypes.data)  # noqa: E731
        self.count, self.c, self.h, self.w = (int(v) for v in img.shape)
        h = C.c_void_p()
        check(self._lib.niti_dataset_create(ptr(img), ptr(lab), self.count, self.c, self.h, self.w, C.byref(h)),
              "dataset_create")
        self._h = h
        self.order_len = 0
        self.oh, self.ow = self.h, self.w
        self.has_windows = False
        if out_hw is not None:
            self.set_output(*out_hw)

    def set_output(self, oh: int, ow: int):
        """The size of a gathered image (niti_dataset_set_output); drops the order."""
        check(self._lib.niti_dataset_set_output(self._h, int(oh), int(ow)), "set_output")
        self.oh, self.ow = int(oh), int(ow)
        self.order_len = 0
        self.has_windows = False

    def set_order(self, index, xform=None, windows=None):
        """The order later steps walk (int32 arrays; index -1 = a padding entry).  windows: int32
        [len][4] = (x0, y0, cw, ch), each entry's crop inside the stored image, resized to the
        output size (xform may then carry the flip bit only).  Replacing an order synchronises the
        device: once per epoch."""
        index = np.ascontiguousarray(index, np.int32)
        xp = None
        if xform is not None:
            xform = np.ascontiguousarray(xform, np.int32)
            if xform.shape != index.shape:
                raise ValueError("xform must have index's shape")
            xp = xform.ctypes.data_as(C.c_void_p)
        if windows is not None:
            windows = np.ascontiguousarray(windows, np.int32)
            if windows.shape != index.shape + (4,):
                raise ValueError("windows must be [len][4]")
            check(self._lib.niti_dataset_set_order_windows(self._h, index.ctypes.data_as(C.c_void_p), xp,
                                                           windows.ctypes.data_as(C.c_void_p), index.size),
                  "set_order_windows")
        else:
            check(self._lib.niti_dataset_set_order(self._h, index.ctypes.data_as(C.c_void_p), xp, index.size),
                  "set_order")
        self.has_windows = windows is not None
        self.order_len = int(index.size)

    def gather(self, first: int, n: int, images_out, labels_out, stream=None):
        """niti_batch_gather: entries [first, first + n) of the order into two device tensors
        (images_out uint8 [n][C][oh][ow], sized by the caller)."""
        from .ops import _stream
        check(self._lib.niti_batch_gather(self._h, int(first), int(n), C.c_void_p(images_out.data_ptr()),
                                          C.c_void_p(labels_out.data_ptr()), _stream(stream)), "batch_gather")

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            self._lib.niti_dataset_destroy(h)
            self._h = None
