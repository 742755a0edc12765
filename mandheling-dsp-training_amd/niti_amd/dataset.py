"""Device-resident dataset (niti_dataset_* of include/niti_hip.h): the whole training or test set
in device memory, an epoch's order (a permutation plus per-image crop offset and flip) set once per
epoch, and every batch gathered out of it on the device -- see NitiModel.fit_epoch /
evaluate_dataset."""
from __future__ import annotations

import ctypes as C

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


class DeviceDataset:
    """uint8 images [count][C][H][W] and int labels [count] (numpy arrays or torch tensors, host or
    device) copied into device memory once."""

    def __init__(self, images, labels):
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

    def set_order(self, index, xform=None):
        """The order later steps walk (int32 arrays; index -1 = a padding entry).  Replacing an
        order synchronises the device: once per epoch."""
        index = np.ascontiguousarray(index, np.int32)
        xp = None
        if xform is not None:
            xform = np.ascontiguousarray(xform, np.int32)
            if xform.shape != index.shape:
                raise ValueError("xform must have index's shape")
            xp = xform.ctypes.data_as(C.c_void_p)
        check(self._lib.niti_dataset_set_order(self._h, index.ctypes.data_as(C.c_void_p), xp, index.size), "set_order")
        self.order_len = int(index.size)

    def gather(self, first: int, n: int, images_out, labels_out, stream=None):
        """niti_batch_gather: entries [first, first + n) of the order into two device tensors."""
        from .ops import _stream
        check(self._lib.niti_batch_gather(self._h, int(first), int(n), C.c_void_p(images_out.data_ptr()),
                                          C.c_void_p(labels_out.data_ptr()), _stream(stream)), "batch_gather")

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            self._lib.niti_dataset_destroy(h)
            self._h = None
