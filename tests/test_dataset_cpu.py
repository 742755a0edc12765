"""CPU-side checks of the device-resident dataset: the NumPy statement of the gather
(dataset_cases.gather_ref) on hand-written answers, so that the GPU parity test's reference is not
circular; niti_dataset_order_check's every refusal; the null-argument refusals of the entry points
(validation comes before any device call); make_order / pack_xform properties."""
import ctypes as C

import numpy as np
import pytest

import dataset_cases as D

INVALID = 5


@pytest.fixture(scope="module")
def L():
    from niti_amd import _lib
    return _lib


IMG = np.array([[[[1, 2, 3], [4, 5, 6], [7, 8, 9]]]], np.uint8)  # 1 x 1 x 3 x 3


def _one(dx=0, dy=0, flip=0, index=0):
    from niti_amd import pack_xform
    out, lab = D.gather_ref(IMG, np.array([5], np.int32), [index], pack_xform([dx], [dy], [flip]))
    return out[0, 0].tolist(), int(lab[0])


def test_gather_ref_hand_values():
    assert _one() == ([[1, 2, 3], [4, 5, 6], [7, 8, 9]], 5)
    assert _one(dx=1) == ([[2, 3, 0], [5, 6, 0], [8, 9, 0]], 5)
    assert _one(dy=-1) == ([[0, 0, 0], [1, 2, 3], [4, 5, 6]], 5)
    assert _one(flip=1) == ([[3, 2, 1], [6, 5, 4], [9, 8, 7]], 5)
    assert _one(flip=1, dx=1) == ([[0, 3, 2], [0, 6, 5], [0, 9, 8]], 5)
    assert _one(dx=3) == ([[0, 0, 0]] * 3, 5)
    assert _one(dx=1, dy=1, flip=1, index=-1) == ([[0, 0, 0]] * 3, -1)
    out, lab = D.gather_ref(IMG, [5], [0, -1, 0])  # no xform: the identity
    assert out[0, 0].tolist() == IMG[0, 0].tolist() and out[2, 0].tolist() == IMG[0, 0].tolist()
    assert not out[1].any() and lab.tolist() == [5, -1, 5]


def _check(L, index, xform, count, batch, allow_pad, length=None):
    index = None if index is None else np.asarray(index, np.int32)
    xform = None if xform is None else np.asarray(xform, np.int32)
    n = (0 if index is None else len(index)) if length is None else length
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
    return L.lib().niti_dataset_order_check(p(index), p(xform), n, count, batch, allow_pad)


def test_order_check(L):
    from niti_amd import pack_xform
    ok_x = pack_xform([-128, 127, 0, 3], [127, -128, 0, -3], [1, 0, 1, 0])
    assert _check(L, [3, 0, 2, 1], ok_x, 4, 2, 0) == 0            # a valid unpadded order
    assert _check(L, [3, 0, 2, 1], None, 4, 4, 0) == 0            # (without xform)
    assert _check(L, [3, 0, -1, -1], ok_x, 4, 2, 1) == 0          # a valid padded order
    assert _check(L, None, None, 4, 2, 1, length=4) == INVALID    # a null index
    assert _check(L, [0, 1], None, 4, 2, 1, length=0) == INVALID  # len <= 0
    assert _check(L, [0, 1], None, 4, 2, 1, length=-2) == INVALID
    assert _check(L, [0, 1, 2], None, 4, 2, 1) == INVALID         # len % batch != 0
    assert _check(L, [0, 4], None, 4, 2, 1) == INVALID            # an index outside [-1, count)
    assert _check(L, [0, -2], None, 4, 2, 1) == INVALID
    assert _check(L, [0, -1], None, 4, 2, 0) == INVALID           # -1 while allow_pad is 0
    for bit in (17, 24, 31):                                      # an xform bit above 16
        assert _check(L, [0, 1], [0, np.int32(np.uint32(1 << bit).view(np.int32))], 4, 2, 1) == INVALID, bit
    assert _check(L, [0, 1], [0, 1 << 16], 4, 2, 1) == 0


def test_null_argument_refusals(L):
    """None of these reaches a device call: they return on a machine without a GPU."""
    lib = L.lib()
    h = C.c_void_p()
    img = np.zeros((2, 1, 3, 3), np.uint8)
    lab = np.zeros(2, np.int32)
    ip, lp = img.ctypes.data_as(C.c_void_p), lab.ctypes.data_as(C.c_void_p)
    assert lib.niti_dataset_create(None, lp, 2, 1, 3, 3, C.byref(h)) == INVALID
    assert lib.niti_dataset_create(ip, None, 2, 1, 3, 3, C.byref(h)) == INVALID
    assert lib.niti_dataset_create(ip, lp, 2, 1, 3, 3, None) == INVALID
    for count, c, hh, w in ((0, 1, 3, 3), (2, 0, 3, 3), (2, 1, 0, 3), (2, 1, 3, -1)):
        assert lib.niti_dataset_create(ip, lp, count, c, hh, w, C.byref(h)) == INVALID
    assert h.value is None
    assert lib.niti_dataset_set_order(None, lp, None, 2) == INVALID
    assert lib.niti_batch_gather(None, 0, 1, ip, lp, None) == INVALID
    assert lib.niti_model_train_steps_dataset(None, None, 0, 1, None) == INVALID
    assert lib.niti_model_eval_steps_dataset(None, None, 0, 1, None) == INVALID
    assert lib.niti_model_train_metrics(None, 1) == INVALID
    assert lib.niti_model_train_metrics_reset(None, None) == INVALID
    assert lib.niti_model_train_metrics_read(None, None, None) == INVALID
    lib.niti_dataset_destroy(None)
    for name in ("niti_dataset_create", "niti_dataset_destroy", "niti_dataset_order_check", "niti_dataset_set_order",
                 "niti_batch_gather", "niti_model_train_steps_dataset", "niti_model_eval_steps_dataset",
                 "niti_model_train_metrics", "niti_model_train_metrics_reset", "niti_model_train_metrics_read"):
        assert name in L.header_functions(), name
        assert getattr(lib, name).argtypes is not None, name


def test_make_order_properties(L):
    from niti_amd import make_order, pack_xform, unpack_xform
    a = make_order(103, 8, seed=5, epoch=2, pad=4, flip=True)
    b = make_order(103, 8, seed=5, epoch=2, pad=4, flip=True)
    assert all(v.dtype == np.int32 for v in a) and all(np.array_equal(x, y) for x, y in zip(a, b))
    c = make_order(103, 8, seed=5, epoch=3, pad=4, flip=True)
    assert not np.array_equal(a[0], c[0]) and not np.array_equal(a[1], c[1])
    assert len(a[0]) == len(a[1]) == 96 and len(set(a[0].tolist())) == 96 and a[0].min() >= 0 and a[0].max() < 103
    idx, xf = make_order(103, 8, seed=5, epoch=2, pad=4, flip=True, drop_last=False)
    assert len(idx) == len(xf) == 104 and idx[-1] == -1
    assert sorted(idx[idx >= 0].tolist()) == list(range(103))
    dx, dy, fl = unpack_xform(xf)
    assert dx.min() >= -4 and dx.max() <= 4 and dy.min() >= -4 and dy.max() <= 4
    assert set(dx.tolist()) == set(range(-4, 5)) and set(fl.tolist()) == {0, 1}
    dx0, dy0, fl0 = unpack_xform(make_order(40, 8, 1, 1)[1])  # pad 0, no flip: the identity transform
    assert not dx0.any() and not dy0.any() and not fl0.any()
    assert _check(L, idx, xf, 103, 8, 1) == 0 and _check(L, a[0], a[1], 103, 8, 0) == 0
    # pack_xform round-trips over the whole range
    gx, gy, gf = np.meshgrid(np.arange(-128, 128), np.array([-128, -1, 0, 1, 127]), np.array([0, 1]), indexing="ij")
    packed = pack_xform(gx.ravel(), gy.ravel(), gf.ravel())
    assert packed.dtype == np.int32 and int((packed.astype(np.int64) & 0xffffffff).max()) < 1 << 17
    rx, ry, rf = unpack_xform(packed)
    assert np.array_equal(rx, gx.ravel()) and np.array_equal(ry, gy.ravel()) and np.array_equal(rf, gf.ravel())
    with pytest.raises(ValueError):
        pack_xform([128], [0], [0])
