"""CPU-side checks of the crop-and-resize gather: the statement of its definition
(resize_cases.resize_ref) on hand-written answers and on the properties the definition promises, so
that the GPU parity test's reference is not circular; its distance from real-valued bilinear
interpolation; niti_dataset_windows_check's every refusal; the window makers against the
reference's crop arithmetic; make_rrc_order's properties."""
import ctypes as C

import numpy as np
import pytest

import resize_cases as R

INVALID = 5


@pytest.fixture(scope="module")
def L():
    from niti_amd import _lib
    return _lib


def _one(img, window, oh, ow, flip=0):
    img = np.asarray(img, np.uint8)
    out, lab = R.resize_ref(img[None, None], [7], [0], [flip << 16], [window], oh, ow)
    assert lab.tolist() == [7]
    return out[0, 0].tolist()


def test_resize_ref_hand_values():
    assert _one([[0, 255], [255, 0]], (0, 0, 2, 2), 3, 3) == [[0, 128, 255], [128, 128, 128], [255, 128, 0]]
    assert _one([[10, 20, 30, 40]], (0, 0, 4, 1), 1, 7) == [[10, 15, 20, 25, 30, 35, 40]]
    assert _one([[10, 20, 30, 40]], (1, 0, 3, 1), 1, 2, flip=1) == [[40, 20]]
    assert [R.pos(o, 224, 256) for o in (0, 1, 222, 223)] == [0, 293, 64987, 65280]
    assert R.pos(0, 1, 9) == 0 and R.pos(4, 5, 1) == 0
    out, lab = R.resize_ref(np.full((1, 2, 3, 3), 9, np.uint8), [4], [0, -1], None, [(0, 0, 3, 3), (0, 0, 1, 1)], 2, 2)
    assert (out[0] == 9).all() and not out[1].any() and lab.tolist() == [4, -1]


def test_resize_ref_properties():
    rng = np.random.default_rng(71)
    data = rng.integers(0, 256, (2, 2, 11, 13)).astype(np.uint8)
    labels = np.array([3, 4], np.int32)
    # a window of exactly ow x oh is the crop, byte for byte
    out, _ = R.resize_ref(data, labels, [1], None, [(4, 2, 7, 5)], 5, 7)
    assert np.array_equal(out[0], data[1, :, 2:7, 4:11])
    # a 1x1 window is a constant image
    out, _ = R.resize_ref(data, labels, [0], None, [(12, 10, 1, 1)], 4, 6)
    assert (out[0] == data[0, :, 10, 12][:, None, None]).all()
    # flip is the unflipped output reversed along x
    wins = [(0, 0, 13, 11), (2, 3, 5, 4), (9, 0, 4, 11)]
    plain, _ = R.resize_ref(data, labels, [0, 1, 0], [0, 0, 0], wins, 6, 9)
    flipped, _ = R.resize_ref(data, labels, [0, 1, 0], [1 << 16] * 3, wins, 6, 9)
    assert np.array_equal(flipped, plain[..., ::-1]) and not np.array_equal(flipped, plain)


def test_resize_ref_within_one_and_a_half_of_float_bilinear():
    """0.5 for the final rounding plus 255 * 2 / 512 for the two positions rounded to 1/256 px."""
    rng = np.random.default_rng(72)
    worst = 0.0
    for case in range(60):
        h, w = (int(v) for v in rng.integers(1, 24, 2))
        oh, ow = (int(v) for v in rng.integers(1, 20, 2))
        if case % 3 == 0:
            plane = rng.integers(0, 2, (h, w)).astype(np.uint8) * 255  # only 0 and 255
        else:
            plane = rng.integers(0, 256, (h, w)).astype(np.uint8)
        cw, ch = int(rng.integers(1, w + 1)), int(rng.integers(1, h + 1))
        win = (int(rng.integers(0, w - cw + 1)), int(rng.integers(0, h - ch + 1)), cw, ch)
        got, _ = R.resize_ref(plane[None, None], [0], [0], None, [win], oh, ow)
        err = np.abs(got[0, 0].astype(np.float64) - R.bilinear_f64(plane, win, oh, ow)).max()
        worst = max(worst, float(err))
        assert err < 1.5, (case, h, w, oh, ow, win, err)
    print("largest deviation from float64 bilinear:", worst)


def _wcheck(L, window, xform, h, w, length=None):
    window = None if window is None else np.ascontiguousarray(window, np.int32)
    xform = None if xform is None else np.ascontiguousarray(xform, np.int32)
    n = (0 if window is None else len(window)) if length is None else length
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
    return L.lib().niti_dataset_windows_check(p(window), p(xform), n, h, w)


def test_windows_check(L):
    h, w = 6, 9
    good = [(0, 0, 9, 6), (8, 5, 1, 1), (2, 1, 3, 4)]
    assert _wcheck(L, good, None, h, w) == 0
    assert _wcheck(L, good, [0, 1 << 16, 1 << 16], h, w) == 0
    assert _wcheck(L, None, None, h, w, length=3) == INVALID       # a NULL window
    assert _wcheck(L, good, None, h, w, length=0) == INVALID       # len <= 0
    assert _wcheck(L, good, None, h, w, length=-1) == INVALID
    assert _wcheck(L, good, None, 0, w) == INVALID and _wcheck(L, good, None, h, -3) == INVALID
    for bad in ((0, 0, 0, 6), (0, 0, 9, 0), (0, 0, -1, 2),         # cw, ch >= 1
                (-1, 0, 3, 3), (0, -1, 3, 3),                      # x0, y0 >= 0
                (1, 0, 9, 6), (7, 0, 3, 1), (9, 0, 1, 1),          # x0 + cw <= w
                (0, 1, 9, 6), (0, 4, 2, 3), (0, 6, 1, 1),          # y0 + ch <= h
                (2**31 - 1, 0, 2**31 - 1, 1), (0, 2**31 - 1, 1, 2**31 - 1)):  # (no 32-bit wrap)
        assert _wcheck(L, [good[0], bad], None, h, w) == INVALID, bad
    # with windows the xform words carry the flip bit only: dx, dy must be 0
    for word in (1, 0xff, 1 << 8, 0x7f00, (1 << 16) | 1, (1 << 16) | (3 << 8), 1 << 17, -1):
        assert _wcheck(L, good, [0, word, 0], h, w) == INVALID, hex(word & 0xffffffff)


def test_null_dataset_refusals_and_exports(L):
    """None of these reaches a device call: they return on a machine without a GPU."""
    lib = L.lib()
    idx = np.zeros(2, np.int32)
    win = np.array([[0, 0, 1, 1]] * 2, np.int32)
    ip, wp = idx.ctypes.data_as(C.c_void_p), win.ctypes.data_as(C.c_void_p)
    assert lib.niti_dataset_set_output(None, 4, 4) == INVALID
    assert lib.niti_dataset_set_order_windows(None, ip, None, wp, 2) == INVALID
    for name in ("niti_dataset_set_output", "niti_dataset_windows_check", "niti_dataset_set_order_windows"):
        assert name in L.header_functions(), name
        assert getattr(lib, name).argtypes is not None, name


def test_window_makers_follow_the_reference_crop():
    from niti_amd import center_windows, random_fraction_windows
    # ImageDataset.cpp:154-159 for 256 -> 224: int(256 * 0.875) = 224, start (256 - 224) / 2 = 16
    c = center_windows(5, 256, 256)
    assert c.dtype == np.int32 and c.shape == (5, 4) and (c == [16, 16, 224, 224]).all()
    # a non-square image and fractions whose product truncates: int(101 * 0.5) = 50, int(64 * 0.9) = 57
    c = center_windows(2, 101, 64, fraction=(0.5, 0.9))
    assert (c == [(64 - 57) // 2, (101 - 50) // 2, 57, 50]).all()
    with pytest.raises(ValueError):
        center_windows(1, 8, 8, fraction=(0.0, 1.0))
    # :161-170: the same size, the start uniform in [0, 256 - 224]
    r = random_fraction_windows(4000, 256, 256, seed=3, epoch=1)
    assert r.dtype == np.int32 and (r[:, 2:] == 224).all()
    assert r[:, 0].min() == 0 and r[:, 0].max() == 32 and r[:, 1].min() == 0 and r[:, 1].max() == 32
    assert np.array_equal(r, random_fraction_windows(4000, 256, 256, seed=3, epoch=1))
    assert not np.array_equal(r, random_fraction_windows(4000, 256, 256, seed=3, epoch=2))


def test_make_rrc_order_properties(L):
    from niti_amd import make_order, make_rrc_order, unpack_xform
    h = w = 256
    a = make_rrc_order(103, 8, seed=5, epoch=2, h=h, w=w)
    b = make_rrc_order(103, 8, seed=5, epoch=2, h=h, w=w)
    assert all(v.dtype == np.int32 for v in a) and all(np.array_equal(x, y) for x, y in zip(a, b))
    assert a[0].shape == (96,) and a[1].shape == (96,) and a[2].shape == (96, 4)
    assert np.array_equal(a[0], make_order(103, 8, seed=5, epoch=2)[0])  # the same permutation
    c = make_rrc_order(103, 8, seed=5, epoch=3, h=h, w=w)
    assert not np.array_equal(a[0], c[0]) and not np.array_equal(a[2], c[2])
    idx, xf, win = make_rrc_order(103, 8, seed=5, epoch=2, h=h, w=w, drop_last=False)
    assert len(idx) == len(xf) == len(win) == 104 and idx[-1] == -1
    dx, dy, fl = unpack_xform(a[1])
    assert not dx.any() and not dy.any() and set(fl.tolist()) == {0, 1}
    assert not unpack_xform(make_rrc_order(16, 8, 1, 1, h, w, flip=False)[1])[2].any()
    # every window inside the image, over many seeds and two shapes, as the library checks it
    for hh, ww, scale, ratio in ((256, 256, (0.08, 1.0), (3 / 4, 4 / 3)), (40, 72, (0.25, 1.0), (0.5, 2.0))):
        for seed in range(40):
            i2, x2, w2 = make_rrc_order(64, 8, seed, seed % 3, hh, ww, scale=scale, ratio=ratio)
            x0, y0, cw, ch = (w2[:, k].astype(np.int64) for k in range(4))
            assert (cw >= 1).all() and (ch >= 1).all() and (x0 >= 0).all() and (y0 >= 0).all()
            assert (x0 + cw <= ww).all() and (y0 + ch <= hh).all()
            assert _wcheck(L, w2, x2, hh, ww) == 0
            # area and aspect inside the asked ranges but for the rounding of both sides to whole
            # pixels (half a pixel each); the fall-back (the whole image here) is exempt
            fallback = (cw == ww) & (ch == hh)
            lo_a = (cw - 0.5) * (ch - 0.5) / (hh * ww)
            hi_a = (cw + 0.5) * (ch + 0.5) / (hh * ww)
            assert (fallback | ((hi_a >= scale[0]) & (lo_a <= scale[1]))).all()
            assert (fallback | (((cw + 0.5) / (ch - 0.5) >= ratio[0]) & ((cw - 0.5) / (ch + 0.5) <= ratio[1]))).all()
    # the draws cover the range: small and large crops, both orientations, many positions
    _, _, big = make_rrc_order(4000, 8, 11, 0, h, w)
    frac = big[:, 2].astype(np.float64) * big[:, 3] / (h * w)
    assert frac.min() < 0.12 and frac.max() > 0.9 and (big[:, 2] > big[:, 3]).any() and (big[:, 2] < big[:, 3]).any()
    assert len(set(big[:, 0].tolist())) > 100
    # a scale no draw can satisfy: every entry is the fall-back, the centred crop of clamped aspect
    _, _, fb = make_rrc_order(16, 8, 1, 1, 40, 100, scale=(4.0, 5.0), ratio=(0.5, 2.0))
    assert (fb == [10, 0, 80, 40]).all()
    _, _, fb = make_rrc_order(16, 8, 1, 1, 100, 40, scale=(4.0, 5.0), ratio=(0.5, 2.0))
    assert (fb == [0, 10, 40, 80]).all()
    _, _, fb = make_rrc_order(16, 8, 1, 1, 50, 60, scale=(4.0, 5.0))
    assert (fb == [0, 0, 60, 50]).all()
