"""Host side of the first layer's weight gradient from the pooled gradient and the pool codes: the
entry's argument checks and grid rule (no device call is made on a refusal), the A/B switch, and the
test cases' own references (tests/conv0_wgrad_codes_cases.py) held against the issue's formula."""
import ctypes as C

import numpy as np
import pytest

import conv0_wgrad_codes_cases as K


@pytest.fixture(scope="module")
def lib():
    from niti_amd import _lib as L
    return L.lib()


def test_slab_count_rule(lib):
    """0: a workgroup per four 64-pixel steps, at most 256; else clamped to the steps."""
    slabs = lib.niti_conv0_wgrad_codes_slabs
    assert slabs(256, 32, 32, 64, 27, 0) == 256      # 1024 steps: one a wave
    assert slabs(512, 32, 32, 64, 27, 0) == 256      # never more than 256 slabs
    assert slabs(16, 32, 32, 64, 27, 0) == 16        # 64 steps
    assert slabs(3, 4, 4, 32, 27, 0) == 1            # 12 pooled pixels: one partial step
    assert slabs(3, 4, 4, 32, 27, 3) == 1            # clamped to the steps
    assert slabs(5, 32, 32, 64, 27, 3) == 3          # 20 steps on 3 workgroups
    assert slabs(5, 32, 32, 64, 27, 1000) == 20
    assert slabs(5, 8, 8, 64, 25, 1) == 1


@pytest.mark.parametrize("args", [(2, 31, 32, 64, 27), (2, 32, 30 + 1, 64, 27), (2, 32, 32, 48, 27), (2, 32, 32, 16, 27),
                                  (2, 32, 32, 64, 33), (2, 32, 32, 64, 0), (0, 32, 32, 64, 27),
                                  (1 << 16, 32, 32, 64, 27)])  # (the last: xcol of 2^31 bytes)
def test_refusals_launch_nothing(lib, args):
    from niti_amd import _lib as L
    n, oh, ow, cop, k = args
    assert lib.niti_conv0_wgrad_codes_slabs(n, oh, ow, cop, k, 0) == 0
    wrote = C.c_int(-1)
    buf = (C.c_char * 64)()
    p = C.cast(buf, C.c_void_p)
    assert lib.niti_conv0_wgrad_codes(n, oh, ow, cop, k, p, p, p, 0, p, 1 << 30, C.byref(wrote), None) == L.INVALID_VALUE
    assert wrote.value == -1


def test_null_operands_and_small_slab(lib):
    from niti_amd import _lib as L
    buf = (C.c_char * 64)()
    p = C.cast(buf, C.c_void_p)
    for a in ((None, p, p, p), (p, None, p, p), (p, p, None, p), (p, p, p, None)):
        assert lib.niti_conv0_wgrad_codes(2, 32, 32, 64, 27, a[0], a[1], a[2], 0, a[3], 1 << 30, None, None) == L.INVALID_VALUE
    # 8 steps on the default grid: 2 slabs of 64 x 32 int32, 16 KiB
    assert lib.niti_conv0_wgrad_codes(2, 32, 32, 64, 27, p, p, p, 0, p, 2 * 8192 - 1, None, None) == L.INVALID_VALUE


def test_switch_and_counter(lib):
    n0 = lib.niti_diag_conv0_wgrad_codes_launches()
    for mode in (1, 0, -1, 7, -7):
        lib.niti_diag_conv0_wgrad_codes(mode)
    lib.niti_diag_conv0_wgrad_codes(-1)
    lib.niti_diag_conv0_wgrad_blocks(3)
    lib.niti_diag_conv0_wgrad_blocks(0)
    assert lib.niti_diag_conv0_wgrad_codes_launches() == n0


@pytest.mark.parametrize("kind", K.KINDS)
@pytest.mark.parametrize("geom,pair", [(K.GEOMS[0], K.PAIRS[1]), (K.GEOMS[3], K.PAIRS[2])])
def test_case_references_follow_the_formula(geom, pair, kind):
    """The oracle's expanded-gradient weight gradient equals the masked sum over (g0, codes, xcol) that
    the kernel is specified by; the route kinds' codes are the single bit they are built for."""
    batch = 3
    c = K.op_case(batch, geom, pair, kind)
    co = pair[0]
    want = K.formula(c["g0"], c["code"], c["xcol"], batch, c["oh"], c["ow"])
    assert np.array_equal(want[:co], c["ref"].astype(np.int64))
    assert not want[co:].any() and not c["ref"][:, c["k"]:].any()
    code = c["code"][:, :co]
    assert np.isin(code, (0, 1, 2, 4, 8)).all()
    if kind.startswith("route"):
        assert (code == 1 << int(kind[-1])).all()
    if kind == "tie":
        assert (code == 1).all()
    if kind == "dead_relu":
        assert not code.any()


def test_recorded_vgg11_reference_is_the_oracles():
    """The first recorded step at batch 4 (tests/golden) against the oracle run here."""
    got = K.vgg11_oracle(4, steps=1)[0]
    ref = K.vgg11_ref(4)[0]
    assert got["exp"] == ref["exp"] and np.array_equal(got["logits"], ref["logits"]) and got["w"] == ref["w"]
    assert len(K.vgg11_ref(36)) == K.STEPS and K.vgg11_ref(36)[0]["logits"].shape[0] == 36
