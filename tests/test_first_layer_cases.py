"""CPU checks of tests/first_layer_cases.py: the tables reach the rule classes they are meant to,
and the numpy restatements (im2col copy, weight columns, pool codes) agree with the oracle."""
import numpy as np
import pytest

import first_layer_cases as F
import niti_oracle as O


@pytest.mark.parametrize("cls", F.CONV0_CLASSES)
@pytest.mark.parametrize("c_out", F.CONV0_COUT)
def test_conv0_cases_reach_their_class(c_out, cls):
    ref = F.conv0_reference(c_out, cls, True)
    s = ref["shift"]
    assert {"raw": s <= 0, "one": s == 1, "psto": s >= 2}[cls], s
    if cls == "raw":
        assert ref["range"] == 128  # the wrapping cell
    if cls == "one":
        assert 129 <= ref["range"] <= 256
    assert ref["pool"].max() > 0 and (ref["code"] == 0).any() and all((ref["code"] == 1 << k).any() for k in range(4))


@pytest.mark.parametrize("shape", F.IM2COL_SHAPES)
def test_xcol_times_wcol_is_the_oracle_conv(shape):
    c, hw, k, pad, co = shape
    ref = F.im2col_reference(c, hw, k, pad, co, False)
    g = O.geom(F.BATCH, c, hw, hw, co, k, pad=pad)
    acc, _ = O.conv_fwd_acc(g, ref["x"], ref["w"])
    mine = ref["xcol"].astype(np.int64) @ F.wcol_of(ref["w"], co).astype(np.int64).T
    assert np.array_equal(mine.reshape(F.BATCH, g.oh, g.ow, co).transpose(0, 3, 1, 2), acc)
    assert ref["range"] == np.abs(mine).max()


def test_pool_code_routes_like_the_oracle_pool_gradient():
    """The code's bit is the window element the oracle's pool gradient (then relu gradient) feeds."""
    ref = F.conv0_reference(20, "psto", True)
    r, p = ref["out"], ref["pool"]
    dy = np.ones(p.shape, np.int8)
    dx = O.relu_grad(r, O.maxpool_grad(r, p, dy))
    for k, (a, b) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        assert np.array_equal(dx[:, :, a::2, b::2] != 0, (ref["code"] >> k) & 1 == 1), k
